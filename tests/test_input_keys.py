"""Every key of a Waiwera input file is honoured, without effect on the numbers, or refused by name
(waiwera_amd/simulation.py: KEY_TABLE, check_input_keys), and the keys the front end newly honours are read as the reference
reads them: mesh.permeability_angle and mesh.faces (face_calculate_permeability_direction, src/face.F90:210-226;
mesh_set_permeability_rotation, src/mesh.F90:316-336; the override of listed faces, src/mesh.F90:1286-1405),
thermodynamics.extrapolate and source.production_component with the component names.  No device: the flow object is the
recording stub of tests/test_input_partition.py."""
import copy
import glob
import json
import os

import numpy as np
import pytest

from tests.test_input_partition import RecordingOde
from waiwera_amd import simulation as S
from waiwera_amd import unstructured
from waiwera_amd.partition import partition_mesh

HERE = os.path.dirname(os.path.abspath(__file__))
INPUTS = os.path.join(HERE, "golden", "inputs")


# ---- the key table ----------------------------------------------------------------------------------------------------------
def schema_paths():
    with open(os.path.join(HERE, "golden", "input_schema_paths.txt")) as f:
        return [line.strip() for line in f if line.strip()]


def test_table_covers_the_schema_exactly():
    want = {S.schema_path(p) for p in schema_paths()}
    assert len(want) > 250
    assert set(S.KEY_TABLE) == want, (sorted(want - set(S.KEY_TABLE)), sorted(set(S.KEY_TABLE) - want))
    assert set(S.KEY_TABLE.values()) == {"handled", "no effect", "refused"}
    # one class per key
    assert not (set(S.HANDLED_KEYS.split()) & set(S.NO_EFFECT_KEYS.split()))
    assert not ((set(S.HANDLED_KEYS.split()) | set(S.NO_EFFECT_KEYS.split())) & set(S.REFUSED_KEYS))
    for key in ("thermodynamics.extrapolate", "source.production_component", "mesh.permeability_angle", "mesh.faces.cells",
                "mesh.faces.permeability_direction"):
        assert S.KEY_TABLE[key] == "handled"


def minimal_input(path):
    """the smallest input that names the key: nested objects along the path, any name for a user-chosen one"""
    inp = leaf = {}
    parts = path.split(".")
    for k, part in enumerate(parts):
        name = "anything" if part == "*" else part
        leaf[name] = {} if k < len(parts) - 1 else 1
        leaf = leaf[name]
    return inp


@pytest.fixture
def no_library(monkeypatch):
    """the walk comes before the library: its loader (waiwera_amd.lib loads the shared library when it is imported) and the
    mesh reader fail for the length of the test"""
    import sys
    import waiwera_amd

    def boom(*a, **k):
        raise AssertionError("a file was read before the input's keys were checked")
    for mod in ("lib", "flow_simulation"):
        monkeypatch.setitem(sys.modules, "waiwera_amd." + mod, None)      # importing it raises ImportError
        monkeypatch.delattr(waiwera_amd, mod, raising=False)
    monkeypatch.setattr(S.gmsh, "read_msh", boom)


@pytest.mark.parametrize("path", sorted(S.REFUSED_KEYS))
def test_refused_key_is_named_before_the_library_is_loaded(path, no_library):
    first = path.split(".")[0]
    parents = [k for k in S.REFUSED_KEYS if path.startswith(k + ".")]
    with pytest.raises(NotImplementedError) as e:
        S.Simulation(minimal_input(path), base_dir=INPUTS)
    # the message names the key refused first on the way down: the path itself, or the refused object that holds it
    assert any(k in str(e.value) for k in [path] + parents), str(e.value)
    assert first in str(e.value)


def test_unknown_key_is_named_with_its_place(no_library):
    inp = {"source": [{"cell": 0, "rate": 1.0}, {"cell": 1, "rat": 2.0}]}
    with pytest.raises(NotImplementedError, match=r"source\[1\]\.rat"):
        S.Simulation(inp, base_dir=INPUTS)
    with pytest.raises(NotImplementedError, match=r"source\[0\]\.cells \(source\.cells\)"):
        S.Simulation({"source": [{"cells": [0, 1]}]}, base_dir=INPUTS)
    # a key given as null is absent; user-chosen names pass
    S.check_input_keys({"mesh": {"filename": "a.msh", "zones": {"any name": {"x": [0, 1]}}, "rebalance": None},
                        "output": {"jacobian": None}, "title": "t"})


@pytest.mark.parametrize("name", sorted(os.path.basename(p) for p in glob.glob(os.path.join(INPUTS, "*.json"))))
def test_golden_inputs_pass_the_walk(name):
    with open(os.path.join(INPUTS, name)) as f:
        S.check_input_keys(json.load(f))


# ---- permeability axes ------------------------------------------------------------------------------------------------------
def test_direction_of_a_normal_as_the_reference_pins_it():
    """face_test.F90:165-221: three normals under the identity rotation -> axes 1, 2, 3"""
    for normal, want in (([1.0, -0.25, 0.3], 1), ([-0.1, 2.1, 0.5], 2), ([1.0, -1.4, -1.6], 3)):
        assert unstructured.permeability_direction(np.array(normal), 3, 0.0) == want


def write_2x2(path, dx=10.0, dy=10.0, dz=5.0):
    """a 2 x 2 x 1 mesh of hexahedra as gmsh MSH 2.2 ASCII; cell i + 2 j.  Interior faces: (0, 1), (2, 3) normal x;
    (0, 2), (1, 3) normal y"""
    node = lambda i, j, k: 1 + i + 3 * j + 9 * k      # noqa: E731
    lines = ["$MeshFormat", "2.2 0 8", "$EndMeshFormat", "$Nodes", "18"]
    for k in range(2):
        for j in range(3):
            for i in range(3):
                lines.append("%d %r %r %r" % (node(i, j, k), i * dx, j * dy, k * dz))
    lines += ["$EndNodes", "$Elements", "4"]
    for j in range(2):
        for i in range(2):
            ring = [(i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1)]
            nodes = [node(a, b, 0) for a, b in ring] + [node(a, b, 1) for a, b in ring]
            lines.append("%d 5 2 1 1 %s" % (1 + i + 2 * j, " ".join(map(str, nodes))))
    lines += ["$EndElements", ""]
    with open(path, "w") as f:
        f.write("\n".join(lines))
    return path


X_FACES, Y_FACES = [(0, 1), (2, 3)], [(0, 2), (1, 3)]
# d = R n, R = [[c, s], [-s, c]] (rotation_matrix_2d, src/utils.F90:207-220): an x normal reads (c, -s), a y normal (s, c)
ANGLES = {0.0: (1, 2), 30.0: (1, 2), 44.9: (1, 2), 45.1: (2, 1), 90.0: (2, 1)}


def directions(lm, gid=None):
    """{(cell, cell) in the input's numbering, smaller first: direction} of a mesh's interior faces"""
    fc = np.asarray(lm.face_cells).reshape(-1, 2)
    n = lm.n_owned + lm.n_halo
    out = {}
    for (a, b), rec in zip(fc, np.asarray(lm.face_geom).reshape(-1, 12)):
        if a < n and b < n:
            a, b = (int(a), int(b)) if gid is None else (int(gid[a]), int(gid[b]))
            out[(min(a, b), max(a, b))] = int(rec[11])
    return out


def base_input(**mesh):
    return {"mesh": dict({"filename": "m.msh"}, **mesh), "eos": {"name": "we"}, "gravity": [0.0, 0.0, 0.0],
            "initial": {"primary": [2.0e5, 20.0], "region": 1},
            "rock": {"types": [{"name": "r", "permeability": [1.0e-13, 1.0e-15, 1.0e-14], "cells": [0, 1, 2, 3]}]},
            "time": {"stop": 1.0, "step": {"size": 1.0}}}


def sim_of(tmp_path, inp, **kw):
    write_2x2(str(tmp_path / "m.msh"))
    return S.Simulation(copy.deepcopy(inp), base_dir=str(tmp_path), ode_factory=RecordingOde, **kw)


@pytest.mark.parametrize("angle", sorted(ANGLES))
def test_permeability_angle_turns_the_axes_before_the_argmax(tmp_path, angle):
    sim = sim_of(tmp_path, base_input(permeability_angle=angle))
    got = directions(sim.mesh)
    want_x, want_y = ANGLES[angle]
    assert got == dict([(f, want_x) for f in X_FACES] + [(f, want_y) for f in Y_FACES])


def test_an_input_without_the_keys_reads_the_bare_normal(tmp_path):
    got = directions(sim_of(tmp_path, base_input()).mesh)
    assert got == {(0, 1): 1, (2, 3): 1, (0, 2): 2, (1, 3): 2}


OVERRIDES = [{"cells": [2, 0], "permeability_direction": 1},      # a y face, named with the larger cell first (mesh_test.F90:474-546)
             {"cells": [2, 3], "permeability_direction": 3},
             {"cells": [0, 3], "permeability_direction": 3},      # no face between them: passed over, as the reference does
             {"cells": [1, 3]}]                                   # the key's default is 1 (mesh.F90:1292)
WITH_OVERRIDES = {(0, 1): 2, (2, 3): 3, (0, 2): 1, (1, 3): 1}    # at 90 degrees the x face (0, 1) reads 2


def test_listed_faces_take_their_direction_in_either_cell_order(tmp_path):
    sim = sim_of(tmp_path, base_input(permeability_angle=90.0, faces=OVERRIDES))
    assert directions(sim.mesh) == WITH_OVERRIDES
    swapped = [dict(f, cells=f["cells"][::-1]) for f in OVERRIDES]
    assert directions(sim_of(tmp_path, base_input(permeability_angle=90.0, faces=swapped)).mesh) == WITH_OVERRIDES
    with pytest.raises(ValueError, match="permeability_direction"):
        sim_of(tmp_path, base_input(faces=[{"cells": [0, 1], "permeability_direction": 4}]))


def test_listed_faces_under_the_compact_cell_order(tmp_path):
    """the cell pairs go through the inverse permutation like every other cell number"""
    sim = sim_of(tmp_path, base_input(permeability_angle=90.0, faces=OVERRIDES), cell_order="compact", subdomain_rows=2)
    assert sim.cell_order_choice.order == "compact" and sorted(sim._perm) == [0, 1, 2, 3]
    assert directions(sim.mesh, gid=sim._perm) == WITH_OVERRIDES
    # and a permutation that is certainly not the identity, through the same two steps the front end takes
    perm = np.array([3, 1, 0, 2])
    inv = np.empty(4, dtype=np.int64)
    inv[perm] = np.arange(4)
    ren = S.renumber_input(base_input(faces=OVERRIDES), perm, inv)
    assert [f["cells"] for f in ren["mesh"]["faces"]] == [[int(inv[a]), int(inv[b])] for a, b in (f["cells"] for f in OVERRIDES)]
    from waiwera_amd import gmsh
    nodes, cells, dim = gmsh.read_msh(write_2x2(str(tmp_path / "p.msh")))
    lm = unstructured.build_mesh(nodes, [cells[p] for p in perm], dim, permeability_angle=90.0,
                                 face_directions=[(f["cells"][0], f["cells"][1], f.get("permeability_direction", 1))
                                                  for f in ren["mesh"]["faces"]])
    assert directions(lm, gid=perm) == WITH_OVERRIDES


@pytest.mark.parametrize("owner", [[0, 0, 1, 1], [0, 1, 1, 0]])
def test_listed_faces_on_two_ranks(tmp_path, owner):
    """every rank builds the whole mesh, then keeps its cells and a ghost layer: each face it holds carries the direction"""
    seen = {}
    for rank in range(2):
        sim = sim_of(tmp_path, base_input(permeability_angle=90.0, faces=OVERRIDES), rank=rank, world=2, comm_id=b"id",
                     owner=np.array(owner))
        got = directions(sim.mesh, gid=sim._gid)
        assert got and all(WITH_OVERRIDES[f] == d for f, d in got.items())
        seen.update(got)
    assert seen == WITH_OVERRIDES
    # the partitioner alone, on the one-rank mesh
    whole = sim_of(tmp_path, base_input(permeability_angle=90.0, faces=OVERRIDES)).mesh
    for rank in range(2):
        lm, gid = partition_mesh(whole, np.array(owner), rank, world=2)
        assert all(WITH_OVERRIDES[f] == d for f, d in directions(lm, gid=gid).items())


def test_mesh_builder_cannot_honour_the_keys(tmp_path):
    def builder(bnds, srcs):
        raise AssertionError("not reached")
    builder.dim, builder.n_cells = 3, 4
    with pytest.raises(NotImplementedError, match="mesh.permeability_angle"):
        sim_of(tmp_path, base_input(permeability_angle=30.0), mesh_builder=builder)


# ---- thermodynamics.extrapolate and source.production_component, as read ---------------------------------------------------------
def test_extrapolate_reaches_the_flow_object(tmp_path):
    for th, want in (("iapws", False), ({"name": "ifc67"}, False), ({"name": "iapws", "extrapolate": True}, True),
                     ({"extrapolate": False}, False)):
        RecordingOde.made.clear()
        sim = sim_of(tmp_path, dict(base_input(), thermodynamics=th))
        assert sim.thermo_extrapolate is want
    # the stub's constructor got the argument (the boundary fluid is evaluated when the object is made)
    seen = {}

    def factory(lm, eos, thermo, relperm, capillary, temperature, **kw):
        seen.update(kw)
        return RecordingOde(lm, eos)
    write_2x2(str(tmp_path / "m.msh"))
    S.Simulation(dict(base_input(), thermodynamics={"name": "ifc67", "extrapolate": True}), base_dir=str(tmp_path), ode_factory=factory)
    assert seen.get("thermo_extrapolate") is True
    seen.clear()
    S.Simulation(base_input(), base_dir=str(tmp_path), ode_factory=factory)
    assert "thermo_extrapolate" not in seen


def test_component_names_as_the_reference_pins_them():
    with open(os.path.join(HERE, "golden", "source_production_components.json")) as f:
        g = json.load(f)
    inp = {"source": [c["source"] for c in g["cases"]]}
    got = S.production_components(inp, g["eos"])
    assert got == [c["production_component"] for c in g["cases"]]
    assert [S.component_index(c["source"].get("component", 0), g["eos"]) for c in g["cases"]] == [c["component"] for c in g["cases"]]
    assert S.component_index("energy", "we") == 2 and S.component_index("Energy", "wsce") == 4 and S.component_index("salt", "wse") == 2
    with pytest.raises(ValueError, match="production_component"):
        S.production_components({"source": [{"cell": 0, "production_component": "gas"}]}, "we")
    with pytest.raises(ValueError, match="production_component"):
        S.production_components({"source": [{"cell": 0, "production_component": 3}]}, "we")


def test_production_components_reach_the_flow_object_per_rank(tmp_path):
    src = [{"cell": 3, "rate": -1.0, "production_component": "energy"}, {"cell": 0, "rate": -2.0},
           {"cell": 2, "rate": -1.0, "production_component": 1}]
    RecordingOde.made.clear()
    sim = sim_of(tmp_path, dict(base_input(), source=src))
    assert [c[1][0] for c in sim.ode.named("set_source_production_component")] == [[2, 0, 1]]
    sim = sim_of(tmp_path, dict(base_input(), source=[src[1]]))
    assert not sim.ode.named("set_source_production_component")      # no key: the call is not made
    given = [2, 0, 1]
    sim = sim_of(tmp_path, dict(base_input(), source=src), rank=0, world=2, comm_id=b"id", owner=np.array([0, 0, 1, 1]))
    # (whether the call is made is decided on the whole input, so on every rank alike; it carries the rank's own sources)
    assert list(sim.owned_source) == [1] and [list(c[1][0]) for c in sim.ode.named("set_source_production_component")] == [[0]]
    sim = sim_of(tmp_path, dict(base_input(), source=src), rank=1, world=2, comm_id=b"id", owner=np.array([0, 0, 1, 1]))
    assert sorted(sim.owned_source) == [0, 2]
    assert [list(c[1][0]) for c in sim.ode.named("set_source_production_component")] == [[given[i] for i in sim.owned_source]]


@pytest.mark.parametrize("extra, met", [({"separator": {"pressure": 5.0e5}}, "separator"),
                                        ({"limiter": {"type": "steam", "limit": 1.0, "separator_pressure": 5.0e5}}, "limiter"),
                                        ({"limiter": {"water": 1.0}}, "limiter"), ({"name": "w1"}, "network")])
def test_production_component_refusals_by_name(extra, met, no_library):
    inp = {"source": [dict({"cell": 0, "rate": -1.0, "production_component": 2}, **extra)],
           "network": {"group": [{"name": "g", "in": ["w1"]}]}}
    with pytest.raises(NotImplementedError, match=r"source\[0\]\.production_component together with .*" + met):
        S.production_components(inp, "we")
    # the same source without the key, and with what combines: deliverability, a limiter on the total flow, direction
    S.production_components({"source": [dict({"cell": 0, "rate": -1.0}, **extra)], "network": inp["network"]}, "we")
    assert S.production_components({"source": [{"cell": 0, "production_component": 2, "deliverability": {"productivity": 1e-12},
                                                "limiter": {"total": 2.0}, "direction": "production", "factor": 0.5}]}, "we") == [2]

"""The compact cell order (cell_order="compact", wai_cell_order) at every layer a host reaches it through without a device:
the C header, the Fortran module, the ctypes binding, Simulation's keywords and the command line; and what the input front
end hands the flow object -- with the recording stub of tests/test_input_partition.py in its place -- for a scrambled
gmsh file under "compact" against the same mesh written in the compact order under "input"."""
import copy
import inspect
import io
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import cell_order_cases as cc
from tests.test_input_partition import RecordingOde, _load, _sim
from waiwera_amd.simulation import Simulation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS, ROWS = (8, 6, 5), 30      # 240 cells, eight leaves of exactly 30: the chunks of 30 of the file written in compact order


def test_entry_point_at_every_layer():
    hdr = open(os.path.join(ROOT, "include", "waiwera_hip.h")).read()
    assert re.search(r"int\s+wai_cell_order\s*\(\s*int\s+n_cells\s*,\s*int\s+n_faces\s*,\s*const\s+int\s*\*\s*face_cells\s*,", hdr)
    f90 = open(os.path.join(ROOT, "waiwera_amd", "fortran", "waiwera_hip_module.F90")).read()
    assert 'bind(c, name = "wai_cell_order")' in f90
    from waiwera_amd import lib
    assert "wai_cell_order" in lib.EXPORTED
    p = inspect.signature(Simulation.__init__).parameters
    assert p["cell_order"].default == "input" and p["subdomain_rows"].default is None
    from waiwera_amd import run
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        run.main(["--help"])
    assert "--cell-order" in buf.getvalue() and "--subdomain-rows" in buf.getvalue()


def test_the_binding_refuses_null_pointers_and_reports_the_text():
    from waiwera_amd import lib
    cen, faces = cc.hex_grid(3, 2, 2)
    n = len(cen)
    fc = np.ascontiguousarray(faces, dtype=np.int32)
    perm, sub, ns = np.zeros(n, dtype=np.int32), np.zeros(n + 1, dtype=np.int32), C.c_int(0)
    P = lambda a: a.ctypes.data_as(lib.pi if a.dtype == np.int32 else lib.pd)      # noqa: E731
    err = C.create_string_buffer(128)
    full = [n, len(fc), P(fc), P(cen), 3, 4, P(perm), C.byref(ns), P(sub), err, len(err)]
    assert lib.LIB.wai_cell_order(*full) == 0 and ns.value == 3 and err.value == b""
    for k in (2, 3, 6, 7, 8):
        args = list(full)
        args[k] = None
        assert lib.LIB.wai_cell_order(*args) == -2, k
        assert b"null argument" in err.value
    args = list(full)
    args[9], args[10] = None, 0        # no room for a text: still refused, nothing written
    args[5] = 0
    assert lib.LIB.wai_cell_order(*args) == -2
    tiny = C.create_string_buffer(8)
    args[9], args[10] = tiny, len(tiny)
    assert lib.LIB.wai_cell_order(*args) == -2 and tiny.value == b"cell or"      # cut to fit, terminated
    # the wrapper: the same as the definition, and the library's text in the exception
    got = lib.cell_order(faces, cen, 4)
    want = cc.compact_order(cen, faces, 4)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    with pytest.raises(lib.WaiError, match="cap must be at least 1"):
        lib.cell_order(faces, cen, 0)
    with pytest.raises(lib.WaiError, match=r"outside \[0, n\)"):
        lib.cell_order(faces + 1, cen, 4)
    bad = cen.copy()
    bad[1, 2] = np.nan
    with pytest.raises(lib.WaiError, match="not finite"):
        lib.cell_order(faces, bad, 4)
    # cell_geom's own stride
    wide = np.concatenate([cen, np.ones((n, 1))], axis=1)
    assert np.array_equal(lib.cell_order(faces, wide, 4)[0], want[0])


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the grid as a scrambled file and as the file written in the compact order of the scrambled one, each with its input"""
    d = tmp_path_factory.mktemp("cell_order_frontend")
    n = int(np.prod(DIMS))
    p = np.random.default_rng(4).permutation(n)      # element k of the scrambled file is x-fastest cell p[k]
    number = np.empty(n, dtype=np.int64)
    number[p] = np.arange(n)
    cc.write_msh(d / "scrambled.msh", *DIMS, order=p)
    scr = cc.layered_input(*DIMS, "scrambled.msh", number)
    RecordingOde.made.clear()
    s = Simulation(copy.deepcopy(scr), base_dir=str(d), ode_factory=RecordingOde, cell_order="compact", subdomain_rows=ROWS)
    (ode,) = RecordingOde.made
    q = p[s._perm]                                    # the compact order in x-fastest numbers
    number2 = np.empty(n, dtype=np.int64)
    number2[q] = np.arange(n)
    cc.write_msh(d / "ordered.msh", *DIMS, order=q)
    return dict(dir=str(d), scrambled=scr, ordered=cc.layered_input(*DIMS, "ordered.msh", number2), sim=s, ode=ode, p=p)


def _handed_over(sim, ode):
    lm = ode.mesh
    out = {k: np.asarray(getattr(lm, k)).copy() for k in
           "face_cells face_geom cell_geom rock src_cell src_rate src_enthalpy src_component bc_primary bc_region sub_ptr".split()}
    out.update(primary=np.asarray(sim.primary).copy(), region=np.asarray(sim.region).copy(), y=np.asarray(sim.y).copy())
    out["set_regions"] = np.asarray(ode.named("set_regions")[0][1][0]).copy()
    return out


def test_a_scrambled_file_in_compact_order_hands_over_the_mesh_of_the_ordered_file(files):
    a = _handed_over(files["sim"], files["ode"])
    RecordingOde.made.clear()
    s = Simulation(copy.deepcopy(files["ordered"]), base_dir=files["dir"], ode_factory=RecordingOde, subdomain_rows=ROWS)
    (ode,) = RecordingOde.made
    b = _handed_over(s, ode)
    assert np.array_equal(b["sub_ptr"], np.arange(0, 241, ROWS))
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    # ... and the ordered file's own compact order is the identity
    RecordingOde.made.clear()
    t = Simulation(copy.deepcopy(files["ordered"]), base_dir=files["dir"], ode_factory=RecordingOde, cell_order="compact", subdomain_rows=ROWS)
    assert np.array_equal(t._perm, np.arange(240))
    c = _handed_over(t, RecordingOde.made[0])
    for k in a:
        assert np.array_equal(a[k], c[k]), k
    # the record
    ch = files["sim"].cell_order_choice
    assert (ch.order, ch.n_sub, ch.largest_subdomain) == ("compact", 8, 30) and ch.cut_after < 0.5 * ch.cut_before
    assert ch.cut_after == s.cell_order_choice.cut_before == s.cell_order_choice.cut_after and s.cell_order_choice.order == "input"
    assert np.array_equal(files["sim"].owned_gid, np.arange(240))


def test_results_come_back_in_the_input_numbering(files):
    """the maps fields() takes cells and faces back by, on what the stub has: the geometry is the input-order mesh's, cell for
    cell (to rounding: a face's area and centroid are summed from the cell that names it first), and so are rock and state"""
    RecordingOde.made.clear()
    plain = Simulation(copy.deepcopy(files["scrambled"]), base_dir=files["dir"], ode_factory=RecordingOde)
    s = files["sim"]
    assert np.allclose(s.mesh.cell_geom[:240][s._inv], plain.mesh.cell_geom[:240], rtol=1e-13, atol=0)
    assert np.array_equal(s.mesh.rock[:240][s._inv], plain.mesh.rock[:240])
    assert np.array_equal(s.primary[s._inv], plain.primary) and np.array_equal(s._perm[s.mesh.src_cell], plain.mesh.src_cell)
    # the faces: each one's place and orientation in the input-order mesh
    old = np.asarray(s.mesh.face_cells, dtype=np.int64).copy()
    own = old < 240
    old[own] = s._perm[old[own]]
    back = np.empty_like(old)
    back[s._face_place] = np.where(s._face_flip[:, None], old[:, ::-1], old)
    assert np.array_equal(back, plain.mesh.face_cells)


def test_without_the_keywords_nothing_changes(files):
    """the default hands the library byte-identical arrays: subdomain_rows=None and cell_order="input" are today's path,
    pinned on problem 5a against the arrays build_mesh makes when called as before"""
    from waiwera_amd import gmsh, unstructured
    inp = _load("problem5a.json")
    RecordingOde.made.clear()
    a = _sim(inp)
    (ode,) = RecordingOde.made
    RecordingOde.made.clear()
    b = _sim(inp, cell_order="input", subdomain_rows=None)
    mesh = inp["mesh"] if isinstance(inp["mesh"], dict) else {"filename": inp["mesh"]}
    nodes, cells, dim = gmsh.read_msh(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inputs", mesh["filename"]))
    ref = unstructured.build_mesh(nodes, cells, dim, thickness=mesh.get("thickness", 1.0), radial=bool(mesh.get("radial", False)))
    for k in "face_cells face_geom cell_geom rock sub_ptr bc_primary bc_region src_cell".split():
        x, y = (np.asarray(getattr(m, k)) for m in (ode.mesh, RecordingOde.made[0].mesh))
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), k
    assert a.y.tobytes() == b.y.tobytes()
    # (ref has no boundaries: its faces are the interior ones, which come first)
    n, m = ref.n_owned, ref.n_faces
    assert np.asarray(ode.mesh.cell_geom)[:n].tobytes() == np.asarray(ref.cell_geom)[:n].tobytes()
    assert np.asarray(ode.mesh.face_cells)[:m].tobytes() == np.asarray(ref.face_cells).tobytes()
    assert np.asarray(ode.mesh.face_geom)[:m, :7].tobytes() == np.asarray(ref.face_geom)[:, :7].tobytes()
    assert np.asarray(ode.mesh.sub_ptr).tobytes() == np.asarray(ref.sub_ptr).tobytes()
    assert a.cell_order_choice.order == "input" and a.cell_order_choice.n_sub == len(ode.mesh.sub_ptr) - 1
    # the cap under the input order
    RecordingOde.made.clear()
    c = _sim(inp, subdomain_rows=7)
    assert np.array_equal(c.mesh.sub_ptr, np.append(np.arange(0, c.mesh.n_owned, 7), c.mesh.n_owned))


def test_refusals_before_the_flow_object_exists(files):
    inp = _load("problem5a.json")
    RecordingOde.made.clear()
    with pytest.raises(ValueError, match="cell_order 'input'"):
        _sim(inp, cell_order="bricks")
    for rows in (0, 1025, 2.5, "64", True):
        with pytest.raises(ValueError, match="subdomain_rows"):
            _sim(inp, subdomain_rows=rows)
    for rank in range(2):
        with pytest.raises(ValueError, match=r"cell_order 'compact' .* world = 2 ranks"):
            _sim(inp, rank, 2, cell_order="compact")
    with pytest.raises(ValueError, match=r"cell_order 'compact' .* MINC zones"):
        _sim(_load("minc_column_minc.json"), mesh="gminc_column.dat", cell_order="compact")

    def builder(bnds, srcs):
        raise AssertionError("the mesh builder was called")
    builder.dim, builder.n_cells = 3, 10
    with pytest.raises(ValueError, match=r"cell_order 'compact' .* a mesh_builder"):
        Simulation(copy.deepcopy(inp), ode_factory=RecordingOde, mesh_builder=builder, cell_order="compact")
    assert not RecordingOde.made

"""cell_order="compact" on the device (waiwera_amd/simulation.py, wai_cell_order): the same equations in another numbering
with other preconditioner blocks, so a compact-order run must give the input-order run's results -- in the input's
numbering -- and need fewer Krylov iterations where the input's chunks cut the strong vertical couplings of thin layers.

The mesh: 16 x 12 x 10 hexahedra of 100 x 100 x 20 m, written as gmsh 2.2 ASCII in file order (x fastest) and scrambled,
eos we, gravity on, subdomain_rows=256, default_pc="bjacobi".  Bounds, none of them measured here:
  residual at the initial state  1e-11 of its largest entry: the device-against-oracle rhs bound of tests/test_hip_parity.py
                                 -- only the order of a cell's face sums differs;
  one time step, whole inputs    1e-4 of a field's largest magnitude: the bound of the two-ranks-against-one-rank input tests
                                 (tests/test_hip_input_multirank_features.py) -- both runs stop Newton at the input's function
                                 tolerance with different preconditioner blocks.  The same bound for subdomains="rank" against
                                 "chunks" under "compact": the tile tests (tests/test_hip_pc_tiles.py) compare whole steps
                                 bit for bit, but between two paths through ONE preconditioner; one block per rank against
                                 one block per leaf are two preconditioners, which is the two-ranks-against-one situation.
Every Simulation of the layered mesh is made once (module scope) and shared."""
import copy
import json
import os

import numpy as np
import pytest

from tests import cell_order_cases as cc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
DIMS, ROWS, TOL = (16, 12, 10), 256, 1.0e-4
N = int(np.prod(DIMS))


def _close(name, got, want, tol=TOL):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    sc = max(np.abs(want).max(), 1e-300) if want.size else 1.0
    err = np.abs(got - want).max() / sc if want.size else 0.0
    print("  %-40s %.2e of its largest magnitude %.4g" % (name, err, sc))
    assert err <= tol, (name, err)


class Layered:
    """the layered mesh's files and inputs; run(file, order, ...) -> what one Simulation gave: the residual terms at the
    initial state and the fields, Krylov count and kernel of one time step (made once per key)"""

    def __init__(self, d):
        self.dir = str(d)
        self.p = np.random.default_rng(7).permutation(N)      # element k of the scrambled file is x-fastest cell p[k]
        number = np.empty(N, dtype=np.int64)
        number[self.p] = np.arange(N)
        self.number = {"file": None, "scrambled": number}
        cc.write_msh(d / "file.msh", *DIMS)
        cc.write_msh(d / "scrambled.msh", *DIMS, order=self.p)
        self.memo = {}

    def run(self, file, order, eos="we", rows=ROWS, subdomains="chunks"):
        key = (file, order, eos, rows, subdomains)
        if key in self.memo:
            return self.memo[key]
        from waiwera_amd.simulation import Simulation
        inp = cc.layered_input(*DIMS, file + ".msh", self.number[file], eos=eos)
        inp["output"] = {"initial": False, "final": True, "frequency": 0, "fields": {"flux": "all"}}
        sim = Simulation(inp, base_dir=self.dir, default_pc="bjacobi", cell_order=order, subdomain_rows=rows, subdomains=subdomains)
        n, bs = sim.mesh.n_owned, sim.y.size // sim.mesh.n_owned
        back = sim._inv if sim._inv is not None else np.arange(n)
        L, R = np.zeros(n * bs), np.zeros(n * bs)
        assert sim.ode.pre_eval(0.0, sim.y) == 0
        sim.ode.lhs(0.0, (0.0, 0.0), sim.y, L)
        sim.ode.rhs(0.0, (0.0, 0.0), sim.y, R)
        out = sim.run()
        res = dict(lhs=L.reshape(n, bs)[back], rhs=R.reshape(n, bs)[back], fields=out, history=list(sim.ts.history),
                   krylov=sum(h[3] for h in sim.ts.history), taken=sim.ts.taken, kernel=sim.ode.pc_kernel_name(),
                   choice=sim.cell_order_choice, owned_gid=np.asarray(sim.owned_gid).copy(), sub_ptr=None if sim.mesh.sub_ptr is None
                   else np.asarray(sim.mesh.sub_ptr).copy())
        sim.ode.destroy()
        self.memo[key] = res
        return res


@pytest.fixture(scope="module")
def layered(tmp_path_factory):
    return Layered(tmp_path_factory.mktemp("cell_order_layered"))


@pytest.mark.parametrize("file", ["file", "scrambled"])
def test_residual_at_the_initial_state(layered, file):
    a, b = layered.run(file, "input"), layered.run(file, "compact")
    assert b["choice"].order == "compact" and b["choice"].n_sub == 8 and b["choice"].largest_subdomain <= ROWS
    assert np.array_equal(b["owned_gid"], np.arange(N))
    assert np.abs(a["rhs"]).max() > 0.0
    for k in ("lhs", "rhs"):
        err = np.abs(b[k] - a[k]).max() / np.abs(a[k]).max()
        print("%s %s: %.2e of the largest entry" % (file, k, err))
        assert err <= 1e-11, (k, err)


@pytest.mark.parametrize("file", ["file", "scrambled"])
def test_one_time_step(layered, file):
    a, b = layered.run(file, "input"), layered.run(file, "compact")
    assert a["taken"] == b["taken"] == 1
    fa, fb = a["fields"], b["fields"]
    assert fa.keys() == fb.keys() and fa["time"] == fb["time"]
    assert np.array_equal(fa["fluid_region"], fb["fluid_region"])
    assert np.array_equal(fa["face_cell_1"], fb["face_cell_1"]) and np.array_equal(fa["face_cell_2"], fb["face_cell_2"])
    assert any(k.startswith("flux_") for k in fa) and np.abs(fa["flux_water"]).max() > 0.0
    for k in fa:
        if k != "time":
            _close(file + " " + k, fb[k], fa[k])


def test_krylov_iterations(layered):
    """fewer Krylov iterations in the step under "compact" than under "input", for both numberings of the file"""
    counts = {(f, o): layered.run(f, o)["krylov"] for f in ("file", "scrambled") for o in ("input", "compact")}
    for (f, o), k in sorted(counts.items()):
        r = layered.run(f, o)
        print("%-9s %-7s krylov %4d history %s kernel %s cut %.3f -> %.3f" % (f, o, k, r["history"], r["kernel"], r["choice"].cut_before, r["choice"].cut_after))
    for f in ("file", "scrambled"):
        assert counts[(f, "compact")] < counts[(f, "input")], counts


def test_kernel_selection(layered):
    """3 x 3 blocks (eos wce), scrambled, subdomains of at most 64 cells: the kernel of the structured generator's bricks"""
    from waiwera_amd.cases import make_case, scaled
    from waiwera_amd.flow_simulation import FlowSimulation
    g, lm, prim, region = make_case(dims=DIMS, brick=(4, 4, 4), eos="wce")
    assert np.diff(lm.sub_ptr).max() <= 64
    sim = FlowSimulation(lm, eos="wce")
    sim.set_regions(region)
    y = scaled(prim, region, "wce").ravel().copy()
    dt = 1.0e4
    for _ in range(5):
        reason, nits, kits = sim.timestep(0.0, dt, y)
        if reason > 0:
            break
        dt *= 0.2
    assert reason > 0
    bricks = sim.pc_kernel_name()
    sim.destroy()
    b = layered.run("scrambled", "compact", eos="wce", rows=64)
    a = layered.run("scrambled", "input", eos="wce", rows=64)
    print("bricks: %s\ncompact: %s (krylov %d)\ninput: %s (krylov %d)" % (bricks, b["kernel"], b["krylov"], a["kernel"], a["krylov"]))
    assert b["taken"] == 1 and np.diff(b["sub_ptr"]).max() <= 64
    assert b["kernel"] == bricks


def test_one_block_per_rank_with_the_leaves_as_tiles(layered):
    a = layered.run("scrambled", "compact")
    b = layered.run("scrambled", "compact", subdomains="rank")
    print("chunks: %s krylov %d; rank: %s krylov %d" % (a["kernel"], a["krylov"], b["kernel"], b["krylov"]))
    assert b["sub_ptr"] is None and b["taken"] == 1
    for k in a["fields"]:
        if k != "time":
            _close(k, b["fields"][k], a["fields"][k])


def _input(name):
    inp = json.load(open(os.path.join(INPUTS, name + ".json")))
    inp["time"]["step"].setdefault("maximum", {})["number"] = 5
    out = dict(inp.get("output") or {}, filename=name + ".h5")
    out["fields"] = dict(out.get("fields") or {}, flux="all")
    inp["output"] = out
    return inp


@pytest.mark.parametrize("name,rows,mesh_file", [("problem5a", 20, None), ("reinjection", 3, "greinjection.dat"), ("doublet", 30, None)])
def test_whole_inputs(tmp_path, name, rows, mesh_file):
    """problem 5a (sources, boundaries, per-cell initial conditions, rock by cells), the reinjection column (MULgraph geometry,
    a source network) and the tracer doublet (a restart file), five steps each: every cell, source, network and face field
    of the compact-order run against the default run's, and the HDF5 files' /cell_index and dataset shapes"""
    from waiwera_amd import hdf5io
    from waiwera_amd.simulation import Simulation
    res = {}
    for order in ("input", "compact"):
        kw = dict(cell_order="compact", subdomain_rows=rows) if order == "compact" else {}
        if mesh_file:
            kw["mesh_file"] = os.path.join(INPUTS, mesh_file)
        d = tmp_path / order
        d.mkdir()
        sim = Simulation(copy.deepcopy(_input(name)), base_dir=INPUTS, output_dir=str(d), **kw)
        out = sim.run()
        assert sim.output_error is None and sim.ts.taken == 5
        res[order] = dict(fields=out, data=sim.datasets(), choice=sim.cell_order_choice, krylov=sum(h[3] for h in sim.ts.history),
                          file=str(d / (name + ".h5")), gid=np.asarray(sim.owned_gid).copy())
        sim.ode.destroy()
    a, b = res["input"], res["compact"]
    print("%s: %d leaves, largest %d, cut %.3f -> %.3f; krylov %d -> %d" % (name, b["choice"].n_sub, b["choice"].largest_subdomain,
                                                                          b["choice"].cut_before, b["choice"].cut_after, a["krylov"], b["krylov"]))
    assert b["choice"].n_sub >= 3 and b["choice"].largest_subdomain <= rows and np.array_equal(a["gid"], b["gid"])
    fa, fb = a["fields"], b["fields"]
    assert list(fa.keys()) == list(fb.keys())
    assert np.array_equal(fa["fluid_region"], fb["fluid_region"])
    assert np.array_equal(fa["face_cell_1"], fb["face_cell_1"]) and np.array_equal(fa["face_cell_2"], fb["face_cell_2"])
    if name == "reinjection":
        assert any(k.startswith("network_") for k in fa)
    if name == "doublet":
        assert fa["tracer_tracer1"].max() > 1e-6
    for k in fa:
        if k != "time":
            _close(k, fb[k], fa[k])
    # the output: the same datasets of the same shapes, every snapshot within the bound, the file's cell index the input's
    assert a["data"].keys() == b["data"].keys()
    for k in a["data"]:
        assert a["data"][k].shape == b["data"][k].shape, k
        if k not in ("/time", "/cell_index") and a["data"][k].dtype.kind == "f":
            _close(k, b["data"][k], a["data"][k])
    for k in ("/cell_index", "/face_cell_1", "/face_cell_2"):
        x, y = hdf5io.read_dataset(a["file"], k), hdf5io.read_dataset(b["file"], k)
        assert x.shape == y.shape and np.array_equal(x, y), k
    n = fa["fluid_pressure"].size
    assert np.array_equal(hdf5io.read_dataset(b["file"], "/cell_index").ravel(), np.arange(n))
    for k in ("/cell_fields/fluid_pressure", "/time"):
        assert hdf5io.read_dataset(a["file"], k).shape == hdf5io.read_dataset(b["file"], k).shape

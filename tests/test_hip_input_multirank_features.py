"""Input files with tracers, MINC zones, rock table controls and source networks on two ranks against the one-rank run of
the same input (waiwera_amd/simulation.py).  Like every multi-rank test here the ranks share ONE GPU
over the loop-back transport of tests/loopback_rccl: what is checked is the front end's per-rank wiring and that no rank
leaves a collective call out -- that would end a case at its queue timeout -- not RCCL between real devices.

Inputs are the reference's own (tests/golden/inputs), cut to a handful of time steps.  Each case: the same number of accepted
steps as on one rank, every cell of the input owned once, equal regions, and fields within 1e-4 of the field's largest
magnitude -- the bound of tests/test_hip_multirank.py::_two_ranks_against_one: both runs stop Newton at 1e-5 (the inputs'
own function tolerance, or the default where an input names none) with different preconditioner subdomains.  The same bound
holds for tracer mass fractions, source rates and enthalpies and the network's nodes: none of these inputs loosens the
linear or auxiliary tolerance beyond 1e-5 (no input names one; the library's default and the reference's auxiliary default
are both 1e-5), so no wider, measured bound is taken anywhere.  Each case prints its figures; measured on an MI355X
the worst were 2.5e-7 (vapour saturation, rock table case), 1.4e-7 (MINC), 4.5e-9 (source and network fields) and 5e-22
(tracers: the doublet starts from its steady state, the flow does not move).

Every case here raises NotImplementedError in Simulation.__init__ without the N-rank front end."""
import copy
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

from tests.test_hip_multirank import LOOPBACK, ROOT, _default_overlap, _free_port, _own_cus

pytestmark = pytest.mark.gpu
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
TOL = 1.0e-4
GEOMETRY = ("cell_geometry", "face_", "flux_")


def _fields(sim, out):
    f = {k: np.asarray(v).copy() for k, v in out.items() if not k.startswith(GEOMETRY) and k != "time"}
    ex = sim.mesh.extras
    if sim._order is not None:      # what /minc/level and /minc/parent of an output file hold, in the fields' order
        f["minc_level"], f["minc_parent"] = np.asarray(ex["minc_level"])[sim._order], np.asarray(ex["minc_parent"])[sim._order]
    if sim._rock_controls:
        f["rock_permeability"] = np.asarray(sim.ode.mesh.rock)[: sim.mesh.n_owned, 0].copy()
    return f


def _worker(rank, world, uid_q, q, inp, kw):
    os.environ["WAI_RCCL_LIB"] = LOOPBACK
    _own_cus(rank, world)
    _default_overlap()
    from waiwera_amd import lib as wl
    from waiwera_amd.simulation import Simulation
    if rank == 0:
        uid = wl.comm_unique_id()
        for _ in range(world - 1):
            uid_q.put(uid)
    else:
        uid = uid_q.get(timeout=120)
    sim = Simulation(inp, base_dir=INPUTS, rank=rank, world=world, comm_id=uid, **kw)
    out = sim.run()
    q.put((rank, np.asarray(sim.owned_gid).copy(), np.asarray(sim.owned_source).copy(), _fields(sim, out), sim.ts.taken))
    sim.ode.destroy()


def _close(name, got, want, tol=TOL):
    sc = max(np.abs(want).max(), 1e-300) if want.size else 1.0
    err = np.abs(got - want).max() / sc if want.size else 0.0
    print("  %-40s %.2e of its largest magnitude %.4g" % (name, err, sc))
    assert err <= tol, (name, err)


def _two_ranks_against_one(inp, owner=None, steps=5, **kw):
    """-> (the one-rank fields, [(rank, owned_gid, owned_source, fields)]) after the checks every case makes"""
    from waiwera_amd.simulation import Simulation
    assert os.path.exists(LOOPBACK), "build first: python __graft_entry__.py"
    inp = copy.deepcopy(inp)
    inp["time"]["step"].setdefault("maximum", {})["number"] = steps
    inp["output"] = dict(inp.get("output") or {}, filename=None)
    ser = Simulation(copy.deepcopy(inp), base_dir=INPUTS, **kw)
    one = _fields(ser, ser.run())
    taken = ser.ts.taken
    ser.ode.destroy()
    assert taken == steps
    world = 2
    ctx = mp.get_context("spawn")
    q, uid_q = ctx.Queue(), ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, uid_q, q, inp, dict(kw, owner=owner))) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=240) for _ in range(world)], key=lambda r: r[0])
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.exitcode is None:
                p.kill()
    assert [p.exitcode for p in procs] == [0] * world
    n = one["fluid_pressure"].size
    cells = [k for k in one if one[k].shape[:1] == (n,) and not k.startswith(("source_", "network_"))]
    par = {k: np.full(one[k].shape, np.nan) for k in cells}
    seen = np.zeros(n, dtype=int)
    ns = len(inp.get("source") or [])
    srcs = [k for k in one if k.startswith("source_")]
    spar = {k: np.full(one[k].shape, np.nan) for k in srcs}
    sseen = np.zeros(ns, dtype=int)
    for rank, gid, sid, f, tk in res:
        assert tk == taken, (rank, tk, taken)
        seen[gid] += 1
        sseen[sid] += 1
        for k in cells:
            par[k][gid] = f[k]
        for k in srcs:
            if sid.size:
                spar[k][sid] = f[k]
        for k in one:      # group and reinjector fields: the same on every rank
            if k.startswith("network_"):
                _close("rank %d %s" % (rank, k), f[k], one[k])
                assert np.array_equal(f[k], res[0][3][k])
    assert (seen == 1).all() and (sseen == 1).all()
    assert np.array_equal(par["fluid_region"], one["fluid_region"])
    for k in cells + srcs:
        if k in ("minc_level", "minc_parent"):
            assert np.array_equal(par[k], one[k]), k
        elif k != "fluid_region":
            _close(k, (par if k in par else spar)[k], one[k])
    return one, [r[:4] for r in res]


def _doublet(nt, table=True):
    """the tracer doublet: injector in cell 0, producer on deliverability in cell 99 -- the two ends of the default split"""
    inp = json.load(open(os.path.join(INPUTS, "doublet.json")))
    if nt == 2:
        t = inp["tracer"]
        inp["tracer"] = [t, dict(t, name="tracer2", decay=1.0e-6)]
    if not table:
        # (an injection TABLE with several tracers is refused on any number of ranks: the table's first value, held)
        inp["source"][0]["tracer"] = [inp["source"][0]["tracer"][0][1]] * nt
    return inp


@pytest.mark.timeout(300)
@pytest.mark.parametrize("nt,mode", [(1, "per_tracer"), (2, "per_tracer"), (2, "coupled")])
def test_tracers(nt, mode):
    """one tracer with its injection table; two tracers (the second decays) solved one by one and in one coupled solve under
    the reference's auxiliary preconditioner (default_aux_pc="bjacobi").  Rank 1 has no tracer source and the mesh no
    boundary: it makes every assembly and solve call all the same, or the case would stop at its timeout"""
    kw = dict(tracer_solve=mode)
    if mode == "coupled":
        kw["default_aux_pc"] = "bjacobi"
    inp = _doublet(nt, table=nt == 1)
    one, res = _two_ranks_against_one(inp, **kw)
    names = ["tracer_tracer1", "tracer_tracer2"][:nt]
    assert all(one[k].max() > 1e-6 for k in names)                     # the tracer is in
    if nt == 2:
        assert np.abs(one[names[0]] - one[names[1]]).max() > 1e-3 * one[names[0]].max()      # and the second one decays
    assert [r[2].tolist() for r in res] == [[0], [1]]                  # injector here, producer there


@pytest.mark.timeout(300)
def test_minc_zones():
    """the MINC column: cells 2..7 carry two matrix cells each, the default split gives rank 0 four of those families and rank 1 two"""
    inp = json.load(open(os.path.join(INPUTS, "minc_column_minc.json")))
    one, res = _two_ranks_against_one(inp, mesh_file=os.path.join(INPUTS, "gminc_column.dat"))
    parent, level = one["minc_parent"], one["minc_level"]
    fams = [set(parent[gid].tolist()) for _, gid, _, _ in res]
    assert not fams[0] & fams[1]                                       # no family on two ranks
    for _, gid, _, f in res:
        assert (level[gid] > 0).sum() in (8, 4) and np.array_equal(f["minc_level"], level[gid]) and np.array_equal(f["minc_parent"], parent[gid])


@pytest.mark.timeout(300)
def test_rock_table_control():
    """problem 5a with its rock type's permeability doubling over the third to fifth step: both runs end with the table's
    value at their final time on every cell, and agree"""
    inp = json.load(open(os.path.join(INPUTS, "problem5a.json")))
    dt, k0 = inp["time"]["step"]["size"], 2.5e-14
    inp["rock"]["types"][0]["permeability"] = [[2.0 * dt, k0, k0], [5.0 * dt, 2.0 * k0, 2.0 * k0]]
    one, res = _two_ranks_against_one(inp)
    assert one["rock_permeability"].min() > 1.2 * k0                   # the change fell inside the run


def _reinjection(timed=False):
    inp = json.load(open(os.path.join(INPUTS, "reinjection.json")))
    if timed:      # a time table in the network: it is handed to the library again before every try
        inp["network"]["reinject"][0]["steam"][0]["rate"] = [[0.0, 1.5], [1.0e9, 1.5]]
    return inp


@pytest.mark.timeout(300)
@pytest.mark.parametrize("owner,timed", [(None, False), ([0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1], False),
                                         ([0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0], False), ([0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1], True)])
def test_source_network(owner, timed):
    """the reinjection column: producers in cells 3, 4, 5 in a group, a reinjector into the wells of cells 0 and 1.  The default
    split leaves rank 1 with a source outside the network only; then the producers on rank 1 and the injectors on rank 0;
    then a rank without any source (cells 6..9), which takes part in every network pass; then a network with a time table"""
    one, res = _two_ranks_against_one(_reinjection(timed), owner=owner, mesh_file=os.path.join(INPUTS, "greinjection.dat"))
    assert one["network_group_rate"][0] < -1.0 and one["network_reinject_output_water_rate"].max() > 0.1      # the network is at work
    if owner is not None and owner[-1] == 1:
        assert res[0][2].tolist() == [4, 5, 6, 7] and res[1][2].tolist() == [0, 1, 2, 3]
    if owner is not None and owner[-1] == 0:
        assert res[1][2].size == 0


@pytest.mark.timeout(300)
def test_run_module_under_the_launcher(tmp_path):
    """`python -m torch.distributed.run --nproc-per-node 2 -m waiwera_amd.run doublet.json -o out.npz`: the two rank files
    hold the one-rank run's tracer and source fields, with the cells' and the sources' numbers in the input"""
    from waiwera_amd.simulation import Simulation
    inp = _doublet(1)
    inp["time"]["step"]["maximum"]["number"] = 5
    inp["output"] = dict(inp["output"], filename=None)
    for f in ("gdoublet.msh", "doublet_ss.h5"):
        shutil.copy(os.path.join(INPUTS, f), tmp_path / f)
    path = str(tmp_path / "doublet.json")
    json.dump(inp, open(path, "w"))
    env = dict(os.environ, WAI_RCCL_LIB=LOOPBACK, WAI_BENCH_LOOPBACK="1", HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT)
    out = str(tmp_path / "out.npz")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), "-m", "waiwera_amd.run", path, "-o", out]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "finished at t =" in r.stdout
    ser = Simulation.from_json(path)
    one = ser.run()
    ser.ode.destroy()
    n = one["fluid_pressure"].size
    x, rate = np.full(n, np.nan), np.full(2, np.nan)
    for rank in range(2):
        d = np.load(str(tmp_path / ("out.rank%d.npz" % rank)))
        x[d["owned_gid"]] = d["tracer_tracer1"]
        rate[d["owned_source"]] = d["source_rate"]
    _close("tracer_tracer1", x, one["tracer_tracer1"])
    _close("source_rate", rate, one["source_rate"])

"""The batched build of the source network's coupling blocks (wai_set_coupling_build, kernels_coupling.hip): every column on
private scratch, all columns in five launches.  The oracle is the column loop, host mode and device mode (they agree bit for
bit, tests/test_hip_network_device.py): cells, blocks, the flag, the Newton step and a residual after the Jacobian must be
the SAME BITS, y and the fluid record must not be touched, and the launches of a build must not depend on the number of
network cells."""
import ctypes as C
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

from tests import network_cases as nc
from tests import test_hip_memory as tm
from tests import test_hip_multirank as mr
from tests.test_hip_network_device import DeviceVector, P, carry, fixture_case, same_bits
from waiwera_amd import lib as wl
from waiwera_amd.cases import make_case, scaled

pytestmark = pytest.mark.gpu
INPUTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inputs")
BATCH_LAUNCHES = 2 + 5      # the pass before the build (k_source_rates, k_network_pass) and the five of one chunk
DF = {"w": 15, "we": 23, "wce": 26}


# ---- 1. bit for bit against both column loops ------------------------------------------------------------------------------
def three_contexts():
    """coupled_pair's arrangement (tests/test_hip_network_device.py) three times: host, device + columns, device + batched"""
    from waiwera_amd.flow_simulation import FlowSimulation
    g, lm, prim, region = make_case(dims=tm.DIMS, brick=tm.BRICK, eos="we", lens=True)
    controls, spec = tm.network(lm)
    rate = np.asarray(lm.src_rate)
    inj = [int(i) for i in np.flatnonzero(rate > 0)]
    spec["reinjectors"][0]["overflow"] = (1, inj[1])
    y = scaled(prim, region, "we").ravel().copy()
    sims = {}
    for name in ("host", "columns", "batched"):
        sim = FlowSimulation(lm, eos="we")
        sim.set_regions(region)
        if name != "host":
            sim.set_network_pass("device")
        if name == "batched":
            sim.set_coupling_build("batched")           # before the network is set
            assert sim.coupling_build() == ("batched", "columns")
        sim.set_source_controls(controls)
        sim.set_source_network(spec)
        want = "batched" if name == "batched" else "columns"
        assert sim.coupling_build() == (want, want)
        sims[name] = sim
    return lm, y, sims


def test_batched_build_equals_both_column_loops_bit_for_bit():
    lm, y, sims = three_contexts()
    got = {}
    for name, sim in sims.items():
        n = sim.num_dof
        L, f, f2 = np.zeros(n), np.zeros(n), np.zeros(n)
        assert sim.pre_eval(0.0, y) == 0
        sim.lhs(0.0, (0.0, 0.0), y, L)
        assert sim.residual(0.0, tm.DT, y, L, f) == 0
        flu0 = sim.fluid()
        rates0 = sim.source_rates()
        yd, Ld = DeviceVector(y), DeviceVector(L)
        assert sim.jacobian(0.0, tm.DT, yd, Ld) == 0
        sim.synchronize()
        assert same_bits(yd.host(), y), "y after wai_jacobian is y before it"
        yd.free(); Ld.free()
        assert same_bits(sim.fluid(), flu0), "the fluid record after wai_jacobian is the one before it"
        stats = sim.coupling_build_stats()
        cells, E = sim.network_couplings()
        G, R = sim.source_network()
        rates1 = sim.source_rates()
        assert same_bits(rates0[0], rates1[0]) and same_bits(rates0[1], rates1[1])
        assert sim.residual(0.0, tm.DT, y, L, f2) == 0      # the factors and enthalpies the build left behind
        y1, f1 = y.copy(), np.zeros(n)
        reason, kits, rnorm = sim.newton_step(0.0, tm.DT, 0, y1, L, f1)
        got[name] = dict(f=f, f2=f2, cells=cells, E=E, G=G, R=R, y1=y1, f1=f1, kits=kits, reason=reason, stats=stats,
                         rate=rates1[0], enth=rates1[1])
        sim.destroy()
    b = got["batched"]
    assert len(b["cells"]) == 7 and np.abs(b["E"]).max() > 0 and b["reason"] > 0
    assert same_bits(b["f"], b["f2"])
    assert b["stats"] == (BATCH_LAUNCHES, 14, 1) and got["columns"]["stats"] == (2 + 13 * 14, 14, 0) and got["host"]["stats"][1:] == (14, 0)
    for other in ("host", "columns"):
        o = got[other]
        assert np.array_equal(o["cells"], b["cells"]) and (o["kits"], o["reason"]) == (b["kits"], b["reason"])
        for key in ("f", "f2", "E", "G", "R", "rate", "enth", "y1", "f1"):
            assert same_bits(o[key], b[key]), (other, key)


# ---- 2. shapes where the kernels can go wrong, against device + columns --------------------------------------------------------
def well_field(lm, cells, n, eos):
    """n sources on the given cells (source i in cells[i % len(cells)]): three in four produce on deliverability behind one
    limited group with a separator, whose water a reinjector hands to the others -- proportions for all but the last, which
    takes the overflow; every other injector keeps its own enthalpy.  (cell, rate, enth, comp, controls, spec)"""
    m = len(cells)
    cell = np.array([cells[i % m] for i in range(n)], dtype=np.int32)
    inj = [i for i in range(n) if i % 4 == 3]
    prod = [i for i in range(n) if i % 4 != 3]
    rate = np.where(np.arange(n) % 4 == 3, 0.5, -1.0)
    enth = np.where(np.arange(n) % 4 == 3, 4.0e5 + 1.0e3 * np.arange(n), 0.0)
    controls = [dict(kind="deliverability", coef=(1.0 + 0.1 * (i % 5)) * 1.0e-12, pressure=0.5e5) if i in prod else dict()
                for i in range(n)]
    outs = [dict(flow=1, out=(1, i), rate=-1.0, proportion=0.8 / len(inj), enthalpy=-1.0) for i in inj[:-1]]
    spec = dict(rate_specified=[0] * n, enthalpy_specified=[int(i in inj and (i // 4) % 2 == 0) for i in range(n)],
                groups=[dict(inputs=[(1, i) for i in prod], scaling=0, limits=[(0, 0.02 * len(prod))],
                             separator=None if eos == "w" else [(640.0e3, 2748.0e3)])],
                reinjectors=[dict(input=(2, 0), overflow=(1, inj[-1]), outputs=outs)])
    return cell, rate, enth, np.zeros(n, dtype=np.int32), controls, spec


def context(dims, eos, cells_of, n_of, device=True):
    """a context on a dims mesh with well_field's network on cells_of(lm) -> (sim, lm, y, cells)"""
    from waiwera_amd.flow_simulation import FlowSimulation
    assert dims[0] * dims[1] * dims[2] <= 108
    g, lm, prim, region = make_case(dims=dims, brick=(2, 2, dims[2]), eos=eos, sources=False)
    sim = FlowSimulation(lm, eos=eos)
    sim.set_regions(region)
    cells = cells_of(lm)
    n = n_of(len(cells))
    cell, rate, enth, comp, controls, spec = well_field(lm, cells, n, eos)
    keep = (wl._i32(cell), wl._f64(rate), wl._f64(enth), wl._i32(comp))
    sim._chk(wl.LIB.wai_set_sources(sim.h, n, P(keep[0]), P(keep[1]), P(keep[2]), P(keep[3])), "set_sources")
    sim._chk(wl.LIB.wai_set_source_controls(sim.h, wl.source_controls(controls)), "set_source_controls")
    if device:
        sim.set_network_pass("device")
    sim.set_source_network(spec)
    y = scaled(prim, region, eos).ravel().copy()
    return sim, lm, y, cells


def build(sim, y, how, dt=tm.DT, method=None):
    """one wai_jacobian with the coupling build `how`: (cells, E, stats, passes, waits)"""
    n = sim.num_dof
    L, f = np.zeros(n), np.zeros(n)
    sim.set_coupling_build(how)
    assert sim.pre_eval(0.0, y) == 0
    sim.lhs(0.0, (0.0, 0.0), y, L)
    if method:
        L2 = 0.97 * L
        sim.set_residual_form(*method, lhs_last2=L2)
    assert sim.residual(0.0, dt, y, L, f) == 0
    flu0 = sim.fluid()
    p0, w0 = sim.network_stats()
    yd, Ld = DeviceVector(y), DeviceVector(L)
    assert sim.jacobian(0.0, dt, yd, Ld) == 0
    p1, w1 = sim.network_stats()
    sim.synchronize()
    assert same_bits(yd.host(), y)
    yd.free(); Ld.free()
    assert same_bits(sim.fluid(), flu0)
    cells, E = sim.network_couplings()
    return cells, E, sim.coupling_build_stats(), p1 - p0, w1 - w0


def check_against_columns(sim, y, m, bs, chunks=1, **kw):
    cc, Ec, sc, pc, wc = build(sim, y, "columns", **kw)
    cb, Eb, sb, pb, wb = build(sim, y, "batched", **kw)
    ncol = m * bs
    assert sim.coupling_build() == ("batched", "batched")
    assert len(cc) == m and np.abs(Ec).max() > 0, "the network couples its cells"
    assert np.array_equal(cc, cb) and Ec.shape == Eb.shape == (m, m, bs, bs)
    assert same_bits(Ec, Eb), np.argwhere(Ec != Eb)[:8]
    assert sc == (2 + 13 * ncol, ncol, 0) and pc == 1 + 2 * ncol
    assert sb == (2 + 5 * chunks, ncol, chunks) and pb == 1 + ncol and wb <= 1
    return Eb


def first_cells(m):
    return lambda lm: list(range(m))


def test_two_network_cells_sharing_a_face():
    """the perturbed cell is another network row's NEIGHBOUR: its private record must stand in there too"""
    def pick(lm):
        fc = np.asarray(lm.face_cells).reshape(-1, 2)
        a, b = [int(x) for x in fc[(fc < lm.n_owned).all(axis=1)][0]]
        far = [c for c in range(lm.n_owned) if c not in (a, b) and not ((fc == c).any(axis=1) & ((fc == a) | (fc == b)).any(axis=1)).any()]
        return [a, b] + far[:2]
    sim, lm, y, cells = context((4, 4, 2), "we", pick, lambda m: 4)
    fc = np.asarray(lm.face_cells).reshape(-1, 2).tolist()
    assert [cells[0], cells[1]] in fc or [cells[1], cells[0]] in fc, "two network cells share a face"
    E = check_against_columns(sim, y, 4, 2)
    order = np.argsort(cells)
    i, j = int(np.flatnonzero(order == 0)[0]), int(np.flatnonzero(order == 1)[0])
    assert np.abs(E[i, j]).max() > 0 or np.abs(E[j, i]).max() > 0
    sim.destroy()


@pytest.mark.parametrize("n", [65, 130])
def test_several_sources_in_one_cell(n):
    """65 and 130 sources on the 32 cells of a 4 x 4 x 2 mesh: every cell's cell_src chain has two to five links"""
    sim, lm, y, cells = context((4, 4, 2), "we", first_cells(32), lambda m: n)
    check_against_columns(sim, y, 32, 2)
    sim.destroy()


def test_reference_fixture_network_on_few_cells(oracle):
    """the reference's reinjector fixture (39 sources, 6 groups, 10 reinjectors, chains and overflows) with further
    producers up to 65 sources, on 32 cells, rates as given: the blocks come from the flowing enthalpies alone"""
    from waiwera_amd.flow_simulation import FlowSimulation
    g, lm, prim, region = make_case(dims=(4, 4, 2), brick=(2, 2, 2), eos="we", sources=False)
    sim = FlowSimulation(lm, eos="we")
    sim.set_regions(region)
    sim.set_network_pass("device")
    carry(sim, lm, nc.with_sources(fixture_case(oracle), 65))
    y = scaled(prim, region, "we").ravel().copy()
    cc, Ec, sc, pc, wc = build(sim, y, "columns")
    cb, Eb, sb, pb, wb = build(sim, y, "batched")
    assert sim.coupling_build() == ("batched", "batched")
    assert np.array_equal(cc, cb) and same_bits(Ec, Eb)
    assert sb[0] == BATCH_LAUNCHES and sb[2] == 1 and sc[2] == 0 and sb[1] == sc[1] > 0 and pb == 1 + sb[1] and wb <= 1
    sim.destroy()


@pytest.mark.parametrize("m", [63, 64, 65, 100])
def test_network_cells_at_the_waves_edges(m):
    """63, 64, 65 and 100 network cells of the 108 of a 6 x 6 x 3 mesh: more rows than a wave holds, 126 .. 200 columns"""
    sim, lm, y, cells = context((6, 6, 3), "we", first_cells(m), lambda k: k)
    assert lm.n_owned == 108
    check_against_columns(sim, y, m, 2)
    sim.destroy()


@pytest.mark.parametrize("eos,m", [("w", 65), ("wce", 85), ("wce", 86)])
def test_one_and_three_primaries(eos, m):
    """eos w (one primary, isothermal) and wce (three): 65, 255 and 258 columns -- the last two on either side of a
    workgroup of k_cb_states"""
    sim, lm, y, cells = context((6, 6, 3), eos, first_cells(m), lambda k: k)
    check_against_columns(sim, y, m, {"w": 1, "wce": 3}[eos])
    sim.destroy()


def test_bdf2_residual_form():
    sim, lm, y, cells = context((4, 4, 2), "we", first_cells(9), lambda k: 13)
    check_against_columns(sim, y, 9, 2, method=("bdf2", 0.7))
    sim.destroy()


def test_three_chunks_give_the_same_bits(monkeypatch):
    """a byte cap that holds a third of the columns (and not one more): three chunks, the last short, fifteen launches"""
    m, n, bs = 10, 13, 2
    sim, lm, y, cells = context((4, 4, 2), "we", first_cells(m), lambda k: n)
    per_col = 8 * (1 + DF["we"] + 5 * n + m * bs)
    E1 = check_against_columns(sim, y, m, bs)
    monkeypatch.setenv("WAI_COUPLING_BATCH_BYTES", str(per_col * 8 - 1))      # 7 columns fit: 7 + 7 + 6
    E3 = check_against_columns(sim, y, m, bs, chunks=3)
    assert same_bits(E1, E3)
    monkeypatch.setenv("WAI_COUPLING_BATCH_BYTES", str(per_col - 1))          # not even one column fits: refused with a text
    with pytest.raises(wl.WaiError) as e:
        build(sim, y, "batched")
    assert "one column's scratch (%d bytes) exceeds the cap (%d bytes)" % (per_col, per_col - 1) in str(e.value)
    monkeypatch.delenv("WAI_COUPLING_BATCH_BYTES")
    assert same_bits(check_against_columns(sim, y, m, bs), E1)
    sim.destroy()


# ---- 3. launches, waits, passes, memory --------------------------------------------------------------------------------------
def test_launches_do_not_depend_on_the_number_of_cells():
    stats = {}
    for m in (7, 100):
        sim, lm, y, cells = context((6, 6, 3), "we", first_cells(m), lambda k: k)
        sim.set_coupling_build("batched")
        build(sim, y, "batched")      # (the first device pass uploads the description: one wait, once)
        cb, Eb, sb, pb, wb = build(sim, y, "batched")
        assert len(cb) == m and sb[1:] == (2 * m, 1) and pb == 1 + 2 * m and wb <= 1
        stats[m] = sb[0]
        sim.destroy()
    assert stats[7] == stats[100] == BATCH_LAUNCHES


def test_building_again_does_not_grow_the_scratch():
    sim, lm, y, cells = context((4, 4, 2), "we", first_cells(12), lambda k: 16)
    build(sim, y, "batched")
    settled = wl.device_memory()
    for how in ("batched", "columns", "batched"):
        build(sim, y, how)
    assert wl.device_memory() == settled
    start = settled
    sim.destroy()
    assert wl.device_memory()[0] < start[0]


# ---- 4. fall-backs -----------------------------------------------------------------------------------------------------------
def test_network_too_large_for_lds_keeps_the_column_loop():
    """the arrangement of test_network_too_large_for_lds_keeps_the_host_pass: asked for the device pass and the batched
    build, the host pass and its column loop stay in force"""
    from waiwera_amd.flow_simulation import FlowSimulation
    g, lm, prim, region = make_case(dims=(4, 4, 2), brick=(2, 2, 2), eos="we", sources=False)
    sim = FlowSimulation(lm, eos="we")
    sim.set_regions(region)
    limit, needed = C.c_int(0), C.c_int(0)

    def flat(n):
        spec = dict(rate_specified=[1] * n, enthalpy_specified=[0] * n, reinjectors=[],
                    groups=[dict(inputs=[(1, i) for i in range(n)], scaling=0, limits=[(0, 0.3 * n)], separator=None)])
        k = np.arange(n)
        return nc.case(spec, -0.5 - 0.01 * (k % 7), 1.0e6 + 1.0e3 * k, nc.separators(n, range(0, n, 3)))
    sim.set_network_pass("device")
    sim.set_coupling_build("batched")
    carry(sim, lm, flat(64))
    sim._chk(wl.LIB.wai_test_network_lds(sim.h, C.byref(limit), C.byref(needed)), "network_lds")
    assert sim.network_pass() == ("device", "device") and sim.coupling_build() == ("batched", "batched")
    n = int(limit.value / (needed.value / 64.0)) + 16
    carry(sim, lm, flat(n))
    sim._chk(wl.LIB.wai_test_network_lds(sim.h, C.byref(limit), C.byref(needed)), "network_lds")
    assert needed.value > limit.value
    assert sim.network_pass() == ("device", "host") and sim.coupling_build() == ("batched", "columns")
    sim.destroy()


def test_host_pass_couplings_off_and_order_of_setting():
    sim, lm, y, cells = context((4, 4, 2), "we", first_cells(6), lambda k: 8, device=False)
    sim.set_coupling_build("batched")                   # after the network is set
    assert sim.network_pass() == ("host", "host") and sim.coupling_build() == ("batched", "columns")
    ch, Eh, sh, ph, wh = build(sim, y, "batched")        # the host pass' column loop runs
    assert sh[1:] == (12, 0) and wh > 12 and len(ch) == 6
    sim.set_network_pass("device")
    assert sim.coupling_build() == ("batched", "batched")
    Eb = check_against_columns(sim, y, 6, 2)
    assert same_bits(Eh, Eb)
    sim.set_network_couplings(False)
    assert sim.coupling_build() == ("batched", "columns")
    cn, En, sn, pn, wn = build(sim, y, "batched")
    assert len(cn) == 0 and sn == (0, 0, 0) and pn == 0, "couplings off: no build"
    sim.set_network_couplings(True)
    assert sim.coupling_build() == ("batched", "batched")
    sim.set_coupling_build("columns")
    assert sim.coupling_build() == ("columns", "columns")
    sim.destroy()


def test_unknown_build_is_refused():
    sim, lm, y, cells = context((4, 4, 2), "we", first_cells(4), lambda k: 4)
    with pytest.raises(wl.WaiError) as e:
        sim._chk(wl.LIB.wai_set_coupling_build(sim.h, 2), "set_coupling_build")
    assert "(-2)" in str(e.value) and "WAI_COUPLING_BUILD_BATCHED" in str(e.value)
    with pytest.raises(ValueError):
        sim.set_coupling_build("rows")
    assert sim.coupling_build() == ("columns", "columns")
    r = C.c_int(-1)
    sim._chk(wl.LIB.wai_get_coupling_build(sim.h, None, C.byref(r)), "get_coupling_build")       # out-arguments may be NULL
    sim._chk(wl.LIB.wai_get_coupling_build(sim.h, C.byref(r), None), "get_coupling_build")
    sim._chk(wl.LIB.wai_test_coupling_build_stats(sim.h, None, None, None), "coupling_build_stats")
    assert r.value == 0
    sim.destroy()


# ---- 5. a whole input run ----------------------------------------------------------------------------------------------------
def test_input_run_identical_with_the_batched_build():
    from waiwera_amd.simulation import Simulation
    runs = {}
    for name, kw in (("default", {}), ("batched", dict(coupling_build="batched", network_pass="device"))):
        sim = Simulation.from_json(os.path.join(INPUTS, "reinjection.json"), mesh_file=os.path.join(INPUTS, "greinjection.dat"), **kw)
        want = ("batched", "batched") if name == "batched" else ("columns", "columns")
        assert sim.coupling_build_choice == want and sim.ode.coupling_build() == want
        out = sim.run()
        runs[name] = (list(sim.ts.history), out, sim.ode.coupling_build_stats())
        sim.ode.destroy()
    (dh, do, ds), (bh, bo, bs) = runs["default"], runs["batched"]
    assert len(dh) > 0 and [tuple(x) for x in dh] == [tuple(x) for x in bh]
    assert sorted(do) == sorted(bo)
    for key in do:
        a, b = np.asarray(do[key]), np.asarray(bo[key])
        assert (same_bits(a, b) if a.dtype == np.float64 else np.array_equal(a, b)), key
    assert bs[0] == BATCH_LAUNCHES and bs[2] == 1 and ds[2] == 0 and bs[1] == ds[1] > 0


# ---- 6. two ranks: the column loop stays -------------------------------------------------------------------------------------
def _two_rank_worker(rank, world, uid_q, q):
    os.environ["WAI_RCCL_LIB"] = mr.LOOPBACK
    mr._own_cus(rank, world)
    mr._default_overlap()
    from waiwera_amd.flow_simulation import FlowSimulation
    if rank == 0:
        uid = wl.comm_unique_id()
        for _ in range(world - 1):
            uid_q.put(uid)
    else:
        uid = uid_q.get(timeout=300)
    g, lm, prim, region, gidx, ng = mr._net_problem(mr.M.partition_shape(world), rank)
    sim = FlowSimulation(lm, eos="we", device=0)
    sim.set_regions(region)
    sim.comm_init(rank, world, uid)
    sim.set_network_pass("device")
    sim.set_coupling_build("batched")
    sim.set_source_global_index(ng, gidx)
    sim.set_source_controls([mr._NET_CONTROLS[g] for g in gidx])
    sim.set_source_network(mr._network_spec(ng))
    choice = (sim.network_pass(), sim.coupling_build())
    y = scaled(prim, region).ravel().copy()
    cp = mr._initial_couplings(sim, lm, y)
    stats = sim.coupling_build_stats()
    hist = mr._run_steps(sim, y, 1)
    q.put((rank, lm.owned_gid.copy(), y[: lm.n_owned * 2].copy(), hist, cp, choice, stats))
    sim.destroy()


@pytest.mark.timeout(900)
def test_two_ranks_keep_the_column_loop():
    """over the loop-back transport the network lives on two ranks: host pass and column loop stay in force whatever is asked
    for, and blocks and a time step equal the one-rank run's as they do today (tests/test_hip_multirank.py)"""
    assert os.path.exists(mr.LOOPBACK), "build first: python __graft_entry__.py"
    os.environ["WAI_RCCL_LIB"] = mr.LOOPBACK
    from waiwera_amd.flow_simulation import FlowSimulation
    world = 2
    ctx = mp.get_context("spawn")
    q, uid_q = ctx.Queue(), ctx.Queue()
    procs = [ctx.Process(target=_two_rank_worker, args=(r, world, uid_q, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=400) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    g, lm, prim, region, gidx, ng = mr._net_problem((1, 1, 1), 0)
    sim = FlowSimulation(lm, eos="we", device=0)
    sim.set_regions(region)
    sim.set_source_controls(mr._NET_CONTROLS)
    sim.set_source_network(mr._network_spec(ng))
    y = scaled(prim, region).ravel().copy()
    gid1, E1, cells1 = mr._initial_couplings(sim, lm, y)
    hist = mr._run_steps(sim, y, 1)
    yser = np.zeros((g.n_global, 2))
    yser[lm.owned_gid] = y[: lm.n_owned * 2].reshape(-1, 2)
    sim.destroy()
    res.sort(key=lambda r: r[0])
    colgid = np.concatenate([r[4][0] for r in res])
    pos1 = {int(gc): i for i, gc in enumerate(gid1)}
    perm = [pos1[int(gc)] for gc in colgid]
    ypar = np.zeros((g.n_global, 2))
    for rank, gid, yy, h, cp, choice, stats in res:
        assert choice == (("device", "host"), ("batched", "columns")), choice
        assert stats[1] == 2 * len(colgid) and stats[2] == 0
        rows, E, cells = cp
        ref = E1[np.ix_([pos1[int(gc)] for gc in rows], perm)]
        assert np.abs(E - ref).max() <= 1e-9 * np.abs(E1).max()
        assert all(r > 0 for r, _, _ in h) and [n for _, n, _ in h] == [n for _, n, _ in hist]
        ypar[gid] = yy.reshape(-1, 2)
    err = np.abs(ypar - yser).max(axis=0) / np.abs(yser).max(axis=0)
    assert err.max() < 1e-7, err

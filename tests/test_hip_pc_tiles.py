"""Tile-scheduled ILU sweeps (wai_set_pc_tiles, k_tile_solve) for subdomains larger than a workgroup: with tiles set, the two
substitution sweeps take one launch per level of TILES; every row does the same subtractions in the same order as on the
launch-per-row-level path, so the level path -- the same context with the tiles cleared -- is the oracle and the comparison
is np.array_equal.  Systems are built by tests/test_hip_pc.py::system (imported)."""
import os

import numpy as np
import pytest

from tests.test_hip_pc import relmax, system
from tests.test_tile_schedule_host import TileTwin, ids

pytestmark = pytest.mark.gpu
BS = {"w": 1, "we": 2, "wce": 3, "wsce": 4}
LEVEL_PATH = "k_spmv + k_lvl_solve per level"
TILE_PATH = "k_spmv + k_tile_solve per tile level"


def one_block(oracle, eos, dims, brick, **kw):
    """one block per rank; the bricks the cells are numbered by are returned as the tiles"""
    from waiwera_amd.cases import make_case
    lens = eos in ("we", "wce")
    tiles = np.asarray(make_case(dims=dims, brick=brick, eos=eos, lens=lens, **kw)[1].sub_ptr, dtype=np.int32)
    lm, sim, osim, J, f = system(oracle, eos, dims, brick, one_block=True, lens=lens, **kw)
    return lm, sim, osim, J, f, tiles


def apply(sim, r):
    z = np.zeros(sim.num_dof)
    sim.pc_apply(r, z)
    return z


def counted_apply(sim, r):
    assert sim.pc_setup() == 0
    k0 = sim.launch_stats()[0]
    z = apply(sim, r)
    return z, sim.launch_stats()[0] - k0


def both_paths(sim, r, tiles, name_tiles=TILE_PATH, name_levels=LEVEL_PATH):
    """(z with tiles, launches, z with the tiles cleared, launches): the tiles are left cleared"""
    sim.set_pc_tiles(tiles)
    zt, kt = counted_apply(sim, r)
    assert sim.pc_kernel_name() == name_tiles, sim.pc_kernel_name()
    sim.set_pc_tiles(None)
    zl, kl = counted_apply(sim, r)
    assert sim.pc_kernel_name() == name_levels, sim.pc_kernel_name()
    return zt, kt, zl, kl


@pytest.mark.parametrize("dims", [(12, 10, 9), (13, 10, 9)])
@pytest.mark.parametrize("eos", ["w", "we", "wce", "wsce"])
def test_same_bits_as_the_level_path(oracle, eos, dims):
    """one block per rank, tiles = the 4 x 5 x 3 bricks (13 x 10 x 9: partial bricks), block sizes 1 - 4: one application and
    whole Krylov solves agree bit for bit with the tiles cleared on the same context; against the oracle within the bounds
    test_subdomains_larger_than_a_workgroup holds this path to"""
    lm, sim, osim, J, f, tiles = one_block(oracle, eos, dims, (4, 5, 3))
    n = sim.num_dof
    assert lm.n_owned > 1024
    assert osim.pc_setup(J) == 0
    r = np.random.default_rng(12).normal(size=n)
    zt, kt, zl, kl = both_paths(sim, r, tiles)
    assert np.array_equal(zt, zl)
    print(eos, dims, "launches per application: tiles", kt, "levels", kl, "against the oracle", relmax(zt, osim.pc_apply(r)))
    assert relmax(zt, osim.pc_apply(r)) < 1e-10
    for ksp, kt_ in (("bcgs", 0), ("gmres", 1)):
        sim.set_opts(ksp_type=ksp, ksp_rtol=1e-12)
        out = {}
        for tag, tp in (("tiles", tiles), ("levels", None)):
            sim.set_pc_tiles(tp)
            x = np.zeros(n)
            its, reason, rn = sim.ksp_solve(f, x)
            assert reason > 0 and sim.pc_kernel_name() == (TILE_PATH if tp is not None else LEVEL_PATH)
            out[tag] = (its, reason, rn, x)
        assert out["tiles"][:3] == out["levels"][:3] and np.array_equal(out["tiles"][3], out["levels"][3]), (ksp, out["tiles"][:3], out["levels"][:3])
        oreason, xo, oits, hist = osim.ksp_solve(J, f, ksp_type=kt_, rtol=1e-12)
        assert oreason > 0 and relmax(out["tiles"][3], xo) < 1e-8, (ksp, relmax(out["tiles"][3], xo))
    sim.destroy(); osim.close()


@pytest.mark.parametrize("dims,expect", [((12, 10, 9), (58, 12)), ((13, 10, 9), (60, 14))])
def test_launch_counts(oracle, dims, expect):
    """around one application the launch counter falls by exactly (row levels) - (tile levels), both sweeps together: the
    numbers come from the pattern (the twin of tests/test_tile_schedule_host.py), are the issue's 58 - 12 and 60 - 14, and are
    what the library reads back"""
    lm, sim, osim, J, f, tiles = one_block(oracle, "we", dims, (4, 5, 3))
    rp, ci = osim.pattern()
    tw = TileTwin(rp, ci, np.array([0, lm.n_owned]), ids(tiles))
    assert (tw.nlev_f + tw.nlev_b, tw.ntl_f + tw.ntl_b) == expect
    r = np.random.default_rng(5).normal(size=sim.num_dof)
    sim.set_pc_tiles(tiles)
    assert sim.pc_setup() == 0
    facts = sim.tile_schedule()
    assert facts == dict(tiles=len(tiles) - 1, ntl_f=tw.ntl_f, ntl_b=tw.ntl_b, max_tile_rows=int(np.diff(tiles).max()),
                         max_in_levels=int(max(tw.ninf.max(), tw.ninb.max())), serve=1, nlev_f=tw.nlev_f, nlev_b=tw.nlev_b), facts
    zt, kt, zl, kl = both_paths(sim, r, tiles)
    print(dims, "launches: tiles", kt, "levels", kl)
    assert kl - kt == expect[0] - expect[1], (kl, kt)
    assert np.array_equal(zt, zl)
    assert sim.tile_schedule()["tiles"] == 0      # cleared
    sim.destroy(); osim.close()


def test_a_chain_of_tiles_keeps_the_level_path(oracle):
    """24 x 12 x 10 in consecutive 64-row ranges: 45 + 45 tile levels against 44 + 44 row levels -- not served: the level
    path's launches, its text, its bits"""
    lm, sim, osim, J, f = system(oracle, "we", (24, 12, 10), (24, 12, 10), one_block=True)
    n = lm.n_owned
    r = np.random.default_rng(6).normal(size=sim.num_dof)
    z0, k0 = counted_apply(sim, r)
    sim.set_pc_tiles(np.append(np.arange(0, n, 64), n))
    z1, k1 = counted_apply(sim, r)
    facts = sim.tile_schedule()
    assert (facts["tiles"], facts["ntl_f"], facts["ntl_b"], facts["nlev_f"], facts["nlev_b"], facts["serve"]) == (45, 45, 45, 44, 44, 0), facts
    assert k1 == k0 and sim.pc_kernel_name() == LEVEL_PATH and np.array_equal(z0, z1)
    sim.destroy(); osim.close()


@pytest.mark.parametrize("pc", ["bjacobi", "asm"])
def test_two_subdomains_of_1440_rows(oracle, pc):
    """24 x 12 x 10 numbered in 6 x 6 x 5 bricks, two slabs of eight bricks as the subdomains, the bricks as tiles: block
    Jacobi, and PCASM overlap 1 (unfused extended system, whose rows inherit their tiles) -- same bits as with the tiles
    cleared, the oracle's application to 1e-10"""
    from oracle import binding as ol
    from waiwera_amd.cases import make_case, scaled
    from waiwera_amd.flow_simulation import FlowSimulation
    from tests.test_hip_pc import KIND
    g, lm, prim, region = make_case(dims=(24, 12, 10), brick=(6, 6, 5), eos="we", lens=True, brick_order="x")
    tiles = np.asarray(lm.sub_ptr, dtype=np.int32).copy()
    lm.sub_ptr = np.array([0, 1440, 2880], dtype=np.int32)
    sim = FlowSimulation(lm, eos="we")
    osim = ol.OracleSim(oracle, lm, KIND["we"])
    sim.set_regions(region); osim.set_regions(region)
    yo = osim.yvec(scaled(prim, region, "we").ravel().copy())
    assert osim.pre_eval(yo) == 0
    L = osim.lhs()
    err, f = osim.residual(yo, 5.0e4, L)
    err, J = osim.jacobian(yo, 5.0e4, L, f, mode=0)
    assert err == 0
    sim.set_jacobian_values(J)
    names = (TILE_PATH, LEVEL_PATH)
    if pc == "asm":
        sim.set_opts(pc_type="asm", asm_overlap=1); osim.set_asm(1)
        names = ("k_spmv + k_tile_solve per tile level on the extended system (ASM, ILU(0))",
                 "k_spmv + k_lvl_solve per level on the extended system (ASM, ILU(0))")
    assert osim.pc_setup(J) == 0
    r = np.random.default_rng(7).normal(size=sim.num_dof)
    zt, kt, zl, kl = both_paths(sim, r, tiles, *names)
    sim.set_pc_tiles(tiles)
    assert sim.pc_setup() == 0
    facts = sim.tile_schedule(extended=(pc == "asm"))
    print(pc, facts, "launches: tiles", kt, "levels", kl)
    assert facts["serve"] == 1 and facts["tiles"] == (32 if pc == "asm" else 16)
    assert kl - kt == facts["nlev_f"] + facts["nlev_b"] - facts["ntl_f"] - facts["ntl_b"]
    assert np.array_equal(zt, zl)
    assert relmax(zt, osim.pc_apply(r)) < 1e-10
    sim.destroy(); osim.close()


def test_iluk_on_the_level_path(oracle, monkeypatch):
    """ILU(1) under block Jacobi on the one-block case (the filled factor's extended system, big by its row count;
    WAI_ILUK_LEVEL_PATH=1 keeps the fused launch away wherever it would serve): the same bits with and without tiles"""
    monkeypatch.setenv("WAI_ILUK_LEVEL_PATH", "1")
    lm, sim, osim, J, f, tiles = one_block(oracle, "we", (12, 10, 9), (4, 5, 3))
    sim.set_opts(pc_type="bjacobi", ilu_levels=1)
    r = np.random.default_rng(8).normal(size=sim.num_dof)
    zt, kt, zl, kl = both_paths(sim, r, tiles, "k_spmv + k_tile_solve per tile level on the extended system (block Jacobi, ILU(1))",
                                "k_spmv + k_lvl_solve per level on the extended system (block Jacobi, ILU(1))")
    assert np.array_equal(zt, zl) and kt < kl
    osim.set_asm(0); osim.set_ilu_levels(1)
    assert osim.pc_setup(J) == 0
    assert relmax(zt, osim.pc_apply(r)) < 1e-10
    sim.destroy(); osim.close()


def test_wide_mesh(oracle):
    """rows of up to 15 blocks (the refined plan) in enough layers that one block per rank exceeds 1024 rows, a tile per
    layer: the big schedule's 8-bit descriptors serve k_tile_solve as they are -- same bits.  A tile per layer is a chain, so
    the tiles serve only because the rows' own chain is longer"""
    from oracle import binding as ol
    from tests import wide_mesh as wm
    from tests.test_hip_pc import KIND
    from waiwera_amd.cases import scaled
    from waiwera_amd.flow_simulation import FlowSimulation
    nc = wm.wide_case("we", layers=3)[0].n_owned // 3
    layers = 1024 // nc + 2
    lm, prim, region, coarse = wm.wide_case("we", layers=layers)
    assert lm.n_owned == nc * layers > 1024
    lm.sub_ptr = None
    sim = FlowSimulation(lm, eos="we")
    lm.sub_ptr = np.array([0, lm.n_owned], dtype=np.int32)
    osim = ol.OracleSim(oracle, lm, KIND["we"])
    sim.set_regions(region); osim.set_regions(region)
    yo = osim.yvec(scaled(prim, region, "we").ravel().copy())
    assert osim.pre_eval(yo) == 0
    L = osim.lhs()
    err, f = osim.residual(yo, 5.0e4, L)
    err, J = osim.jacobian(yo, 5.0e4, L, f, mode=0)
    assert err == 0
    sim.set_jacobian_values(J)
    tiles = np.arange(0, lm.n_owned + 1, nc)
    r = np.random.default_rng(9).normal(size=sim.num_dof)
    sim.set_pc_tiles(tiles)
    assert sim.pc_setup() == 0
    facts = sim.tile_schedule()
    print("wide mesh", facts)
    assert facts["tiles"] == layers and facts["serve"] == 1
    zt, kt, zl, kl = both_paths(sim, r, tiles)
    assert np.array_equal(zt, zl) and kl - kt == facts["nlev_f"] + facts["nlev_b"] - 2 * layers
    assert osim.pc_setup(J) == 0 and relmax(zt, osim.pc_apply(r)) < 1e-10
    sim.destroy(); osim.close()


def test_per_tracer_solve():
    """the tracers' scalar systems (block size 1) share the flow system's schedule: an auxiliary solve after a flow step, one
    block per rank of 1080 rows, with and without tiles -- same bits, same iteration counts"""
    from tests.test_hip_tracer_coupled import ACT, DECAY, DIFF, PHASES
    from waiwera_amd.cases import make_case, scaled
    from waiwera_amd.flow_simulation import FlowSimulation
    g, lm, prim, region = make_case(dims=(12, 10, 9), brick=(4, 5, 3), eos="we", lens=True)
    tiles = np.asarray(lm.sub_ptr, dtype=np.int32).copy()
    lm.sub_ptr = None
    sim = FlowSimulation(lm, eos="we")
    sim.set_regions(region)
    nt = 2
    rng = np.random.default_rng(11)
    bc = rng.uniform(0, 1e-3, (lm.n_bc, nt))
    inj = np.where(np.asarray(lm.src_rate)[:, None] > 0, rng.uniform(0, 1e-2, (lm.n_src, nt)), 0.0)
    n = lm.n_owned * nt
    X0 = rng.uniform(0, 1e-3, n)
    sim.set_tracers(PHASES[:nt], DECAY[:nt], ACT[:nt], DIFF[:nt], bc=bc, injection=inj)
    sim.set_opts(pc_type="bjacobi", ksp_rtol=1e-10, ftol_rel=1e-9)
    sim.set_pc_tiles(tiles)
    y = scaled(prim, region, "we").ravel().copy()
    assert sim.pre_eval(0.0, y) == 0
    Al = np.zeros(n)
    sim.aux_lhs(0.0, None, Al)
    alx1 = Al * X0
    dt = 1.0e4
    for _ in range(5):
        reason, nits, kits = sim.timestep(0.0, dt, y)
        if reason > 0:
            break
        dt *= 0.2
    assert reason > 0 and sim.pc_kernel_name() == TILE_PATH
    sim.set_tracer_solve_mode("per_tracer")
    sim.set_aux_solver("gmres", rtol=1e-12)
    out = {}
    for tag, tp in (("tiles", tiles), ("levels", None)):
        sim.set_pc_tiles(tp)
        X, new = X0.copy(), np.zeros(n)
        reason, its = sim.aux_solve("beuler", dt, 1.0, alx1, None, X, new)
        assert reason > 0
        out[tag] = (X, new, reason, its)
    print("per-tracer solves: iterations", out["tiles"][3], out["levels"][3])
    assert out["tiles"][2:] == out["levels"][2:]
    assert np.array_equal(out["tiles"][0], out["levels"][0]) and np.array_equal(out["tiles"][1], out["levels"][1])
    assert not np.array_equal(out["tiles"][0], X0)
    sim.destroy()


def _two_rank_worker(rank, world, uid_q, q, dims, brick):
    from tests import test_hip_multirank as T
    from waiwera_amd import mesh as M
    os.environ["WAI_RCCL_LIB"] = T.LOOPBACK
    T._own_cus(rank, world)
    T._default_overlap()
    from waiwera_amd import lib as wl
    from waiwera_amd.cases import make_case, scaled
    from waiwera_amd.flow_simulation import FlowSimulation
    if rank == 0:
        uid = wl.comm_unique_id()
        for _ in range(world - 1):
            uid_q.put(uid)
    else:
        uid = uid_q.get(timeout=300)
    g, lm, prim, region = make_case(dims=dims, brick=brick, eos="we", lens=True, part=M.partition_shape(world), rank=rank)
    tiles = np.asarray(lm.sub_ptr, dtype=np.int32).copy()
    lm.sub_ptr = None
    sim = FlowSimulation(lm, eos="we", device=0)
    sim.set_regions(region)
    sim.comm_init(rank, world, uid)
    sim.set_opts(pc_type="bjacobi", ksp_rtol=1e-12)
    y = scaled(prim, region, "we").ravel().copy()
    n = lm.n_owned * 2
    dt = 2.0e4
    assert sim.pre_eval(0.0, y) == 0
    L, f = np.zeros(n), np.zeros(n)
    sim.lhs(0.0, (0.0, 0.0), y, L)
    assert sim.residual(dt, dt, y, L, f) == 0
    assert sim.jacobian(dt, dt, y, L) == 0
    res = []
    for tp in (tiles, None):     # both ranks take the same path at a time: the solves are collective
        sim.set_pc_tiles(tp)
        assert sim.pc_setup() == 0
        x = np.zeros(n)
        its, reason, rn = sim.ksp_solve(f, x)
        res.append((x, its, reason, rn, sim.pc_kernel_name()))
    q.put((rank, lm.n_owned, res))
    sim.destroy()


@pytest.mark.timeout(600)
def test_two_ranks():
    """block Jacobi, one block per rank (1440 rows each, no communication inside the application) over the loop-back
    transport, the rank's own bricks as tiles: each rank's solution is the one it computes with the tiles cleared, bit for bit"""
    import torch.multiprocessing as mp
    from tests import test_hip_multirank as T
    assert os.path.exists(T.LOOPBACK), "build first: python __graft_entry__.py"
    dims, brick, world = (24, 12, 10), (6, 6, 5), 2
    ctx = mp.get_context("spawn")
    q, uid_q = ctx.Queue(), ctx.Queue()
    procs = [ctx.Process(target=_two_rank_worker, args=(r, world, uid_q, q, dims, brick)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, n_owned, (tl, lv) in res:
        assert n_owned == 1440
        assert tl[4] == TILE_PATH and lv[4] == LEVEL_PATH, (tl[4], lv[4])
        assert tl[2] > 0 and tl[1:4] == lv[1:4] and np.array_equal(tl[0], lv[0]), (rank, tl[1:4], lv[1:4])


def test_refusals(oracle):
    """each refusal by its text (-1), the context untouched by a refused call, and clearing restores the level path"""
    from waiwera_amd.flow_simulation import WaiError
    lm, sim, osim, J, f, tiles = one_block(oracle, "we", (12, 10, 9), (4, 5, 3))
    n = lm.n_owned
    r = np.random.default_rng(10).normal(size=sim.num_dof)
    sim.set_pc_tiles(tiles)
    zt = apply(sim, r)
    t = tiles.tolist()
    for bad, text in (([0, 60, 50] + t[3:], "tile_ptr must ascend from 0 to n_owned (tile 1 ends before it starts)"),
                      ([3] + t[1:], "tile_ptr must ascend from 0 to n_owned (tile 0 starts at row 3)"),
                      (t[:-1] + [n - 1], "tile_ptr must ascend from 0 to n_owned (tile 17 ends at row 1079)"),
                      ([0, 60, 60] + t[2:], "tile 1 is empty"),
                      ([0, 1025, n], "tile 0 has 1025 rows, more than 1024")):
        with pytest.raises(WaiError) as e:
            sim.set_pc_tiles(bad)
        assert "(-1)" in str(e.value) and str(e.value).endswith("wai_set_pc_tiles: " + text), str(e.value)
        assert sim.pc_kernel_name() == TILE_PATH and np.array_equal(apply(sim, r), zt)      # the tiles in force stand
    sim.set_pc_tiles(None)
    zl = apply(sim, r)
    assert sim.pc_kernel_name() == LEVEL_PATH and np.array_equal(zl, zt)
    sim.destroy(); osim.close()
    # a tile across a subdomain boundary: two bricks of 12 x 10 x 9 cells each
    lm, sim, osim, J, f = system(oracle, "we", (24, 10, 9), (12, 10, 9))
    assert list(lm.sub_ptr) == [0, 1080, 2160]
    with pytest.raises(WaiError) as e:
        sim.set_pc_tiles([0, 540, 1400, 2160])
    assert "(-1)" in str(e.value) and str(e.value).endswith("wai_set_pc_tiles: tile 1 straddles a subdomain boundary (row 1080)"), str(e.value)
    sim.set_pc_tiles([0, 540, 1080, 1620, 2160])
    sim.destroy(); osim.close()


def test_device_memory_returns(oracle):
    """set_pc_tiles, a set-up of both the system's own and an extended schedule, then destroy: the live device memory is what
    it was before the context"""
    from waiwera_amd.lib import device_memory
    before = device_memory()
    lm, sim, osim, J, f, tiles = one_block(oracle, "we", (12, 10, 9), (4, 5, 3))
    sim.set_pc_tiles(tiles)
    assert sim.pc_setup() == 0
    sim.set_opts(pc_type="asm", asm_overlap=1)
    assert sim.pc_setup() == 0
    sim.set_pc_tiles(None)
    sim.set_pc_tiles(tiles)
    assert device_memory() != before
    sim.destroy(); osim.close()
    assert device_memory() == before

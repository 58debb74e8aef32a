"""Meshes whose cells have up to 16 faces on the device: a layered quad grid in which coarse columns are enclosed by
3 x 3-refined neighbours (tests/wide_mesh.py: rows of up to 15 blocks, triangles in the cell graph), against the CPU
oracle, which has no face-count limit.  Each case also asserts that the fused wide kernel (k_pc_wide) serves, not the
launch-per-level path, and that meshes of at most 8 faces per cell keep the kernels they had."""
import os
import sys

import numpy as np
import pytest

from oracle import binding as ol
from waiwera_amd.cases import make_case, scaled

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_mesh as wm  # noqa: E402

pytestmark = pytest.mark.gpu

KIND = {"w": 0, "we": 1, "wce": 2, "wsce": 5}
BS = {"w": 1, "we": 2, "wce": 3, "wsce": 4}
LEVEL_PATH = "k_spmv + k_lvl_solve per level"


def relmax(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300)


def wide_system(oracle, eos, dt=5.0e4, **kw):
    from waiwera_amd.flow_simulation import FlowSimulation
    lm, prim, region, coarse = wm.wide_case(eos, **kw)
    sim = FlowSimulation(lm, eos=eos)
    osim = ol.OracleSim(oracle, lm, KIND[eos])
    sim.set_regions(region); osim.set_regions(region)
    y = scaled(prim, region, eos).ravel().copy()
    return lm, sim, osim, y, coarse


def bsr(osim, J, bs, n):
    import scipy.sparse as sp
    rp, ci = osim.pattern()
    return sp.bsr_matrix((J.reshape(-1, bs, bs), ci, rp), shape=(n, n)), rp, ci


@pytest.mark.parametrize("eos", ["w", "we", "wce", "wsce"])
def test_wide_mesh_against_oracle(oracle, eos):
    """residual, FD Jacobian, SpMV, one block-Jacobi ILU(0) application, BiCGStab and GMRES solves on rows of up to
    15 blocks, block sizes 1 - 4"""
    bs, dt = BS[eos], 5.0e4
    lm, sim, osim, y, coarse = wide_system(oracle, eos, dt)
    name = sim.pc_kernel_name()
    assert name == "k_pc_wide<%d,spmv>" % bs and name != LEVEL_PATH, name
    n = sim.num_dof
    yo = osim.yvec(y)
    assert osim.pre_eval(yo) == 0
    L = osim.lhs()
    err, f = osim.residual(yo, dt, L)
    err, J = osim.jacobian(yo, dt, L, f, mode=0)
    assert err == 0
    A, rp, ci = bsr(osim, J, bs, n)
    assert (np.diff(rp)).max() == 15 and all(np.diff(rp)[coarse] >= 14)
    # the device's residual and its own FD Jacobian (the default column-wise assembly)
    assert sim.pre_eval(0.0, y) == 0
    fd = np.zeros(n)
    assert sim.residual(0.0, dt, y, L, fd) == 0 and relmax(fd, f) < 1e-11
    assert sim.jacobian(0.0, dt, y, L) == 0
    Jg = sim.jacobian_values()
    worst = ol.jacobian_parity(Jg, J, rp, ci, yo, L, bs, bar=True)[2]
    assert worst <= 1.0, worst
    # the operator on the oracle's Jacobian
    sim.set_jacobian_values(J)
    x = np.random.default_rng(5).normal(size=n)
    ysp = np.zeros(n)
    sim.spmv(x, ysp)
    assert relmax(ysp, A @ x) < 1e-13
    assert sim.pc_setup() == 0 and osim.pc_setup(J) == 0
    r = np.random.default_rng(3).normal(size=n)
    z = np.zeros(n)
    sim.pc_apply(r, z)
    assert relmax(z, osim.pc_apply(r)) < 1e-10
    for ksp, kt in (("bcgs", 0), ("gmres", 1)):
        sim.set_opts(ksp_type=ksp, ksp_rtol=1e-12)
        xs = np.zeros(n)
        its, reason, rn = sim.ksp_solve(f, xs)
        oreason, xo, oits, hist = osim.ksp_solve(J, f, ksp_type=kt, rtol=1e-12)
        assert reason > 0 and oreason > 0, (ksp, reason, oreason)
        assert relmax(xs, xo[:n]) < 1e-8 and abs(its - oits) <= max(2, oits // 10), (ksp, its, oits)
    sim.destroy(); osim.close()


@pytest.mark.parametrize("eos", ["we", "wce"])
def test_wide_mesh_time_steps(oracle, eos):
    """three backward-Euler steps: the same Newton counts and solution as the oracle"""
    lm, sim, osim, y, coarse = wide_system(oracle, eos)
    assert sim.pc_kernel_name().startswith("k_pc_wide<")
    sim.set_opts(ksp_rtol=1e-10, ftol_rel=1e-9)
    o = osim.opts()
    o.ksp_rtol, o.ftol_rel = 1e-10, 1e-9
    yo = osim.yvec(y)
    t = 0.0
    for dt in (1.0e4, 3.0e4, 1.0e5):
        reason, nits, kits = sim.timestep(t, dt, y)
        onits, okits = osim.timestep(yo, dt, o)       # (Newton iterations, > 0: converged; Krylov iterations)
        assert reason > 0 and onits > 0 and nits == onits, (dt, reason, nits, onits)
        assert abs(kits - okits) <= max(2, okits // 10), (dt, kits, okits)
        t += dt
    assert relmax(y, yo[: y.size]) < 1e-7
    sim.destroy(); osim.close()


def test_wide_mesh_asm(oracle):
    """PCASM overlap 1 on the wide mesh: its extended system is served by k_pc_wide's sweeps-only form"""
    eos, bs, dt = "we", 2, 5.0e4
    lm, sim, osim, y, coarse = wide_system(oracle, eos, dt)
    n = sim.num_dof
    yo = osim.yvec(y)
    assert osim.pre_eval(yo) == 0
    L = osim.lhs()
    err, f = osim.residual(yo, dt, L)
    err, J = osim.jacobian(yo, dt, L, f, mode=0)
    sim.set_jacobian_values(J)
    sim.set_opts(pc_type="asm", asm_overlap=1, ksp_rtol=1e-12)
    osim.set_asm(1)
    assert sim.pc_setup() == 0 and osim.pc_setup(J) == 0
    assert "k_pc_wide on the extended system" in sim.pc_kernel_name(), sim.pc_kernel_name()
    r = np.random.default_rng(11).normal(size=n)
    z = np.zeros(n)
    sim.pc_apply(r, z)
    assert relmax(z, osim.pc_apply(r)) < 1e-10
    x = np.zeros(n)
    its, reason, rn = sim.ksp_solve(f, x)
    oreason, xo, oits, hist = osim.ksp_solve(J, f, rtol=1e-12)
    assert reason > 0 and oreason > 0
    assert relmax(x, xo[:n]) < 1e-8 and abs(its - oits) <= max(2, oits // 10), (its, oits)
    sim.destroy(); osim.close()


def test_row_wise_jacobian_refuses_wide_mesh(oracle, monkeypatch):
    """WAI_JAC_SYM=0 (the row-wise kernels, at most 8 faces per cell) says so instead of computing a wrong Jacobian"""
    from waiwera_amd.flow_simulation import WaiError
    lm, sim, osim, y, coarse = wide_system(oracle, "we")
    L = np.zeros(sim.num_dof)
    assert sim.pre_eval(0.0, y) == 0
    assert sim.lhs(0.0, 1.0, y, L) >= 0
    monkeypatch.setenv("WAI_JAC_SYM", "0")
    with pytest.raises(WaiError, match="at most 8 faces"):
        sim.jacobian(0.0, 5.0e4, y, L)
    sim.destroy(); osim.close()


def test_cell_with_18_faces_is_refused():
    from waiwera_amd.flow_simulation import FlowSimulation
    lm, prim, region, coarse = wm.wide_case("we")
    c = coarse[len(coarse) // 2]                  # a middle-layer coarse cell: 14 faces
    fc = np.asarray(lm.face_cells)
    nbrs = set(fc[fc[:, 0] == c, 1]) | set(fc[fc[:, 1] == c, 0])
    far = [q for q in range(lm.n_owned) if q != c and q not in nbrs][:4]
    extra = np.array([(c, q) for q in far], dtype=np.int32)
    nb = lm.n_bc
    # interior faces first, boundary faces last (as build_mesh orders them)
    ni = lm.n_faces - nb
    lm.face_cells = np.concatenate([fc[:ni], extra, fc[ni:]]).astype(np.int32)
    g = np.asarray(lm.face_geom)
    lm.face_geom = np.concatenate([g[:ni], np.repeat(g[:1], len(far), axis=0), g[ni:]])
    lm.n_faces = lm.face_cells.shape[0]
    with pytest.raises(Exception, match="cell %d has 18 faces" % c):
        FlowSimulation(lm, eos="we")


@pytest.mark.parametrize("eos,prefix", [("we", "k_pc_park<"), ("wce", "k_pc_wave<")])
def test_seven_point_mesh_keeps_its_kernels(eos, prefix):
    from waiwera_amd.flow_simulation import FlowSimulation
    g, lm, prim, region = make_case(dims=(8, 8, 8), brick=(4, 4, 4), eos=eos)
    sim = FlowSimulation(lm, eos=eos)
    name = sim.pc_kernel_name()
    assert name.startswith(prefix) and "wide" not in name, name
    sim.destroy()


def test_wide_mesh_tracer_step(oracle):
    """one backward-Euler tracer step after a flow step: the assembled system (rows of up to 15 blocks by ELL slot) and
    its solution against the oracle"""
    eos, dt = "we", 1.0e4
    lm, sim, osim, y, coarse = wide_system(oracle, eos)
    rng = np.random.default_rng(13)
    nt = 1
    bc = rng.uniform(0, 1e-3, (lm.n_bc, nt))
    inj = np.where(np.asarray(lm.src_rate)[:, None] > 0, rng.uniform(0, 1e-2, (lm.n_src, nt)), 0.0)
    for s in (sim, osim):
        s.set_tracers([0], [1e-8], [0.0], [1e-6], bc=bc, injection=inj)
    sim.set_aux_solver("gmres", rtol=1e-12)
    sim.set_opts(ksp_rtol=1e-10, ftol_rel=1e-9)
    o = osim.opts()
    o.ksp_rtol, o.ftol_rel = 1e-10, 1e-9
    n = lm.n_owned * nt
    X0 = rng.uniform(0, 1e-3, n)
    yo = osim.yvec(y)
    assert sim.pre_eval(0.0, y) == 0 and osim.pre_eval(yo) == 0
    alx1 = osim.tracer_lhs() * X0
    reason, nits, kits = sim.timestep(0.0, dt, y)
    r, k = osim.timestep(yo, dt, o)
    assert reason > 0 and r > 0
    Ag, bg = sim.aux_system(0, "beuler", dt, 1.0, alx1, alx1)
    Ao, bo = osim.tracer_system(0, 0, dt, 1.0, alx1, alx1)
    assert np.abs(Ag - Ao).max() <= 1e-6 * np.abs(Ao).max()
    assert np.abs(bg - bo).max() <= 1e-6 * max(np.abs(bo).max(), 1e-300)
    Xg, newg = X0.copy(), np.zeros(n)
    rg, ig = sim.aux_solve("beuler", dt, 1.0, alx1, None, Xg, newg)
    Xo = X0.copy()
    ro, io, newo = osim.tracer_solve(0, dt, 1.0, alx1, None, Xo, ksp_type=1, rtol=1e-12)
    assert rg > 0 and ro > 0
    assert relmax(Xg, Xo) < 1e-6
    sim.destroy(); osim.close()


@pytest.mark.parametrize("eos", ["wce", "wsce"])
def test_wide_mesh_unparked_rows(oracle, eos):
    """one subdomain of all 438 rows (3 x 3 and 4 x 4 blocks): the upper blocks of the later rows do not fit the 64 KB of
    LDS and are re-read from the factor in the backward sweep -- both branches of k_pc_wide in one launch"""
    dt = 5.0e4
    lm, sim, osim, y, coarse = wide_system(oracle, eos, dt, chunk=1024)
    assert len(lm.sub_ptr) == 2 and sim.pc_kernel_name().startswith("k_pc_wide<")
    n = sim.num_dof
    yo = osim.yvec(y)
    assert osim.pre_eval(yo) == 0
    L = osim.lhs()
    err, f = osim.residual(yo, dt, L)
    err, J = osim.jacobian(yo, dt, L, f, mode=0)
    bs = BS[eos]
    rp, ci = osim.pattern()
    nup = sum(int((ci[rp[i]:rp[i + 1]] > i).sum()) for i in range(lm.n_owned))
    T = (lm.n_owned + 63) // 64 * 64
    assert nup * bs * bs * 8 > 64 * 1024 - (T * bs + 80) * 8        # not every row parks its upper blocks
    sim.set_jacobian_values(J)
    assert sim.pc_setup() == 0 and osim.pc_setup(J) == 0
    r = np.random.default_rng(17).normal(size=n)
    z = np.zeros(n)
    sim.pc_apply(r, z)
    assert relmax(z, osim.pc_apply(r)) < 1e-10
    sim.set_opts(ksp_rtol=1e-12)
    x = np.zeros(n)
    its, reason, rn = sim.ksp_solve(f, x)
    oreason, xo, oits, hist = osim.ksp_solve(J, f, rtol=1e-12)
    assert reason > 0 and oreason > 0
    assert relmax(x, xo[:n]) < 1e-8 and abs(its - oits) <= max(2, oits // 10), (its, oits)
    sim.destroy(); osim.close()


def test_wide_mesh_ilu_k_keeps_the_level_path(oracle):
    """ILU(k) fill on a wide mesh stays on the launch-per-level path (out of the fused kernel's scope)"""
    lm, sim, osim, y, coarse = wide_system(oracle, "we")
    sim.set_opts(pc_type="bjacobi", ilu_levels=1)
    assert sim.pre_eval(0.0, y) == 0
    L = np.zeros(sim.num_dof)
    sim.lhs(0.0, 1.0, y, L)
    assert sim.jacobian(0.0, 5.0e4, y, L) == 0
    assert sim.pc_setup() == 0
    assert "k_lvl_solve per level" in sim.pc_kernel_name() and "ILU(1)" in sim.pc_kernel_name(), sim.pc_kernel_name()
    sim.destroy(); osim.close()


SPLIT = 224     # a multiple of the subdomain size: both runs have the same block-Jacobi blocks


def _wide_rank_worker(rank, world, uid_q, q, lm, prim, region, eos, dts):
    from tests.test_hip_multirank import LOOPBACK, _default_overlap, _own_cus
    os.environ["WAI_RCCL_LIB"] = LOOPBACK
    _own_cus(rank, world)
    _default_overlap()
    from waiwera_amd import lib as wl
    from waiwera_amd.flow_simulation import FlowSimulation
    from waiwera_amd.partition import partition_mesh
    if rank == 0:
        uid = wl.comm_unique_id()
        for _ in range(world - 1):
            uid_q.put(uid)
    else:
        uid = uid_q.get(timeout=300)
    owner = (np.arange(lm.n_owned) >= SPLIT).astype(np.int64)
    lmr, gid = partition_mesh(lm, owner, rank, chunk=16, world=world)
    # rows with a partition-ghost column and more than 8 blocks: the face bricks hold wide rows
    N, H = lmr.n_owned, lmr.n_halo
    fc = np.asarray(lmr.face_cells)
    blocks = np.ones(N, dtype=int)
    ghost = np.zeros(N, dtype=bool)
    for a, b in fc:
        for u, v in ((a, b), (b, a)):
            if u < N and v < N + H:
                blocks[u] += 1
                ghost[u] |= v >= N
    wide_face_rows = int((ghost & (blocks > 8)).sum())
    sim = FlowSimulation(lmr, device=0, eos=eos)
    sim.set_regions(region[gid])
    sim.comm_init(rank, world, uid)
    name = sim.pc_kernel_name()
    y = np.ascontiguousarray(sim.scale(prim[gid], region[gid]).ravel())
    sim.set_opts(ksp_rtol=1e-12, ftol_rel=1e-10)
    hist, t = [], 0.0
    for dt in dts:
        hist.append(sim.timestep(t, dt, y))
        t += dt
    bs = sim.num_primary_variables
    q.put((rank, lmr.owned_gid.copy(), y[: N * bs].copy(), hist, name, wide_face_rows, H))
    sim.destroy()


@pytest.mark.timeout(900)
def test_wide_mesh_two_ranks():
    """the wide mesh split by partition_mesh over two ranks on the asynchronous test transport (the face bricks' rows
    have ghost columns and up to 15 blocks; k_pc_wide on the interior / face subdomain lists of the overlapped halo
    exchange): the same Newton counts and solution as one rank with the same subdomains"""
    import torch.multiprocessing as mp
    from waiwera_amd.flow_simulation import FlowSimulation
    eos, world = "we", 2
    lm, prim, region, coarse = wm.wide_case(eos, chunk=16)
    dts = [1.0e4, 3.0e4, 1.0e5]
    ser = FlowSimulation(lm, device=0, eos=eos)
    ser.set_regions(region)
    assert ser.pc_kernel_name() == "k_pc_wide<2,spmv>"
    y = np.ascontiguousarray(ser.scale(prim, region).ravel())
    ser.set_opts(ksp_rtol=1e-12, ftol_rel=1e-10)
    hist, t = [], 0.0
    for dt in dts:
        hist.append(ser.timestep(t, dt, y))
        t += dt
    assert all(h[0] > 0 for h in hist), hist
    ser.destroy()
    ctx = mp.get_context("spawn")
    q, uid_q = ctx.Queue(), ctx.Queue()
    procs = [ctx.Process(target=_wide_rank_worker, args=(r, world, uid_q, q, lm, prim, region, eos, dts)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    bs = 2
    ypar = np.zeros((lm.n_owned, bs))
    seen = np.zeros(lm.n_owned, dtype=int)
    for rank, gid, yy, h, name, wide_face_rows, n_halo in res:
        assert name == "k_pc_wide<2,spmv>" and n_halo > 0 and wide_face_rows > 0, (rank, name, wide_face_rows, n_halo)
        assert all(a[0] > 0 for a in h) and [a[1] for a in h] == [b[1] for b in hist], (h, hist)
        ypar[gid] = yy.reshape(-1, bs)
        seen[gid] += 1
    assert (seen == 1).all()
    yser = y[: lm.n_owned * bs].reshape(-1, bs)
    err = np.abs(ypar - yser).max(axis=0) / np.abs(yser).max(axis=0)
    assert err.max() < 1e-7, err


def test_json_input_with_polygon_columns(oracle, tmp_path):
    """a JSON input whose mesh is a MULgraph geometry with 12-node columns runs through Simulation to its end time; its
    first step agrees with the oracle's"""
    import json
    from waiwera_amd.mesh import liquid_density_estimate
    from waiwera_amd.simulation import Simulation
    xy, columns, coarse = wm.refined_plan()
    tops = [0.0, -100.0, -200.0, -300.0]
    wm.write_mulgraph(str(tmp_path / "gwide.dat"), xy, columns, tops)
    nc = len(columns)
    depth = np.repeat([50.0, 150.0, 250.0], nc)
    T = 20.0 + 0.05 * depth
    P = 1.0e5 + 9.8 * liquid_density_estimate(T) * depth
    n = 3 * nc
    inp = {
        "title": "polygon columns", "mesh": {"filename": "gwide.dat"}, "gravity": 9.8, "eos": {"name": "we"},
        "initial": {"region": 1, "primary": [[float(p), float(t)] for p, t in zip(P, T)]},
        "boundaries": [{"region": 1, "primary": [1.0e5, 20.0], "faces": {"cells": list(range(nc)), "normal": [0.0, 0.0, 1.0]}}],
        "source": [{"cell": nc + coarse[0], "rate": -2.0}, {"cell": 2 * nc + coarse[1], "rate": 1.0, "enthalpy": 1.0e5}],
        "rock": {"types": [{"name": "r", "porosity": 0.1, "permeability": [1e-13, 1e-13, 1e-14], "cells": list(range(n))}]},
        "time": {"start": 0.0, "stop": 7.0e4, "step": {"size": 1.0e4, "method": "beuler", "maximum": {"number": 20},
                 "adapt": {"on": False},
                 "solver": {"nonlinear": {"tolerance": {"function": {"relative": 1e-10, "absolute": 1e-12}}},
                            "linear": {"tolerance": {"relative": 1e-12}}}}},
        "output": {"initial": True, "frequency": 1, "final": True},
    }
    path = tmp_path / "polygon.json"
    path.write_text(json.dumps(inp))
    sim = Simulation.from_json(str(path), output_dir=str(tmp_path))
    assert sim.mesh.n_owned == n
    lm = sim.mesh
    osim = ol.OracleSim(oracle, lm, 1)
    osim.set_regions(np.ones(n, dtype=np.int32))
    yo = osim.yvec(scaled(np.column_stack([P, T]), np.ones(n, dtype=np.int32)).ravel().copy())
    out = sim.run()
    assert abs(out["time"] - 7.0e4) < 1e-6 and len(sim.outputs) >= 8
    assert "k_pc_wide" in sim.ode.pc_kernel_name(), sim.ode.pc_kernel_name()
    o = osim.opts()
    o.ksp_rtol, o.ftol_rel, o.ftol_abs = 1e-12, 1e-10, 1e-12
    onits, okits = osim.timestep(yo, 1.0e4, o)
    assert onits > 0
    first = sim.outputs[1]
    assert abs(first["time"] - 1.0e4) < 1e-6
    assert relmax(first["fluid_pressure"], yo[0: 2 * n: 2] * 1.0e6) < 1e-7
    assert relmax(first["fluid_temperature"], yo[1: 2 * n: 2] * 1.0e2) < 1e-7
    sim.ode.destroy(); osim.close()

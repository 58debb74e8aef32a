"""The coupled tracer solve on two ranks over the loop-back transport: the [cell][tracer] vector's ghost entries travel with
nt values per cell, the reductions are the drivers' own -- same solutions and same Al o X as one rank, to the multi-rank
tests' 1e-7 (tests/test_hip_multirank.py::test_tracer_solve_across_ranks, whose problem and helpers this reuses)."""
import multiprocessing as mp
import os

import numpy as np
import pytest

from tests import test_hip_multirank as T
from waiwera_amd import mesh as M
from waiwera_amd.cases import scaled

pytestmark = pytest.mark.gpu


def _run(sim, lm, y, ksp):
    """T._tracer_run with the auxiliary KSP type of choice (its own is GMRES)"""
    real = sim.set_aux_solver
    sim.set_aux_solver = lambda _ksp, *a: real(ksp, *a)
    try:
        return T._tracer_run(sim, lm, "we", y)
    finally:
        sim.set_aux_solver = real


def _coupled_worker(rank, world, uid_q, q, ksp):
    os.environ["WAI_RCCL_LIB"] = T.LOOPBACK
    T._own_cus(rank, world)
    T._default_overlap()
    from waiwera_amd import lib as wl
    from waiwera_amd.flow_simulation import FlowSimulation
    if rank == 0:
        uid = wl.comm_unique_id()
        for _ in range(world - 1):
            uid_q.put(uid)
    else:
        uid = uid_q.get(timeout=300)
    g, lm, prim, region = T._problem(M.partition_shape(world), rank)
    sim = FlowSimulation(lm, eos="we", device=0)
    sim.set_regions(region)
    sim.comm_init(rank, world, uid)
    sim.set_tracer_solve_mode("coupled")
    y = scaled(prim, region).ravel().copy()
    s0 = sim.tracer_assembly_sweeps()
    nits, out = _run(sim, lm, y, ksp)
    q.put((rank, lm.owned_gid.copy(), nits, out, sim.tracer_assembly_sweeps() - s0))
    sim.destroy()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("ksp", ["gmres", "bcgs"])
def test_coupled_tracer_solve_across_ranks(ksp):
    """GMRES: no inner products in the operator, the overlapped interior / face launches; BiCGStab: the products reduced
    behind the launch and all-reduced"""
    assert os.path.exists(T.LOOPBACK), "build first: python __graft_entry__.py"
    os.environ["WAI_RCCL_LIB"] = T.LOOPBACK
    from waiwera_amd.flow_simulation import FlowSimulation
    world = 2
    ctx = mp.get_context("spawn")
    q, uid_q = ctx.Queue(), ctx.Queue()
    procs = [ctx.Process(target=_coupled_worker, args=(r, world, uid_q, q, ksp)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=400) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    g, lm, prim, region = T._problem((1, 1, 1), 0)
    sim = FlowSimulation(lm, eos="we", device=0)
    sim.set_regions(region)
    sim.set_tracer_solve_mode("coupled")
    y = scaled(prim, region).ravel().copy()
    nits1, out1 = _run(sim, lm, y, ksp)
    sim.destroy()
    N, nt = g.n_global, 2
    for method in ("beuler", "bdf2"):
        Xs, As = np.zeros((N, nt)), np.zeros((N, nt))
        Xs[lm.owned_gid], As[lm.owned_gid] = out1[method][0], out1[method][1]
        Xp, Ap = np.zeros((N, nt)), np.zeros((N, nt))
        its = set()
        for rank, gid, nits, out, sweeps in res:
            assert nits == nits1 and sweeps == 2     # one sweep per solve, two solves
            Xp[gid], Ap[gid] = out[method][0], out[method][1]
            its.add(out[method][2])
        assert len(its) == 1 and its.pop() > 0       # ONE solve: every rank reports the same count
        ex = np.abs(Xp - Xs).max(axis=0) / np.abs(Xs).max(axis=0)
        ea = np.abs(Ap - As).max(axis=0) / np.abs(As).max(axis=0)
        print("coupled tracer solve on 2 ranks, %s: X %s, Al o X %s" % (method, ex, ea))
        assert ex.max() < 1e-7 and ea.max() < 1e-7, (method, ex, ea)

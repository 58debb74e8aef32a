"""The tracers' own preconditioner on two ranks over the loop-back transport: the flow solver under asm overlap 1 (the
overlapped blocks reach across the rank boundary), the tracers under block Jacobi, per tracer and coupled -- the same tracer
fields as the one-rank run to the solves' tolerance, the bounds of tests/test_hip_tracer_coupled_multirank.py (whose problem
and helpers, tests/test_hip_multirank.py's, this reuses)."""
import multiprocessing as mp
import os

import numpy as np
import pytest

from tests import test_hip_multirank as T
from waiwera_amd import mesh as M
from waiwera_amd.cases import scaled

pytestmark = pytest.mark.gpu


def _configure(sim, mode):
    sim.set_opts(pc_type="asm", asm_overlap=1)
    sim.set_aux_pc("bjacobi")
    sim.set_tracer_solve_mode(mode)


def _worker(rank, world, uid_q, q, mode):
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
    _configure(sim, mode)
    y = scaled(prim, region).ravel().copy()
    s0 = sim.tracer_assembly_sweeps()
    nits, out = T._tracer_run(sim, lm, "we", y)
    q.put((rank, lm.owned_gid.copy(), nits, out, sim.tracer_assembly_sweeps() - s0))
    sim.destroy()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("mode", ["per_tracer", "coupled"])
def test_flow_asm_tracers_bjacobi_across_ranks(mode):
    assert os.path.exists(T.LOOPBACK), "build first: python __graft_entry__.py"
    # (the ranks name the loop-back transport in their own processes: this process keeps its environment, and with it the
    # real librccl for the tests that run after this file)
    from waiwera_amd.flow_simulation import FlowSimulation
    world = 2
    ctx = mp.get_context("spawn")
    q, uid_q = ctx.Queue(), ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, uid_q, q, mode)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=400) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    g, lm, prim, region = T._problem((1, 1, 1), 0)
    sim = FlowSimulation(lm, eos="we", device=0)
    sim.set_regions(region)
    _configure(sim, mode)
    y = scaled(prim, region).ravel().copy()
    nits1, out1 = T._tracer_run(sim, lm, "we", y)
    sim.destroy()
    N, nt = g.n_global, 2
    for method in ("beuler", "bdf2"):
        Xs, As = np.zeros((N, nt)), np.zeros((N, nt))
        Xs[lm.owned_gid], As[lm.owned_gid] = out1[method][0], out1[method][1]
        Xp, Ap = np.zeros((N, nt)), np.zeros((N, nt))
        its = set()
        for rank, gid, nits, out, sweeps in res:
            assert nits == nits1
            assert sweeps == (2 if mode == "coupled" else 2 * nt)     # one sweep per coupled solve, nt per per-tracer solve; two solves
            Xp[gid], Ap[gid] = out[method][0], out[method][1]
            its.add(out[method][2])
        assert len(its) == 1 and its.pop() > 0       # every rank reports the same count
        ex = np.abs(Xp - Xs).max(axis=0) / np.abs(Xs).max(axis=0)
        ea = np.abs(Ap - As).max(axis=0) / np.abs(As).max(axis=0)
        print("flow asm, tracers bjacobi (%s) on 2 ranks, %s: X %s, Al o X %s" % (mode, method, ex, ea))
        assert ex.max() < 1e-7 and ea.max() < 1e-7, (method, ex, ea)

"""Sub-preconditioner lu on the device (wai_set_sub_pc, WAI_SUB_LU): the exact LU of every subdomain block under bjacobi,
of every overlapped block under asm, factored by k_sublu_factor and applied by k_sublu_solve -- against dense solves of
the same blocks on the host, beyond the dense path's 8192 unknowns, through the switch, on two ranks and from the input
front end."""
import json
import os

import numpy as np
import pytest

from tests.test_hip_pc import relmax, system

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
BS = {"w": 1, "we": 2, "wce": 3, "wsce": 4}
# pc_apply against numpy.linalg.solve of the same block: the project's figure for these matrices is cond ~ 6e10
# (tests/test_hip_pc.py::test_lu_blocks, which holds the dense inverses to the same bound)
TOL = 1e-6


def dense(sim, osim, J, bs):
    import scipy.sparse as sp
    n = sim.num_dof
    rp, ci = osim.pattern()
    return sp.bsr_matrix((J.reshape(-1, bs, bs), ci, rp), shape=(n, n)).toarray()


def block_jacobi_reference(A, sub, bs, r):
    ref = np.zeros_like(r)
    for a, b in zip(sub[:-1], sub[1:]):
        ref[bs * a:bs * b] = np.linalg.solve(A[bs * a:bs * b, bs * a:bs * b], r[bs * a:bs * b])
    return ref


def schwarz_reference(A, sub, bs, r, overlap):
    """restricted additive Schwarz with exact local solves: every brick's row set grown by `overlap` layers over the
    matrix graph, the dense sub-matrix solved on the gathered residual, the owned rows kept"""
    N = A.shape[0] // bs
    adj = np.abs(A.reshape(N, bs, N, bs)).sum(axis=(1, 3)) != 0
    ref = np.zeros_like(r)
    for a, b in zip(sub[:-1], sub[1:]):
        rows = np.zeros(N, dtype=bool)
        rows[a:b] = True
        for _ in range(overlap):
            rows |= adj[rows].any(axis=0)
        cells = np.nonzero(rows)[0]
        sc = (cells[:, None] * bs + np.arange(bs)).ravel()
        z = np.linalg.solve(A[np.ix_(sc, sc)], r[sc]).reshape(-1, bs)
        own = (cells >= a) & (cells < b)
        ref.reshape(N, bs)[cells[own]] = z[own]
    return ref


@pytest.mark.parametrize("eos,one_block", [("we", False), ("we", True), ("w", False), ("wce", False), ("wsce", False)])
def test_block_jacobi_with_exact_blocks(oracle, eos, one_block):
    """bjacobi + WAI_SUB_LU: every diagonal block solved exactly.  6 x 6 x 4 cells in 3 x 3 x 2 bricks (1 x 1 .. 4 x 4
    blocks) and, for eos we, as one block: BiCGStab then stops within two iterations at the dense solution.
    Tolerance 1e-6 relative (cond ~ 6e10); the figure and, for eos we, the dense inverses' on the same system are printed."""
    bs = BS[eos]
    lm, sim, osim, J, f = system(oracle, eos, (6, 6, 4), (6, 6, 4) if one_block else (3, 3, 2), one_block=one_block,
                                 lens=(eos == "we"))
    n = sim.num_dof
    A = dense(sim, osim, J, bs)
    sim.set_opts(pc_type="bjacobi", ksp_rtol=1e-10)
    sim.set_sub_pc("lu")
    assert sim.pc_setup() == 0
    assert "k_sublu_solve" in sim.pc_kernel_name() and "block Jacobi" in sim.pc_kernel_name(), sim.pc_kernel_name()
    r = np.random.default_rng(14).normal(size=n)
    z = np.zeros(n)
    sim.pc_apply(r, z)
    sub = [0, lm.n_owned] if one_block else list(lm.sub_ptr)
    err = relmax(z, block_jacobi_reference(A, sub, bs, r))
    if eos == "we":   # the parent's dense path on the same system, for the record
        sim.set_opts(pc_type="lu")
        zd = np.zeros(n)
        sim.pc_apply(r, zd)
        print("dense inverses (pc_type lu) on the same system:", relmax(zd, block_jacobi_reference(A, sub, bs, r)))
        sim.set_opts(pc_type="bjacobi")
    print(eos, "one block" if one_block else "bricks", "pc_apply vs numpy.linalg.solve:", err)
    assert err < TOL
    x = np.zeros(n)
    its, reason, rn = sim.ksp_solve(f, x)
    print("  BiCGStab", its, reason)
    assert reason > 0 and relmax(x, np.linalg.solve(A, f)) < 1e-5
    if one_block:
        assert its <= 2
    sim.destroy(); osim.close()


@pytest.mark.parametrize("one_block,overlap", [(False, 1), (False, 2), (True, 1)])
def test_overlapped_schwarz_with_exact_local_solves(oracle, one_block, overlap):
    """asm + WAI_SUB_LU against its definition on the host, and a whole Krylov solve: the dense solution, in no more
    iterations than asm + ILU(0) takes on the same system -- exact local solves cannot be weaker."""
    lm, sim, osim, J, f = system(oracle, "we", (6, 6, 4), (6, 6, 4) if one_block else (3, 3, 2), one_block=one_block)
    n = sim.num_dof
    A = dense(sim, osim, J, 2)
    sim.set_opts(pc_type="asm", asm_overlap=overlap, ksp_rtol=1e-10)
    x0 = np.zeros(n)
    its0, reason0, _ = sim.ksp_solve(f, x0)       # asm + ILU(0)
    assert reason0 > 0
    sim.set_sub_pc("lu")
    assert sim.pc_setup() == 0
    assert "k_sublu_solve" in sim.pc_kernel_name() and "ASM" in sim.pc_kernel_name(), sim.pc_kernel_name()
    r = np.random.default_rng(15).normal(size=n)
    z = np.zeros(n)
    sim.pc_apply(r, z)
    sub = [0, lm.n_owned] if one_block else list(lm.sub_ptr)
    err = relmax(z, schwarz_reference(A, sub, 2, r, overlap))
    print("asm overlap", overlap, "one block" if one_block else "bricks", "pc_apply vs the dense definition:", err)
    assert err < TOL
    x = np.zeros(n)
    its, reason, rn = sim.ksp_solve(f, x)
    print("  BiCGStab: sub lu", its, "ILU(0)", its0)
    assert reason > 0 and relmax(x, np.linalg.solve(A, f)) < 1e-5
    assert its <= its0
    sim.destroy(); osim.close()


def test_a_block_beyond_the_dense_limit(oracle):
    """one block of 64 x 66 x 1 cells, 8448 unknowns, natural-numbering half-bandwidth 64 blocks: the dense path refuses
    it, the device factorisation sets up and agrees with scipy's sparse LU (the vector stays in global memory here: it
    does not fit the 64 KB of LDS)."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    from waiwera_amd.flow_simulation import WaiError
    lm, sim, osim, J, f = system(oracle, "we", (64, 66, 1), (64, 66, 1), one_block=True)
    n = sim.num_dof
    assert n == 8448
    rp, ci = osim.pattern()
    band = max(abs(int(c) - i) for i in range(lm.n_owned) for c in ci[rp[i]:rp[i + 1]])
    assert band < 120, band
    sim.set_opts(pc_type="lu")
    with pytest.raises(WaiError, match="8192") as e:
        sim.pc_setup()
    assert "(-2)" in str(e.value)
    sim.set_opts(pc_type="bjacobi")
    sim.set_sub_pc("lu")
    assert sim.pc_setup() == 0
    r = np.random.default_rng(16).normal(size=n)
    z = np.zeros(n)
    sim.pc_apply(r, z)
    A = sp.bsr_matrix((J.reshape(-1, 2, 2), ci, rp), shape=(n, n)).tocsc()
    err = relmax(z, spl.splu(A).solve(r))
    print("8448 unknowns in one block, pc_apply vs scipy splu:", err)
    assert err < TOL
    sim.destroy(); osim.close()


def test_fill_beyond_the_row_cap_is_refused(oracle):
    """21 x 20 x 10 cells as one block: complete fill gives factor rows of more than 255 blocks.  Refused with -2, naming
    sub-preconditioner lu, the width found and the cap -- never an incomplete factor; the context then solves with
    ILU(0) as before."""
    from waiwera_amd.flow_simulation import WaiError
    lm, sim, osim, J, f = system(oracle, "we", (21, 20, 10), (21, 20, 10), one_block=True)
    n = sim.num_dof
    sim.set_opts(pc_type="bjacobi", ksp_rtol=1e-8)
    sim.set_sub_pc("lu")
    with pytest.raises(WaiError) as e:
        sim.pc_setup()
    text = str(e.value)
    assert "(-2)" in text and "sub-preconditioner lu" in text and "255" in text, text
    import re
    assert int(re.search(r"factor row of (\d+) blocks", text).group(1)) > 255
    sim.set_sub_pc("ilu")
    x = np.zeros(n)
    its, reason, rn = sim.ksp_solve(f, x)
    assert reason > 0
    oreason, xo, oits, hist = osim.ksp_solve(J, f, rtol=1e-8)
    assert relmax(x, xo) < 1e-5
    sim.destroy(); osim.close()


def test_switching_back_restores_ilu0_bit_for_bit(oracle):
    from waiwera_amd.cases import make_case, scaled
    from waiwera_amd.flow_simulation import FlowSimulation, WaiError
    from waiwera_amd.lib import LIB
    lm, sim, osim, J, f = system(oracle, "we", (6, 6, 4), (3, 3, 2))
    n = sim.num_dof
    r = np.random.default_rng(17).normal(size=n)
    z0, z1, z2 = np.zeros(n), np.zeros(n), np.zeros(n)
    sim.pc_apply(r, z0)
    sim.set_sub_pc("lu")
    sim.pc_apply(r, z1)
    assert relmax(z1, z0) > 1e-6      # another preconditioner
    sim.set_sub_pc("ilu")
    assert "sublu" not in sim.pc_kernel_name()
    sim.pc_apply(r, z2)
    assert np.array_equal(z2, z0)
    with pytest.raises(WaiError, match="unknown sub-preconditioner"):
        sim._chk(LIB.wai_set_sub_pc(sim.h, 7), "set_sub_pc")
    sim.destroy(); osim.close()
    # a time step after the round trip is the step of a context that never switched
    ys = []
    for switch in (False, True):
        g, lm, prim, region = make_case(dims=(6, 6, 4), brick=(3, 3, 2), eos="we", lens=True)
        s = FlowSimulation(lm, eos="we")
        s.set_regions(region)
        s.set_opts(ksp_rtol=1e-10, ftol_rel=1e-9)
        y = scaled(prim, region).ravel().copy()
        if switch:
            s.set_sub_pc("lu")
            reason, nits, kits = s.timestep(0.0, 1.0e4, y.copy())
            assert reason > 0
            s.set_sub_pc("ilu")
            s.set_regions(region)      # (the step above may have moved cells to another region)
        reason, nits, kits = s.timestep(0.0, 1.0e4, y)
        assert reason > 0
        ys.append((y, nits, kits))
        s.destroy()
    assert ys[0][1:] == ys[1][1:] and relmax(ys[1][0], ys[0][0]) < 1e-12


def test_coupled_tracer_mode_refuses_sub_lu():
    from tests.test_hip_tracer_coupled import Case
    from waiwera_amd.flow_simulation import WaiError
    c = Case("we", 2)
    sim = c.sim
    sim.set_tracer_solve_mode("coupled")
    sim.set_sub_pc("lu")
    with pytest.raises(WaiError) as e:
        sim.aux_solve("beuler", c.dt, 1.0, c.alx1, None, c.X0.copy(), np.zeros(c.n))
    assert "(-2)" in str(e.value) and "WAI_SUB_LU" in str(e.value) and "coupled" in str(e.value), str(e.value)
    sim.set_sub_pc("ilu")      # ... and the context is usable afterwards
    sim.aux_solve("beuler", c.dt, 1.0, c.alx1, None, c.X0.copy(), np.zeros(c.n))


# ---- two ranks on the loop-back transport -------------------------------------------------------------------------------

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
    sim = FlowSimulation(lm, eos="we", device=0)
    sim.set_regions(region)
    sim.comm_init(rank, world, uid)
    sim.set_opts(pc_type="asm", asm_overlap=1, ksp_rtol=1e-12)
    sim.set_sub_pc("lu")
    q.put((rank,) + _solve(sim, lm, prim, region))
    sim.destroy()


def _solve(sim, lm, prim, region):
    from waiwera_amd.cases import scaled
    y = scaled(prim, region, "we").ravel().copy()
    n = lm.n_owned * 2
    dt = 2.0e4
    assert sim.pre_eval(0.0, y) == 0
    L, f = np.zeros(n), np.zeros(n)
    sim.lhs(0.0, (0.0, 0.0), y, L)
    assert sim.residual(dt, dt, y, L, f) == 0
    assert sim.jacobian(dt, dt, y, L) == 0
    assert sim.pc_setup() == 0
    x = np.zeros(n)
    its, reason, rn = sim.ksp_solve(f, x)
    return lm.owned_gid.copy(), x, its, reason, sim.pc_kernel_name()


@pytest.mark.timeout(600)
def test_two_ranks_match_one_rank():
    """asm overlap 1 + WAI_SUB_LU with the overlapped blocks reaching across the rank boundary (the ghost cells' rows come
    from their owners): the Krylov solution of two ranks is the one-rank solution to 1e-7"""
    import torch.multiprocessing as mp
    from tests import test_hip_multirank as T
    from waiwera_amd.cases import make_case
    from waiwera_amd.flow_simulation import FlowSimulation
    assert os.path.exists(T.LOOPBACK), "build first: python __graft_entry__.py"
    dims, brick, world = (8, 6, 4), (4, 3, 2), 2
    ctx = mp.get_context("spawn")
    q, uid_q = ctx.Queue(), ctx.Queue()
    procs = [ctx.Process(target=_two_rank_worker, args=(r, world, uid_q, q, dims, brick)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    g, lm, prim, region = make_case(dims=dims, brick=brick, eos="we", lens=True)
    sim = FlowSimulation(lm, eos="we", device=0)
    sim.set_regions(region)
    sim.set_opts(pc_type="asm", asm_overlap=1, ksp_rtol=1e-12)
    sim.set_sub_pc("lu")
    gid1, x1, its1, reason1, name = _solve(sim, lm, prim, region)
    sim.destroy()
    assert reason1 > 0 and "k_sublu_solve" in name
    xs = np.zeros((g.n_global, 2))
    xs[gid1] = x1.reshape(-1, 2)
    worst = 0.0
    for rank, gid, x, its, reason, rname in res:
        assert reason > 0 and "k_sublu_solve" in rname
        worst = max(worst, np.abs(x.reshape(-1, 2) - xs[gid]).max() / np.abs(xs).max())
    print("asm + sub lu, two ranks against one: %.2e (iterations %s, one rank %d)" % (worst, [r[3] for r in res], its1))
    assert worst < 1e-7


# ---- the input front end --------------------------------------------------------------------------------------------------

def test_front_end_maps_sub_lu_to_the_device(tmp_path):
    """an input that asks for sub-preconditioner lu under the (default) asm preconditioner: sub_lu="device" keeps asm with
    overlap 1 and sets WAI_SUB_LU, says so in pc_choice, and ends at the fields of the default mapping (dense inverses,
    no overlap) to the tolerance the benchmarks compare preconditioners at"""
    from waiwera_amd.simulation import Simulation
    inp = json.load(open(os.path.join(INPUTS, "problem1.json")))
    lin = inp["time"]["step"].setdefault("solver", {}).setdefault("linear", {})
    lin.setdefault("preconditioner", {})["sub"] = {"preconditioner": {"type": "lu"}}
    a = Simulation(inp, base_dir=INPUTS, output_dir=str(tmp_path), sub_lu="device")
    assert a.pc_choice[:2] == ("asm", "reference default") and "on the device" in a.pc_choice[2], a.pc_choice
    assert "k_sublu_solve" in a.ode.pc_kernel_name() and "ASM" in a.ode.pc_kernel_name()
    b = Simulation(inp, base_dir=INPUTS, output_dir=str(tmp_path))
    assert "dense block inverses" in b.pc_choice[2] and "overlap is dropped" in b.pc_choice[2], b.pc_choice
    assert "k_lu_apply" in b.ode.pc_kernel_name()
    oa, ob = a.run(), b.run()
    assert a.ts.taken == b.ts.taken
    for k in ("fluid_pressure", "fluid_temperature"):
        sc = max(np.abs(ob[k]).max(), 1e-300)
        assert np.abs(oa[k] - ob[k]).max() <= 1e-4 * sc, k
    a.ode.destroy(); b.ode.destroy()

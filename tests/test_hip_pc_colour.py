"""Block-Jacobi ILU(0) in multicolour order (wai_set_pc_ordering) on the device, against the long-double reference of
tests/colour_reference.py: the fused launch k_pc_colour, the launch-per-colour path k_colour_sweep, one against the other,
whole Krylov solves against the oracle's solves of the symmetrically permuted system, a time step, the round trip back to
the natural order, the refusals, the tracers and two ranks.

Bars (tests/test_hip_fused_operator.py's Checker): z within 1e-12 of max |z_ref|, an inner product within 1e-13 of
sum |a_i b_i|.  Fused against sweeps: 1e-10 of max |z| (tests/test_hip_asm_fused.py's bar between a fused launch and the
launches it replaces)."""
import os
import types

import numpy as np
import pytest
import torch.multiprocessing as mp

from oracle import binding as ol
from tests import colour_reference as cr
from tests import fused_reference as fr
from tests import test_hip_fused_operator as fo
from tests import test_hip_memory as tm
from tests import test_hip_multirank as mr
from tests import wide_mesh
from waiwera_amd.cases import make_case, scaled
from waiwera_amd.lib import WaiError

pytestmark = pytest.mark.gpu

KIND, BS = fo.KIND, fo.BS
SWEEPS = "k_spmv + k_colour_sweep per colour (block Jacobi, multicolour ILU(0))"


def fused_name(bs):
    return "k_pc_colour<%d,spmv>" % bs


def relmax(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300)


class ColourChecker(fo.Checker):
    """Checker on the multicolour reference"""

    def __init__(self, sim, rp, ci, sub, bs, val, label):
        super().__init__(sim, rp, ci, sub, bs, val, label)
        self.ref = cr.ColourILU0(rp, ci, val, bs, sub)


def colour_sim(lm, eos):
    from waiwera_amd.flow_simulation import FlowSimulation
    sim = FlowSimulation(lm, eos=eos)
    sim.set_pc_ordering("multicolour")
    return sim


# id: (eos, dims, brick, make_case extras)
FUSED = {
    "w": ("w", (6, 6, 4), (3, 3, 2), {}),
    "we": ("we", (6, 6, 4), (3, 3, 2), {}),
    "wce": ("wce", (6, 6, 4), (3, 3, 2), {}),
    "wsce": ("wsce", (6, 6, 4), (3, 3, 2), {}),
    "we_bench_brick": ("we", (20, 18, 5), (16, 16, 2), {}),     # a full 512-row brick beside ragged ones
    "wce_minc": ("wce", (8, 4, 2), (4, 4, 1), {"minc": True}),
}


@pytest.mark.parametrize("case", list(FUSED))
def test_fused_launch_against_long_double_reference(case):
    """z = B^-1 x and z = B^-1 A x, dot modes 0 - 4, finished in the launch and by k_finalize; a composed operand and the
    interior / face split are refused"""
    eos, dims, brick, extra = FUSED[case]
    bs = BS[eos]
    g, lm, prim, region = make_case(dims=dims, brick=brick, eos=eos, **extra)
    sim = colour_sim(lm, eos)
    rp, ci = sim.setup_jacobian()
    sub = np.asarray(lm.sub_ptr)
    val = fr.random_values(rp, ci, bs, np.random.default_rng(12))
    ck = ColourChecker(sim, rp, ci, sub, bs, val, (case, "random"))
    assert sim.pc_kernel_name() == fused_name(bs), sim.pc_kernel_name()
    assert sim.pc_ordering() == ("multicolour", 2)
    assert not sim.pc_axpy_capable()
    with pytest.raises(WaiError):
        ck.apply(x2=ck.x2)
    with pytest.raises(WaiError):
        ck.apply(split=True)
    for tag, spmv in (("B^-1 x", False), ("B^-1 A x", True)):
        ck.variant(tag, spmv, False, False)
    ck.local_input(sub, rp, ci)
    ck.report(sim.pc_kernel_name())
    sim.destroy()


def one_block_case():
    g, lm, prim, region = make_case(dims=(20, 18, 5), brick=(16, 16, 2), eos="we")
    lm.sub_ptr = np.array([0, lm.n_owned], dtype=np.int32)
    return lm, "we"


def triangle_case():
    return fr.triangle_mesh("we")[1], "we"


def wide_case():
    return wide_mesh.wide_case()[0], "we"


SWEEP_CASES = {"one_block_1800": (one_block_case, 2), "triangles": (triangle_case, None), "wide_rows": (wide_case, None)}


@pytest.mark.parametrize("case", list(SWEEP_CASES))
def test_sweeps_against_long_double_reference(case):
    """the launch-per-colour path where the fused launch does not serve: a subdomain of 1800 rows, a cell graph with
    triangles (off-diagonal updates in the factor), rows of 15 blocks; 2 max_colours - 1 sweep launches per application"""
    make, want_colours = SWEEP_CASES[case]
    lm, eos = make()
    bs = BS[eos]
    sim = colour_sim(lm, eos)
    rp, ci = sim.setup_jacobian()
    sub = np.asarray(lm.sub_ptr)
    val = fr.random_values(rp, ci, bs, np.random.default_rng(12))
    ck = ColourChecker(sim, rp, ci, sub, bs, val, (case, "random"))
    assert sim.pc_kernel_name() == SWEEPS, sim.pc_kernel_name()
    ordering, colours = sim.pc_ordering()
    assert ordering == "multicolour" and colours == int(ck.ref.ncolours.max())
    if want_colours is not None:
        assert colours == want_colours
    else:
        assert colours >= 3
    assert ck.ref.offdiag_updates == (case != "one_block_1800")
    for tag, spmv in (("B^-1 x", False), ("B^-1 A x", True)):
        ck.variant(tag, spmv, False, False)
    r, z = ck.x.copy(), np.zeros(ck.x.size)
    k0, _ = sim.launch_stats()
    sim.pc_apply(r, z)
    k1, _ = sim.launch_stats()
    assert k1 - k0 == 2 * colours - 1, (k1 - k0, colours)
    assert fo.relerr(z, ck.ref.solve(r)) <= 1e-12
    ck.report(sim.pc_kernel_name())
    sim.destroy()


@pytest.mark.parametrize("case", ["we", "wce", "we_bench_brick", "wce_minc"])
def test_fused_against_sweeps(case, monkeypatch):
    """the same factor applied by the launches the fused one replaces (WAI_COLOUR_SWEEPS=1): within 1e-10; fused again
    afterwards: the bits it gave first"""
    eos, dims, brick, extra = FUSED[case]
    bs = BS[eos]
    g, lm, prim, region = make_case(dims=dims, brick=brick, eos=eos, **extra)
    sim = colour_sim(lm, eos)
    rp, ci = sim.setup_jacobian()
    sim.set_jacobian_values(fr.random_values(rp, ci, bs, np.random.default_rng(12)))
    n = len(rp) - 1
    rng = np.random.default_rng(5)
    r, x = rng.normal(size=n * bs), fr.spread_vector(n, bs, rng)
    out = {}
    for path in ("fused", "sweeps", "again"):
        if path == "sweeps":
            monkeypatch.setenv("WAI_COLOUR_SWEEPS", "1")
        if path == "again":
            monkeypatch.delenv("WAI_COLOUR_SWEEPS")
        assert sim.pc_setup() == 0
        assert sim.pc_kernel_name() == (SWEEPS if path == "sweeps" else fused_name(bs)), (path, sim.pc_kernel_name())
        z = np.zeros(n * bs)
        sim.pc_apply(r, z)
        out[path] = (z, sim.pc_operator(x, spmv=True)[0])
    for a, b in zip(out["fused"], out["sweeps"]):
        print(case, "fused against sweeps", relmax(a, b))
        assert relmax(a, b) < 1e-10
    for a, b in zip(out["fused"], out["again"]):
        assert np.array_equal(a, b)
    sim.destroy()


_systems = {}


def system(oracle, eos="we", dims=(12, 10, 9), brick=(4, 4, 2)):
    """mesh, FD Jacobian and right-hand side of the case's state: computed once and shared, never modified"""
    key = (eos, dims, brick)
    if key not in _systems:
        g, lm, prim, region = make_case(dims=dims, brick=brick, eos=eos, lens=(eos == "we"))
        rp, ci, J = fo.fd_jacobian(oracle, lm, eos, prim, region)
        osim = ol.OracleSim(oracle, lm, KIND[eos])
        osim.set_regions(region)
        yo = osim.yvec(scaled(prim, region, eos).ravel().copy())
        assert osim.pre_eval(yo) == 0
        err, f = osim.residual(yo, 5.0e4, osim.lhs())
        osim.close()
        _systems[key] = dict(lm=lm, prim=prim, region=region, rp=rp, ci=ci, J=J, f=f)
    return _systems[key]


def permuted_oracle(oracle, S, eos):
    """the oracle on the mesh renumbered by P (every brick's cells by (colour, cell)): its pattern is P J P^T's and its
    natural-order block ILU(0) on the same bricks is the multicolour factor.  Returns (osim, new, src)"""
    lm, rp, ci = S["lm"], S["rp"], S["ci"]
    sub = np.asarray(lm.sub_ptr)
    new = cr.permutation(cr.greedy_colours(rp, ci, sub), sub)
    prp, pci, src = cr.permuted_csr(rp, ci, new)
    fc = np.asarray(lm.face_cells).copy()
    own = fc < lm.n_owned
    fc[own] = new[fc[own]]
    old = np.argsort(new)
    pm = types.SimpleNamespace(n_owned=lm.n_owned, n_halo=lm.n_halo, n_bc=lm.n_bc, n_faces=lm.n_faces, face_cells=fc.astype(np.int32),
                               face_geom=lm.face_geom, cell_geom=np.asarray(lm.cell_geom)[old], rock=np.asarray(lm.rock)[old],
                               bc_primary=lm.bc_primary, bc_region=lm.bc_region, n_src=0, sub_ptr=lm.sub_ptr)
    assert lm.n_halo == 0
    osim = ol.OracleSim(oracle, pm, KIND[eos])
    orp, oci = osim.pattern()
    assert np.array_equal(orp, prp) and np.array_equal(oci, pci)
    return osim, new, src


@pytest.mark.parametrize("ksp,kt", [("bcgs", 0), ("gmres", 1)])
def test_whole_solves_against_the_oracle(oracle, ksp, kt):
    """BiCGStab and GMRES under the fused multicolour launch at rtol 1e-10 against the oracle's solves of P J P^T y = P f with
    its block ILU(0) on the same bricks; the bars of tests/test_hip_asm_fused.py::test_whole_solves_against_the_oracle"""
    eos, bs = "we", 2
    S = system(oracle, eos)
    n = len(S["rp"]) - 1
    sim = colour_sim(S["lm"], eos)
    sim.set_regions(S["region"])
    sim.set_opts(ksp_type=ksp, ksp_rtol=1e-10)
    sim.set_jacobian_values(S["J"])
    assert sim.pc_setup() == 0 and sim.pc_kernel_name() == fused_name(bs)
    osim, new, src = permuted_oracle(oracle, S, eos)
    Jp = np.asarray(S["J"]).reshape(-1, bs, bs)[src].ravel()
    fp = np.zeros(n * bs)
    fp.reshape(n, bs)[new] = np.asarray(S["f"]).reshape(n, bs)
    x = np.zeros(n * bs)
    its, reason, rn = sim.ksp_solve(S["f"], x)
    oreason, xo, oits, hist = osim.ksp_solve(Jp, fp, ksp_type=kt, rtol=1e-10)
    xo = xo.reshape(n, bs)[new].ravel()
    print(ksp, "its", its, oits, "reason", reason, oreason, "x", relmax(x, xo))
    assert reason > 0 and reason == oreason, (reason, oreason)
    assert abs(its - oits) <= 1, (its, oits)
    assert relmax(x, xo) < 1e-7
    sim.destroy(); osim.close()


def test_bicgstab_iteration_is_four_launches(oracle):
    """one BiCGStab iteration under k_pc_colour: fused A P, S = R - alpha V, fused A S, the X / R / P update -- the count
    tests/test_hip_asm_fused.py asserts for k_pc_wide's four-launch form"""
    S = system(oracle, "we")
    n = len(S["rp"]) - 1
    sim = colour_sim(S["lm"], "we")
    sim.set_regions(S["region"])
    sim.set_opts(ksp_type="bcgs", ksp_rtol=1e-10)
    sim.set_jacobian_values(S["J"])
    assert sim.pc_setup() == 0 and sim.pc_kernel_name() == fused_name(2) and not sim.bcgs_composed()
    x = np.zeros(n * 2)
    k0, c0 = sim.launch_stats()
    its, reason, rn = sim.ksp_solve(S["f"], x)
    k1, c1 = sim.launch_stats()
    print("BiCGStab under k_pc_colour: %d launches in %d iterations" % (k1 - k0, its))
    assert reason > 0 and its >= 5
    assert 4 * its <= k1 - k0 <= 4 * its + 8, (its, k1 - k0)
    sim.destroy()


def test_timestep_against_the_natural_order():
    """one backward-Euler step at ksp_rtol 1e-12, ftol_rel 1e-9: the Newton iterates do not depend on the preconditioner --
    the natural order's Newton count, its solution within 1e-9 relative"""
    from waiwera_amd.flow_simulation import FlowSimulation
    res = {}
    for tag in ("natural", "multicolour"):
        g, lm, prim, region = make_case(dims=(8, 8, 6), brick=(4, 4, 2), eos="we", lens=True)
        sim = FlowSimulation(lm, eos="we")
        sim.set_regions(region)
        sim.set_pc_ordering(tag)
        sim.set_opts(ksp_rtol=1e-12, ftol_rel=1e-9)
        y = scaled(prim, region, "we").ravel().copy()
        reason, nits, kits = sim.timestep(0.0, 1.0e4, y)
        name = sim.pc_kernel_name()
        assert reason > 0 and name.startswith("k_pc_colour") == (tag == "multicolour"), (tag, reason, name)
        res[tag] = (nits, y.reshape(-1, 2).copy(), kits)
        sim.destroy()
    print("timestep: Newton", res["natural"][0], res["multicolour"][0], "Krylov", res["natural"][2], res["multicolour"][2])
    assert res["natural"][0] == res["multicolour"][0]
    yn, ym = res["natural"][1], res["multicolour"][1]
    err = np.abs(ym - yn).max(axis=0) / np.abs(yn).max(axis=0)
    print("timestep: multicolour against natural", err)
    assert err.max() < 1e-9, err


@pytest.mark.parametrize("mesh", ["box", "triangles"])
def test_round_trip(mesh):
    """natural -> multicolour -> natural: the last application equals that of a context that never switched, bit for bit,
    and the kernel name is back"""
    from waiwera_amd.flow_simulation import FlowSimulation
    if mesh == "box":
        g, lm, prim, region = make_case(dims=(12, 10, 9), brick=(4, 4, 2), eos="we")
    else:
        g, lm, prim, region = fr.triangle_mesh("we")
    sim, never = FlowSimulation(lm, eos="we"), FlowSimulation(lm, eos="we")
    rp, ci = sim.setup_jacobian()
    n = len(rp) - 1
    val = fr.random_values(rp, ci, 2, np.random.default_rng(12))
    x = fr.spread_vector(n, 2, np.random.default_rng(3))
    for s in (sim, never):
        s.set_jacobian_values(val)
        assert s.pc_setup() == 0
    name0 = sim.pc_kernel_name()
    assert sim.pc_ordering() == ("natural", 0)
    z0 = sim.pc_operator(x, spmv=True)[0]
    sim.set_pc_ordering("multicolour")
    assert sim.pc_ordering() == ("multicolour", 0)      # no set-up under multicolour yet
    zc = sim.pc_operator(x, spmv=True)[0]
    ordering, colours = sim.pc_ordering()
    assert (colours == 2) if mesh == "box" else (colours >= 3), colours
    assert sim.pc_kernel_name() != name0 and "colour" in sim.pc_kernel_name()
    assert not np.array_equal(zc, z0)                   # another preconditioner
    ref = cr.ColourILU0(rp, ci, val, 2, np.asarray(lm.sub_ptr))
    assert fo.relerr(zc, ref.operator(val, x)) <= 1e-12
    sim.set_pc_ordering("natural")
    z1 = sim.pc_operator(x, spmv=True)[0]
    assert sim.pc_kernel_name() == name0 == never.pc_kernel_name()
    assert np.array_equal(z1, never.pc_operator(x, spmv=True)[0]) and np.array_equal(z1, z0)
    sim.destroy(); never.destroy()


def test_refusals():
    """what the ordering does not combine with is refused by the set-up with -2, the setting's name and the other party's;
    the context is usable afterwards.  Value 7 is unknown"""
    from waiwera_amd import lib as wl
    g, lm, prim, region = make_case(dims=tm.DIMS, brick=tm.BRICK, eos="we", lens=True)
    sim = colour_sim(lm, "we")
    sim.set_regions(region)
    n = sim.num_dof
    y = scaled(prim, region, "we").ravel().copy()
    L, r = np.zeros(n), np.zeros(n)
    assert sim.pre_eval(0.0, y) == 0
    sim.lhs(0.0, (0.0, 0.0), y, L)
    assert sim.residual(0.0, tm.DT, y, L, r) == 0 and sim.jacobian(0.0, tm.DT, y, L) == 0
    assert sim.pc_setup() == 0

    def refused(party):
        with pytest.raises(WaiError) as e:
            sim.pc_setup()
        msg = str(e.value)
        assert "(-2)" in msg and "wai_set_pc_ordering" in msg and "WAI_PC_ORDER_MULTICOLOUR" in msg and party in msg, msg

    sim.set_opts(pc_type="asm")
    refused("WAI_PC_ASM")
    sim.set_opts(pc_type="bjacobi", ilu_levels=1)
    refused("ilu_levels")
    sim.set_opts(ilu_levels=0)
    sim.set_sub_pc("lu")
    refused("WAI_SUB_LU")
    sim.set_sub_pc("ilu")
    assert sim.pc_setup() == 0 and sim.pc_kernel_name() == fused_name(2)
    for pc in ("none", "lu"):                 # ignored there
        sim.set_opts(pc_type=pc)
        assert sim.pc_setup() == 0
    sim.set_opts(pc_type="bjacobi")
    with pytest.raises(WaiError) as e:
        sim._chk(wl.LIB.wai_set_pc_ordering(sim.h, 7), "set_pc_ordering")
    assert "(-2)" in str(e.value) and "unknown" in str(e.value)
    with pytest.raises(ValueError):
        sim.set_pc_ordering("red-black")
    assert sim.pc_ordering()[0] == "multicolour"
    # the source network's blocks inside the factor's pattern
    controls, spec = tm.network(lm)
    sim.set_source_controls(controls)
    sim.set_source_network(spec)
    assert sim.pre_eval(0.0, y) == 0
    sim.lhs(0.0, (0.0, 0.0), y, L)
    assert sim.residual(0.0, tm.DT, y, L, r) == 0 and sim.jacobian(0.0, tm.DT, y, L) == 0
    cells, E = sim.network_couplings()
    assert len(cells) > 0 and np.abs(E).max() > 0
    refused("source-network")
    sim.set_network_couplings(True, in_preconditioner=False)      # in the operator only: served, by the unfused product
    assert sim.pc_setup() == 0
    x = np.zeros(n)
    its, reason, rn = sim.ksp_solve(r, x)
    assert reason > 0 and np.isfinite(x).all()
    sim.destroy()


def test_tracers_keep_the_natural_order():
    """the same fluid state in both contexts (pre_eval of one y, no flow solve): per tracer and coupled, the multicolour
    context's tracer solves are the natural-order context's bit for bit -- before and after a multicolour flow set-up"""
    from waiwera_amd.flow_simulation import FlowSimulation
    g, lm, prim, region = make_case(dims=tm.DIMS, brick=tm.BRICK, eos="we", lens=True)
    y = scaled(prim, region, "we").ravel().copy()
    sols = {}
    for tag in ("natural", "multicolour"):
        sim = FlowSimulation(lm, eos="we")
        sim.set_regions(region)
        sim.set_pc_ordering(tag)
        n = sim.num_dof
        L = np.zeros(n)
        assert sim.pre_eval(0.0, y) == 0
        sim.lhs(0.0, (0.0, 0.0), y, L)
        assert sim.jacobian(0.0, tm.DT, y, L) == 0 and sim.pc_setup() == 0      # the flow factor in force, in its order
        tr = tm.Tracers(sim, lm, 2)
        res = []
        for mode in ("per_tracer", "coupled"):
            sim.set_tracer_solve_mode(mode)
            X, new = tr.X0.copy(), np.zeros(tr.n)
            reason, its = sim.aux_solve("beuler", 1.0e3, 1.0, tr.alx, tr.alx, X, new)
            assert reason > 0
            res.append((its, X.copy()))
        assert sim.pc_setup() == 0 and ("colour" in sim.pc_kernel_name()) == (tag == "multicolour")
        sols[tag] = res
        sim.destroy()
    for (ia, xa), (ib, xb) in zip(sols["natural"], sols["multicolour"]):
        assert ia == ib and np.array_equal(xa, xb)


def _colour_worker(rank, world, uid_q, q):
    os.environ["WAI_RCCL_LIB"] = mr.LOOPBACK
    mr._own_cus(rank, world)
    mr._default_overlap()
    from waiwera_amd import lib as wl
    from waiwera_amd import mesh as M
    from waiwera_amd.flow_simulation import FlowSimulation
    if rank == 0:
        uid = wl.comm_unique_id()
        for _ in range(world - 1):
            uid_q.put(uid)
    else:
        uid = uid_q.get(timeout=300)
    g, lm, prim, region = mr._problem(M.partition_shape(world), rank)
    sim = FlowSimulation(lm, eos="we", device=0)
    sim.set_regions(region)
    sim.comm_init(rank, world, uid)
    sim.set_pc_ordering("multicolour")
    y = scaled(prim, region).ravel().copy()
    hist = mr._run_steps(sim, y, 1)
    q.put((rank, lm.owned_gid.copy(), y[: lm.n_owned * 2].copy(), hist, sim.pc_kernel_name(), sim.pc_ordering()))
    sim.destroy()


@pytest.mark.timeout(600)
def test_two_ranks_match_one_rank():
    """two ranks on the loop-back transport (bricks never straddle ranks: the same preconditioner) take the launch-per-colour
    path with the operator's halo exchange in front of it, and reproduce the one-rank step: same Newton count, solution to
    1e-7 (the bar of tests/test_hip_multirank.py for block Jacobi)"""
    from waiwera_amd.flow_simulation import FlowSimulation
    world = 2
    assert os.path.exists(mr.LOOPBACK), "build first: python __graft_entry__.py"
    ctx = mp.get_context("spawn")
    q, uid_q = ctx.Queue(), ctx.Queue()
    procs = [ctx.Process(target=_colour_worker, args=(r, world, uid_q, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=400) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    g, lm, prim, region = mr._problem((1, 1, 1), 0)
    sim = FlowSimulation(lm, eos="we", device=0)
    sim.set_regions(region)
    sim.set_pc_ordering("multicolour")
    y = scaled(prim, region).ravel().copy()
    hist = mr._run_steps(sim, y, 1)
    assert sim.pc_kernel_name() == fused_name(2)
    yser = np.zeros((g.n_global, 2))
    yser[lm.owned_gid] = y[: lm.n_owned * 2].reshape(-1, 2)
    sim.destroy()
    ypar = np.zeros((g.n_global, 2))
    for rank, gid, yy, h, name, (ordering, colours) in res:
        assert name == SWEEPS and ordering == "multicolour" and colours == 2, (rank, name, colours)
        assert h[0][0] > 0 and h[0][1] == hist[0][1], (rank, h, hist)
        ypar[gid] = yy.reshape(-1, 2)
    err = np.abs(ypar - yser).max(axis=0) / np.abs(yser).max(axis=0)
    print("two ranks against one:", err, "Krylov", [h[0][2] for _, _, _, h, _, _ in res], hist[0][2])
    assert err.max() < 1e-7, err

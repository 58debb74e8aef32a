"""The two-level preconditioner's coarse level (wai_set_pc_coarse) on the device, one launch at a time against the long-double
reference of tests/coarse_reference.py (pinned on the CPU by tests/test_coarse_reference.py), then whole applications,
solves, the switch and the front end.

Bounds.  Nothing is tuned to what the device returns.
- restrict, prolong: purely additive, so the derivable bound is used: |error| <= k eps sum |terms|, k the aggregate's size
  (k = 1 for the prolongation's one addition; the prolongation that only writes is exact).
- GEMV, Galerkin, inverse, one application: the bound is the error of the float64 numpy restatement of the same formula
  (coarse_reference with dtype=float64) against the long-double reference ON THE SAME CASE, times 4 -- the factor for a
  different but legitimate order of summation.  Both errors are maxima over all entries, relative to the largest entry of
  the reference.  The restatement is of the whole formula: its one-level part M^-1 is the matrix of the long-double
  one-level solve, each entry rounded to double once, applied and summed in double (coarse_reference.TwoLevel.Minv).  No
  fixed term is added anywhere.
- inner products: |error| <= n eps sum |a_i b_i| for the summation, plus sum |a_i| times the bound on z where z is a factor.
- solves: the two-level solution is held to the one-level one within the solve's own rtol, |x2 - x1| <= rtol |x1|, as the
  issue states it.  (Both solves end on |B^-1 (b - A x)| <= rtol |B^-1 b|, which bounds the distance by
  (cond(B1^-1 A) + cond(B2^-1 A)) rtol |x|; that figure, about 3 rtol on this system, is printed beside the assertion.)  Each
  two-level solve's own criterion is evaluated by the reference too, with 5 % for the recurrence's rounding.

MEASURED on the CPU (the restatement's errors, this file's cases; the bound is 4 x):

    case                        GEMV      Galerkin   inverse    |Ac Ainv - I|inf
    6x5x3, 7 aggregates  w      1.2e-16   3.7e-16    6.1e-17    2.4e-16
                         we     1.6e-16   1.3e-15    1.7e-16    5.4e-16
                         wce    1.6e-16   2.4e-16    1.9e-16    5.9e-16
                         wsce   5.1e-17   7.1e-16    2.1e-16    6.1e-16
    16x16x8, 512 aggr.   we     4.8e-16   3.1e-16    --         3.6e-15   (residual in double on both sides)
    wide mesh, 5 aggr.   we     --        7.5e-16    1.9e-16    2.1e-16
    one application, 8x8x4 we, 8 boxes (wai_pc_apply's r; the drivers' x as B^-1 x; as B^-1 A x):
                                          bjacobi ILU(0)  additive 3.7e-16 1.8e-16 2.1e-16  deflated 1.9e-16 1.9e-16 2.6e-16
                                          asm overlap 1   additive 1.5e-16 1.8e-16 1.6e-16  deflated 2.4e-16 1.4e-16 3.2e-16
                                          bjacobi ILU(1)  additive 2.2e-16 1.7e-16 3.9e-16  deflated 3.4e-16 1.2e-16 2.3e-16

MEASURED on the device (MI355X; every test prints its figures before it asserts): GEMV between 0.85 and 2.5 of the
restatement's error (worst 2.5: wsce, 1.3e-16 of a bound of 2.0e-16); Galerkin 0.03 to 0.67 of it; the inverse the
restatement's own figure to three digits (the same elimination order); wai_pc_apply 2.0e-16 to 4.1e-16, 0.13 to 0.51 of its
bound; the drivers' applications at most 0.75 of theirs; restriction at most 0.19 of its derived bound.  Solves, rtol 1e-9:
|x2 - x1| / |x1| 1.3e-10 to 8.5e-10, under the rtol asserted (the condition-number figure is 3.1e-9 to 4.2e-9).  Iterations on the
64 x 1 x 1 case: BiCGStab 37 / 17 / 10, GMRES(30) 489 / 18 / 12 (one level / additive / deflated).

Iteration counts of the reference (numpy GMRES(30) and BiCGStab on the float64 restatement, 64 x 1 x 1 eos w without a top
boundary, 4-cell subdomains, 8 aggregates of 8 cells, dt 1e6, b = default_rng(5).normal, rtol 1e-5), checked before this case
was committed:  GMRES one level 477, additive 18, deflated 12;  BiCGStab one level 38, additive 16, deflated 10.  (With the
top boundary on every cell of a one-layer mesh the rows keep 6 % of diagonal excess, information does not travel and the
additive mode takes MORE iterations than one level -- 15 against 12: the case needs the boundary off.)"""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import asm_reference as ar
from tests import coarse_reference as cr
from tests import fused_reference as fr
from tests import test_hip_memory as tm
from tests import test_hip_multirank as mr
from tests import wide_mesh
from waiwera_amd.cases import make_case, scaled
from waiwera_amd.flow_simulation import FlowSimulation, box_aggregates
from waiwera_amd.lib import WaiError

pytestmark = pytest.mark.gpu

LD = cr.LD
EPS = float(np.finfo(np.float64).eps)
BS = {"w": 1, "we": 2, "wce": 3, "wsce": 4}
GUARD = 24
SENTINEL = -7.25e300
INPUTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inputs")


def uneven_aggregates(n=90):
    """7 uneven aggregates of the 6 x 5 x 3 mesh, scattered: 65 cells (more than a wave), one cell, 5, 4, 6, 3, 6"""
    sizes = [65, 1, 5, 4, 6, 3, 6]
    assert sum(sizes) == n
    agg = np.repeat(np.arange(len(sizes)), sizes)
    return agg[np.random.default_rng(17).permutation(n)].astype(np.int32), len(sizes)


def context(eos, dims, brick, seed=3, **kw):
    """(sim, rowptr, colidx, random O(1) values set as the Jacobian, lm)"""
    g, lm, prim, region = make_case(dims=dims, brick=brick, eos=eos, lens=False, **kw)
    sim = FlowSimulation(lm, eos=eos)
    rp, ci = sim.setup_jacobian()
    val = fr.random_values(rp, ci, BS[eos], np.random.default_rng(seed))
    sim.set_jacobian_values(val)
    return sim, np.asarray(rp), np.asarray(ci), val, lm


def small(eos):
    sim, rp, ci, val, lm = context(eos, (6, 5, 3), (3, 5, 3))
    agg, nc = uneven_aggregates()
    return sim, rp, ci, val, agg, nc


def cap():
    """16 x 16 x 8 with 512 aggregates of 2 x 2 x 1 cells at bs 2: nc bs = 1024, the cap"""
    sim, rp, ci, val, lm = context("we", (16, 16, 8), (8, 8, 4))
    agg = box_aggregates(lm.owned_ijk, (8, 8, 8))
    assert agg.max() + 1 == 512
    return sim, rp, ci, val, agg, 512


def relmax(got, ref):
    ref = np.asarray(ref, dtype=LD)
    return float(np.abs(np.asarray(got, dtype=LD) - ref).max() / max(np.abs(ref).max(), LD(1e-300)))


def guarded(host, fill=None):
    """a device vector with GUARD sentinels behind it"""
    t = torch.full((host.size + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    t[:host.size] = torch.from_numpy(np.ascontiguousarray(host)) if fill is None else fill
    torch.cuda.synchronize()
    return t


def run_alone(sim, what, vin, n_out, out0=None):
    """one launch through wai_test_coarse on guarded device vectors, twice: (result, same bits both times, untouched)"""
    res = []
    for _ in range(2):
        tin = guarded(vin)
        tout = guarded(np.zeros(n_out) if out0 is None else out0, fill=None if out0 is not None else float("nan"))
        sim.test_coarse(what, tin, tout)
        sim.synchronize()
        hin, hout = tin.cpu().numpy(), tout.cpu().numpy()
        assert np.array_equal(hin[:vin.size], vin) and np.all(hin[vin.size:] == SENTINEL), what      # input and its guards untouched
        assert np.all(hout[n_out:] == SENTINEL), what                                                # nothing written behind n
        res.append(hout[:n_out].copy())
    assert np.array_equal(res[0], res[1]), what
    return res[0]


CASES_ALONE = [("small", e) for e in ("w", "we", "wce", "wsce")] + [("cap", "we")]


@pytest.mark.parametrize("mesh,eos", CASES_ALONE)
def test_restrict_gemv_prolong_alone(mesh, eos):
    sim, rp, ci, val, agg, nc = small(eos) if mesh == "small" else cap()
    bs, n = BS[eos], len(rp) - 1
    m = nc * bs
    sim.set_pc_coarse("additive", aggregates=agg)
    assert sim.pc_coarse() == ("additive", nc)
    rng = np.random.default_rng(23)
    r = fr.spread_vector(n, bs, rng)
    # restrict: exact to k eps sum |terms|
    rc = run_alone(sim, "restrict", r, m)
    ref = cr.restrict(agg, nc, bs, r)
    bar = cr.restrict(agg, nc, bs, np.abs(r)) * np.repeat(np.bincount(agg, minlength=nc), bs) * LD(EPS)
    err = np.abs(rc.astype(LD) - ref)
    print(mesh, eos, "restrict worst error / bound", float((err / np.maximum(bar, LD(1e-300))).max()))
    assert np.all(err <= bar)
    # a host vector takes the same launch: same bits
    out = np.zeros(m)
    sim.test_coarse("restrict", r, out)
    assert np.array_equal(out, rc)
    # prolong: the write is exact, the addition one rounding
    yc = rng.normal(size=m)
    t = run_alone(sim, "prolong_set", yc, n * bs)
    assert np.array_equal(t, cr.prolong(agg, bs, yc).astype(np.float64))
    z0 = fr.spread_vector(n, bs, rng)
    z = run_alone(sim, "prolong_add", yc, n * bs, out0=z0)
    want = z0.astype(LD) + cr.prolong(agg, bs, yc)
    assert np.all(np.abs(z.astype(LD) - want) <= LD(EPS) * (np.abs(z0) + np.abs(cr.prolong(agg, bs, yc))))
    # GEMV on the inverse the device holds: 4 x the double restatement's error
    Ainv = np.zeros(m * m)
    assert sim.test_coarse("ainv", None, Ainv) == 0
    Ainv = Ainv.reshape(m, m)
    yd = run_alone(sim, "gemv", rc, m)
    ref = cr.matvec(Ainv, rc)
    e64 = relmax(cr.matvec(Ainv, rc, dtype=np.float64), ref)
    e = relmax(yd, ref)
    print(mesh, eos, "gemv restatement %.2e bound %.2e device %.2e" % (e64, 4 * e64, e))
    assert e64 > 0 and e <= 4 * e64
    sim.destroy()


def wide_context():
    lm = wide_mesh.wide_case()[0]
    sim = FlowSimulation(lm, eos="we")
    rp, ci = sim.setup_jacobian()
    rp, ci = np.asarray(rp), np.asarray(ci)
    assert int(np.diff(rp).max()) == 15
    val = fr.random_values(rp, ci, 2, np.random.default_rng(4))
    sim.set_jacobian_values(val)
    n = len(rp) - 1
    return sim, rp, ci, val, (np.arange(n) * 5 // n).astype(np.int32), 5


def download(sim, m):
    Ac, Ainv = np.zeros(m * m), np.zeros(m * m)
    assert sim.test_coarse("ac", None, Ac) == 0 and sim.test_coarse("ainv", None, Ainv) == 0
    return Ac.reshape(m, m), Ainv.reshape(m, m)


@pytest.mark.parametrize("mesh,eos", CASES_ALONE + [("wide", "we")])
def test_galerkin_and_inverse(mesh, eos):
    sim, rp, ci, val, agg, nc = wide_context() if mesh == "wide" else (small(eos) if mesh == "small" else cap())
    bs = BS[eos]
    m = nc * bs
    sim.set_pc_coarse("deflated", aggregates=agg)
    assert sim.pc_setup() == 0
    Ac, Ainv = download(sim, m)
    # Galerkin, entry by entry
    ref = cr.galerkin(rp, ci, val, bs, agg, nc)
    e64 = relmax(cr.galerkin(rp, ci, val, bs, agg, nc, dtype=np.float64), ref)
    e = relmax(Ac, ref)
    print(mesh, eos, "galerkin restatement %.2e bound %.2e device %.2e" % (e64, 4 * e64, e))
    assert e <= 4 * e64
    assert np.array_equal(Ac == 0.0, np.asarray(ref == 0))       # the blocks outside the coarse pattern are exact zeros
    # two set-ups on the same values: the same bits
    sim.set_jacobian_values(val)
    assert sim.pc_setup() == 0
    Ac2, Ainv2 = download(sim, m)
    assert np.array_equal(Ac, Ac2) and np.array_equal(Ainv, Ainv2)
    # the inverse of the matrix the device holds
    eye = np.eye(m)
    if mesh == "cap":
        # (1024 unknowns: a long-double elimination takes minutes, so this case is reduced to the residual, both sides evaluated
        # in double; the entry-by-entry comparison with the long-double inverse runs on the other cases)
        r64 = cr.inverse(Ac, dtype=np.float64)
        res64 = float(np.abs(Ac @ r64 - eye).sum(axis=1).max())
        res = float(np.abs(Ac @ Ainv - eye).sum(axis=1).max())
    else:
        ref = cr.inverse(Ac)
        r64 = cr.inverse(Ac, dtype=np.float64)
        e64, e = relmax(r64, ref), relmax(Ainv, ref)
        print(mesh, eos, "inverse restatement %.2e bound %.2e device %.2e" % (e64, 4 * e64, e))
        assert e <= 4 * e64
        AcL = Ac.astype(LD)
        res64 = float(np.abs(AcL @ r64.astype(LD) - eye).sum(axis=1).max())
        res = float(np.abs(AcL @ Ainv.astype(LD) - eye).sum(axis=1).max())
    print(mesh, eos, "|Ac Ainv - I|inf restatement %.2e bound %.2e device %.2e" % (res64, 4 * res64, res))
    assert res <= 4 * res64
    sim.destroy()


def ending(sim, n):
    """wai_pc_setup -> 1; wai_ksp_solve -> reason -11 after 0 iterations with x = 0 and rnorm 0 (tests/test_hip_solve_endings.py)"""
    assert sim.pc_setup() == 1
    x = np.full(n, 7.0)
    its, reason, rn = sim.ksp_solve(np.ones(n), x)
    assert (its, reason, rn) == (0, -11, 0.0) and np.all(x == 0.0)
    z = np.full(n, 7.0)
    assert sim.pc_apply(np.ones(n), z) == 1 and np.all(z == 7.0)      # nothing applied


def test_singular_coarse_matrix():
    sim, rp, ci, val, agg, nc = small("we")
    n = (len(rp) - 1) * 2
    sim.set_pc_coarse("additive", aggregates=agg)
    assert sim.pc_setup() == 0
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    V = val.reshape(-1, 2, 2).copy()
    V[agg[rows] == 4] = 0.0           # every fine row of aggregate 4: zero blocks
    sim.set_jacobian_values(V.ravel())
    ending(sim, n)
    # the values back: the same context sets up and solves again
    sim.set_jacobian_values(val)
    assert sim.pc_setup() == 0
    x = np.zeros(n)
    assert sim.ksp_solve(np.ones(n), x)[1] > 0
    sim.destroy()


def test_singular_coarse_matrix_under_a_regular_fine_one():
    """A is regular and its ILU(0) pivots invert, but the entries of one aggregate's rows sum to zero column aggregate by
    column aggregate: 8 x 1 x 1, scalar, aggregate 0 = cells {0, 1} with rows (2, -1) and (-3, 2, 0): the block's determinant is
    1, ILU(0)'s pivots are 2 and 0.5, and row 0 of Ac is (2 - 1 - 3 + 2, 0) = exact zeros"""
    g, lm, prim, region = make_case(dims=(8, 1, 1), brick=(4, 1, 1), eos="w", lens=False, top_bc=False)
    sim = FlowSimulation(lm, eos="w")
    rp, ci = sim.setup_jacobian()
    rp, ci = np.asarray(rp), np.asarray(ci)
    rows = np.repeat(np.arange(8), np.diff(rp))
    val = np.where(ci == rows, 4.0, -1.0)
    val[(rows == 0) & (ci == 0)], val[(rows == 0) & (ci == 1)] = 2.0, -1.0
    val[(rows == 1) & (ci == 0)], val[(rows == 1) & (ci == 1)], val[(rows == 1) & (ci == 2)] = -3.0, 2.0, 0.0
    agg = (np.arange(8) // 2).astype(np.int32)
    assert not cr.galerkin(rp, ci, val, 1, agg, 4)[0].any()
    sim.set_jacobian_values(val)
    assert sim.pc_setup() == 0        # one level: every pivot inverts
    sim.set_pc_coarse("deflated", aggregates=agg)
    ending(sim, 8)
    sim.destroy()


APPLY = {"bjacobi_ilu0": dict(pc_type="bjacobi", ilu_levels=0), "asm_overlap1": dict(pc_type="asm", asm_overlap=1, ilu_levels=0),
         "bjacobi_ilu1": dict(pc_type="bjacobi", ilu_levels=1)}


def one_level_reference(name, rp, ci, val, bs, sub):
    if name == "bjacobi_ilu0":
        return fr.BlockILU0(rp, ci, val, bs, sub)
    return ar.AsmRef(ar.AsmPattern(rp, ci, sub, 1 if name == "asm_overlap1" else 0, levels=1 if name == "bjacobi_ilu1" else 0), val, bs)


@pytest.mark.parametrize("name", list(APPLY))
def test_one_application(name):
    """wai_pc_apply and the drivers' pc_amul / pc_solve with every dot mode, both modes, against the long-double reference"""
    sim, rp, ci, val, lm = context("we", (8, 8, 4), (4, 4, 2))
    bs, n = 2, len(rp) - 1
    agg = box_aggregates(lm.owned_ijk, (2, 2, 2))
    sim.set_opts(**APPLY[name])
    one = one_level_reference(name, rp, ci, val, bs, np.asarray(lm.sub_ptr))
    hi = cr.TwoLevel(rp, ci, val, bs, agg, 8, one.solve)
    lo = cr.TwoLevel(rp, ci, val, bs, agg, 8, one.solve, dtype=np.float64)
    rng = np.random.default_rng(31)
    r, x, aux = (fr.spread_vector(n, bs, rng) for _ in range(3))
    scal_in = np.zeros(16)
    for mode in ("additive", "deflated"):
        sim.set_pc_coarse(mode, aggregates=agg)
        z = np.zeros(n * bs)
        assert sim.pc_apply(r, z) == 0
        zref = hi.apply(mode, r)
        e64 = relmax(lo.apply(mode, r), zref)
        bound = 4 * e64
        e = relmax(z, zref)
        print(name, mode, "apply restatement %.2e bound %.2e device %.2e" % (e64, bound, e))
        assert e <= bound
        z2 = np.zeros(n * bs)
        sim.pc_apply(r, z2)
        assert np.array_equal(z, z2)
        for spmv in (False, True):
            zref = hi.operator(mode, x) if spmv else hi.apply(mode, x)
            e64 = relmax(lo.operator(mode, x) if spmv else lo.apply(mode, x), zref)
            zbound = 4 * e64 * float(np.abs(zref).max())
            for dot_mode in range(5):
                for phase in (-2, -1):
                    zd, s = sim.pc_operator(x, dot_mode=dot_mode, aux=aux if dot_mode in (1, 4) else None, spmv=spmv,
                                            fin_phase=phase, scal_in=scal_in)
                    print(name, mode, "spmv" if spmv else "solve", dot_mode, phase, "restatement %.2e bound %.2e device %.2e" % (e64, 4 * e64, relmax(zd, zref)))
                    assert np.abs(zd.astype(LD) - zref).max() <= zbound, (name, mode, spmv, dot_mode, phase)
                    for slot, a, b in fr.mode_products(dot_mode, x.astype(LD), zref, aux):
                        d, bar = fr.dot(a, b)
                        tol = n * bs * EPS * float(bar)
                        for v, w in ((a, b), (b, a)):
                            if v is zref:
                                tol += float(np.abs(np.asarray(w, dtype=LD)).sum()) * zbound
                        if a is zref and b is zref:
                            tol += n * bs * zbound ** 2
                        assert abs(s[slot] - float(d)) <= tol, (name, mode, spmv, dot_mode, phase, slot, s[slot], float(d), tol)
        with pytest.raises(WaiError):      # no composed operand, no interior / face split beside a coarse level
            sim.pc_operator(x, x2=aux, alpha=0.3)
    sim.destroy()


def dense_operator(T, n):
    """the operator x -> T(x) as a matrix, column by column"""
    return np.stack([np.asarray(T(e), dtype=np.float64) for e in np.eye(n)], axis=1)


@pytest.fixture(scope="module")
def solve_case():
    """a random system of 8 x 8 x 2 cells of 2 x 2 blocks in 4 x 4 x 2 bricks, 2 x 2 x 1 boxes; both references; cond(B^-1 A)"""
    sim, rp, ci, val, lm = context("we", (8, 8, 2), (4, 4, 2), seed=9)
    n = (len(rp) - 1) * 2
    agg = box_aggregates(lm.owned_ijk, (2, 2, 1))
    one = fr.BlockILU0(rp, ci, val, 2, np.asarray(lm.sub_ptr))
    hi = cr.TwoLevel(rp, ci, val, 2, agg, 4, one.solve)
    cond = {"one": float(np.linalg.cond(dense_operator(lambda e: one.solve(hi.spmv(e)), n)))}
    for mode in ("additive", "deflated"):
        cond[mode] = float(np.linalg.cond(dense_operator(lambda e: hi.operator(mode, e), n)))
    b = np.random.default_rng(41).normal(size=n)
    yield sim, agg, hi, one, cond, b
    sim.destroy()


@pytest.mark.parametrize("ksp", ["bcgs", "gmres"])
@pytest.mark.parametrize("mode", ["additive", "deflated"])
def test_solves_reach_the_one_level_solution(solve_case, ksp, mode):
    sim, agg, hi, one, cond, b = solve_case
    rtol = 1e-9
    sim.set_opts(ksp_type=ksp, ksp_rtol=rtol)
    sim.set_pc_coarse("off")
    x1 = np.zeros(b.size)
    its1, reason1, _ = sim.ksp_solve(b, x1)
    sim.set_pc_coarse(mode, aggregates=agg)
    x2 = np.zeros(b.size)
    its2, reason2, _ = sim.ksp_solve(b, x2)
    assert reason1 > 0 and reason2 > 0
    # the two-level solve's own criterion, evaluated by the reference
    res = hi.apply(mode, b.astype(LD) - hi.spmv(x2))
    crit = float(np.sqrt((res * res).sum()) / np.sqrt((hi.apply(mode, b) ** 2).sum()))
    diff = float(np.linalg.norm(x2 - x1) / np.linalg.norm(x1))
    bound = (cond["one"] + cond[mode]) * rtol
    print(ksp, mode, "its one level %d two level %d; criterion %.2e of rtol %.0e; |x2 - x1| / |x1| %.2e bound %.2e (cond %.1f, %.1f)"
          % (its1, its2, crit, rtol, diff, bound, cond["one"], cond[mode]))
    assert crit <= 1.05 * rtol
    assert diff <= rtol


@pytest.mark.parametrize("ksp", ["bcgs", "gmres"])
def test_fewer_iterations_than_one_level(ksp):
    """64 x 1 x 1 eos w, 4-cell subdomains, 8 aggregates, no boundary, dt 1e6: the flux terms dominate the accumulation, one
    level passes information one subdomain per application (the reference's counts: the module docstring)"""
    g, lm, prim, region = make_case(dims=(64, 1, 1), brick=(4, 1, 1), eos="w", lens=False, top_bc=False)
    sim = FlowSimulation(lm, eos="w")
    sim.set_regions(region)
    y = scaled(prim, region, "w").ravel().copy()
    L = np.zeros(sim.num_dof)
    assert sim.pre_eval(0.0, y) == 0
    sim.lhs(0.0, (0.0, 0.0), y, L)
    assert sim.jacobian(0.0, 1.0e6, y, L) == 0
    sim.set_opts(ksp_type=ksp, ksp_rtol=1e-5, ksp_max_its=1000)
    b = np.random.default_rng(5).normal(size=64)
    agg = box_aggregates(lm.owned_ijk, (8, 1, 1))
    its = {}
    for mode in ("off", "additive", "deflated"):
        sim.set_pc_coarse(mode, aggregates=None if mode == "off" else agg)
        x = np.zeros(64)
        its[mode], reason, _ = sim.ksp_solve(b, x)
        assert reason > 0, (mode, reason)
    print(ksp, "iterations", its)
    assert its["additive"] < its["off"] and its["deflated"] < its["off"]
    sim.destroy()


def test_switching_and_refusals():
    sim, rp, ci, val, lm = context("we", (8, 8, 4), (4, 4, 2))
    n = (len(rp) - 1) * 2
    agg = box_aggregates(lm.owned_ijk, (2, 2, 2))
    r = fr.spread_vector(len(rp) - 1, 2, np.random.default_rng(2))
    z0, z1, z2 = np.zeros(n), np.zeros(n), np.zeros(n)
    assert sim.pc_coarse() == ("off", 0)
    sim.pc_apply(r, z0)
    name = sim.pc_kernel_name()
    k0 = sim.launch_stats()[0]
    x = np.zeros(n)
    its0 = sim.ksp_solve(r, x)[0]
    per_it_one = (sim.launch_stats()[0] - k0) / max(its0, 1)
    sim.set_pc_coarse("additive", boxes=(2, 2, 2))
    assert sim.pc_coarse() == ("additive", 8)
    sim.pc_apply(r, z1)
    assert not np.array_equal(z0, z1)
    # off again: the one-level bits, the one-level kernel and its launches per iteration
    sim.set_pc_coarse("off")
    assert sim.pc_coarse() == ("off", 0)
    sim.pc_apply(r, z2)
    assert np.array_equal(z0, z2) and sim.pc_kernel_name() == name
    k0 = sim.launch_stats()[0]
    x2 = np.zeros(n)
    its2 = sim.ksp_solve(r, x2)[0]
    assert its2 == its0 and np.array_equal(x, x2) and (sim.launch_stats()[0] - k0) / max(its2, 1) == per_it_one

    def refused(text, call):
        with pytest.raises(WaiError) as e:
            call()
        msg = str(e.value)
        assert "(-2)" in msg and "wai_set_pc_coarse" in msg and text in msg, msg
        assert sim.pc_coarse() == ("off", 0)         # what was in force stays in force
        sim.pc_apply(r, z2)
        assert np.array_equal(z0, z2)

    from waiwera_amd import lib as wl
    bad = agg.copy()
    bad[3] = 8
    refused("agg[3] = 8 is outside [0, nc = 8)", lambda: sim._chk(wl.LIB.wai_set_pc_coarse(sim.h, 1, 8, bad.ctypes.data_as(wl.pi)), "set_pc_coarse"))
    refused("aggregate 7 is empty", lambda: sim.set_pc_coarse("additive", aggregates=np.where(agg == 7, 8, agg)))
    many = (np.arange(256) * 2).astype(np.int32)
    many[-1] = 512          # nc = 513 at bs 2: the cap is looked at before anything else
    refused("nc * bs = 1026 coarse unknowns, more than 1024", lambda: sim.set_pc_coarse("additive", aggregates=many))
    with pytest.raises(WaiError) as e:
        sim._chk(wl.LIB.wai_set_pc_coarse(sim.h, 5, 8, agg.ctypes.data_as(wl.pi)), "set_pc_coarse")
    assert "(-2)" in str(e.value) and "unknown" in str(e.value)
    for pc, text in (("none", "WAI_PC_NONE"), ("lu", "WAI_PC_LU")):
        sim.set_opts(pc_type=pc)
        with pytest.raises(WaiError) as e:
            sim.set_pc_coarse("deflated", aggregates=agg)
        assert "(-2)" in str(e.value) and text in str(e.value)
        assert sim.pc_coarse() == ("off", 0)
    sim.set_opts(pc_type="bjacobi")
    sim.set_pc_ordering("multicolour")
    with pytest.raises(WaiError) as e:
        sim.set_pc_coarse("additive", aggregates=agg)
    assert "(-2)" in str(e.value) and "WAI_PC_ORDER_MULTICOLOUR" in str(e.value)
    sim.set_pc_ordering("natural")
    # set first, met later: the set-up refuses the same way
    sim.set_pc_coarse("additive", aggregates=agg)
    sim.set_opts(pc_type="lu")
    with pytest.raises(WaiError) as e:
        sim.pc_setup()
    assert "(-2)" in str(e.value) and "wai_set_pc_coarse" in str(e.value) and "WAI_PC_LU" in str(e.value)
    sim.set_opts(pc_type="bjacobi")
    assert sim.pc_setup() == 0
    sim.set_pc_coarse("off")
    # tracers: the auxiliary systems
    sim.set_tracers([0])
    with pytest.raises(WaiError) as e:
        sim.set_pc_coarse("additive", aggregates=agg)
    assert "(-2)" in str(e.value) and "tracer" in str(e.value)
    with pytest.raises(ValueError):
        sim.set_pc_coarse("multiplicative", aggregates=agg)
    with pytest.raises(ValueError):
        sim.set_pc_coarse("additive")
    sim.destroy()


def test_source_network_is_refused():
    g, lm, prim, region = make_case(dims=tm.DIMS, brick=tm.BRICK, eos="we", lens=True)
    sim = FlowSimulation(lm, eos="we")
    sim.set_regions(region)
    controls, spec = tm.network(lm)
    sim.set_source_controls(controls)
    sim.set_source_network(spec)
    with pytest.raises(WaiError) as e:
        sim.set_pc_coarse("additive", aggregates=np.zeros(lm.n_owned, dtype=np.int32))
    assert "(-2)" in str(e.value) and "source-network couplings" in str(e.value)
    sim.destroy()


def _rank_worker(rank, world, uid_q, q):
    os.environ["WAI_RCCL_LIB"] = mr.LOOPBACK
    mr._own_cus(rank, world)
    from waiwera_amd import lib as wl
    from waiwera_amd import mesh as M
    if rank == 0:
        uid = wl.comm_unique_id()
        for _ in range(world - 1):
            uid_q.put(uid)
    else:
        uid = uid_q.get(timeout=300)
    g, lm, prim, region = mr._problem(M.partition_shape(world), rank)
    sim = FlowSimulation(lm, eos="we", device=0)
    sim.comm_init(rank, world, uid)
    try:
        sim.set_pc_coarse("additive", aggregates=np.zeros(lm.n_owned, dtype=np.int32))
        q.put((rank, "accepted"))
    except WaiError as e:
        q.put((rank, str(e)))
    sim.destroy()


@pytest.mark.timeout(300)
def test_more_than_one_rank_is_refused():
    assert os.path.exists(mr.LOOPBACK), "build first: python __graft_entry__.py"
    ctx = mp.get_context("spawn")
    q, uid_q = ctx.Queue(), ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, uid_q, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=200) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, msg in res:
        assert "(-2)" in msg and "more than one rank" in msg, (rank, msg)


def test_front_end_problem5a():
    """problem 5a with pc_coarse="additive" ends where the one-level run ends, within the bar tests/test_hip_input.py holds two
    preconditioners to (1e-4 of each field: the Newton tolerance's reach), and says what it ran"""
    from waiwera_amd.simulation import Simulation
    path = os.path.join(INPUTS, "problem5a.json")
    a = Simulation.from_json(path)
    b = Simulation.from_json(path, pc_coarse="additive", coarse_aggregates=8)
    mode, nc = b.ode.pc_coarse()
    assert mode == "additive" and 8 <= nc <= 16
    assert b.pc_choice[:2] == a.pc_choice[:2] and b.pc_choice[-1] == "coarse level additive over %d aggregates (wai_set_pc_coarse)" % nc
    assert a.ode.pc_coarse() == ("off", 0)
    oa, ob = a.run(), b.run()
    assert a.ts.taken == b.ts.taken == 200
    for k in ("fluid_pressure", "fluid_temperature", "fluid_vapour_saturation"):
        sc = max(np.abs(oa[k]).max(), 1e-300)
        assert np.abs(oa[k] - ob[k]).max() <= 1e-4 * sc, k
    a.ode.destroy(); b.ode.destroy()
    with pytest.raises(ValueError):
        Simulation.from_json(path, pc_coarse="multiplicative")

"""tests/solve_endings_reference.py pinned before any GPU run (no GPU here): the block_inverse restatement and the
rank-deficient blocks it must flag; singular_at; the prescribed systems' stated properties; the long-double BiCGStab and
GMRES restatements against numpy.linalg.solve and on every ending they state; and the measurement the GPU tests' bounds
rest on -- how far the double-precision run of a restatement lies from its long-double run after k <= 5 iterations
(printed with -s; tests/test_hip_solve_endings.py quotes the figures and takes ten times them)."""
import numpy as np
import pytest

from tests import fused_reference as fr
from tests import solve_endings_reference as se
from waiwera_amd.cases import make_case

LD = se.LD
BS = se.BS


def box(eos):
    return se.box(eos)


@pytest.fixture(scope="module")
def dominant():
    """{(eos, pc): (A values, b, M, B^-1 b, dense A)} of the pinned systems (se.dominant: the ones the GPU tests run)"""
    out = {}
    for eos in ("w", "we", "wce", "wsce"):
        for pc in ("bjacobi", "none"):
            d = se.dominant(eos, pc)
            out[eos, pc] = (d["val"], d["b"], d["M"], d["rb"], se.dense(d["rp"], d["ci"], d["val"], d["bs"], np.float64))
    return out


@pytest.mark.parametrize("bs", [1, 2, 3, 4])
def test_block_inverse_flags_the_pinned_singular_blocks_and_no_sound_one(bs):
    inv, ok = se.block_inverse(se.SINGULAR[bs])
    assert not ok
    assert np.linalg.matrix_rank(se.SINGULAR[bs]) < bs
    assert np.all(se.SINGULAR[bs] == np.round(se.SINGULAR[bs])) and np.abs(se.SINGULAR[bs]).max() <= 8
    rng = np.random.default_rng(bs)
    for _ in range(50):
        a = rng.uniform(-1.0, 1.0, size=(bs, bs)) + 2.0 * bs * np.eye(bs)
        if rng.uniform() < 0.5:
            a = a[rng.permutation(bs)]      # rows out of order: the pivot search has to swap
        inv, ok = se.block_inverse(a)
        assert ok
        assert np.abs(inv @ a - np.eye(bs)).max() < 1e-13
    # the first row of largest magnitude wins a tie: [[1, 1], [-1, 1]] keeps row 0
    inv, ok = se.block_inverse(np.array([[1.0, 1.0], [-1.0, 1.0]]))
    assert ok and np.array_equal(inv, np.array([[0.5, -0.5], [0.5, 0.5]]))


@pytest.mark.parametrize("eos", ["w", "we", "wce", "wsce"])
def test_singular_at_leaves_the_block_as_the_pivot(eos):
    """under the ILU(0) of tests/fused_reference.py (long double, any subdomains) the pivot of the row is SINGULAR[bs]
    bit for bit, at the first row of the first subdomain, a middle row of a middle one and the last row of the last"""
    lm, rp, ci = box(eos)
    bs = BS[eos]
    sub = np.asarray(lm.sub_ptr)
    val = se.diag_dominant_values(rp, ci, bs)
    mid = (len(sub) - 1) // 2
    for row in (0, (sub[mid] + sub[mid + 1]) // 2, lm.n_owned - 1):
        sv = se.singular_at(val, rp, ci, row, bs)
        changed = np.nonzero((sv != val).reshape(-1, bs, bs).any(axis=(1, 2)))[0]
        assert np.all((changed >= rp[row]) & (changed < rp[row + 1]))     # that row alone
        with np.errstate(all="ignore"):
            ilu = fr.BlockILU0(rp, ci, sv, bs, sub)
            one = fr.BlockILU0(rp, ci, sv, bs, np.array([0, lm.n_owned]))
        for f in (ilu, one):
            assert np.array_equal(f.F[f.diag[row]].astype(np.float64), se.SINGULAR[bs])
        assert not se.block_inverse(ilu.F[ilu.diag[row]].astype(np.float64))[1]
        # every other pivot before it is sound
        assert all(se.block_inverse(ilu.F[ilu.diag[i]].astype(np.float64))[1] for i in range(row))
    whole = se.singular_at(val, rp, ci, 5, bs, whole_row=True).reshape(-1, bs, bs)
    for q in range(rp[5], rp[6]):
        assert np.array_equal(whole[q], se.SINGULAR[bs] if ci[q] == 5 else np.zeros((bs, bs)))


def test_the_prescribed_systems_are_what_they_say():
    for eos in ("w", "we", "wce", "wsce"):
        lm, rp, ci = box(eos)
        bs = BS[eos]
        V = se.diag_dominant_values(rp, ci, bs).reshape(-1, bs, bs)
        rows = np.repeat(np.arange(lm.n_owned), np.diff(rp))
        off = ci != rows
        assert np.sqrt((V[off] ** 2).sum(axis=(1, 2))).max() <= 0.1 * (1 + 1e-15)
        assert np.abs(V[~off] - np.eye(bs)).max() <= 0.2
        assert np.array_equal(se.diag_dominant_values(rp, ci, bs), V.ravel())      # fixed seed
        # power-of-two block diagonal: B^-1 A = I exactly, B^-1 b = A^-1 b exactly, a unit-norm start
        P = se.pow2_block_diagonal(rp, ci, bs)
        M, apply = se.preconditioned(rp, ci, P, bs, np.asarray(lm.sub_ptr))
        assert np.array_equal(M, np.eye(lm.n_owned * bs, dtype=LD))
        x = se.unit_norm_solution(lm.n_owned, bs)
        b = se.dense(rp, ci, P, bs, np.float64) @ x
        assert np.array_equal(apply(b).astype(np.float64), x) and np.count_nonzero(x) == 64
        for order in (np.arange(x.size), np.random.default_rng(1).permutation(x.size)):
            assert np.add.reduce((x * x)[order]) == 64.0
    # the skew chain: (A b, b) = 1 - 1 + exact zeros in any order
    g, lm, prim, region = make_case(dims=(64, 1, 1), brick=(16, 1, 1), eos="w", lens=False)
    rp, ci = se.mesh_pattern(lm)
    A = se.dense(rp, ci, se.skew_chain_values(rp, ci), 1, np.float64)
    assert np.array_equal(A, -A.T) and np.all(np.diag(A) == 0.0)
    v = A @ np.ones(64)
    assert np.array_equal(v, np.r_[1.0, np.zeros(62), -1.0])


@pytest.mark.parametrize("eos,pc", [("w", "bjacobi"), ("we", "bjacobi"), ("wce", "bjacobi"), ("we", "none")])
def test_the_restatements_solve_the_system(dominant, eos, pc):
    val, b, M, rb, A = dominant[eos, pc]
    xs = np.linalg.solve(A, b)
    reason, its, rn, x, hist = se.bcgs(M, rb, rtol=1e-14)
    assert reason == 2 and se.distance(x, xs) < 1e-12, (reason, its, se.distance(x, xs))
    assert float(rn) <= 1e-14 * float(np.sqrt(rb @ rb))
    # the recursive norm is the norm of B^-1 (b - A x)
    assert abs(float(rn) - float(np.sqrt(((rb - M @ x) ** 2).sum()))) <= 1e-3 * float(rn) + 1e-18 * float(np.sqrt(rb @ rb))
    for restart in (30, 3):
        reason, gits, rn, x = se.gmres(M, rb, restart=restart, rtol=1e-14)
        assert reason == 2 and se.distance(x, xs) < 1e-12, (restart, reason, gits)
    # the two forms of the norm agree, and so do the double-precision runs
    r2 = se.bcgs(M, rb, rtol=1e-14, merged=False)
    assert r2[:2] == (2, its) and se.distance(r2[3], x) < 1e-12
    rd = se.bcgs(M, rb, rtol=1e-12, dtype=np.float64)
    assert rd[0] == 2 and se.distance(rd[3], xs) < 1e-10


def test_every_ending_the_restatements_state(dominant):
    val, b, M, rb, A = dominant["we", "bjacobi"]
    # the cap: -3 at exactly k, the history's k-th entry returned
    for k in (1, 2, 3):
        reason, its, rn, x, hist = se.bcgs(M, rb, rtol=1e-30, maxits=k)
        assert (reason, its, len(hist)) == (-3, k, k) and np.array_equal(x, hist[-1][0]) and rn == hist[-1][1]
    for k in (2, 3, 5):
        reason, its, rn, x = se.gmres(M, rb, restart=2, rtol=1e-30, maxits=k)
        assert (reason, its) == (-3, k)
    # a capped run is the prefix of an uncapped one
    full = se.bcgs(M, rb, rtol=1e-12)
    assert np.array_equal(se.bcgs(M, rb, rtol=1e-30, maxits=2)[3], full[4][1][0])
    # atol above the first iterate's residual: 3 at its = 1; above the start's: 3 at its = 0
    first = float(full[4][0][1])
    assert se.bcgs(M, rb, rtol=1e-30, atol=1.5 * first)[:2] == (3, 1)
    assert se.bcgs(M, rb, rtol=1e-30, atol=2.0 * float(np.sqrt(rb @ rb)))[:2] == (3, 0)
    g1 = se.gmres(M, rb, rtol=1e-30, maxits=1)
    assert se.gmres(M, rb, rtol=1e-30, atol=1.5 * float(g1[2]))[:2] == (3, 1)
    # zero right-hand side, NaN
    z = np.zeros_like(rb)
    assert se.bcgs(M, z)[:2] == (3, 0) and se.gmres(M, z)[:2] == (3, 0)
    assert not se.bcgs(M, z)[3].any() and not se.gmres(M, z)[3].any()
    bad = rb.copy()
    bad[3] = np.nan
    assert se.bcgs(M, bad)[:2] == (-9, 0) and se.gmres(M, bad)[:2] == (-9, 0)
    # solved in one step: B^-1 A = I
    n = rb.size
    x1 = se.unit_norm_solution(n // 2, 2)
    for dtype in (LD, np.float64):
        reason, its, rn, x, hist = se.bcgs(np.eye(n), x1, dtype=dtype)
        assert (reason, its, float(rn)) == (3, 1, 0.0) and np.array_equal(x.astype(np.float64), x1)
        reason, its, rn, x = se.gmres(np.eye(n), x1, dtype=dtype)
        assert (reason, its, float(rn)) == (3, 1, 0.0) and np.array_equal(x.astype(np.float64), x1), (reason, its, rn)
    # the skew chain: (V, RP) = 0 at the first iteration
    g, lm, prim, region = make_case(dims=(64, 1, 1), brick=(16, 1, 1), eos="w", lens=False)
    rp, ci = se.mesh_pattern(lm)
    S, _ = se.preconditioned(rp, ci, se.skew_chain_values(rp, ci), 1, None)
    for dtype in (LD, np.float64):
        assert se.bcgs(S, np.ones(64), dtype=dtype)[:2] == (-5, 1)
    print("GMRES on the skew chain:", se.gmres(S, np.ones(64), maxits=200)[:3], se.gmres(S, np.ones(64), maxits=200, dtype=np.float64)[:3])


def test_double_against_long_double_after_k_iterations(dominant):
    """the figure the GPU tests' bounds are ten times of: x and rnorm of the double-precision run against the long-double
    run of the same restatement, capped at k <= 5.  A system beyond 1e-10 is too ill-conditioned for the purpose"""
    worst = {}
    for (eos, pc), (val, b, M, rb, A) in dominant.items():
        worst[eos, pc, "bcgs merged"] = se.double_distance(M, rb, "bcgs", (1, 2, 3), merged=True)
        worst[eos, pc, "bcgs petsc"] = se.double_distance(M, rb, "bcgs", (1, 2, 3), merged=False)
        worst[eos, pc, "gmres(30)"] = se.double_distance(M, rb, "gmres", (1, 2, 3), restart=30)
        worst[eos, pc, "gmres(2)"] = se.double_distance(M, rb, "gmres", (2, 3, 5), restart=2)
    print()
    for key, (dx, dr) in sorted(worst.items()):
        print("%-4s %-8s %-12s x %.2e  rnorm %.2e" % (key + (dx, dr)))
        assert dx <= 1e-10 and dr <= 1e-10, key

"""tests/coarse_reference.py held to exact rational arithmetic (fractions.Fraction) on a system of 12 unknowns: 6 cells of
2 x 2 blocks in a ring with one chord, three uneven aggregates.  P, Ac, Ac^-1 and both modes' z are formed from the
definition over the rationals, with an exact block-Jacobi solve (two subdomains) as M^-1; the long-double reference must
agree to a few units of its own rounding."""
from fractions import Fraction

import numpy as np

from tests import coarse_reference as cr

LD = cr.LD
BS, N, NC = 2, 6, 3
AGG = np.array([0, 2, 0, 1, 2, 2])      # aggregates of 2, 1 and 3 cells
SUB = [0, 3, 6]


def system():
    nb = [sorted({i, (i + 1) % N, (i - 1) % N} | ({3} if i == 0 else set()) | ({0} if i == 3 else set())) for i in range(N)]
    rp = np.concatenate([[0], np.cumsum([len(s) for s in nb])])
    ci = np.concatenate(nb)
    rng = np.random.default_rng(3)
    V = rng.integers(-9, 10, size=(ci.size, BS, BS)).astype(np.float64) / 8.0      # exact in binary and as fractions
    rows = np.repeat(np.arange(N), np.diff(rp))
    V[ci == rows] += 6.0 * np.eye(BS)
    r = rng.integers(-40, 41, size=N * BS).astype(np.float64) / 16.0
    return rp, ci, V, r


def frac(a):
    return np.vectorize(lambda v: Fraction(float(v)), otypes=[object])(np.asarray(a, dtype=np.float64))


def exact_inverse(A):
    m = A.shape[0]
    W = np.concatenate([A, frac(np.eye(m))], axis=1)
    for k in range(m):
        p = next(i for i in range(k, m) if W[i, k] != 0)
        W[[k, p]] = W[[p, k]]
        W[k] = W[k] / W[k, k]
        for i in range(m):
            if i != k:
                W[i] = W[i] - W[i, k] * W[k]
    return W[:, m:]


def dense(rp, ci, V):
    A = np.zeros((N * BS, N * BS))
    for i in range(N):
        for q in range(rp[i], rp[i + 1]):
            A[i * BS:(i + 1) * BS, ci[q] * BS:(ci[q] + 1) * BS] = V[q]
    return A


def block_jacobi_exact(A):
    Minv = frac(np.zeros_like(A, dtype=np.float64))
    for s in range(len(SUB) - 1):
        sl = slice(SUB[s] * BS, SUB[s + 1] * BS)
        Minv[sl, sl] = exact_inverse(A[sl, sl])
    return Minv


def test_reference_against_exact_rationals():
    rp, ci, V, r = system()
    Af = frac(dense(rp, ci, V))
    P = frac(cr.prolongation(AGG, NC, BS, dtype=np.float64))
    Ac = P.T.dot(Af).dot(P)
    Ainv = exact_inverse(Ac)
    Minv = block_jacobi_exact(Af)
    rf = frac(r)
    y = Ainv.dot(P.T.dot(rf))
    z_add = Minv.dot(rf) + P.dot(y)
    z_def = Minv.dot(rf - Af.dot(P.dot(y))) + P.dot(y)

    Minv_ld = np.array([[LD(v.numerator) / LD(v.denominator) for v in row] for row in Minv])
    ref = cr.TwoLevel(rp, ci, V.ravel(), BS, AGG, NC, lambda v: cr.matvec(Minv_ld, v))
    eps = np.finfo(LD).eps

    def close(got, want, k):
        want_ld = np.vectorize(lambda v: LD(v.numerator) / LD(v.denominator), otypes=[LD])(want)
        scale = np.abs(want_ld).max()
        assert np.abs(np.asarray(got, dtype=LD) - want_ld).max() <= k * eps * scale, (np.abs(got - want_ld).max(), scale)

    assert np.array_equal(cr.prolongation(AGG, NC, BS), np.vectorize(float)(P).astype(LD))
    # Ac: sums of at most 9 exactly representable terms -- exact in long double
    assert np.array_equal(ref.Ac, np.vectorize(lambda v: LD(v.numerator) / LD(v.denominator), otypes=[LD])(Ac))
    assert np.array_equal(cr.restrict(AGG, NC, BS, r), np.vectorize(float)(P.T.dot(rf)).astype(LD))
    # 6 x 6 elimination, condition number O(10): a few hundred roundings at most
    close(ref.Ainv, Ainv, 512)
    close(ref.coarse(r), y, 1024)
    close(ref.apply("additive", r), z_add, 2048)
    close(ref.apply("deflated", r), z_def, 4096)
    # the operator form is the application to A x
    x = frac(np.arange(1, N * BS + 1) / 4.0)
    close(ref.operator("deflated", np.vectorize(float)(x)), Minv.dot(Af.dot(x) - Af.dot(P.dot(Ainv.dot(P.T.dot(Af.dot(x)))))) +
          P.dot(Ainv.dot(P.T.dot(Af.dot(x)))), 8192)


def test_double_restatement_is_the_same_formula():
    """dtype=float64 runs the same code in double: its error against the long-double result is a few double roundings"""
    rp, ci, V, r = system()
    A = dense(rp, ci, V)
    Minv = np.zeros_like(A)
    for s in range(len(SUB) - 1):
        sl = slice(SUB[s] * BS, SUB[s + 1] * BS)
        Minv[sl, sl] = np.linalg.inv(A[sl, sl])
    one = lambda v: cr.matvec(Minv, v)   # noqa: E731
    hi = cr.TwoLevel(rp, ci, V.ravel(), BS, AGG, NC, one)
    lo = cr.TwoLevel(rp, ci, V.ravel(), BS, AGG, NC, one, dtype=np.float64)
    assert lo.Ainv.dtype == np.float64 and hi.Ainv.dtype == LD
    for mode in ("additive", "deflated"):
        a, b = hi.apply(mode, r), lo.apply(mode, r)
        assert b.dtype == np.float64
        assert 0 < np.abs(a - b).max() <= 200 * np.finfo(np.float64).eps * np.abs(a).max()
    # the one-level part is applied in double as well: a matrix of doubles, not the long-double function
    assert lo.Minv.dtype == np.float64 and hi.Minv is None
    assert np.array_equal(lo.Minv, Minv)


def test_singular_coarse_matrix_has_no_inverse():
    rp, ci, V, r = system()
    rows = np.repeat(np.arange(N), np.diff(rp))
    V = V.copy()
    V[AGG[rows] == 1] = 0.0          # every fine row of aggregate 1: zero blocks
    Ac = cr.galerkin(rp, ci, V.ravel(), BS, AGG, NC)
    assert not Ac[BS:2 * BS].any() and cr.inverse(Ac) is None

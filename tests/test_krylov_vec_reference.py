"""tests/krylov_vec_reference.py against exact rational arithmetic (fractions.Fraction) at n <= 64, and its restated
derive_scalars phases against hand-worked values, the three breakdown codes included.  No GPU.

A long-double result of an expression of t terms differs from the exact one by at most (t + 2) roundings of 2^-64 of the
sum of the terms' magnitudes (products, the running sum, and the scalar products alpha * beta); the bar below is that with
a factor 2 to spare -- ten thousand times finer than the 2^-53 the device results are held to."""
from fractions import Fraction

import numpy as np
import pytest

from tests import krylov_vec_reference as kr

LD = kr.LD
SIZES = [1, 2, 3, 17, 63, 64]


def frac(x):
    """exact rational value of a double or long double (80-bit: 64 mantissa bits = two doubles, exactly)"""
    x = LD(x)
    hi = float(x)
    return Fraction(hi) + Fraction(float(x - LD(hi)))


def fracs(a):
    return [frac(v) for v in np.asarray(a).ravel()]


def close(got, want, mag, terms):
    """every long-double entry within 2 (terms + 2) 2^-64 of the exact value, relative to the exact magnitude sum"""
    bar = Fraction(2 * (terms + 2), 2 ** 64)
    for g, w, m in zip(fracs(got), want, mag):
        assert abs(g - w) <= bar * m, (float(g), float(w), float(m))


def vectors(n, count, seed):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=n) for _ in range(count)]


@pytest.mark.parametrize("n", SIZES)
def test_elementwise_updates_are_exact_to_long_double_rounding(n):
    X, R, P, V, S, T = vectors(n, 6, 100 + n)
    alpha, omega, beta = 0.37, -1.3, 2.1
    a, o, b = Fraction(alpha), Fraction(omega), Fraction(beta)
    fX, fR, fP, fV, fS, fT = (fracs(v) for v in (X, R, P, V, S, T))
    w, M = kr.waxpy(alpha, X, R)
    close(w, [a * x + r for x, r in zip(fX, fR)], [abs(a * x) + abs(r) for x, r in zip(fX, fR)], 2)
    close(M, [abs(a * x) + abs(r) for x, r in zip(fX, fR)], [abs(a * x) + abs(r) for x, r in zip(fX, fR)], 2)
    p, M = kr.bcgs_p(P, R, V, beta, omega)
    mp = [abs(r) + abs(b * q) + abs(b * o * v) for q, r, v in zip(fP, fR, fV)]
    close(p, [r + b * (q - o * v) for q, r, v in zip(fP, fR, fV)], mp, 3)
    close(M, mp, mp, 3)
    s, M = kr.bcgs_s(R, V, alpha)
    close(s, [r - a * v for r, v in zip(fR, fV)], [abs(r) + abs(a * v) for r, v in zip(fR, fV)], 2)
    (x1, MX), (r1, MR) = kr.bcgs_xr(X, P, S, T, alpha, omega)
    close(x1, [x + a * q + o * s_ for x, q, s_ in zip(fX, fP, fS)], [abs(x) + abs(a * q) + abs(o * s_) for x, q, s_ in zip(fX, fP, fS)], 3)
    close(r1, [s_ - o * t for s_, t in zip(fS, fT)], [abs(s_) + abs(o * t) for s_, t in zip(fS, fT)], 2)
    # the one-pass form is the three separate updates composed
    (x2, MX2), (r2, MR2), (p2, MP2) = kr.bcgs_xrp(X, R, P, V, T, alpha, omega, beta)
    eS = [r - a * v for r, v in zip(fR, fV)]
    mS = [abs(r) + abs(a * v) for r, v in zip(fR, fV)]
    eX = [x + a * q + o * s_ for x, q, s_ in zip(fX, fP, eS)]
    mX = [abs(x) + abs(a * q) + abs(o) * m for x, q, m in zip(fX, fP, mS)]
    eR = [s_ - o * t for s_, t in zip(eS, fT)]
    mR = [m + abs(o * t) for m, t in zip(mS, fT)]
    eP = [r + b * (q - o * v) for r, q, v in zip(eR, fP, fV)]
    mP = [m + abs(b * q) + abs(b * o * v) for m, q, v in zip(mR, fP, fV)]
    close(x2, eX, mX, 5)
    close(r2, eR, mR, 4)
    close(p2, eP, mP, 7)
    close(MX2, mX, mX, 5)
    close(MR2, mR, mR, 4)
    close(MP2, mP, mP, 7)
    q, M = kr.scale_to(X, 2.75)
    for g, x in zip(fracs(q), fX):   # (x / sqrt(2.75))^2 * 2.75 = x^2 to long-double rounding
        assert abs(g * g * Fraction(2.75) - x * x) <= Fraction(8, 2 ** 64) * x * x


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("k,pad", [(1, 0), (3, 1), (9, 16)])
def test_basis_operations_are_exact_to_long_double_rounding(n, k, pad):
    ldim = n + pad
    rng = np.random.default_rng(7 * n + k)
    basis = rng.normal(size=(k + 1) * ldim)
    w, x = rng.normal(size=n), rng.normal(size=n)
    h = rng.uniform(0.1, 3.0, size=k) * rng.choice([-1.0, 1.0], size=k)
    fw, fx, fh = fracs(w), fracs(x), fracs(h)
    fB = [fracs(basis[j * ldim: j * ldim + n]) for j in range(k)]
    d, bar = kr.mdot(w, basis, ldim, k, n)
    for j in range(k):
        terms = [a * b for a, b in zip(fw, fB[j])]
        close([d[j]], [sum(terms)], [sum(abs(t) for t in terms)], n)
        close([bar[j]], [sum(abs(t) for t in terms)], [sum(abs(t) for t in terms)], n)
    for fn, v, fv, sign in ((kr.maxpy, w, fw, -1), (kr.update_x, x, fx, 1)):
        got, M = fn(v, basis, ldim, k, n, h)
        want = [fv[i] + sign * sum(fh[j] * fB[j][i] for j in range(k)) for i in range(n)]
        mag = [abs(fv[i]) + sum(abs(fh[j] * fB[j][i]) for j in range(k)) for i in range(n)]
        close(got, want, mag, k + 1)
        close(M, mag, mag, k + 1)


@pytest.mark.parametrize("n", SIZES)
def test_dot_and_its_bar(n):
    a, b = vectors(n, 2, 300 + n)
    d, bar = kr.dot(a, b)
    terms = [x * y for x, y in zip(fracs(a), fracs(b))]
    close([d], [sum(terms)], [sum(abs(t) for t in terms)], n)
    close([bar], [sum(abs(t) for t in terms)], [sum(abs(t) for t in terms)], n)


def scalars(**kw):
    s = np.zeros(kr.NSCAL)
    s[:16] = [11.0, 12.0, 13.0, 14.0, 15.0, 16.0, 17.0, 18.0, 19.0, 20.0, 21.0, 22.0, 23.0, 24.0, 25.0, 0.0]
    for name, v in kw.items():
        s[getattr(kr, "S_" + name)] = v
    return s


def check(s_in, phase, **want):
    out, scale = kr.derive(s_in, phase)
    slots = {getattr(kr, "S_" + name): v for name, v in want.items()}
    for slot, v in slots.items():
        assert out[slot] == v or (np.isnan(v) and np.isnan(out[slot])), (phase, slot, out[slot], v)
    assert set(scale) <= set(slots), (phase, sorted(scale), sorted(slots))      # every written slot is stated above
    others = [i for i in range(kr.NSCAL) if i not in slots]
    assert out[others].tobytes() == np.asarray(s_in)[others].tobytes()


def test_phase_formulas_hand_worked():
    # 0: rho = (R,R) = 9, rho_old = alpha = omega = 1, beta = (9 / 1) (1 / 1), the code cleared
    check(scalars(DP2=9.0, BREAK=3.0), 0, RHO=9.0, RHOOLD=1.0, ALPHA=1.0, OMEGA=1.0, BETA=9.0, BREAK=0.0)
    # 2: alpha = rho / (V,RP) = 3 / 4
    check(scalars(RHO=3.0, D1=4.0), 2, ALPHA=0.75)
    # 3: omega = (S,T) / (T,T) = 3 / 4
    check(scalars(D1=3.0, D2=4.0), 3, OMEGA=0.75)
    # 5: omega = 2 / 4; (R,R) = (3 - 2 * 0.5 * 2) + 0.25 * 4 = 2; (R,RP) = 5 - 0.5 * 6 = 2
    m = dict(D1=2.0, D2=4.0, DP2=3.0, RHONEW=5.0, W2=6.0)
    check(scalars(**m), 5, OMEGA=0.5, DP2=2.0, RHONEW=2.0)
    # 6: the same, then rho_old = 8, rho = 2, beta = (2 / 8) (0.25 / 0.5) = 0.125
    check(scalars(RHO=8.0, ALPHA=0.25, **m), 6, OMEGA=0.5, DP2=2.0, RHONEW=2.0, RHOOLD=8.0, RHO=2.0, BETA=0.125)
    # 4: the rotation alone: beta = (6 / 3) (0.5 / 4) = 0.25
    check(scalars(RHO=3.0, RHONEW=6.0, ALPHA=0.5, OMEGA=4.0), 4, RHOOLD=3.0, RHO=6.0, BETA=0.25)
    # (R,R) that rounds below zero is clamped: omega = 2, (1 - 2 * 2 * 2) + 4 * 1 = -3 -> 0
    check(scalars(D1=2.0, D2=1.0, DP2=1.0, RHONEW=5.0, W2=1.0), 5, OMEGA=2.0, DP2=0.0, RHONEW=3.0)


def test_breakdown_codes_hand_worked():
    inf = float("inf")
    # code 1: (V,RP) = 0 in phase 2 (alpha = 3 / 0), and rho = 0 in phase 0 (beta = 0)
    check(scalars(RHO=3.0, D1=0.0), 2, ALPHA=inf, BREAK=1.0)
    check(scalars(DP2=0.0), 0, RHO=0.0, RHOOLD=1.0, ALPHA=1.0, OMEGA=1.0, BETA=0.0, BREAK=1.0)
    # code 2 and omega = 0 for (T,T) = 0: phase 3, and the merged phases, where (R,R) = (S,S) and (R,RP) = (S,RP) follow
    check(scalars(D1=3.0, D2=0.0), 3, OMEGA=0.0, BREAK=2.0)
    z = dict(D1=2.0, D2=0.0, DP2=3.0, RHONEW=5.0, W2=6.0)
    check(scalars(**z), 5, OMEGA=0.0, DP2=3.0, RHONEW=5.0, BREAK=2.0)
    check(scalars(RHO=8.0, ALPHA=0.25, **z), 6, OMEGA=0.0, DP2=3.0, RHONEW=5.0, RHOOLD=8.0, RHO=5.0, BETA=inf, BREAK=2.0)
    # code 3: the next rho vanishes (phase 4; phase 6 with (S,RP) = omega (T,RP) = 3)
    check(scalars(RHO=3.0, RHONEW=0.0, ALPHA=0.5, OMEGA=4.0), 4, RHOOLD=3.0, RHO=0.0, BETA=0.0, BREAK=3.0)
    check(scalars(RHO=8.0, ALPHA=0.25, D1=2.0, D2=4.0, DP2=3.0, RHONEW=3.0, W2=6.0), 6,
          OMEGA=0.5, DP2=2.0, RHONEW=0.0, RHOOLD=8.0, RHO=0.0, BETA=0.0, BREAK=3.0)
    # ... but an earlier code stays: 2 from this phase's (T,T) = 0 with (S,RP) = 0, and a 4 that came in
    check(scalars(RHO=8.0, ALPHA=0.25, D1=2.0, D2=0.0, DP2=3.0, RHONEW=0.0, W2=6.0), 6,
          OMEGA=0.0, DP2=3.0, RHONEW=0.0, RHOOLD=8.0, RHO=0.0, BETA=float("nan"), BREAK=2.0)
    check(scalars(RHO=3.0, RHONEW=0.0, ALPHA=0.5, OMEGA=4.0, BREAK=4.0), 4, RHOOLD=3.0, RHO=0.0, BETA=0.0, BREAK=4.0)
    # a code 4 that came in is preserved through phase 0 (the reduction that fed it lost a partial sum)
    check(scalars(DP2=9.0, BREAK=4.0), 0, RHO=9.0, RHOOLD=1.0, ALPHA=1.0, OMEGA=1.0, BETA=9.0, BREAK=4.0)


def test_scales_are_the_magnitude_sums():
    s = scalars(RHO=8.0, ALPHA=0.25, D1=2.0, D2=4.0, DP2=3.0, RHONEW=5.0, W2=-6.0)
    out, scale = kr.derive(s, 6)
    # omega = 0.5: (R,R) = 3 - 2 + 1, terms 3 + 2 + 1; rho = 5 + 3 = 8, terms 5 + 3; beta = (8 / 8) (0.25 / 0.5)
    assert (scale[kr.S_OMEGA], scale[kr.S_DP2], scale[kr.S_RHONEW], scale[kr.S_RHO]) == (0.5, 6.0, 8.0, 8.0)
    assert out[kr.S_BETA] == 0.5 and scale[kr.S_BETA] == 0.5 and scale[kr.S_RHOOLD] == 8.0
    # a cancelled rho carries its relative error into beta: rho = 5 - 0.5 * 6 = 2 of terms 8, beta's scale 4 |beta|
    out, scale = kr.derive(scalars(RHO=8.0, ALPHA=0.25, D1=2.0, D2=4.0, DP2=3.0, RHONEW=5.0, W2=6.0), 6)
    assert scale[kr.S_RHO] == 8.0 and scale[kr.S_BETA] == 4.0 * abs(out[kr.S_BETA])
    with pytest.raises(ValueError):
        kr.derive(s, 1)

"""An extended-precision restatement of the Krylov drivers' vector and reduction steps (waiwera_amd/csrc/krylov_vec.hip.h),
for tests/test_hip_krylov_vec.py -- written from the operations' definitions, not from the kernels:

- every element-wise update in numpy.longdouble, together with M_i, the sum of the magnitudes of the terms of element i's
  expression: the scale a rounding-error bar of c * 2^-53 * M_i is taken against;
- inner products in long double together with sum |a_i b_i|;
- derive_scalars' phases 0, 2, 3, 4, 5 and 6 (reductions.hip.h) in IEEE doubles, in the kernel's order of operations, with
  the breakdown codes, and for each scalar a phase writes the sum of the magnitudes of its formula's terms.

tests/test_krylov_vec_reference.py checks this file against exact rational arithmetic and hand-worked values."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "the reference needs 80-bit (or wider) long double"

# device scalar slots (waiwera_amd/csrc/context.hpp); S_H + j: the Gram-Schmidt coefficient h_j; COEF + j: where
# gmres_update_x parks its coefficients
S_RHO, S_RHOOLD, S_ALPHA, S_OMEGA, S_BETA, S_D1, S_D2, S_DP2, S_RHONEW, S_W2, S_BREAK, S_H = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16
COEF, NSCAL, MAX_RESTART = 64, 128, 40
U = 2.0 ** -53


def ld(a):
    return np.asarray(a, dtype=LD)


def dot(a, b):
    """(a, b) and sum |a_i b_i| in long double"""
    p = ld(a) * ld(b)
    return p.sum(), np.abs(p).sum()


# ---- element-wise updates: (result, M) per output vector ------------------------------------------------------------------
def waxpy(alpha, x, y):
    """w = alpha x + y"""
    t = LD(alpha) * ld(x)
    return t + ld(y), np.abs(t) + np.abs(ld(y))


def bcgs_p(P, R, V, beta, omega):
    """P = R + beta (P - omega V)"""
    bp, bv = LD(beta) * ld(P), LD(beta) * LD(omega) * ld(V)
    return ld(R) + (bp - bv), np.abs(ld(R)) + np.abs(bp) + np.abs(bv)


def bcgs_s(R, V, alpha):
    """S = R - alpha V"""
    av = LD(alpha) * ld(V)
    return ld(R) - av, np.abs(ld(R)) + np.abs(av)


def bcgs_xr(X, P, S, T, alpha, omega):
    """X += alpha P + omega S; R = S - omega T: ((X, M_X), (R, M_R))"""
    ap, os_, ot = LD(alpha) * ld(P), LD(omega) * ld(S), LD(omega) * ld(T)
    return (ld(X) + ap + os_, np.abs(ld(X)) + np.abs(ap) + np.abs(os_)), (ld(S) - ot, np.abs(ld(S)) + np.abs(ot))


def bcgs_xrp(X, R, P, V, T, alpha, omega, beta):
    """S = R - alpha V (never stored); X += alpha P + omega S; R = S - omega T; P = R + beta (P - omega V), the new R:
    ((X, M_X), (R, M_R), (P, M_P)).  S and the new R are intermediate results of the later expressions, so their
    magnitude sums M carry through"""
    S, MS = bcgs_s(R, V, alpha)
    ap, ot = LD(alpha) * ld(P), LD(omega) * ld(T)
    Xn, MX = ld(X) + ap + LD(omega) * S, np.abs(ld(X)) + np.abs(ap) + abs(LD(omega)) * MS
    Rn, MR = S - ot, MS + np.abs(ot)
    bp, bv = LD(beta) * ld(P), LD(beta) * LD(omega) * ld(V)
    return (Xn, MX), (Rn, MR), (Rn + (bp - bv), MR + np.abs(bp) + np.abs(bv))


def basis_view(basis, ldim, k):
    """the k vectors v_j = basis[j * ldim : ...] as rows (whole leading dimension)"""
    return np.asarray(basis)[: k * ldim].reshape(k, ldim)


def mdot(w, basis, ldim, k, n):
    """h_j = (w, v_j), j < k: (sums, sums of magnitudes)"""
    Bv = ld(basis_view(basis, ldim, k)[:, :n])
    p = Bv * ld(w)[None, :n]
    return p.sum(axis=1), np.abs(p).sum(axis=1)


def maxpy(w, basis, ldim, k, n, h):
    """w - sum_j h_j v_j over the first n entries: (result, M)"""
    t = ld(h)[:k, None] * ld(basis_view(basis, ldim, k)[:, :n])
    return ld(w)[:n] - t.sum(axis=0), np.abs(ld(w)[:n]) + np.abs(t).sum(axis=0)


def update_x(x, basis, ldim, k, n, coef):
    """x + sum_j coef_j v_j over the first n entries: (result, M)"""
    t = ld(coef)[:k, None] * ld(basis_view(basis, ldim, k)[:, :n])
    return ld(x)[:n] + t.sum(axis=0), np.abs(ld(x)[:n]) + np.abs(t).sum(axis=0)


def scale_to(src, norm2):
    """src / sqrt(norm2): (result, M)"""
    r = ld(src) / np.sqrt(LD(norm2))
    return r, np.abs(r)


# ---- derive_scalars ----------------------------------------------------------------------------------------------------
def _merged(s, scale):
    st, tt, ss, srp, trp = s[S_D1], s[S_D2], s[S_DP2], s[S_RHONEW], s[S_W2]
    if tt == 0.0:
        s[S_BREAK], s[S_OMEGA] = 2.0, 0.0
        scale[S_BREAK] = 0.0
    else:
        s[S_OMEGA] = st / tt
    om = s[S_OMEGA]
    rr = (ss - 2.0 * om * st) + om * om * tt
    s[S_DP2] = rr if rr > 0.0 else 0.0
    s[S_RHONEW] = srp - om * trp
    scale.update({S_OMEGA: abs(om), S_DP2: abs(ss) + abs(2.0 * om * st) + abs(om * om * tt), S_RHONEW: abs(srp) + abs(om * trp)})


def _rotate(s, scale):
    rho_terms = scale.get(S_RHONEW, abs(s[S_RHONEW]))
    s[S_RHOOLD], s[S_RHO] = s[S_RHO], s[S_RHONEW]
    if s[S_RHO] == 0.0 and s[S_BREAK] == 0.0:
        s[S_BREAK] = 3.0
        scale[S_BREAK] = 0.0
    s[S_BETA] = (s[S_RHO] / s[S_RHOOLD]) * (s[S_ALPHA] / s[S_OMEGA])
    # beta is a product of quotients: relative to itself, but its numerator rho may be a cancelled difference
    rel = rho_terms / abs(s[S_RHO]) if s[S_RHO] != 0.0 else 1.0
    scale.update({S_RHOOLD: abs(s[S_RHOOLD]), S_RHO: rho_terms, S_BETA: abs(s[S_BETA]) * rel})


def derive(s_in, phase):
    """(the scalars after derive_scalars(phase), {slot written: sum of the magnitudes of its formula's terms}).  A slot that
    is not in the dictionary comes back with the bits that went in; a scale of 0.0 means an exact value (a constant or a
    breakdown code).  IEEE doubles throughout: a division by zero gives the infinity or NaN the device gives"""
    with np.errstate(all="ignore"):
        s = [np.float64(v) for v in s_in]
        scale = {}
        if phase == 0:
            s[S_RHO] = s[S_DP2]
            s[S_RHOOLD] = s[S_ALPHA] = s[S_OMEGA] = np.float64(1.0)
            if s[S_BREAK] != 4.0:
                s[S_BREAK] = np.float64(0.0)
            s[S_BETA] = (s[S_RHO] / s[S_RHOOLD]) * (s[S_ALPHA] / s[S_OMEGA])
            if s[S_RHO] == 0.0:
                s[S_BREAK] = np.float64(1.0)
            scale = {S_RHO: 0.0, S_RHOOLD: 0.0, S_ALPHA: 0.0, S_OMEGA: 0.0, S_BETA: 0.0, S_BREAK: 0.0}
        elif phase == 2:
            if s[S_D1] == 0.0:
                s[S_BREAK] = np.float64(1.0)
                scale[S_BREAK] = 0.0
            s[S_ALPHA] = s[S_RHO] / s[S_D1]
            scale[S_ALPHA] = abs(s[S_ALPHA])
        elif phase == 3:
            if s[S_D2] == 0.0:
                s[S_BREAK], s[S_OMEGA] = np.float64(2.0), np.float64(0.0)
                scale[S_BREAK] = 0.0
            else:
                s[S_OMEGA] = s[S_D1] / s[S_D2]
            scale[S_OMEGA] = abs(s[S_OMEGA])
        elif phase == 4:
            _rotate(s, scale)
        elif phase in (5, 6):
            _merged(s, scale)
            if phase == 6:
                _rotate(s, scale)
        else:
            raise ValueError("no phase %r" % (phase,))
        return np.array(s, dtype=np.float64), scale

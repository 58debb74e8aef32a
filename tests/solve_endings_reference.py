"""What the tests of how linear solves end (tests/test_hip_solve_endings.py) prescribe and compare against -- written
from the definitions and from the stopping rules krylov.hip states, not from the kernels:

- block_inverse: linalg_device.hip.h's Gauss-Jordan with partial pivoting (swap to the FIRST row of largest magnitude,
  multiply by the pivot's reciprocal, flag m[p][p] == 0.0), in numpy doubles; SINGULAR pins one rank-deficient block of
  small integers per block size 1 to 4 for which that arithmetic reaches an exact 0.0 (every pivot on the way is +-1 or a
  power of two, so neither the reciprocal nor a fused multiply-add rounds anything);
- singular_at: such a block on one row's diagonal, the row's lower blocks zeroed, so that the pivot the factorisation
  meets on that row is the block exactly;
- prescribed systems on a mesh's own pattern: diagonally dominant, power-of-two block diagonal, the skew chain;
- the dense preconditioned operator B^-1 A in long double from the definition (tests/fused_reference.py's ILU(0) per
  subdomain), and left-preconditioned BiCGStab and GMRES(m) (classical Gram-Schmidt) on it with PETSc's stopping rules
  as krylov.hip states them, in long double or -- to measure what double rounding moves -- in double.

Reasons (KSPConvergedReason): 2 rtol, 3 atol (also "solved exactly"), -3 iteration cap, -4 divergence, -5 breakdown, -9 NaN."""
import numpy as np

from tests import fused_reference as fr

LD = fr.LD


# ---- block_inverse ------------------------------------------------------------------------------------------------------
def block_inverse(a):
    """(inverse, ok) of one bs x bs block, linalg_device.hip.h's arithmetic in doubles; ok False: a pivot was exactly 0.0
    (the inverse then holds what 1 / 0 leaves, as on the device)"""
    a = np.asarray(a, dtype=np.float64)
    bs = a.shape[0]
    m = np.concatenate([a, np.eye(bs)], axis=1)
    ok = True
    with np.errstate(all="ignore"):
        for p in range(bs):
            piv = p
            for r in range(p + 1, bs):
                if abs(m[r, p]) > abs(m[piv, p]):
                    piv = r
            if piv != p:
                m[[p, piv]] = m[[piv, p]]
            if m[p, p] == 0.0:
                ok = False
            d = 1.0 / m[p, p]
            m[p] = m[p] * d
            for r in range(bs):
                if r != p:
                    m[r] = m[r] - m[r, p] * m[p]
    return m[:, bs:].copy(), ok


# rank-deficient blocks of small integers; the elimination of each, by hand:
#  2: rows swap (|2| > |1|), row 0 / 2 = [1 2], row 1 - 1 [1 2] = [0 0]: pivot 1 is 0.0
#  3: swap rows 0 and 1, row 0 = [1 2 3], row 1 = 0, row 2 = [0 -1 -2]; swap rows 1 and 2, row 1 = [0 1 2], row 0 = [1 0 -1];
#     pivot 2 is row 1's old 0.0
#  4: the same two steps with a fourth column and a last row [0 0 0 1]: column 2 of rows 2 and 3 is 0.0 and 0.0
SINGULAR = {
    1: np.array([[0.0]]),
    2: np.array([[1.0, 2.0], [2.0, 4.0]]),
    3: np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [1.0, 1.0, 1.0]]),
    4: np.array([[1.0, 2.0, 3.0, 4.0], [2.0, 4.0, 6.0, 8.0], [1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 1.0]]),
}


def singular_at(values, rowptr, colidx, row, bs, whole_row=False):
    """a copy of the BCSR values with SINGULAR[bs] on `row`'s diagonal and the row's blocks left of the diagonal zeroed
    (every one of them: those inside the row's subdomain, whatever the subdomains are), so that no elimination step
    touches the pivot.  whole_row: the blocks right of the diagonal too -- for factorisations that do not keep the natural
    order (the multicolour ordering, PCASM's extended subdomains), where "left" is not col < row"""
    V = np.array(values, dtype=np.float64).reshape(-1, bs, bs).copy()
    lo, hi = int(rowptr[row]), int(rowptr[row + 1])
    found = False
    for q in range(lo, hi):
        j = int(colidx[q])
        if j == row:
            V[q] = SINGULAR[bs]
            found = True
        elif j < row or whole_row:
            V[q] = 0.0
    assert found, "row %d has no diagonal block" % row
    return V.ravel()


# ---- prescribed systems on a pattern -------------------------------------------------------------------------------------
def mesh_pattern(lm):
    """(rowptr, colidx) of a one-rank mesh's Jacobian: a row's columns are the sorted set of the cell and its neighbours
    that have a column (the GPU tests hold it equal to wai_jacobian_pattern's)"""
    n = lm.n_owned
    cols = [{i} for i in range(n)]
    for a, b in np.asarray(lm.face_cells):
        if a < n and b < n:
            cols[a].add(int(b))
            cols[b].add(int(a))
    rowptr = np.zeros(n + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum([len(c) for c in cols])
    return rowptr, np.array([j for c in cols for j in sorted(c)], dtype=np.int32)


def _rows(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def diag_dominant_values(rowptr, colidx, bs, seed=5):
    """unit-scale diagonal blocks (I + a perturbation of norm <= 0.2), off-diagonal blocks of Frobenius norm <= 0.1"""
    rng = np.random.default_rng(seed)
    V = rng.uniform(-1.0, 1.0, size=(len(colidx), bs, bs))
    V *= (0.1 * rng.uniform(0.3, 1.0, size=len(colidx)) / np.sqrt((V * V).sum(axis=(1, 2))))[:, None, None]
    dq = np.nonzero(np.asarray(colidx) == _rows(rowptr))[0]
    V[dq] = np.eye(bs)[None] + 2.0 * V[dq]
    return V.ravel()


def pow2_block_diagonal(rowptr, colidx, bs):
    """A = diag(2^k I), k = -3 .. 4 by row, every off-diagonal block zero: any ILU's factor is A itself, every pivot's
    inverse and every product with it exact, B^-1 A = I exactly"""
    V = np.zeros((len(colidx), bs, bs))
    rows = _rows(rowptr)
    dq = np.nonzero(np.asarray(colidx) == rows)[0]
    V[dq] = (2.0 ** ((rows[dq] % 8) - 3))[:, None, None] * np.eye(bs)[None]
    return V.ravel()


def unit_norm_solution(n, bs, count=64):
    """x with `count` entries +-1 (count a power of four) and zeros elsewhere: |x|^2 = count and x / |x| are exact in any
    summation order, so that (v0, v0) = 1.0 exactly"""
    x = np.zeros(n * bs)
    idx = (np.arange(count) * (n * bs)) // count
    x[idx] = np.where(np.arange(count) % 3 == 0, -1.0, 1.0)
    return x


def skew_chain_values(rowptr, colidx):
    """bs = 1 on a chain: A[i, i+1] = 1, A[i+1, i] = -1, zero diagonal.  With b = ones, A b = (1, 0, .., 0, -1)"""
    rows = _rows(rowptr)
    ci = np.asarray(colidx)
    assert np.all(np.abs(ci - rows) <= 1), "not a chain in its natural order"
    return np.where(ci == rows + 1, 1.0, np.where(ci == rows - 1, -1.0, 0.0))


def dense(rowptr, colidx, val, bs, dtype=LD):
    n = len(rowptr) - 1
    A = np.zeros((n * bs, n * bs), dtype=dtype)
    V = np.asarray(val, dtype=dtype).reshape(-1, bs, bs)
    for i in range(n):
        for q in range(rowptr[i], rowptr[i + 1]):
            j = int(colidx[q])
            A[i * bs:(i + 1) * bs, j * bs:(j + 1) * bs] = V[q]
    return A


def preconditioned(rowptr, colidx, val, bs, sub_ptr=None):
    """(M, apply): M = B^-1 A dense in long double and r -> B^-1 r, B the block-Jacobi ILU(0) of the subdomains of sub_ptr;
    sub_ptr None: no preconditioner"""
    A = dense(rowptr, colidx, val, bs)
    if sub_ptr is None:
        return A, lambda r: np.asarray(r, dtype=LD).copy()
    ilu = fr.BlockILU0(rowptr, colidx, val, bs, sub_ptr)
    M = np.stack([ilu.solve(A[:, k]) for k in range(A.shape[1])], axis=1)
    return M, ilu.solve


# ---- the pinned systems ----------------------------------------------------------------------------------------------------
BS = {"w": 1, "we": 2, "wce": 3, "wsce": 4}
BOX = ((6, 4, 4), (3, 2, 2))      # 96 cells in 8 bricks of 12 rows
_PINNED = {}


def box(eos, dims=BOX[0], brick=BOX[1]):
    """(LocalMesh, rowptr, colidx) of the small box the solve-ending tests run on"""
    from waiwera_amd.cases import make_case
    g, lm, prim, region = make_case(dims=dims, brick=brick, eos=eos, lens=False)
    rp, ci = mesh_pattern(lm)
    return lm, rp, ci


def dominant(eos, pc):
    """the diagonally dominant system on the box, computed once per process: dict with the mesh, pattern, values, b,
    M = B^-1 A and rb = B^-1 b in long double (pc "bjacobi": ILU(0) on the mesh's bricks; "none")"""
    if (eos, pc) not in _PINNED:
        lm, rp, ci = box(eos)
        bs = BS[eos]
        val = diag_dominant_values(rp, ci, bs)
        b = np.random.default_rng(7).normal(size=lm.n_owned * bs)
        M, apply = preconditioned(rp, ci, val, bs, np.asarray(lm.sub_ptr) if pc == "bjacobi" else None)
        _PINNED[eos, pc] = dict(lm=lm, rp=rp, ci=ci, bs=bs, val=val, b=b, M=M, rb=apply(b), apply=apply)
    return _PINNED[eos, pc]


def double_distance(M, rb, driver, ks, **kw):
    """(x, rnorm): how far the double-precision run of a restatement lies from its long-double run, capped at each k of
    ks -- the worst over them, relative (x to max |x|).  Ten times this is the device's bound"""
    fn = bcgs if driver == "bcgs" else gmres
    dx = dr = 0.0
    for k in ks:
        ref, dbl = fn(M, rb, rtol=1e-30, maxits=k, **kw), fn(M, rb, rtol=1e-30, maxits=k, dtype=np.float64, **kw)
        assert ref[:2] == dbl[:2] == (-3, k), (ref[:2], dbl[:2])
        dx, dr = max(dx, distance(dbl[3], ref[3])), max(dr, abs(float(dbl[2]) - float(ref[2])) / float(ref[2]))
    return dx, dr


# ---- the drivers, restated -----------------------------------------------------------------------------------------------
def _norm(v):
    return np.sqrt(np.dot(v, v))


def _decide(dp, ttol, atol):
    return 3 if dp <= atol else 2


def bcgs(M, rb, rtol=1e-5, atol=1e-50, maxits=10000, dtype=LD, merged=True):
    """KSPBCGS as ksp_bcgs states it, on M = B^-1 A and rb = B^-1 b, zero initial guess.  merged: the residual norm and the
    next rho derived from (S,T), (T,T), (S,S), (S,RP), (T,RP) (derive_merged; every launch form but "petsc"), else reduced
    from R itself.  Returns reason, its, rnorm, x and the history [(x_k, rnorm_k)] of the iterations made"""
    M = np.asarray(M, dtype=dtype)
    R = np.asarray(rb, dtype=dtype).copy()
    n = R.size
    X, P, V = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
    RP = R.copy()
    one = dtype(1.0)
    with np.errstate(all="ignore"):
        dp = _norm(R)
        dp0, ttol = dp, max(dtype(rtol) * dp, dtype(atol))
        rho, rhoold, alpha, omega = np.dot(R, R), one, one, one
        hist = []
        if np.isnan(dp):
            return -9, 0, dp, X, hist
        if dp <= ttol:
            return _decide(dp, ttol, atol), 0, dp, X, hist
        for i in range(maxits):
            beta = (rho / rhoold) * (alpha / omega)
            P = R + beta * (P - omega * V)
            V = M @ P
            d1 = np.dot(V, RP)
            brk = 1 if (d1 == 0.0 or rho == 0.0) else 0
            alpha = rho / d1
            S = R - alpha * V
            T = M @ S
            st, tt = np.dot(S, T), np.dot(T, T)
            if tt == 0.0:
                brk = brk or 2
                omega = dtype(0.0)
            else:
                omega = st / tt
            X = X + alpha * P + omega * S
            R = S - omega * T
            if merged:
                ss, srp, trp = np.dot(S, S), np.dot(S, RP), np.dot(T, RP)
                rr = (ss - 2 * omega * st) + omega * omega * tt
                dp = np.sqrt(rr if rr > 0.0 else dtype(0.0))
                rhonew = srp - omega * trp
            else:
                dp = _norm(R)
                rhonew = np.dot(R, RP)
            rhoold, rho = rho, rhonew
            if rho == 0.0 and brk == 0:
                brk = 3
            hist.append((X.copy(), dp))
            its = i + 1
            if brk == 1:
                return -5, its, dp, X, hist
            if brk == 2:
                return (3 if dp == 0.0 else -5), its, dp, X, hist
            if np.isnan(dp):
                return -9, its, dp, X, hist
            if dp <= ttol:
                return _decide(dp, ttol, atol), its, dp, X, hist
            if brk == 3:
                return -5, its, dp, X, hist
            if dp >= 1.0e4 * dp0:
                return -4, its, dp, X, hist
    return -3, maxits, dp, X, hist


def gmres(M, rb, restart=30, rtol=1e-5, atol=1e-50, maxits=10000, dtype=LD):
    """KSPGMRES as ksp_gmres states it: restarted, classical Gram-Schmidt without refinement, Givens rotations, the
    residual estimate |g_{j+1}| tested per iteration; at a restart the residual B^-1 b - M x is formed anew.  Returns
    reason, its, rnorm (the estimate) and x"""
    M = np.asarray(M, dtype=dtype)
    rb = np.asarray(rb, dtype=dtype)
    n, m = rb.size, max(int(restart), 1)
    x = np.zeros(n, dtype=dtype)
    it, reason = 0, 0
    res = res0 = ttol = dtype(0.0)
    with np.errstate(all="ignore"):
        while not reason:
            v0 = rb.copy() if it == 0 else rb - M @ x
            res = _norm(v0)
            if it == 0:
                res0, ttol = res, max(dtype(rtol) * res, dtype(atol))
                if np.isnan(res):
                    reason = -9
                    break
                if res <= ttol:
                    reason = _decide(res, ttol, atol)
                    break
            if res == 0.0:
                reason = 3
                break
            Vb = np.zeros((m + 1, n), dtype=dtype)
            Vb[0] = v0 * (dtype(1.0) / res)
            H = np.zeros((m + 1, m), dtype=dtype)
            cs, sn, g = np.zeros(m, dtype=dtype), np.zeros(m, dtype=dtype), np.zeros(m + 1, dtype=dtype)
            g[0] = res
            j = 0
            while j < m and not reason:
                w = M @ Vb[j]
                h = Vb[:j + 1] @ w
                w = w - h @ Vb[:j + 1]
                hn = _norm(w)
                Vb[j + 1] = w * (dtype(1.0) / hn)
                H[:j + 1, j] = h
                H[j + 1, j] = hn
                for i in range(j):
                    a, b = H[i, j], H[i + 1, j]
                    H[i, j], H[i + 1, j] = cs[i] * a + sn[i] * b, -sn[i] * a + cs[i] * b
                a, b = H[j, j], H[j + 1, j]
                d = np.sqrt(a * a + b * b)
                cs[j], sn[j] = a / d, b / d
                H[j, j], H[j + 1, j] = d, 0.0
                g[j + 1] = -sn[j] * g[j]
                g[j] = cs[j] * g[j]
                res = abs(g[j + 1])
                it += 1
                if np.isnan(res):
                    reason = -9
                elif res <= ttol:
                    reason = _decide(res, ttol, atol)
                elif res >= 1.0e4 * res0:
                    reason = -4
                elif it >= maxits:
                    reason = -3
                elif hn == 0.0:
                    reason = 3
                j += 1
            y = np.zeros(j, dtype=dtype)
            for i in range(j - 1, -1, -1):
                y[i] = (g[i] - H[i, i + 1:j] @ y[i + 1:]) / H[i, i]
            x = x + y @ Vb[:j]
    return reason, it, res, x


def distance(a, b):
    """max |a - b| / max |b|, in long double"""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), LD(1e-300)))

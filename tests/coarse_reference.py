"""The two-level preconditioner (wai_set_pc_coarse) written from its definition, in numpy.longdouble -- and, with
dtype=numpy.float64, the same formulas as a plain double restatement, whose error against the long-double result is what the
GPU tests take their bounds from (tests/test_hip_pc_coarse.py).

agg[i] in [0, nc) is cell i's aggregate; P is the n bs x nc bs prolongation with P[(i,k),(I,k)] = 1 where agg[i] = I.
    Ac = P^T A P          block (I, J) = sum of the blocks A_ij over i in I, j in J
    restrict   rc = P^T r       prolong   (P y)_i = y[agg[i]]
    additive   z = M^-1 r + P Ac^-1 P^T r
    deflated   y = Ac^-1 P^T r,  z = M^-1 (r - A P y) + P y
M^-1 is the one-level preconditioner, handed in as a function: fused_reference.BlockILU0(...).solve or
asm_reference.AsmRef(...).solve.  Ac^-1 is formed explicitly by Gaussian elimination with partial pivoting.
The double restatement applies M^-1 in double too: as the matrix of that function -- built column by column in long double,
each entry rounded to double once -- times the vector, summed in double."""
import numpy as np

from tests import fused_reference as fr

LD = fr.LD


def prolongation(agg, nc, bs, dtype=LD):
    """P as a dense matrix (small cases only)"""
    agg = np.asarray(agg)
    P = np.zeros((agg.size * bs, nc * bs), dtype=dtype)
    for k in range(bs):
        P[np.arange(agg.size) * bs + k, agg * bs + k] = 1
    return P


def restrict(agg, nc, bs, r, dtype=LD):
    rc = np.zeros((nc, bs), dtype=dtype)
    np.add.at(rc, np.asarray(agg), np.asarray(r, dtype=dtype).reshape(-1, bs))
    return rc.ravel()


def prolong(agg, bs, y, dtype=LD):
    return np.asarray(y, dtype=dtype).reshape(-1, bs)[np.asarray(agg)].ravel()


def galerkin(rowptr, colidx, val, bs, agg, nc, dtype=LD):
    """Ac = P^T A P, dense (nc bs) x (nc bs); columns >= n (ghosts) belong to no aggregate"""
    rowptr, colidx, agg = np.asarray(rowptr), np.asarray(colidx), np.asarray(agg)
    n = len(rowptr) - 1
    V = np.asarray(val, dtype=dtype).reshape(-1, bs, bs)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    own = colidx < n
    Ac = np.zeros((nc, nc, bs, bs), dtype=dtype)
    np.add.at(Ac, (agg[rows[own]], agg[colidx[own]]), V[own])
    return Ac.transpose(0, 2, 1, 3).reshape(nc * bs, nc * bs).copy()


def inverse(A, dtype=LD):
    """A^-1 by Gaussian elimination with partial pivoting on [A | I]; None where a pivot is exactly zero"""
    A = np.asarray(A, dtype=dtype)
    m = A.shape[0]
    W = np.concatenate([A, np.eye(m, dtype=dtype)], axis=1)
    for k in range(m):
        p = k + int(np.argmax(np.abs(W[k:, k])))
        if W[p, k] == 0:
            return None
        if p != k:
            W[[k, p]] = W[[p, k]]
        W[k] = W[k] / W[k, k]
        f = W[:, k].copy()
        f[k] = 0
        W -= f[:, None] * W[k][None, :]
    return W[:, m:].copy()


def matvec(A, x, dtype=LD):
    return (np.asarray(A, dtype=dtype) * np.asarray(x, dtype=dtype)[None, :]).sum(axis=1)


class TwoLevel:
    """both modes' z for one matrix: one_level(r) -> M^-1 r (long double in, long double out)"""

    def __init__(self, rowptr, colidx, val, bs, agg, nc, one_level, dtype=LD):
        self.rp, self.ci, self.val, self.bs = np.asarray(rowptr), np.asarray(colidx), val, bs
        self.agg, self.nc, self.one_level, self.dtype = np.asarray(agg), nc, one_level, dtype
        self.n = len(self.rp) - 1
        self.Ac = galerkin(rowptr, colidx, val, bs, agg, nc, dtype)
        self.Ainv = inverse(self.Ac, dtype)
        self.Minv = None
        if dtype is not LD:      # M^-1 as a matrix of doubles
            eye = np.eye(self.n * bs)
            self.Minv = np.stack([np.asarray(one_level(e.astype(LD)), dtype=dtype) for e in eye], axis=1)

    def coarse(self, r):
        """y = Ac^-1 P^T r"""
        return matvec(self.Ainv, restrict(self.agg, self.nc, self.bs, r, self.dtype), self.dtype)

    def _m(self, r):
        if self.Minv is None:
            return np.asarray(self.one_level(np.asarray(r, dtype=LD)), dtype=LD)
        return matvec(self.Minv, r, self.dtype)

    def spmv(self, x):
        xx = np.zeros(max(int(self.ci.max()) + 1, self.n) * self.bs, dtype=self.dtype)
        xx[:self.n * self.bs] = np.asarray(x, dtype=self.dtype)
        if self.dtype is LD:
            return fr.spmv(self.rp, self.ci, self.val, self.bs, xx)
        V = np.asarray(self.val, dtype=self.dtype).reshape(-1, self.bs, self.bs)
        y = np.zeros((self.n, self.bs), dtype=self.dtype)
        np.add.at(y, np.repeat(np.arange(self.n), np.diff(self.rp)), np.einsum("kab,kb->ka", V, xx.reshape(-1, self.bs)[self.ci]))
        return y.ravel()

    def apply(self, mode, r):
        r = np.asarray(r, dtype=self.dtype)
        y = self.coarse(r)
        Py = prolong(self.agg, self.bs, y, self.dtype)
        if mode == "additive":
            return self._m(r) + Py
        assert mode == "deflated", mode
        return self._m(r - self.spmv(Py)) + Py

    def operator(self, mode, x):
        """z = B^-1 A x"""
        return self.apply(mode, self.spmv(x))

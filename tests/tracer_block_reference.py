"""Host-side helpers of the coupled tracer tests: the coupled system's values ([block][tracer], diagonal blocks stored
as their diagonals) as full BCSR blocks for the oracle's block Krylov solver, and scipy's direct solve of every tracer's
system."""
import numpy as np


def block_values(V):
    """(nnzb, nt) diagonals -> (nnzb, nt, nt) diagonal blocks, row-major inside a block"""
    V = np.asarray(V)
    nnzb, nt = V.shape
    out = np.zeros((nnzb, nt, nt))
    for t in range(nt):
        out[:, t, t] = V[:, t]
    return out


def csr_of(rowptr, colidx, val):
    """one tracer's matrix over the owned cells (columns of ghost / boundary cells do not occur: eliminated into the rhs)"""
    import scipy.sparse as sp
    n = len(rowptr) - 1
    ncol = max(n, int(np.max(colidx)) + 1)
    return sp.csr_matrix((np.asarray(val), np.asarray(colidx), np.asarray(rowptr)), shape=(n, ncol))[:, :n].tocsr()


def direct_solutions(rowptr, colidx, V, b):
    """scipy's direct solve of each tracer's system, interleaved [cell][tracer] like b"""
    import scipy.sparse.linalg as spl
    V = np.asarray(V)
    nt = V.shape[1]
    x = np.zeros_like(np.asarray(b, dtype=np.float64))
    for t in range(nt):
        x[t::nt] = spl.spsolve(csr_of(rowptr, colidx, V[:, t]).tocsc(), b[t::nt])
    return x

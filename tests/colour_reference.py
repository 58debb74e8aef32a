"""Block-Jacobi ILU(0) in multicolour order, in long double, written from the definition (wai_set_pc_ordering):

1. colours, per subdomain of sub_ptr: rows in ascending index, each takes the smallest colour >= 0 none of its already
   coloured in-subdomain neighbours (off-diagonal columns of the pattern inside the subdomain) has;
2. the factor of subdomain s is the block ILU(0) of P A_ss P^T, P sorting the subdomain's rows by (colour, row index),
   with fused_reference.BlockILU0's arithmetic: the matrix is permuted symmetrically (rows, and the columns inside every
   row re-sorted ascending in the new numbering), BlockILU0 runs on it, and vectors are mapped in and out -- the caller
   keeps its numbering."""
import numpy as np

from tests import fused_reference as fr

LD = fr.LD


def mesh_pattern(lm):
    """(rowptr, colidx) of the owned cells' block rows of a LocalMesh: the cell itself and its neighbours among the owned
    and ghost cells, ascending -- what wai_jacobian_pattern returns, without a library"""
    n = lm.n_owned
    nb = [{i} for i in range(n)]
    for a, b in np.asarray(lm.face_cells).tolist():
        if a < n and b < lm.n_prim:
            nb[a].add(b)
        if b < n and a < lm.n_prim:
            nb[b].add(a)
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum([len(s) for s in nb])
    return rp, np.array([j for s in nb for j in sorted(s)], dtype=np.int64)


def greedy_colours(rowptr, colidx, sub_ptr):
    n = len(rowptr) - 1
    sub = np.asarray(sub_ptr)
    owner = np.repeat(np.arange(len(sub) - 1), np.diff(sub))
    colour = np.full(n, -1, dtype=np.int64)
    for i in range(n):
        taken = set()
        for j in colidx[rowptr[i]:rowptr[i + 1]]:
            if j < i and owner[j] == owner[i]:
                taken.add(int(colour[j]))
        c = 0
        while c in taken:
            c += 1
        colour[i] = c
    return colour


def permutation(colour, sub_ptr):
    """new[i]: the position of row i when every subdomain's rows are sorted by (colour, row index)"""
    sub = np.asarray(sub_ptr)
    n = colour.size
    new = np.zeros(n, dtype=np.int64)
    for s in range(len(sub) - 1):
        rows = np.arange(sub[s], sub[s + 1])
        order = rows[np.lexsort((rows, colour[rows]))]
        new[order] = rows
    return new


def permuted_csr(rowptr, colidx, new):
    """P A P^T as CSR with ascending columns: (rowptr, colidx, src), src[q] the block of the caller's pattern that permuted
    block q is; columns >= n (partition ghosts) keep their numbers"""
    rowptr, colidx = np.asarray(rowptr, dtype=np.int64), np.asarray(colidx, dtype=np.int64)
    n = len(rowptr) - 1
    old = np.zeros(n, dtype=np.int64)
    old[new] = np.arange(n)
    prp, pci, src = [0], [], []
    for p in range(n):
        i = old[p]
        q = np.arange(rowptr[i], rowptr[i + 1])
        cols = np.where(colidx[q] < n, new[np.minimum(colidx[q], n - 1)], colidx[q])
        o = np.argsort(cols, kind="stable")
        pci.extend(cols[o].tolist())
        src.extend(q[o].tolist())
        prp.append(len(pci))
    return np.array(prp, dtype=np.int64), np.array(pci, dtype=np.int64), np.array(src, dtype=np.int64)


class ColourILU0:
    def __init__(self, rowptr, colidx, val, bs, sub_ptr):
        rowptr, colidx = np.asarray(rowptr, dtype=np.int64), np.asarray(colidx, dtype=np.int64)
        n = len(rowptr) - 1
        self.n, self.bs, self.rowptr, self.colidx = n, bs, rowptr, colidx
        self.colour = greedy_colours(rowptr, colidx, sub_ptr)
        sub = np.asarray(sub_ptr)
        self.ncolours = np.array([self.colour[sub[s]:sub[s + 1]].max() + 1 for s in range(len(sub) - 1)])
        self.new = new = permutation(self.colour, sub_ptr)
        V = np.asarray(val, dtype=LD).reshape(-1, bs, bs)
        prp, pci, self.src = permuted_csr(rowptr, colidx, new)
        self.ilu = fr.BlockILU0(prp, pci, V[self.src].ravel(), bs, sub_ptr)
        self.offdiag_updates = self.ilu.offdiag_updates

    def factor_blocks(self):
        """the stored factor in the caller's numbering: {(i, j): block} -- L multipliers below the permuted diagonal, U on
        and above it (the pivot itself, not inverted)"""
        old = np.zeros(self.n, dtype=np.int64)
        old[self.new] = np.arange(self.n)
        L, U = self.ilu.L_blocks()
        out = {(int(old[a]), int(old[b])): blk for (a, b), blk in L.items()}
        out.update({(int(old[a]), int(old[b])): blk for (a, b), blk in U.items()})
        return out

    def solve(self, r):
        bs = self.bs
        R = np.asarray(r, dtype=LD).reshape(self.n, bs)
        rp = np.zeros_like(R)
        rp[self.new] = R
        zp = self.ilu.solve(rp.ravel()).reshape(self.n, bs)
        return zp[self.new].ravel()

    def operator(self, val, x):
        return self.solve(fr.spmv(self.rowptr, self.colidx, val, self.bs, x))

"""Restricted additive Schwarz (PCASM, restrict) with ILU(k) sub-solves, restated from the definitions for the tests of the
fused PCASM launch (tests/test_hip_asm_fused.py) -- pure Python, no GPU:

- the extended row sets: per block of sub_ptr the owned rows plus `overlap` rounds of graph neighbours (the pattern's
  columns), sorted;
- the extended system E: every block's rows restricted to its own set (columns outside it dropped), in one numbering,
  block b's rows at ext_ptr[b] .. ext_ptr[b + 1];
- ILU(k) fill of E by iluk_pattern of tests/test_hip_iluk_fused.py (imported, not copied);
- the application in long double by fused_reference.BlockILU0 on E with sub = ext_ptr: gather r by ext_row, solve, keep the
  rows each block owns."""
import numpy as np

from tests import fused_reference as fr


def extended_sets(rp, ci, sub, overlap):
    """(ext_ptr, ext_row, owned): block b's overlapped rows are ext_row[ext_ptr[b]:ext_ptr[b + 1]], ascending; owned marks
    the rows of the block's own [sub[b], sub[b + 1])"""
    rp, ci, sub = np.asarray(rp), np.asarray(ci), np.asarray(sub)
    n = len(rp) - 1
    ext_ptr, rows_all, owned_all = [0], [], []
    for b in range(len(sub) - 1):
        rows = np.arange(sub[b], sub[b + 1])
        front = rows
        for _ in range(overlap):
            nb = np.concatenate([ci[rp[i]:rp[i + 1]] for i in front]) if front.size else front
            nb = np.unique(nb[nb < n])
            front = np.setdiff1d(nb, rows, assume_unique=True)
            rows = np.union1d(rows, front)
        rows_all.append(rows)
        owned_all.append((rows >= sub[b]) & (rows < sub[b + 1]))
        ext_ptr.append(ext_ptr[-1] + rows.size)
    return np.array(ext_ptr, dtype=np.int64), np.concatenate(rows_all).astype(np.int64), np.concatenate(owned_all)


def extended_pattern(rp, ci, ext_ptr, ext_row):
    """E's BCSR pattern in the extended numbering and, per entry, the index of the entry of (rp, ci) it holds"""
    rp, ci = np.asarray(rp), np.asarray(ci)
    n = len(rp) - 1
    erp, eci, esrc = [0], [], []
    loc = np.full(n, -1, dtype=np.int64)
    for b in range(len(ext_ptr) - 1):
        a0, b0 = ext_ptr[b], ext_ptr[b + 1]
        loc[ext_row[a0:b0]] = np.arange(a0, b0)
        for q in range(a0, b0):
            i = ext_row[q]
            e = np.arange(rp[i], rp[i + 1])
            cols = ci[e]
            keep = cols < n
            e, cols = e[keep], cols[keep]
            keep = loc[cols] >= 0
            eci.append(loc[cols[keep]])
            esrc.append(e[keep])
            erp.append(erp[-1] + int(keep.sum()))
        loc[ext_row[a0:b0]] = -1
    return np.array(erp, dtype=np.int64), np.concatenate(eci), np.concatenate(esrc)


class AsmPattern:
    """everything of the reference that depends on the pattern alone: shared among matrices"""

    def __init__(self, rp, ci, sub, overlap, levels=0):
        self.rp, self.ci = np.asarray(rp), np.asarray(ci)
        self.n = len(self.rp) - 1
        self.ext_ptr, self.ext_row, self.owned = extended_sets(rp, ci, sub, overlap)
        erp, eci, esrc = extended_pattern(rp, ci, self.ext_ptr, self.ext_row)
        if levels > 0:
            from tests.test_hip_iluk_fused import iluk_pattern
            rpf, cif, src, width = iluk_pattern(erp, eci, self.ext_ptr, levels)
            self.erp, self.eci = rpf, cif
            self.esrc = np.where(src >= 0, esrc[np.maximum(src, 0)], -1)   # -1: fill, starts at zero
        else:
            self.erp, self.eci, self.esrc = erp, eci, esrc
            width = int(np.diff(erp).max())
        self.width = int(width)                              # most blocks of any row of E
        self.max_rows = int(np.diff(self.ext_ptr).max())     # rows of the largest extended block
        # every row is owned by exactly one block
        assert np.array_equal(np.sort(self.ext_row[self.owned]), np.arange(self.n))


class AsmRef:
    """z = sum_b R~_b^T ILU(k)(R_b A R_b^T)^-1 R_b r in long double; solve / operator as fused_reference.BlockILU0 has them"""

    def __init__(self, pat, val, bs):
        self.pat, self.bs = pat, bs
        V = np.asarray(val).reshape(-1, bs, bs)
        Vf = np.zeros((pat.eci.size, bs, bs))
        have = pat.esrc >= 0
        Vf[have] = V[pat.esrc[have]]
        self.ilu = fr.BlockILU0(pat.erp, pat.eci, Vf.ravel(), bs, pat.ext_ptr)

    def solve(self, r):
        p, bs = self.pat, self.bs
        r_ext = np.asarray(r, dtype=fr.LD).reshape(-1, bs)[p.ext_row]
        z_ext = self.ilu.solve(r_ext.ravel()).reshape(-1, bs)
        z = np.zeros((p.n, bs), dtype=fr.LD)
        z[p.ext_row[p.owned]] = z_ext[p.owned]
        return z.ravel()

    def operator(self, val, x):
        return self.solve(fr.spmv(self.pat.rp, self.pat.ci, val, self.bs, x))


# ---- the shapes the tests share: id -> (eos, dims, brick, overlap, ILU level) ---------------------------------------------
CASES = {
    "we_ragged": ("we", (12, 10, 9), (4, 4, 2), 1, 0),        # ragged bricks, 45 blocks (not a multiple of 8), 2 x 2 staged form
    "wce_ragged": ("wce", (13, 9, 5), (5, 4, 2), 1, 0),       # 3 x 3 blocks: the parked form
    "w_bs1": ("w", (12, 10, 9), (4, 4, 4), 1, 0),             # 1 x 1 blocks
    "wsce_bs4": ("wsce", (8, 8, 4), (4, 4, 4), 1, 0),         # 4 x 4 blocks
    "we_overlap2": ("we", (12, 10, 9), (4, 4, 2), 2, 0),      # rows two layers out
    "we_ilu1": ("we", (12, 10, 9), (4, 4, 2), 1, 1),          # filled E
    "we_full_block": ("we", (48, 42, 6), (16, 14, 2), 1, 0),  # an interior block of 1016 rows: 16 waves, the last partly idle
}
# an interior 16 x 16 x 2 brick extends to 1152 rows at overlap 1: more than a workgroup has threads
TOO_BIG = ("we", (48, 48, 6), (16, 16, 2), 1, 0)


def interior_rows(a, b, c):
    """rows of an interior a x b x c brick of a 7-point mesh at overlap 1: the brick and its six faces' neighbours (the
    overlap follows graph adjacency: no edge or corner cells)"""
    return a * b * c + 2 * (a * b + a * c + b * c)

"""An independent extended-precision restatement of one preconditioned-operator application, for the tests of the fused
launches (tests/test_hip_fused_operator.py) -- written from the definitions, not from the kernels or the oracle:

- A x from the BCSR pattern and values (setup_jacobian / jacobian_values: bs x bs row-major blocks);
- block ILU(0) on each subdomain of sub_ptr: the general IKJ elimination restricted to the pattern (what PCBJACOBI with
  ILU(0) sub-solves computes), couplings that leave a subdomain dropped; pivot blocks inverted by Gauss-Jordan in
  long double (numpy.linalg has no long-double loops);
- inner products in long double together with sum |a_i b_i| for the error bar;
- the BiCGStab scalars the fused launches derive (derive_scalars, derive_merged, derive_rotate of reductions.hip.h),
  restated as formulas in double.

Everything runs in numpy.longdouble: 80-bit extended precision on x86-64 hosts, so that the reference carries no fp64
rounding of its own."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "the reference needs 80-bit (or wider) long double"

# device scalar slots (waiwera_amd/csrc/context.hpp)
S_RHO, S_RHOOLD, S_ALPHA, S_OMEGA, S_BETA, S_D1, S_D2, S_DP2, S_RHONEW, S_W2, S_BREAK = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15


def inv_blocks(B):
    """inverses of a stack of small blocks (m, bs, bs): Gauss-Jordan with partial pivoting, in long double"""
    B = np.asarray(B, dtype=LD)
    m, bs, _ = B.shape
    A = np.concatenate([B, np.broadcast_to(np.eye(bs, dtype=LD), (m, bs, bs))], axis=2).copy()
    ar = np.arange(m)
    for c in range(bs):
        p = c + np.argmax(np.abs(A[:, c:, c]), axis=1)
        rc, rp = A[ar, c].copy(), A[ar, p].copy()
        A[ar, p] = rc
        A[ar, c] = rp
        A[:, c] /= A[:, c, c].copy()[:, None]
        for r in range(bs):
            if r != c:
                A[:, r] -= A[:, r, c].copy()[:, None] * A[:, c]
    return A[:, :, bs:].copy()


def spmv(rowptr, colidx, val, bs, x):
    """y = A x in long double (x: n_cols * bs, any float type)"""
    n = len(rowptr) - 1
    V = np.asarray(val, dtype=LD).reshape(-1, bs, bs)
    X = np.asarray(x, dtype=LD).reshape(-1, bs)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    prod = np.einsum("kab,kb->ka", V, X[colidx])
    y = np.zeros((n, bs), dtype=LD)
    np.add.at(y, rows, prod)
    return y.ravel()


def dot(a, b):
    """(a, b) and sum |a_i b_i| in long double"""
    p = np.asarray(a, dtype=LD) * np.asarray(b, dtype=LD)
    return p.sum(), np.abs(p).sum()


class BlockILU0:
    """Block-Jacobi ILU(0) over the subdomains [sub_ptr[s], sub_ptr[s + 1]): for every row i in order, for every
    in-subdomain k < i of its pattern in ascending order, L_ik = A_ik inv(U_kk), then A_ij -= L_ik U_kj for every j > k
    in both row i's and row k's pattern -- off-diagonal fill included, no assumption that ILU(0) is DILU.  Rows are
    processed level by level (a row's level: one more than its in-subdomain lower neighbours'), which is the same
    arithmetic in a different order of independent rows."""

    def __init__(self, rowptr, colidx, val, bs, sub_ptr):
        rowptr, colidx = np.asarray(rowptr), np.asarray(colidx)
        self.n, self.bs = n, bs = len(rowptr) - 1, bs
        self.rowptr, self.colidx = rowptr, colidx
        sub = np.asarray(sub_ptr)
        owner = np.repeat(np.arange(len(sub) - 1), np.diff(sub))
        assert owner.size == n
        F = np.asarray(val, dtype=LD).reshape(-1, bs, bs).copy()
        lower, upper, diag, pos = [], [], np.zeros(n, dtype=np.int64), []
        for i in range(n):
            lo, hi = rowptr[i], rowptr[i + 1]
            d = {}
            li, ui = [], []
            for q in range(lo, hi):
                j = int(colidx[q])
                if j >= n or owner[j] != owner[i]:
                    continue                       # dropped: the coupling leaves the subdomain
                d[j] = q
                if j < i:
                    li.append((j, q))
                elif j > i:
                    ui.append((j, q))
                else:
                    diag[i] = q
            assert i in d, "row %d has no diagonal block" % i
            lower.append(sorted(li))
            upper.append(sorted(ui))
            pos.append(d)
        levf = np.zeros(n, dtype=np.int64)
        for i in range(n):
            if lower[i]:
                levf[i] = 1 + max(levf[k] for k, _ in lower[i])
        levb = np.zeros(n, dtype=np.int64)
        for i in range(n - 1, -1, -1):
            if upper[i]:
                levb[i] = 1 + max(levb[j] for j, _ in upper[i])
        # the elimination, batched over the rows of a level and the p-th lower coupling of each
        dinv = np.zeros((n, bs, bs), dtype=LD)
        nlev = int(levf.max()) + 1
        by_lev = [[] for _ in range(nlev)]
        for i in range(n):
            by_lev[levf[i]].append(i)
        for lev in range(nlev):
            rows = by_lev[lev]
            maxl = max(len(lower[i]) for i in rows)
            for p in range(maxl):
                sc_q, sc_k, up_ij, up_ik, up_kj = [], [], [], [], []
                for i in rows:
                    if len(lower[i]) <= p:
                        continue
                    k, qik = lower[i][p]
                    sc_q.append(qik)
                    sc_k.append(k)
                    for j, qij in pos[i].items():
                        if j > k and j in pos[k]:
                            up_ij.append(qij)
                            up_ik.append(qik)
                            up_kj.append(pos[k][j])
                sc_q = np.array(sc_q, dtype=np.int64)
                F[sc_q] = np.matmul(F[sc_q], dinv[np.array(sc_k, dtype=np.int64)])
                if up_ij:
                    up_ij = np.array(up_ij, dtype=np.int64)
                    F[up_ij] -= np.matmul(F[np.array(up_ik, dtype=np.int64)], F[np.array(up_kj, dtype=np.int64)])
            r = np.array(rows, dtype=np.int64)
            dinv[r] = inv_blocks(F[diag[r]])
        self.F, self.dinv, self.diag = F, dinv, diag
        self.lower, self.upper = lower, upper
        # off-diagonal fill: did any elimination step update a block other than a diagonal one?
        self.offdiag_updates = any(j != i and j in pos[k] for i in range(n) for k, _ in lower[i] for j in pos[i] if j > k)
        # the sweeps' batches: forward by levf ascending, backward by levb ascending
        self._fw = self._batches(levf, lower)
        self._bw = self._batches(levb, upper)

    @staticmethod
    def _batches(lev, nbrs):
        out = []
        for L in range(int(lev.max()) + 1):
            rows = np.nonzero(lev == L)[0]
            ii, qq, kk = [], [], []
            for i in rows:
                for k, q in nbrs[i]:
                    ii.append(i); qq.append(q); kk.append(k)
            out.append((rows, np.array(ii, dtype=np.int64), np.array(qq, dtype=np.int64), np.array(kk, dtype=np.int64)))
        return out

    def L_blocks(self):
        """{(i, k): L_ik} of the factor (unit diagonal implied) and {(i, j): U_ij} with U_ii = the pivot"""
        L = {(i, k): self.F[q] for i in range(self.n) for k, q in self.lower[i]}
        U = {(i, j): self.F[q] for i in range(self.n) for j, q in self.upper[i]}
        for i in range(self.n):
            U[(i, i)] = self.F[self.diag[i]]
        return L, U

    def solve(self, r):
        """z = U^-1 L^-1 r in long double"""
        bs = self.bs
        y = np.asarray(r, dtype=LD).reshape(self.n, bs).copy()
        for rows, ii, qq, kk in self._fw:
            if ii.size:
                acc = np.zeros((self.n, bs), dtype=LD)
                np.add.at(acc, ii, np.einsum("mab,mb->ma", self.F[qq], y[kk]))
                y[rows] -= acc[rows]
        z = y
        for rows, ii, qq, kk in self._bw:
            if ii.size:
                acc = np.zeros((self.n, bs), dtype=LD)
                np.add.at(acc, ii, np.einsum("mab,mb->ma", self.F[qq], z[kk]))
                z[rows] -= acc[rows]
            z[rows] = np.einsum("mab,mb->ma", self.dinv[rows], z[rows])
        return z.ravel()

    def operator(self, val, x):
        """z = B^-1 A x"""
        return self.solve(spmv(self.rowptr, self.colidx, val, self.bs, x))


# ---- the BiCGStab scalars of the in-launch finalisation (reductions.hip.h: derive_merged, derive_rotate, derive_scalars),
# restated in double.  The breakdown codes are left to the kernels except where noted.
def derive_merged(s):
    st, tt, ss, srp, trp = s[S_D1], s[S_D2], s[S_DP2], s[S_RHONEW], s[S_W2]
    if tt == 0.0:
        s[S_BREAK], s[S_OMEGA] = 2.0, 0.0
    else:
        s[S_OMEGA] = st / tt
    om = s[S_OMEGA]
    rr = (ss - 2.0 * om * st) + om * om * tt
    s[S_DP2] = rr if rr > 0.0 else 0.0
    s[S_RHONEW] = srp - om * trp


def derive_rotate(s):
    s[S_RHOOLD], s[S_RHO] = s[S_RHO], s[S_RHONEW]
    s[S_BETA] = (s[S_RHO] / s[S_RHOOLD]) * (s[S_ALPHA] / s[S_OMEGA])


def derive(s_in, phase):
    """the scalars after derive_scalars(phase) of the 16 scalars s_in; which slots it writes (with a scale for each:
    the sum of the magnitudes of the terms, for a relative bar that survives cancellation)"""
    s = [float(v) for v in s_in]
    scale = {}
    if phase == 0:
        s[S_RHO] = s[S_DP2]
        s[S_RHOOLD] = s[S_ALPHA] = s[S_OMEGA] = 1.0
        s[S_BETA] = (s[S_RHO] / s[S_RHOOLD]) * (s[S_ALPHA] / s[S_OMEGA])
        scale = {S_RHO: abs(s[S_RHO]), S_RHOOLD: 1.0, S_ALPHA: 1.0, S_OMEGA: 1.0, S_BETA: abs(s[S_BETA])}
        if s[S_BREAK] != 4.0:
            s[S_BREAK] = 1.0 if s[S_RHO] == 0.0 else 0.0
            scale[S_BREAK] = 0.0
    elif phase == 2:
        s[S_ALPHA] = s[S_RHO] / s[S_D1]
        scale = {S_ALPHA: abs(s[S_ALPHA])}
    elif phase == 3:
        s[S_OMEGA] = s[S_D1] / s[S_D2]
        scale = {S_OMEGA: abs(s[S_OMEGA])}
    elif phase in (5, 6):
        st, tt, ss, srp, trp = s[S_D1], s[S_D2], s[S_DP2], s[S_RHONEW], s[S_W2]
        derive_merged(s)
        om = s[S_OMEGA]
        scale = {S_OMEGA: abs(om), S_DP2: abs(ss) + abs(2.0 * om * st) + abs(om * om * tt), S_RHONEW: abs(srp) + abs(om * trp)}
        if phase == 6:
            derive_rotate(s)
            scale.update({S_RHOOLD: abs(s[S_RHOOLD]), S_RHO: scale[S_RHONEW], S_BETA: abs(s[S_BETA])})
    elif phase == 4:
        derive_rotate(s)
        scale = {S_RHOOLD: abs(s[S_RHOOLD]), S_RHO: abs(s[S_RHO]), S_BETA: abs(s[S_BETA])}
    return np.array(s), scale


# ---- the products each dot mode forms (krylov.hip: pc_dots / mode_slots) ------------------------------------------------
def mode_products(dot_mode, x, z, aux):
    """[(slot, a, b)] of a dot mode: x is the operand (x - alpha x2 where composed)"""
    return {0: [], 1: [(S_D1, z, aux)], 2: [(S_D1, x, z), (S_D2, z, z)], 3: [(S_DP2, z, z)],
            4: [(S_D1, x, z), (S_D2, z, z), (S_DP2, x, x), (S_RHONEW, x, aux), (S_W2, z, aux)]}[dot_mode]


# ---- meshes the tests share ----------------------------------------------------------------------------------------------
def triangle_mesh(eos="we", dims=(10, 9, 1), brick=(5, 3, 1)):
    """a one-layer structured mesh with diagonal connections (i, j) - (i + 1, j + 1) added: the cell graph has
    triangles, the IKJ elimination updates off-diagonal blocks and the library takes the stored-factor kernels
    (tests/test_hip_pc.py::test_ilu0_with_off_diagonal_fill builds the same mesh)"""
    from waiwera_amd.cases import make_case
    g, lm, prim, region = make_case(dims=dims, brick=brick, eos=eos, lens=False, top_bc=False)
    ijk = np.asarray(lm.owned_ijk)
    idx = {(int(a), int(b)): q for q, (a, b, c) in enumerate(ijk)}
    fc = np.asarray(lm.face_cells)
    fg_x = None
    for f in range(lm.n_faces):
        a, b = fc[f]
        if a < lm.n_owned and b < lm.n_owned and abs(ijk[a][0] - ijk[b][0]) == 1:
            fg_x = np.asarray(lm.face_geom)[f].copy()
            break
    extra_c, extra_g = [], []
    for (i, j), q in idx.items():
        if (i + 1, j + 1) in idx:
            row = fg_x.copy()
            row[0] *= 0.3
            row[1] = row[2] = 0.5 * np.hypot(10.0, 10.0)
            row[3] = row[1] + row[2]
            extra_c.append((q, idx[(i + 1, j + 1)]))
            extra_g.append(row)
    lm.face_cells = np.concatenate([fc, np.array(extra_c, dtype=np.int32)]).astype(np.int32)
    lm.face_geom = np.concatenate([np.asarray(lm.face_geom), np.array(extra_g)])
    lm.n_faces = lm.face_cells.shape[0]
    return g, lm, prim, region


def random_values(rowptr, colidx, bs, rng):
    """O(1) random blocks on the pattern, every block entry filled (also where a single-phase cell's block is
    structurally zero), diagonal blocks made dominant"""
    n = len(rowptr) - 1
    V = rng.uniform(-1.0, 1.0, size=(len(colidx), bs, bs))
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    dq = np.nonzero(colidx == rows)[0]
    rowsum = np.zeros((n, bs))
    np.add.at(rowsum, rows, np.abs(V).sum(axis=2))
    V[dq] += (rowsum[rows[dq]] + 1.0)[:, :, None] * np.eye(bs)[None]
    return V.ravel()


def spread_vector(n, bs, rng, decades=4):
    """per-component magnitudes spread over several decades (like scaled primaries), entries of both signs"""
    comp = 10.0 ** (-np.arange(bs) * decades / max(bs - 1, 1))
    return (rng.normal(size=(n, bs)) * comp * 10.0 ** rng.uniform(-1.0, 1.0, size=(n, 1))).ravel()

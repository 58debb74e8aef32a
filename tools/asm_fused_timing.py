"""Times one preconditioned-operator application z = B^-1 (A x) with its (z, aux) product under PCASM (overlap 1, ILU(0))
two ways on the same matrix and factor pattern (wai_bench_kernel 2: what a BiCGStab half-iteration runs): the fused
launch (k_pc_wide with a row map on the extended system) and, under WAI_ASM_UNFUSED=1, the launches it replaces (k_spmv,
k_asm_gather, k_pc on the extended system, k_asm_scatter, k_dots, k_finalize); beside them block Jacobi on the same bricks.
One JSON line per case:

    python tools/asm_fused_timing.py > profiles/asm_fused_timing.json

Algorithmic bytes (bs x bs blocks of 8-byte entries, 4-byte indices; N rows and nnzb blocks of A, n_ext rows and nnz_E
blocks of the extended system E -- both counted here from the mesh: a cell joins every block it is adjacent to, a
connection every block that holds both its cells):
  fused    A's rows once per block that holds them (nnz_A_ext blocks + columns: every row of E multiplies its row of A, an
           overlap row's product is formed again by each block it lies in -- where the unfused path gathers 8 bs bytes),
           x, E (nnz_E blocks + columns), ext_row and the row descriptor (12 bytes per row of E), z written, aux read;
  unfused  k_spmv: A, x, t written; gather: t read at n_ext rows, ext_row, r_ext written; k_pc on E: E (nnz_E blocks +
           columns), the inverted pivots and the descriptor per row of E, r_ext read and written; scatter: r_ext, ext_row,
           z written; k_dots: z and aux read.
Each as a share of the 8 TB/s HBM peak at the time measured."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waiwera_amd.cases import make_case, scaled  # noqa: E402
from waiwera_amd.flow_simulation import FlowSimulation  # noqa: E402

PEAK = 8.0e12
# (eos, dims, brick): 16 x 14 x 2 bricks extend to at most 1016 rows at overlap 1 (16 x 16 x 2: 1152, unfused either way)
# -- and a 12 096-cell mesh of the same bricks, where the launches themselves are what an application costs
CASES = [("we", (216, 216, 216), (16, 14, 2)), ("we", (100, 100, 100), (16, 14, 2)), ("we", (48, 42, 6), (16, 14, 2))]


def extended_counts(lm):
    """(n_ext, nnz_E, nnz_A_ext) at overlap 1: rows and blocks of the extended system over all blocks, and the blocks of A's
    rows summed over the rows of E"""
    n = lm.n_owned
    sub = np.asarray(lm.sub_ptr)
    owner = np.repeat(np.arange(len(sub) - 1, dtype=np.int64), np.diff(sub))
    fc = np.asarray(lm.face_cells, dtype=np.int64)
    fc = fc[(fc[:, 0] < n) & (fc[:, 1] < n)]
    u, v = fc[:, 0], fc[:, 1]
    nb = np.int64(len(sub))
    cross = owner[u] != owner[v]
    member = np.unique(np.concatenate([np.arange(n, dtype=np.int64) * nb + owner, u[cross] * nb + owner[v[cross]],
                                       v[cross] * nb + owner[u[cross]]]))            # (cell, block) pairs, sorted
    cell = member // nb
    start = np.searchsorted(cell, np.arange(n + 1))
    cnt = np.diff(start)
    both = 0
    for k in range(int(cnt.max())):       # the k-th block cell u belongs to: does it hold v too?
        has = cnt[u] > k
        key = v[has] * nb + member[start[u[has]] + k] % nb
        pos = np.searchsorted(member, key)
        both += int((member[np.minimum(pos, member.size - 1)] == key).sum())
    rowcnt = 1 + np.bincount(u, minlength=n) + np.bincount(v, minlength=n)
    return int(member.size), int(member.size + 2 * both), int(rowcnt[cell].sum())


def main():
    for eos, dims, brick in CASES:
        g, lm, prim, region = make_case(dims=dims, brick=brick, eos=eos, lens=True)
        bs = 2
        n_ext, nnz_e, nnz_a_ext = extended_counts(lm)
        sim = FlowSimulation(lm, eos=eos)
        sim.set_regions(region)
        sim.set_opts(pc_type="asm", asm_overlap=1, ilu_levels=0)
        rp, ci = sim.setup_jacobian()
        N, nnzb = lm.n_owned, len(ci)
        y = scaled(prim, region, eos).ravel().copy()
        L = np.zeros(sim.num_dof)
        assert sim.pre_eval(0.0, y) == 0
        sim.lhs(0.0, 1.0, y, L)
        assert sim.jacobian(0.0, 5.0e4, y, L) == 0
        blk, vec = bs * bs * 8 + 4, bs * 8
        a_bytes, e_bytes = nnzb * blk, nnz_e * blk
        nbytes = dict(fused=nnz_a_ext * blk + N * vec + e_bytes + n_ext * 12 + 2 * N * vec,
                      unfused=(a_bytes + 2 * N * vec) + (n_ext * (2 * vec + 4)) + (e_bytes + n_ext * (bs * bs * 8 + 4 + 2 * vec))
                      + (N * 2 * vec + n_ext * 4) + 2 * N * vec)
        row = dict(eos=eos, dims=dims, brick=brick, bricks=len(lm.sub_ptr) - 1, n=N, n_ext=n_ext, nnzb=nnzb, nnz_ext=nnz_e, nnz_a_over_ext_rows=nnz_a_ext)
        for form in ("fused", "unfused"):
            if form == "unfused":
                os.environ["WAI_ASM_UNFUSED"] = "1"
            else:
                os.environ.pop("WAI_ASM_UNFUSED", None)
            assert sim.pc_setup() == 0
            ms = sim.bench_kernel(2, reps=50)
            row[form] = dict(kernel=sim.pc_kernel_name(), ms=ms, solve_only_ms=sim.bench_kernel(1, reps=50),
                             algorithmic_bytes=nbytes[form], share_of_hbm_peak=nbytes[form] / (ms * 1e-3) / PEAK)
        os.environ.pop("WAI_ASM_UNFUSED", None)
        row["spmv_ms"] = sim.bench_kernel(0, reps=50)
        sim.set_opts(pc_type="bjacobi")
        assert sim.pc_setup() == 0
        row.update(bjacobi_kernel=sim.pc_kernel_name(), bjacobi_fused_ms=sim.bench_kernel(2, reps=50))
        print(json.dumps(row), flush=True)
        sim.destroy()


if __name__ == "__main__":
    main()

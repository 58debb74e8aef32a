// The fused kernel for rows of 9 .. 16 blocks, k_pc_wide.
#pragma once
#include "reductions.hip.h"

namespace wai {

// ---- K6+K8 fused for rows of 9 .. 16 blocks (stored factor) ---------------------------------------
// Meshes whose cells have up to 16 faces (polygonal columns, quad columns refined around the wells: a coarse column and
// two fine neighbours along one side are pairwise adjacent) have triangles in their cell graph: ILU(0) fills
// off-diagonal blocks, so the factor is stored (k_ilu_factor_wide) and the DILU forms never apply.  k_pc holds a row's
// factor in registers; at 16 slots that is 64 doubles for 2 x 2 blocks and 144 for 3 x 3, beyond the register file.  Here
// a thread keeps nothing of its row across the sweeps but the inverted pivot block:
//   load phase  t = A x streamed slot by slot (ell_row_mult, 16 guarded slots); the row's in-subdomain upper blocks of the
//               factor are parked in LDS behind the solution vector while the loads of the whole brick are in flight --
//               as many rows as fit the 64 KB a workgroup may ask for (rows in order, a row parks all of its upper blocks
//               or none: `ucap`); the others re-read theirs from memory in the backward sweep;
//   forward     y_i = t_i - sum_k L_ik y_k at the row's level, each lower block read once from memory;
//   backward    x_i = inv(D_i) (y_i - sum_j U_ij x_j), upper blocks from LDS where parked.
// Every factor block is read once per application, so the launch moves about what the launch-per-level path moves
// without its 2 x levels launches and the separate SpMV.  One workgroup per subdomain (<= 1024 rows), one thread per block
// row; k_pc's interface: dot modes, finaliser workgroups, sub_list (the interior / face split of the halo exchange).
// FILL: two patterns in one launch -- block-Jacobi ILU(k), k > 0, on a mesh of at most 8 blocks per row.  The operator keeps
// the Jacobian's narrow rows (W <= 8 slots on `col`, neighbour gathers included: ell_row_mult as the narrow kernels call
// it); the factor has the filled pattern (<= 16 slots per row, in-brick columns only) on column planes of its own, `fcol`,
// which the descriptor's slots, the two sweeps and the parked upper blocks refer to.  Both have n rows in the same order.
// NS > 0 (FILL, 1 x 1 and 2 x 2 blocks; rows of at most NS lower and NS upper in-brick blocks): nothing is fetched inside a
// level.  In the form above a row waits for its lower blocks at its own level, so every one of a brick's levels pays a
// memory round trip -- and ILU(1) in a 16 x 16 x 2 brick has about three times the levels of ILU(0).  Here all rows of the
// brick fetch their lower blocks and columns into registers at once before the forward sweep, and their upper blocks into
// the SAME registers at once between the sweeps: two round trips per brick instead of two per level, the sweeps touch LDS
// alone, and nothing is parked (LDS: the solution and the reduction scratch).  Same arithmetic in the same order as the
// form above.  tools/iluk_fused_timing.py times both forms against the launch-per-level path on the same factor.
// MAP (with FILL): the factor's rows are not the operator's -- PCASM's extended system (AsmSystem::E, any overlap, ILU(k),
// k >= 0).  Two row counts: thread tid of block s is FACTOR row fi = sub_ptr[s] + tid of nf = n_ext rows, and everything read
// through the factor's planes (fval, fcol, row_infow, row_uoffw, the parked blocks) is indexed by fi with plane stride nf;
// it stands for OPERATOR row i = ext_row[fi] & 0x7fffffff of n rows, and everything of the operator (col, aval, rowptr,
// in, aux, z) is indexed by i with plane stride n.  The load phase is t_fi = (A x)_i by the same ell_row_mult call as
// k_spmv makes on row i (the bits the unfused path gathers), or in[i]; the sweeps are unchanged; z[i] is stored only where
// ext_row[fi] < 0 -- the rows the block owns (restricted Schwarz), each owned by exactly one block, so the inner products
// masked the same way are the whole-vector products.  NOT in place: a block reads `in` at rows another block writes
// (launch_pc_on refuses z == in).
// stage_blocks issues NS column and block loads for every row, branch-free: a row with fewer blocks re-reads its own pivot
// slot as filler (in bounds, never used; the same lines the pivot load fetches, so cache hits rather than HBM bytes).
template <int BS, int NS>
__device__ __forceinline__ void stage_blocks(int n, int i, int lo, int q0, int cnt, int dslot, const int* __restrict__ fc,
                                             const double* __restrict__ fval, int (&kc)[NS], double (&m)[NS][BS * BS]) {
#pragma unroll
  for (int p = 0; p < NS; p++) {
    const int q = p < cnt ? q0 + p : dslot;   // a slot of the row's own either way (the pivot's: not used)
    kc[p] = fc[(size_t)q * n + i] - lo;
    load_block<BS>(fval, n, q, i, m[p]);
  }
}
template <int BS, int NS>
__device__ __forceinline__ void staged_row_sub(int cnt, const int (&kc)[NS], const double (&m)[NS][BS * BS], const double* ys, double* a) {
#pragma unroll
  for (int p = 0; p < NS; p++) {
    if (p < cnt) {
      double yk[BS];
#pragma unroll
      for (int c = 0; c < BS; c++) yk[c] = ys[kc[p] * BS + c];
#pragma unroll
      for (int r = 0; r < BS; r++)
#pragma unroll
        for (int c = 0; c < BS; c++) a[r] -= m[p][r * BS + c] * yk[c];
    }
  }
}

template <int BS, bool SPMV, bool FILL = false, int NS = 0, bool MAP = false>
__global__ __launch_bounds__(1024) void k_pc_wide(int n, int W, int nsub, const int* __restrict__ sub_ptr,
                                                  const int* __restrict__ sub_nlev,
                                                  const unsigned long long* __restrict__ row_infow,
                                                  const int* __restrict__ row_uoffw, const int* __restrict__ col,
                                                  const int* __restrict__ rowptr, const double* __restrict__ aval,
                                                  const double* __restrict__ fval, const double* __restrict__ in,
                                                  double* __restrict__ z, const double* __restrict__ aux, double* partials,
                                                  int nb_max, int dot, int ucap, const int* __restrict__ sub_list, Fin fin,
                                                  const int* __restrict__ fcol, int nf_map,
                                                  const int* __restrict__ ext_row) {
  static_assert(FILL || !MAP, "a row map needs the factor's own column planes");
  constexpr int BB = BS * BS;
  const int nf = MAP ? nf_map : n;   // rows (plane stride) of the factor; n: of the operator
  const int* __restrict__ fc = FILL ? fcol : col;   // the factor's column planes
  extern __shared__ __attribute__((aligned(16))) double lds[];  // [T * BS] solution, 80 doubles reduction scratch, [ucap][BB] parked upper blocks
  if (fin_block(fin, partials, nb_max)) return;
  int s = xcd_remap(blockIdx.x, nsub);
  if (s >= nsub) return;
  if (sub_list) s = sub_list[s];
  const int lo = sub_ptr[s], R = sub_ptr[s + 1] - lo;
  const int nl = sub_nlev[s], nlf = nl & 0xffff, nlb = nl >> 16;
  const int tid = threadIdx.x, fi = lo + tid;   // the factor's row ...
  const bool active = tid < R;
  int i = fi;                                   // ... and the operator's
  bool own = active;                            // z[i] is this block's to write
  if constexpr (MAP) {
    const int er = active ? ext_row[fi] : 0;
    i = er & 0x7fffffff;
    own = er < 0;
  }
  double* ys = lds;
  double* red = lds + (size_t)blockDim.x * BS;
  double* park = red + 80;
  int lfirst = 0, dslot = 0, ulast = 0, lf = -1, lb = -1, uo = 0;
  bool parked = false;
  constexpr int NSR = NS > 0 ? NS : 1;
  int kc[NSR];            // NS > 0: the staged blocks' columns (brick-local) and values
  double mb[NSR][BB];
  if (active) {
    unpack_info_w(row_infow[fi], lfirst, dslot, ulast, lf, lb);
    double acc[BS];
    if constexpr (SPMV) {
#pragma unroll
      for (int r = 0; r < BS; r++) acc[r] = 0.0;
      ell_row_mult<BS, FILL ? WMAX : WMAX_WIDE>(n, rowptr ? rowptr[i + 1] - rowptr[i] : W, i, col, aval, in, acc);
    } else {
      load_x<BS>(in, i, acc);
    }
    if constexpr (NS > 0) {
      stage_blocks<BS, NS>(nf, fi, lo, lfirst, dslot - lfirst, dslot, fc, fval, kc, mb);
    } else {
      uo = row_uoffw[fi];
      parked = uo + (ulast - dslot - 1) <= ucap;
    }
    if (parked) {
      for (int q = dslot + 1; q < ulast; q++) {
        double blk[BB];
        load_block<BS>(fval, nf, q, fi, blk);
        double* p = park + (size_t)(uo + q - dslot - 1) * BB;
#pragma unroll
        for (int e = 0; e < BB; e++) p[e] = blk[e];
      }
    }
#pragma unroll
    for (int r = 0; r < BS; r++) ys[tid * BS + r] = acc[r];
  }
  __syncthreads();
  for (int lev = 1; lev < nlf; lev++) {  // level-0 rows have no lower couplings
    if (lf == lev) {
      double a[BS];
#pragma unroll
      for (int r = 0; r < BS; r++) a[r] = ys[tid * BS + r];
      if constexpr (NS > 0) {
        staged_row_sub<BS, NS>(dslot - lfirst, kc, mb, ys, a);
      } else {
        for (int q = lfirst; q < dslot; q++) {
          const int k = fc[(size_t)q * nf + fi] - lo;
          double m[BB], yk[BS];
          load_block<BS>(fval, nf, q, fi, m);
#pragma unroll
          for (int c = 0; c < BS; c++) yk[c] = ys[k * BS + c];
#pragma unroll
          for (int r = 0; r < BS; r++)
#pragma unroll
            for (int c = 0; c < BS; c++) a[r] -= m[r * BS + c] * yk[c];
        }
      }
#pragma unroll
      for (int r = 0; r < BS; r++) ys[tid * BS + r] = a[r];
    }
    __syncthreads();
  }
  // the inverted pivot: fetched once the forward sweep is over, so that it does not hold registers through the load
  // phase (4 x 4 blocks: 127 VGPRs and spills with it loaded there)
  double out[BS], dv[BB];
#pragma unroll
  for (int r = 0; r < BS; r++) out[r] = 0.0;
#pragma unroll
  for (int e = 0; e < BB; e++) dv[e] = 0.0;
  if (active) load_block<BS>(fval, nf, dslot, fi, dv);
  if constexpr (NS > 0) {   // the upper blocks take the lower blocks' registers
    if (active) stage_blocks<BS, NS>(nf, fi, lo, dslot + 1, ulast - dslot - 1, dslot, fc, fval, kc, mb);
  }
  for (int lev = 0; lev < nlb; lev++) {
    if (lb == lev) {
      double a[BS];
#pragma unroll
      for (int r = 0; r < BS; r++) a[r] = ys[tid * BS + r];
      if constexpr (NS > 0) staged_row_sub<BS, NS>(ulast - dslot - 1, kc, mb, ys, a);
      for (int q = dslot + 1; NS == 0 && q < ulast; q++) {
        const int k = fc[(size_t)q * nf + fi] - lo;
        double m[BB], xk[BS];
        if (parked) {
          const double* p = park + (size_t)(uo + q - dslot - 1) * BB;
#pragma unroll
          for (int e = 0; e < BB; e++) m[e] = p[e];
        } else {
          load_block<BS>(fval, nf, q, fi, m);
        }
#pragma unroll
        for (int c = 0; c < BS; c++) xk[c] = ys[k * BS + c];
#pragma unroll
        for (int r = 0; r < BS; r++)
#pragma unroll
          for (int c = 0; c < BS; c++) a[r] -= m[r * BS + c] * xk[c];
      }
#pragma unroll
      for (int r = 0; r < BS; r++) {
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < BS; c++) t += dv[r * BS + c] * a[c];
        out[r] = t;
      }
#pragma unroll
      for (int r = 0; r < BS; r++) ys[tid * BS + r] = out[r];
    }
    if (lev + 1 < nlb) __syncthreads();
  }
  if (own) {
#pragma unroll
    for (int r = 0; r < BS; r++) z[(size_t)i * BS + r] = out[r];
  }
  if (dot != 0) {
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if constexpr (MAP) {   // an overlap row's result is some other block's term (modes 2 and 3 sum unmasked rows)
#pragma unroll
      for (int r = 0; r < BS; r++) out[r] = own ? out[r] : 0.0;
    }
    pc_row_dots<BS, false, false>(dot, v, out, own, [&](double (&x)[BS]) {   // the operand again (an L2 hit), not held
#pragma unroll
      for (int r = 0; r < BS; r++) x[r] = 0.0;
      if (own) load_x<BS>(in, i, x);
    }, [&](double (&a)[BS]) { load_x_stream<BS>(aux, i, a); });
    __syncthreads();
    pc_reduce_dots(dot, v, red, partials, nb_max, s);
  }
}

}  // namespace wai

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
template <int BS, bool SPMV>
__global__ __launch_bounds__(1024) void k_pc_wide(int n, int W, int nsub, const int* __restrict__ sub_ptr,
                                                  const int* __restrict__ sub_nlev,
                                                  const unsigned long long* __restrict__ row_infow,
                                                  const int* __restrict__ row_uoffw, const int* __restrict__ col,
                                                  const int* __restrict__ rowptr, const double* __restrict__ aval,
                                                  const double* __restrict__ fval, const double* __restrict__ in,
                                                  double* __restrict__ z, const double* __restrict__ aux, double* partials,
                                                  int nb_max, int dot, int ucap, const int* __restrict__ sub_list, Fin fin) {
  constexpr int BB = BS * BS;
  extern __shared__ __attribute__((aligned(16))) double lds[];  // [T * BS] solution, 80 doubles reduction scratch, [ucap][BB] parked upper blocks
  if (fin_block(fin, partials, nb_max)) return;
  int s = xcd_remap(blockIdx.x, nsub);
  if (s >= nsub) return;
  if (sub_list) s = sub_list[s];
  const int lo = sub_ptr[s], R = sub_ptr[s + 1] - lo;
  const int nl = sub_nlev[s], nlf = nl & 0xffff, nlb = nl >> 16;
  const int tid = threadIdx.x, i = lo + tid;
  const bool active = tid < R;
  double* ys = lds;
  double* red = lds + (size_t)blockDim.x * BS;
  double* park = red + 80;
  int lfirst = 0, dslot = 0, ulast = 0, lf = -1, lb = -1, uo = 0;
  bool parked = false;
  if (active) {
    unpack_info_w(row_infow[i], lfirst, dslot, ulast, lf, lb);
    double acc[BS];
    if constexpr (SPMV) {
#pragma unroll
      for (int r = 0; r < BS; r++) acc[r] = 0.0;
      ell_row_mult<BS, WMAX_WIDE>(n, rowptr ? rowptr[i + 1] - rowptr[i] : W, i, col, aval, in, acc);
    } else {
      load_x<BS>(in, i, acc);
    }
    uo = row_uoffw[i];
    parked = uo + (ulast - dslot - 1) <= ucap;
    if (parked) {
      for (int q = dslot + 1; q < ulast; q++) {
        double blk[BB];
        load_block<BS>(fval, n, q, i, blk);
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
      for (int q = lfirst; q < dslot; q++) {
        const int k = col[(size_t)q * n + i] - lo;
        double m[BB], yk[BS];
        load_block<BS>(fval, n, q, i, m);
#pragma unroll
        for (int c = 0; c < BS; c++) yk[c] = ys[k * BS + c];
#pragma unroll
        for (int r = 0; r < BS; r++)
#pragma unroll
          for (int c = 0; c < BS; c++) a[r] -= m[r * BS + c] * yk[c];
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
  if (active) load_block<BS>(fval, n, dslot, i, dv);
  for (int lev = 0; lev < nlb; lev++) {
    if (lb == lev) {
      double a[BS];
#pragma unroll
      for (int r = 0; r < BS; r++) a[r] = ys[tid * BS + r];
      for (int q = dslot + 1; q < ulast; q++) {
        const int k = col[(size_t)q * n + i] - lo;
        double m[BB], xk[BS];
        if (parked) {
          const double* p = park + (size_t)(uo + q - dslot - 1) * BB;
#pragma unroll
          for (int e = 0; e < BB; e++) m[e] = p[e];
        } else {
          load_block<BS>(fval, n, q, i, m);
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
  if (active) {
#pragma unroll
    for (int r = 0; r < BS; r++) z[(size_t)i * BS + r] = out[r];
  }
  if (dot != 0) {
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    pc_row_dots<BS, false, false>(dot, v, out, active, [&](double (&x)[BS]) {   // the operand again (an L2 hit), not held
#pragma unroll
      for (int r = 0; r < BS; r++) x[r] = 0.0;
      if (active) load_x<BS>(in, i, x);
    }, [&](double (&a)[BS]) { load_x_stream<BS>(aux, i, a); });
    __syncthreads();
    pc_reduce_dots(dot, v, red, partials, nb_max, s);
  }
}

}  // namespace wai

// The fused preconditioned-operator kernel of the multicolour ordering (wai_set_pc_ordering): k_pc_colour.
#pragma once
#include "reductions.hip.h"

namespace wai {

// ---- z = U^-1 L^-1 (A x)  or  z = U^-1 L^-1 r  with the subdomain's rows eliminated by (colour, row) --------------------------
// One workgroup per subdomain, one thread per block row; k_pc's interface: the dot modes, the Fin finaliser workgroups,
// xcd_remap, the launch list.  Served where ILU(0) in this order updates no off-diagonal block (ColourFacts::diag_only: no
// triangle in the cell graph inside a subdomain -- hexahedral and MINC meshes), so L_ik = A_ik inv(P_k) and U_ij = A_ij
// exactly: the DILU form of k_pc.  The matrix row a thread pulls in for the product stays in registers and serves both
// substitutions; of the factor only the row's inverted pivot is read.  LDS holds w_k = inv(P_k) y_k, then x_k:
//   load      t_i = (A x)_i (or in_i); colour-0 rows (no lower coupling) put w_i = inv(P_i) t_i, the others t_i
//   forward   colours 1 .. C - 1:   y_i = t_i - sum over the row's lower couplings A_ik w_k,   w_i = inv(P_i) y_i
//   backward  colours C - 1 .. 0:   x_i = w_i - inv(P_i) sum over its upper couplings A_ij x_j
// with ONE barrier per colour -- 2 C - 1 barriers (3 on a hexahedral mesh) where the natural order of a 16 x 16 x 2 brick has
// 64.  A row's lower and upper couplings are bit masks over its slots, made from the descriptor (ColourSchedule::slots,
// counts): the slot loops are unrolled and predicated, no register array is indexed at run time; the couplings are
// subtracted in slot order.
// TMAX: the workgroup's thread limit, which sets the registers a thread may have.  A row of 7 blocks is 28 doubles at BS 2, 63
// at BS 3, 112 at BS 4: 1024 threads (128 VGPRs) hold the first, 512 (256 VGPRs) the second, 256 (512 VGPRs) the third --
// pc_colour_threads() is the rule, and the set-up keeps larger subdomains on the launch-per-colour path.
constexpr int pc_colour_threads(int bs) { return bs <= 2 ? 1024 : (bs == 3 ? 512 : 256); }

template <int BS, bool SPMV>
__global__ __launch_bounds__(pc_colour_threads(BS)) void k_pc_colour(int n, int W, int nsub, const int* __restrict__ sub_ptr,
                     const int* __restrict__ sub_ncol, const unsigned long long* __restrict__ slots,
                     const int* __restrict__ counts, const int* __restrict__ col, const double* __restrict__ aval,
                     const double* __restrict__ dinv, const double* __restrict__ in, double* __restrict__ z,
                     const double* __restrict__ aux, double* partials, int nb_max, int dot, const int* __restrict__ sub_list,
                     Fin fin) {
  constexpr int BB = BS * BS;
  extern __shared__ __attribute__((aligned(16))) double lds[];  // [T * BS] solution vector, then 80 doubles reduction scratch
  if (fin_block(fin, partials, nb_max)) return;
  int s = xcd_remap(blockIdx.x, nsub);
  if (s >= nsub) return;
  if (sub_list) s = sub_list[s];
  const int lo = sub_ptr[s], R = sub_ptr[s + 1] - lo;
  const int ncol = sub_ncol[s];
  const int tid = threadIdx.x, i = lo + tid;
  const bool active = tid < R;
  double* ys = lds;
  double f[WMAX][BB];
  int fc[WMAX];
  double dv[BB], xin[BS], out[BS];
  unsigned lmask = 0, umask = 0;
  int mine = -1;
#pragma unroll
  for (int r = 0; r < BS; r++) { xin[r] = 0.0; out[r] = 0.0; }
#pragma unroll
  for (int e = 0; e < BB; e++) dv[e] = 0.0;
#pragma unroll
  for (int q = 0; q < WMAX; q++) {
    fc[q] = 0;
#pragma unroll
    for (int e = 0; e < BB; e++) f[q][e] = 0.0;
  }
  // w = inv(P_i) a
  auto pivot_mult = [&](double (&a)[BS]) {
    double w[BS];
#pragma unroll
    for (int r = 0; r < BS; r++) {
      w[r] = 0.0;
#pragma unroll
      for (int k = 0; k < BS; k++) w[r] += dv[r * BS + k] * a[k];
    }
#pragma unroll
    for (int r = 0; r < BS; r++) a[r] = w[r];
  };
  if (active) {
    const unsigned long long sl = slots[i];
    const int ct = counts[i], nl = colour_nlower(ct), nu = colour_nupper(ct);
    mine = colour_of(ct);
    for (int p = 0; p < nl; p++) lmask |= 1u << colour_slot(sl, p);
    for (int p = nl; p < nl + nu; p++) umask |= 1u << colour_slot(sl, p);
    double acc[BS];
#pragma unroll
    for (int r = 0; r < BS; r++) acc[r] = 0.0;
    // one pass over the matrix row: the product, and the row kept in registers for the substitutions
#pragma unroll
    for (int q = 0; q < WMAX; q++) {
      if (q < W) {
        const int cg = col[(size_t)q * n + i];
        load_block<BS>(aval, n, q, i, f[q]);
        fc[q] = cg - lo;
        if constexpr (SPMV) {
          double xv[BS];
          load_x<BS>(in, cg, xv);
#pragma unroll
          for (int r = 0; r < BS; r++)
#pragma unroll
            for (int k = 0; k < BS; k++) acc[r] += f[q][r * BS + k] * xv[k];
        }
      }
    }
    if constexpr (!SPMV) load_x<BS>(in, i, acc);
    if (dot == PC_DOT_XZ || dot == PC_DOT_MERGED) load_x<BS>(in, i, xin);
    load_pivot<BS>(dinv, n, i, dv);
    if (mine == 0) pivot_mult(acc);
#pragma unroll
    for (int r = 0; r < BS; r++) ys[tid * BS + r] = acc[r];
  }
  __syncthreads();
  // sum over the slots of `mask` of A_iq v_q, the coupled rows' entries out of LDS
  auto gather = [&](unsigned mask, double (&sum)[BS]) {
#pragma unroll
    for (int r = 0; r < BS; r++) sum[r] = 0.0;
#pragma unroll
    for (int q = 0; q < WMAX; q++) {
      if ((mask >> q) & 1u) {
        double vk[BS];
#pragma unroll
        for (int c = 0; c < BS; c++) vk[c] = ys[fc[q] * BS + c];
#pragma unroll
        for (int r = 0; r < BS; r++)
#pragma unroll
          for (int c = 0; c < BS; c++) sum[r] += f[q][r * BS + c] * vk[c];
      }
    }
  };
  for (int c = 1; c < ncol; c++) {   // forward: colour 0 is done
    if (mine == c) {
      double a[BS], sum[BS];
      gather(lmask, sum);
#pragma unroll
      for (int r = 0; r < BS; r++) a[r] = ys[tid * BS + r] - sum[r];
      pivot_mult(a);
#pragma unroll
      for (int r = 0; r < BS; r++) ys[tid * BS + r] = a[r];
    }
    __syncthreads();
  }
  for (int c = ncol - 1; c >= 0; c--) {   // backward: the last colour has no upper coupling, x = w
    if (mine == c) {
      double sum[BS];
      gather(umask, sum);
      pivot_mult(sum);
#pragma unroll
      for (int r = 0; r < BS; r++) {
        out[r] = ys[tid * BS + r] - sum[r];
        ys[tid * BS + r] = out[r];
      }
    }
    if (c > 0) __syncthreads();
  }
  if (active) {
    if constexpr (BS == 2) *reinterpret_cast<double2*>(z + (size_t)i * 2) = make_double2(out[0], out[1]);
    else {
#pragma unroll
      for (int r = 0; r < BS; r++) z[(size_t)i * BS + r] = out[r];
    }
  }
  if (dot != 0) {
    double* red = lds + (size_t)blockDim.x * BS;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    pc_row_dots<BS, false, false>(dot, v, out, active, [&](double (&x)[BS]) {
#pragma unroll
      for (int r = 0; r < BS; r++) x[r] = xin[r];
    }, [&](double (&a)[BS]) { load_x_stream<BS>(aux, i, a); });
    __syncthreads();
    pc_reduce_dots(dot, v, red, partials, nb_max, s);
  }
}

}  // namespace wai

// The fused kernel with one thread per scalar row, k_pc_rows.
#pragma once
#include "reductions.hip.h"

namespace wai {

// ---- K6+K8 fused, one thread per SCALAR row (any block size; pivot-scaled DILU) ---------------
// With the rows pre-scaled by the inverted pivots the diagonal blocks of the factor are identities,
// so the BS components of a block row no longer depend on each other inside a substitution level:
//   y_i[r] = t_i[r] - sum_p L_p[r][:] . y_p[:]          x_i[r] = y_i[r] - sum_p U_p[r][:] . x_p[:]
// Thread (i, r) therefore owns block-row r of every block of row i: NL + NU rows of BS doubles stay in
// registers through both sweeps (3 x 3 blocks, 3 + 3 couplings: 36 VGPRs instead of the 108 a whole
// block row costs, which is what pushed the one-thread-per-block-row kernel into scratch memory for
// bs = 3, 4: MEASURED 3.25 ms at 5 M rows, 12 % of HBM peak), nothing is parked in LDS, and a
// workgroup of up to 16 waves per brick keeps the loads of 2 bricks (32 waves) in flight per CU.
// Threads are component-major (tid = r * R + row), so a wave instruction reads 64 consecutive
// BS-vectors of one (slot, r) plane.  Vectors move through LDS in block order: the result is written
// (and the dot-product partners are read) with tid-linear, fully coalesced accesses.
// registers: 58 (bs 2), 69 (bs 3), 90 (bs 4) without spills -> 8 / 7 / 5 waves per SIMD; asking for 8
// everywhere spills 150-600 registers at bs = 3, 4.  Four couplings per sweep (NL = 4: MINC inside 3-D
// bricks) cost 12 more: 5 and 4 waves (at 7 and 5 they spilled 200 bytes per lane)
template <int BS, bool SPMV, int NL, int NU, bool AX>
__global__ __launch_bounds__(1024, (BS <= 2 ? 8 : (BS == 3 ? (NL <= 3 ? 7 : 5) : (NL <= 3 ? 5 : 4)))) void k_pc_rows(
    int n, int W, int nsub, const int* __restrict__ sub_ptr, const int* __restrict__ sub_nlev,
    const int* __restrict__ row_info, const int* __restrict__ col, const double* __restrict__ sval,
    const double* __restrict__ dinv, const double* __restrict__ in, const double* __restrict__ in2,
    const double* __restrict__ scal, double* __restrict__ z,
    const double* __restrict__ aux, double* partials, int nb_max, int dot, const int* __restrict__ sub_list,
    const int* __restrict__ rowptr, const int* __restrict__ sub_split, Fin fin) {
  extern __shared__ __attribute__((aligned(16))) double lds[];  // [R*BS] solution in block order, [BS] zeros, then reduction scratch
  if (fin_block(fin, partials, nb_max)) return;
  int s = xcd_remap(blockIdx.x, nsub);
  if (s >= nsub) return;
  if (sub_list) s = sub_list[s];
  const int lo = sub_ptr[s], R = sub_ptr[s + 1] - lo;
  const int nl = sub_nlev[s];
  const int nlf = nl & 0xffff, nlb = nl >> 16;
  const int tid = threadIdx.x;
  const double nalpha = AX ? -scal[S_ALPHA] : 0.0;   // input = in - alpha in2
  // component-major over the R1 leading (long) rows, then component-major over the short ones
  const int R1 = sub_split ? (sub_split[s] & 0xffff) : R;
  const bool shortrow = tid >= R1 * BS;
  const int tt = shortrow ? tid - R1 * BS : tid, RR = shortrow ? max(R - R1, 1) : R1;
  const int r = min(tt / RR, BS - 1), il = (shortrow ? R1 : 0) + tt - (tt / RR) * RR, i = lo + il;
  const bool active = tid < R * BS;
  double* ys = lds;
  double Lf[NL][BS], Uf[NU][BS];
  int Lc[NL], Uc[NU], lf = -1, lb = -1;
#pragma unroll
  for (int p = 0; p < NL; p++) {
    Lc[p] = R * BS;  // the zero entries behind the vector
#pragma unroll
    for (int k = 0; k < BS; k++) Lf[p][k] = 0.0;
  }
#pragma unroll
  for (int p = 0; p < NU; p++) {
    Uc[p] = R * BS;
#pragma unroll
    for (int k = 0; k < BS; k++) Uf[p][k] = 0.0;
  }
  if (tid < BS) ys[R * BS + tid] = 0.0;
  if (active) {
    int lfirst, dslot, ulast;
    unpack_info(row_info[i], lfirst, dslot, ulast, lf, lb);
    const int cnt = rowptr ? rowptr[i + 1] - rowptr[i] : W;   // padding slots of short rows are not read
    // the column indices of all slots first: one round trip instead of one per slot (MEASURED: fused
    // launch 0.2587 -> 0.2382 ms at C5's short rows, no change at C4).  Making the whole slot loop
    // straight-line code as well (fixed width, no `q < cnt`) puts ~10 loads per lane in flight but costs
    // registers: 0.917 ms against 0.712 at C4 (spills under the 72-VGPR cap)
    int cgs[WMAX];
#pragma unroll
    for (int q = 0; q < WMAX; q++) {
      cgs[q] = i;
      if (q < cnt) cgs[q] = load_col(col, (size_t)q * n + i);
    }
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < WMAX; q++) {
      if (q < cnt) {
        const int cg = cgs[q];
        double blk[BS];
#pragma unroll
        for (int k = 0; k < BS; k++) blk[k] = __builtin_nontemporal_load(sval + ell_ix(BS, (size_t)n, q, r, k, (size_t)i));
        if constexpr (SPMV) {
          double xv[BS];
          load_xs<BS, AX>(in, in2, nalpha, cg, xv);
#pragma unroll
          for (int k = 0; k < BS; k++) acc += blk[k] * xv[k];
        }
        const bool isl = (q >= lfirst) && (q < dslot), isu = (q > dslot) && (q < ulast);
#pragma unroll
        for (int p = 0; p < NL; p++) {
          const bool tl = isl && (q - lfirst == p);
          Lc[p] = tl ? (cg - lo) * BS : Lc[p];
#pragma unroll
          for (int k = 0; k < BS; k++) Lf[p][k] = tl ? blk[k] : Lf[p][k];
        }
#pragma unroll
        for (int p = 0; p < NU; p++) {
          const bool tu = isu && (q - dslot - 1 == p);
          Uc[p] = tu ? (cg - lo) * BS : Uc[p];
#pragma unroll
          for (int k = 0; k < BS; k++) Uf[p][k] = tu ? blk[k] : Uf[p][k];
        }
      }
    }
    if constexpr (!SPMV) {  // plain application to an unscaled vector: scale it by the inverted pivot
#pragma unroll
      for (int k = 0; k < BS; k++) acc += dinv[ell_ix1(BS, (size_t)n, r, k, (size_t)i)] * in[(size_t)i * BS + k];
    }
    ys[il * BS + r] = acc;
  }
  // the dot product's partner (block order, tid-linear): in flight through the sweeps
  double avp = 0.0;
  if (active && (dot == PC_DOT_ZA || dot == PC_DOT_MERGED)) avp = __builtin_nontemporal_load(aux + (size_t)lo * BS + tid);
  __syncthreads();
  for (int lev = 1; lev < nlf; lev++) {  // forward: y_i = t_i - sum A'_ik y_k
    if (lf == lev) {
      double a = ys[il * BS + r];
#pragma unroll
      for (int p = 0; p < NL; p++)
#pragma unroll
        for (int k = 0; k < BS; k++) a -= Lf[p][k] * ys[Lc[p] + k];
      ys[il * BS + r] = a;
    }
    __syncthreads();
  }
  for (int lev = 0; lev < nlb; lev++) {  // backward: x_i = y_i - sum A'_ij x_j
    if (lb == lev) {
      double a = ys[il * BS + r];
#pragma unroll
      for (int p = 0; p < NU; p++)
#pragma unroll
        for (int k = 0; k < BS; k++) a -= Uf[p][k] * ys[Uc[p] + k];
      ys[il * BS + r] = a;
    }
    __syncthreads();
  }
  // block-order, tid-linear epilogue: store the result, reduce the dot products
  double out = 0.0;
  const size_t g = (size_t)lo * BS + tid;
  if (active) {
    out = ys[tid];
    __builtin_nontemporal_store(out, z + g);
  }
  if (dot != 0) {
    double* red = lds + (size_t)R * BS + BS;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    pc_row_dots<1, true, true>(dot, v, {out}, active, [&](double (&x)[1]) { x[0] = AX ? __builtin_fma(nalpha, in2[g], in[g]) : in[g]; },
                               [&](double (&a)[1]) { a[0] = avp; });
    __syncthreads();
    pc_reduce_dots(dot, v, red, partials, nb_max, s);
  }
}

}  // namespace wai

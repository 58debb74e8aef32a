// Sub-preconditioner lu (wai_set_sub_pc, WAI_SUB_LU): the exact LU factorisation of every subdomain block of the extended
// system -- ILU with every level of fill kept (asm_pattern.hpp: iluk_fill without a level bound) -- and its two substitutions.
// Complete fill gives rows of tens to a few hundred blocks and a dependency chain as long as the block (one row per
// level), so neither the thread-per-row brick kernels nor a launch per level fit: both kernels here give a block to ONE
// workgroup that walks its rows in order and spreads the entries of a row over its lanes.  Rows are ordered by
// __syncthreads() inside that workgroup; nothing waits on another workgroup.
// Stored factor, as the launch-per-level path keeps it: L multipliers (already times the inverted pivot of their
// column), U, and the inverted pivot blocks in the diagonal slot and in dinv.  Row descriptors: the 8-bit form
// (unpack_info_wide), rows of up to 255 blocks.
#pragma once
#include "linalg_device.hip.h"

namespace wai {

constexpr int SUBLU_FACTOR_THREADS = 256;   // one lane per entry of a pivot row (<= 254 right of its diagonal)
constexpr int SUBLU_SOLVE_WAVES = 8;        // rows in flight per round of a substitution sweep
constexpr int SUBLU_MAXQ = 4;               // entries of a row per lane: 4 x 64 >= 255

// ---- numeric factorisation (IKJ, up-looking), one workgroup per block ---------------------------------------------------
// Row i lives in LDS while it is eliminated.  Its lower entries k are taken in ascending order -- L_ik is final only when
// every earlier elimination has been applied -- and each elimination is shared by the whole workgroup: lane t takes entry
// t of pivot row k to the right of its diagonal and subtracts L_ik U_kj from the entry of row i with the same column.
// Both column lists ascend and, with complete fill, row i holds every column of pivot row k beyond k, so entry t of the
// pivot row can only sit between positions q + 1 + t and ulast - (cnt - t) of row i: the lane bisects that window of the
// LDS copy of row i's columns (<= 8 probes), where the brick kernels scan the row.
// The pivot row's columns, blocks and inverted pivot for the NEXT elimination are requested before the current one is
// applied: they depend on nothing row i computes, and the two dependent global round trips per elimination (descriptor,
// then columns and blocks) would otherwise be the whole cost of a row.
// what an elimination with pivot row k needs: lane t's entry of it right of the diagonal (column j, block u; j = -1: none),
// its inverted pivot d, its length cnt
template <int BS>
__device__ __forceinline__ void sublu_fetch(int n, int k, int t, const int* __restrict__ row_info, const int* __restrict__ col,
                                            const double* fval, int& j, int& cnt, double (&u)[BS * BS], double (&d)[BS * BS]) {
  constexpr int BB = BS * BS;
  int kl, kd, ku;
  unpack_info_wide(row_info[k], kl, kd, ku);
  cnt = ku - kd - 1;
  j = -1;
#pragma unroll
  for (int e = 0; e < BB; e++) { d[e] = fval[vix<BS>(n, kd, e, k)]; u[e] = 0.0; }
  if (t < cnt) {
    j = col[(size_t)(kd + 1 + t) * n + k];
#pragma unroll
    for (int e = 0; e < BB; e++) u[e] = fval[vix<BS>(n, kd + 1 + t, e, k)];
  }
}

template <int BS>
__global__ __launch_bounds__(SUBLU_FACTOR_THREADS) void k_sublu_factor(int n, int nsub, int W, const int* __restrict__ sub_ptr,
                                                                       const int* __restrict__ row_info, const int* __restrict__ col,
                                                                       double* fval, double* dinv, int* flags) {
  constexpr int BB = BS * BS;
  extern __shared__ double sm[];   // row i: [W][BB] blocks, then its W columns
  double* wrow = sm;
  int* icol = reinterpret_cast<int*>(sm + (size_t)W * BB);
  const int s = blockIdx.x;
  if (s >= nsub) return;
  const int lo = sub_ptr[s], hi = sub_ptr[s + 1];
  const int t = threadIdx.x;
  for (int i = lo; i < hi; i++) {
    int lfirst, dslot, ulast;
    unpack_info_wide(row_info[i], lfirst, dslot, ulast);
    if (t >= lfirst && t < ulast) {
      icol[t] = col[(size_t)t * n + i];
#pragma unroll
      for (int e = 0; e < BB; e++) wrow[t * BB + e] = fval[vix<BS>(n, t, e, i)];
    }
    int cj = -1, ccnt = 0, nj = -1, ncnt = 0;
    double cu[BB], cd[BB], nu[BB], nd[BB];
#pragma unroll
    for (int e = 0; e < BB; e++) { cu[e] = 0.0; cd[e] = 0.0; nu[e] = 0.0; nd[e] = 0.0; }
    if (lfirst < dslot) sublu_fetch<BS>(n, col[(size_t)lfirst * n + i], t, row_info, col, fval, cj, ccnt, cu, cd);
    __syncthreads();
    for (int q = lfirst; q < dslot; q++) {
      nj = -1; ncnt = 0;
      if (q + 1 < dslot) sublu_fetch<BS>(n, icol[q + 1], t, row_info, col, fval, nj, ncnt, nu, nd);
      // L_ik = A_ik inv(P_k): every lane forms it (LDS broadcast), lane 0 stores it
      double l[BB];
#pragma unroll
      for (int r = 0; r < BS; r++)
#pragma unroll
        for (int c = 0; c < BS; c++) {
          double acc = 0.0;
#pragma unroll
          for (int e = 0; e < BS; e++) acc += wrow[q * BB + r * BS + e] * cd[e * BS + c];
          l[r * BS + c] = acc;
        }
      if (t == 0) {
#pragma unroll
        for (int e = 0; e < BB; e++) fval[vix<BS>(n, q, e, i)] = l[e];
      }
      if (cj >= 0) {
        int a = q + 1 + t, b = ulast - (ccnt - t);   // the window of row i that can hold column cj
        if (b >= ulast) b = ulast - 1;
        while (a < b) {
          const int m = (a + b) >> 1;
          if (icol[m] < cj) a = m + 1; else b = m;
        }
        if (a < ulast && icol[a] == cj) {
#pragma unroll
          for (int r = 0; r < BS; r++)
#pragma unroll
            for (int c = 0; c < BS; c++) {
              double acc = 0.0;
#pragma unroll
              for (int e = 0; e < BS; e++) acc += l[r * BS + e] * cu[e * BS + c];
              wrow[a * BB + r * BS + c] -= acc;
            }
        }
      }
      cj = nj; ccnt = ncnt;
#pragma unroll
      for (int e = 0; e < BB; e++) { cu[e] = nu[e]; cd[e] = nd[e]; }
      __syncthreads();   // the next elimination reads entries this one updated (and wrow[q] is not read again)
    }
    if (t == dslot) {
      double piv[BB], inv[BB];
#pragma unroll
      for (int e = 0; e < BB; e++) piv[e] = wrow[dslot * BB + e];
      if (!block_inverse<BS>(piv, inv)) atomicMax(&flags[0], 1);
#pragma unroll
      for (int e = 0; e < BB; e++) {
        fval[vix<BS>(n, dslot, e, i)] = inv[e];
        dinv[dix<BS>(n, e, i)] = inv[e];
      }
    } else if (t > dslot && t < ulast) {
#pragma unroll
      for (int e = 0; e < BB; e++) fval[vix<BS>(n, t, e, i)] = wrow[t * BB + e];
    }
    __threadfence_block();
    __syncthreads();   // row i is a pivot row from here on; its LDS copy may be overwritten
  }
}

// ---- the two substitutions, one workgroup per block, in place on z --------------------------------------------------------
// forward: y_i = z_i - sum_{k < i} L_ik y_k; backward: x_i = inv(P_i) (y_i - sum_{j > i} U_ij x_j).
// The sweeps are sequential over the rows, but a row's columns and blocks do not depend on the vector: the workgroup's
// waves take SUBLU_SOLVE_WAVES consecutive rows per round, each wave loads its row's entries into registers (<= 4 per lane),
// and then the rows are finished one after the other -- products with the known entries of the vector, a wave reduction,
// the pivot applied by lane 0 -- with a __syncthreads() between them.  One memory latency per round, not per row.
// LDSV: the block's part of the vector is held in LDS during both sweeps; otherwise it stays in global memory (z itself).
template <int BS, bool LDSV, bool FWD>
__device__ __forceinline__ void sublu_sweep(int n, int lo, int hi, const int* __restrict__ row_info, const int* __restrict__ col,
                                            const double* __restrict__ fval, const double* __restrict__ dinv, double* v) {
  constexpr int BB = BS * BS, NW = SUBLU_SOLVE_WAVES;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int R = hi - lo;
  for (int base = 0; base < R; base += NW) {
    const int li = FWD ? base + w : R - 1 - base - w;   // local row of this wave in this round
    const bool have = FWD ? li < R : li >= 0;
    const int i = lo + li;
    int cs[SUBLU_MAXQ];
    double m[SUBLU_MAXQ][BB], d[BB];
    int q0 = 0, q1 = 0;
    if (have) {
      int lfirst, dslot, ulast;
      unpack_info_wide(row_info[i], lfirst, dslot, ulast);
      q0 = FWD ? lfirst : dslot + 1;
      q1 = FWD ? dslot : ulast;
#pragma unroll
      for (int p = 0; p < SUBLU_MAXQ; p++) {
        const int q = q0 + lane + 64 * p;
        cs[p] = -1;
        if (q < q1) {
          cs[p] = col[(size_t)q * n + i] - lo;
#pragma unroll
          for (int e = 0; e < BB; e++) m[p][e] = fval[vix<BS>(n, q, e, i)];
        }
      }
      if constexpr (!FWD) {
        if (lane == 0) {
#pragma unroll
          for (int e = 0; e < BB; e++) d[e] = dinv[dix<BS>(n, e, i)];
        }
      }
    }
    for (int turn = 0; turn < NW; turn++) {
      if (turn == w && have) {
        double acc[BS];
#pragma unroll
        for (int r = 0; r < BS; r++) acc[r] = 0.0;
#pragma unroll
        for (int p = 0; p < SUBLU_MAXQ; p++)
          if (cs[p] >= 0) {
#pragma unroll
            for (int r = 0; r < BS; r++)
#pragma unroll
              for (int c = 0; c < BS; c++) acc[r] += m[p][r * BS + c] * v[(size_t)cs[p] * BS + c];
          }
#pragma unroll
        for (int r = 0; r < BS; r++) acc[r] = wave_sum(acc[r]);
        if (lane == 0) {
#pragma unroll
          for (int r = 0; r < BS; r++) acc[r] = v[(size_t)li * BS + r] - acc[r];
          if constexpr (FWD) {
#pragma unroll
            for (int r = 0; r < BS; r++) v[(size_t)li * BS + r] = acc[r];
          } else {
#pragma unroll
            for (int r = 0; r < BS; r++) {
              double o = 0.0;
#pragma unroll
              for (int c = 0; c < BS; c++) o += d[r * BS + c] * acc[c];
              v[(size_t)li * BS + r] = o;
            }
          }
        }
        if constexpr (!LDSV) __threadfence_block();
      }
      __syncthreads();
    }
  }
}

template <int BS, bool LDSV>
__global__ __launch_bounds__(64 * SUBLU_SOLVE_WAVES) void k_sublu_solve(int n, int nsub, const int* __restrict__ sub_ptr,
                                                                        const int* __restrict__ row_info, const int* __restrict__ col,
                                                                        const double* __restrict__ fval, const double* __restrict__ dinv,
                                                                        double* z) {
  extern __shared__ double sv[];   // LDSV: the block's entries of the vector
  const int s = blockIdx.x;
  if (s >= nsub) return;
  const int lo = sub_ptr[s], hi = sub_ptr[s + 1];
  const int len = (hi - lo) * BS;
  double* zb = z + (size_t)lo * BS;
  double* v = LDSV ? sv : zb;
  if constexpr (LDSV) {
    for (int e = threadIdx.x; e < len; e += blockDim.x) sv[e] = zb[e];
    __syncthreads();
  }
  sublu_sweep<BS, LDSV, true>(n, lo, hi, row_info, col, fval, dinv, v);
  sublu_sweep<BS, LDSV, false>(n, lo, hi, row_info, col, fval, dinv, v);
  if constexpr (LDSV) {
    for (int e = threadIdx.x; e < len; e += blockDim.x) zb[e] = sv[e];
  }
}

}  // namespace wai

// The generic fused preconditioned-operator kernel k_pc: any block size, stored factor or DILU.
#pragma once
#include "reductions.hip.h"

namespace wai {

// ---- K6+K8 fused: z = U^-1 L^-1 (A x)  or  z = U^-1 L^-1 r ------------------------------------

constexpr int PC_MIN_WAVES = 4;   // waves per SIMD k_pc is compiled for; 5 or 6 force spills and measured 1.2x / 3x slower

// DILU = true: the symbolic phase found that ILU(0) never updates an off-diagonal block inside
// any subdomain (true for hexahedral / MINC connectivity: no triangles in the cell graph), so
// L_ik = A_ik inv(D_k) and U_ij = A_ij exactly and the factor is just the modified pivots.  The
// matrix row a thread pulled in for the SpMV is then reused for both substitutions and only the
// inverted pivot block is read from the factor: ~300 instead of ~520 bytes per block row.
template <int BS, bool SPMV, int DILU, bool FAST>
__global__ __launch_bounds__(1024, (BS <= 2 ? PC_MIN_WAVES : 4)) void k_pc(int n, int W, int nsub, const int* __restrict__ sub_ptr,
                     const int* __restrict__ sub_nlev, const int* __restrict__ row_info,
                     const int* __restrict__ col, const double* __restrict__ aval,
                     const double* __restrict__ fval, const double* __restrict__ dinv,
                     const double* __restrict__ in,
                     double* __restrict__ z, const double* __restrict__ aux, double* partials,
                     int nb_max, int dot, int dbg,
    const int* __restrict__ sub_list, Fin fin) {
  constexpr int BB = BS * BS;
  // DILU == 2: rows pre-scaled by the inverted pivots (k_scale_rows): A' = inv(P) A lives in fval,
  // the pivots of ILU(0)(A') are identities, so neither dinv nor its two products per row are needed
  constexpr bool SC = (DILU == 2);
  const double* __restrict__ mat = SC ? fval : aval;
  extern __shared__ __attribute__((aligned(16))) double lds[];  // [T * BS] solution vector, then 80 doubles reduction scratch
  if (fin_block(fin, partials, nb_max)) return;
  int s = xcd_remap(blockIdx.x, nsub);
  if (s >= nsub) return;
  if (sub_list) s = sub_list[s];
  const int lo = sub_ptr[s], R = sub_ptr[s + 1] - lo;
  const int nl = sub_nlev[s];
  const int nlf = (dbg & 1) ? 0 : (nl & 0xffff), nlb = (dbg & 1) ? 1 : (nl >> 16);  // dbg: timing probe
  const int tid = threadIdx.x, i = lo + tid;
  const bool active = tid < R;
  double* ys = lds;
  double f[WMAX][BB];
  int fc[WMAX];
  int lfirst = 0, dslot = 0, ulast = 0, lf = -1, lb = -1;
  double xin[BS];
#pragma unroll
  for (int r = 0; r < BS; r++) xin[r] = 0.0;
#pragma unroll
  for (int q = 0; q < WMAX; q++) {
    fc[q] = 0;
#pragma unroll
    for (int e = 0; e < BB; e++) f[q][e] = 0.0;
  }
  double dv[BB];
#pragma unroll
  for (int e = 0; e < BB; e++) dv[e] = 0.0;
  // FAST: every row has at most 3 lower and 3 upper couplings inside its subdomain and the
  // first in-subdomain slot / the diagonal slot are < 4 (7-point stencils).  The lower / upper
  // blocks are compacted into fixed positions with register selects, so a level update is 3
  // unconditional LDS reads + straight-line FMAs instead of one divergent branch and LDS wait
  // per matrix slot.  In the DILU case the compaction happens slot by slot as the blocks are
  // consumed by the SpMV, which keeps the live register set (and so the occupancy) small.
  constexpr int MLU = 3;
  double Lf[MLU][BB], Uf[MLU][BB];
  int Lc[MLU], Uc[MLU];
#pragma unroll
  for (int p = 0; p < MLU; p++) {
    Lc[p] = tid; Uc[p] = tid;
#pragma unroll
    for (int e = 0; e < BB; e++) { Lf[p][e] = 0.0; Uf[p][e] = 0.0; }
  }
  if (active) {
    unpack_info(row_info[i], lfirst, dslot, ulast, lf, lb);
    double acc[BS];
    if constexpr (DILU) {
      // one pass over the matrix row: keep it in registers for the substitutions
#pragma unroll
      for (int q = 0; q < WMAX; q++) {
        if (q < W) {
          const int cg = col[(size_t)q * n + i];
          double blk[BB];
          load_block<BS>(mat, n, q, i, blk);
          if constexpr (SPMV) {
            double xv[BS];
            load_x<BS>(in, cg, xv);
            if (q == 0) {
#pragma unroll
              for (int r = 0; r < BS; r++) acc[r] = 0.0;
            }
#pragma unroll
            for (int r = 0; r < BS; r++)
#pragma unroll
              for (int k = 0; k < BS; k++) acc[r] += blk[r * BS + k] * xv[k];
          }
          if constexpr (FAST) {
            const bool isl = (q >= lfirst) && (q < dslot), isu = (q > dslot) && (q < ulast);
#pragma unroll
            for (int p = 0; p < MLU; p++) {
              const bool tl = isl && (q - lfirst == p), tu = isu && (q - dslot - 1 == p);
              Lc[p] = tl ? cg - lo : Lc[p];
              Uc[p] = tu ? cg - lo : Uc[p];
#pragma unroll
              for (int e = 0; e < BB; e++) {
                Lf[p][e] = tl ? blk[e] : Lf[p][e];
                Uf[p][e] = tu ? blk[e] : Uf[p][e];
              }
            }
          } else {
            fc[q] = cg - lo;
#pragma unroll
            for (int e = 0; e < BB; e++) f[q][e] = blk[e];
          }
        }
      }
      if constexpr (!SPMV) load_x<BS>(in, i, acc);
      if (dot == PC_DOT_XZ || dot == PC_DOT_MERGED) load_x<BS>(in, i, xin);
      if constexpr (!SC) load_pivot<BS>(dinv, n, i, dv);
      if constexpr (SC && !SPMV) {  // plain application to an unscaled vector: scale it first
        load_pivot<BS>(dinv, n, i, dv);
        double w0[BS];
#pragma unroll
        for (int r = 0; r < BS; r++) {
          w0[r] = 0.0;
#pragma unroll
          for (int k = 0; k < BS; k++) w0[r] += dv[r * BS + k] * acc[k];
        }
#pragma unroll
        for (int r = 0; r < BS; r++) acc[r] = w0[r];
      }
    } else {
      if constexpr (SPMV) {
#pragma unroll
        for (int r = 0; r < BS; r++) acc[r] = 0.0;
        ell_row_mult<BS>(n, W, i, col, aval, in, acc);
        if (dot == PC_DOT_XZ || dot == PC_DOT_MERGED) load_x<BS>(in, i, xin);
      } else {
        load_x<BS>(in, i, acc);
      }
      // factor row -> registers (independent loads, all in flight before the first barrier)
#pragma unroll
      for (int q = 0; q < WMAX; q++) {
        if (q < W) {
          fc[q] = col[(size_t)q * n + i] - lo;
          load_block<BS>(fval, n, q, i, f[q]);
        }
      }
#pragma unroll
      for (int q = 0; q < WMAX; q++)
        if (q == dslot) {
#pragma unroll
          for (int e = 0; e < BB; e++) dv[e] = f[q][e];
        }
    }
    if constexpr (DILU == 1) {
      if (lf == 0) {  // level-0 rows: w = inv(D) t straight away
        double w0[BS];
#pragma unroll
        for (int r = 0; r < BS; r++) {
          w0[r] = 0.0;
#pragma unroll
          for (int k = 0; k < BS; k++) w0[r] += dv[r * BS + k] * acc[k];
        }
#pragma unroll
        for (int r = 0; r < BS; r++) acc[r] = w0[r];
      }
    }
#pragma unroll
    for (int r = 0; r < BS; r++) ys[tid * BS + r] = acc[r];
  }
  if constexpr (FAST && !DILU) {  // stored-factor path: compact from the loaded factor row
    const int nL = dslot - lfirst, nU = ulast - dslot - 1;
#pragma unroll
    for (int p = 0; p < MLU; p++) {
#pragma unroll
      for (int o = 0; o < 4; o++) {  // candidate source slots p + o (lower), p + 1 + o (upper)
        const bool tl = active && (lfirst == o) && (p < nL);
        const bool tu = active && (dslot == o) && (p < nU);
        if (p + o < WMAX) {
          Lc[p] = tl ? fc[p + o] : Lc[p];
#pragma unroll
          for (int e = 0; e < BB; e++) Lf[p][e] = tl ? f[p + o][e] : Lf[p][e];
        }
        if (p + 1 + o < WMAX) {
          Uc[p] = tu ? fc[p + 1 + o] : Uc[p];
#pragma unroll
          for (int e = 0; e < BB; e++) Uf[p][e] = tu ? f[p + 1 + o][e] : Uf[p][e];
        }
      }
    }
  }
  __syncthreads();
  // One forward-level / backward-level update of this thread's row, out of LDS.
  // General: L y = t (unit block diagonal), then x_i = inv(D_i) (y_i - sum U_ij x_j).
  // DILU:    y_i = t_i - sum A_ik w_k with w_k = inv(D_k) y_k (LDS holds w), then
  //          x_i = w_i - inv(D_i) sum A_ij x_j.
  double out[BS];
#pragma unroll
  for (int r = 0; r < BS; r++) out[r] = 0.0;
  auto gather3 = [&](const int (&cc)[MLU], const double (&ff)[MLU][BB], double* sum) {
    double yk[MLU][BS];
#pragma unroll
    for (int p = 0; p < MLU; p++) {
      if constexpr (BS == 2) {
        const double2 t = *reinterpret_cast<const double2*>(ys + cc[p] * 2);
        yk[p][0] = t.x; yk[p][1] = t.y;
      } else {
#pragma unroll
        for (int c = 0; c < BS; c++) yk[p][c] = ys[cc[p] * BS + c];
      }
    }
#pragma unroll
    for (int r = 0; r < BS; r++) {
      double part[MLU];
#pragma unroll
      for (int p = 0; p < MLU; p++) {
        part[p] = 0.0;
#pragma unroll
        for (int c = 0; c < BS; c++) part[p] += ff[p][r * BS + c] * yk[p][c];
      }
      sum[r] = (part[0] + part[1]) + part[2];
    }
  };
  auto fwd_row = [&]() {
    double a[BS];
#pragma unroll
    for (int r = 0; r < BS; r++) a[r] = ys[tid * BS + r];
    if constexpr (FAST) {
      double sum[BS];
      gather3(Lc, Lf, sum);
#pragma unroll
      for (int r = 0; r < BS; r++) a[r] -= sum[r];
    } else {
#pragma unroll
      for (int q = 0; q < WMAX; q++) {
        if (q >= lfirst && q < dslot) {
          double yk[BS];
#pragma unroll
          for (int c = 0; c < BS; c++) yk[c] = ys[fc[q] * BS + c];
#pragma unroll
          for (int r = 0; r < BS; r++)
#pragma unroll
            for (int c = 0; c < BS; c++) a[r] -= f[q][r * BS + c] * yk[c];
        }
      }
    }
    if constexpr (DILU == 1) {
      double w1[BS];
#pragma unroll
      for (int r = 0; r < BS; r++) {
        w1[r] = 0.0;
#pragma unroll
        for (int k = 0; k < BS; k++) w1[r] += dv[r * BS + k] * a[k];
      }
#pragma unroll
      for (int r = 0; r < BS; r++) a[r] = w1[r];
    }
#pragma unroll
    for (int r = 0; r < BS; r++) ys[tid * BS + r] = a[r];
  };
  auto bwd_row = [&]() {
    double a[BS], sum[BS];
#pragma unroll
    for (int r = 0; r < BS; r++) { a[r] = ys[tid * BS + r]; sum[r] = 0.0; }
    if constexpr (FAST) {
      gather3(Uc, Uf, sum);
    } else {
#pragma unroll
      for (int q = 0; q < WMAX; q++) {
        if (q > dslot && q < ulast) {
          double xk[BS];
#pragma unroll
          for (int c = 0; c < BS; c++) xk[c] = ys[fc[q] * BS + c];
#pragma unroll
          for (int r = 0; r < BS; r++)
#pragma unroll
            for (int c = 0; c < BS; c++) sum[r] += f[q][r * BS + c] * xk[c];
        }
      }
    }
#pragma unroll
    for (int r = 0; r < BS; r++) {
      double t = 0.0;
      if constexpr (SC) {
        out[r] = a[r] - sum[r];
      } else if constexpr (DILU == 1) {
#pragma unroll
        for (int c = 0; c < BS; c++) t += dv[r * BS + c] * sum[c];
        out[r] = a[r] - t;
      } else {
#pragma unroll
        for (int c = 0; c < BS; c++) t += dv[r * BS + c] * (a[c] - sum[c]);
        out[r] = t;
      }
    }
#pragma unroll
    for (int r = 0; r < BS; r++) ys[tid * BS + r] = out[r];
  };
  {
    for (int lev = 1; lev < nlf; lev++) {  // level-0 rows have no lower couplings
      if (lf == lev) fwd_row();
      __syncthreads();
    }
    for (int lev = 0; lev < nlb; lev++) {
      if (lb == lev) bwd_row();
      if (lev + 1 < nlb) __syncthreads();
    }
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

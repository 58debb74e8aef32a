// The coupled tracer system (wai_set_tracer_solve_mode, WAI_TRACER_COUPLED): the nt scalar tracer systems as ONE system on
// the interleaved [cell][tracer] vector, as the reference keeps one auxiliary matrix with nt degrees of freedom per cell
// (src/ode.F90:306-315) and solves it once per step (src/timestepper.F90:2345-2355).  Its nt x nt blocks are diagonal, so
// they are stored as their diagonals -- nt value planes per slot on the ONE set of column planes of the flow Jacobian
// (Bcsr::dg: val[(slot * nt + t) * n + row]) -- and block ILU(0) is nt independent scalar ILU(0)s on one pattern: the
// same dependency levels, the same barriers, the same launches for every tracer.
//
// Kernels here: the diagonal-block SpMV, the factorisation and the fused preconditioned operator z = U^-1 L^-1 (A x) of the
// brick schedules (one workgroup per brick, one thread per row, the level structure of k_ilu_factor / k_pc), and the
// launch-per-level forms for subdomains of more than 1024 rows.  A thread works on NC tracers at a time (NC = nt for
// nt <= 4; above, chunks of four: the row's descriptor and column indices stay in registers across the chunks, the
// values of 8 slots x 4 tracers are the 32 doubles k_pc<2> holds for its 8 blocks).  No launch count depends on nt.
// The Krylov drivers' inner products of a preconditioner result are reduced by the vector kernels (launch_pc_on).
#include "linalg_device.hip.h"

namespace wai {

// a row's descriptor in the schedule's encoding: ENC 0 brick (row_info, 4-bit slots), 1 brick of 9 .. 16-block rows
// (row_infow), 2 launch-per-level (row_info, 8-bit slots, no levels)
template <int ENC>
__device__ __forceinline__ void dg_info(const int* __restrict__ row_info, const unsigned long long* __restrict__ row_infow,
                                        int i, int& lfirst, int& dslot, int& ulast, int& lf, int& lb) {
  if constexpr (ENC == 0) unpack_info(row_info[i], lfirst, dslot, ulast, lf, lb);
  else if constexpr (ENC == 1) unpack_info_w(row_infow[i], lfirst, dslot, ulast, lf, lb);
  else { unpack_info_wide(row_info[i], lfirst, dslot, ulast); lf = 0; lb = 0; }
}
__device__ __forceinline__ size_t dg_ix(int n, int nt, int s, int t, int i) { return ((size_t)s * nt + t) * n + i; }

// ---- y[c][t] = sum_slot a[slot][t][c] x[col][t]: the column index read once per slot ------------------------------------
template <int NC>
__global__ __launch_bounds__(TPB) void k_dg_spmv(int n, int W, int nt, int nblk, const int* __restrict__ col,
                                                 const double* __restrict__ val, const double* __restrict__ x,
                                                 double* __restrict__ y) {
  const int b = xcd_remap(blockIdx.x, nblk);
  const int i = b * TPB + threadIdx.x;
  if (b >= nblk || i >= n) return;
  for (int t0 = 0; t0 < nt; t0 += NC) {
    double acc[NC];
#pragma unroll
    for (int k = 0; k < NC; k++) acc[k] = 0.0;
    for (int s = 0; s < W; s++) {
      const int cg = col[(size_t)s * n + i];
#pragma unroll
      for (int k = 0; k < NC; k++)
        if (t0 + k < nt) acc[k] += val[dg_ix(n, nt, s, t0 + k, i)] * x[(size_t)cg * nt + t0 + k];
    }
#pragma unroll
    for (int k = 0; k < NC; k++)
      if (t0 + k < nt) y[(size_t)i * nt + t0 + k] = acc[k];
  }
}

// ---- ILU(0) of the nt systems in one pass (IKJ, in place on a copy of the values) ---------------------------------------
// One row's elimination for every tracer: the pattern work (columns, descriptors, the search for the matching slot) is
// done once, the arithmetic nt times.  On exit the diagonal slot holds the inverted pivots.
template <int ENC>
__device__ __forceinline__ void dg_factor_row(int n, int nt, int i, int lfirst, int dslot, int ulast,
                                              const int* __restrict__ row_info, const unsigned long long* __restrict__ row_infow,
                                              const int* __restrict__ col, double* fval, int* flags) {
  for (int q = lfirst; q < dslot; q++) {
    const int k = col[(size_t)q * n + i];
    int kl, kd, ku, kf, kb;
    dg_info<ENC>(row_info, row_infow, k, kl, kd, ku, kf, kb);
    double w[MAX_TRACERS];
#pragma unroll
    for (int t = 0; t < MAX_TRACERS; t++) {
      w[t] = 0.0;
      if (t < nt) {
        w[t] = fval[dg_ix(n, nt, q, t, i)] * fval[dg_ix(n, nt, kd, t, k)];
        fval[dg_ix(n, nt, q, t, i)] = w[t];
      }
    }
    for (int r2 = kd + 1; r2 < ku; r2++) {
      const int j = col[(size_t)r2 * n + k];
      for (int q2 = q + 1; q2 < ulast; q2++) {
        if (col[(size_t)q2 * n + i] != j) continue;
#pragma unroll
        for (int t = 0; t < MAX_TRACERS; t++)
          if (t < nt) fval[dg_ix(n, nt, q2, t, i)] -= w[t] * fval[dg_ix(n, nt, r2, t, k)];
        break;
      }
    }
  }
  for (int t = 0; t < nt; t++) {
    const double p = fval[dg_ix(n, nt, dslot, t, i)];
    if (p == 0.0) atomicMax(&flags[0], 1);
    fval[dg_ix(n, nt, dslot, t, i)] = 1.0 / p;
  }
}

template <int ENC>
__global__ void k_dg_factor(int n, int nt, int nsub, const int* __restrict__ sub_ptr, const int* __restrict__ sub_nlev,
                            const int* __restrict__ row_info, const unsigned long long* __restrict__ row_infow,
                            const int* __restrict__ col, double* fval, int* flags) {
  const int s = xcd_remap(blockIdx.x, nsub);
  if (s >= nsub) return;
  const int lo = sub_ptr[s], R = sub_ptr[s + 1] - lo;
  const int nlf = sub_nlev[s] & 0xffff;
  const int i = lo + threadIdx.x;
  const bool active = (int)threadIdx.x < R;
  int lfirst = 0, dslot = 0, ulast = 0, lf = -1, lb = 0;
  if (active) dg_info<ENC>(row_info, row_infow, i, lfirst, dslot, ulast, lf, lb);
  for (int lev = 0; lev < nlf; lev++) {
    if (active && lf == lev) dg_factor_row<ENC>(n, nt, i, lfirst, dslot, ulast, row_info, row_infow, col, fval, flags);
    __threadfence_block();
    __syncthreads();
  }
}

// The same factor where ILU(0) never updates an off-diagonal entry inside a subdomain (IluSchedule::diag_only: no triangles
// in the cell graph): U = A, L_ik = A_ik / p_k, and only the pivots p_i = A_ii - sum_k (A_ik / p_k) A_ki recur.  As
// k_dilu_pivots does for the flow matrix, A_ik, A_ki and k of a row's (<= 4) in-brick lower couplings are fetched BEFORE
// the level loop, all rows of the brick at once, and the loop reads inverted pivots out of LDS only -- k_dg_factor pays
// dependent global round trips (column, descriptor, columns of k, values) in every one of a 16 x 16 x 2 brick's 32 levels
// (MEASURED at 100^3, nt = 4: 2.25 ms of a 3.8-ms solve).  Same products in the same order: the same factor.
// k_dg_pivots leaves the inverted pivots in the diagonal slots; k_dg_scale_lower then forms L, a row at a time.
template <int NC>
__global__ __launch_bounds__(1024) void k_dg_pivots(int n, int nt, int nsub, const int* __restrict__ sub_ptr,
                                                    const int* __restrict__ sub_nlev, const int* __restrict__ row_info,
                                                    const int* __restrict__ col, const double* __restrict__ aval,
                                                    double* __restrict__ fval, int* flags) {
  constexpr int NPL = 4;
  extern __shared__ double pinv[];  // [T][NC]
  const int s = xcd_remap(blockIdx.x, nsub);
  if (s >= nsub) return;
  const int lo = sub_ptr[s], R = sub_ptr[s + 1] - lo;
  const int nlf = sub_nlev[s] & 0xffff;
  const int tid = threadIdx.x, i = lo + tid;
  const bool active = tid < R;
  int lfirst = 0, dslot = 0, ulast = 0, lf = -1, lb = 0;
  int koff[NPL], kslot[NPL];
#pragma unroll
  for (int p = 0; p < NPL; p++) { koff[p] = -1; kslot[p] = -1; }
  if (active) {
    unpack_info(row_info[i], lfirst, dslot, ulast, lf, lb);
#pragma unroll
    for (int p = 0; p < NPL; p++) {
      const int q = lfirst + p;
      if (q < dslot) {
        const int k = col[(size_t)q * n + i];
        int kl, kd, ku, kf, kb;
        unpack_info(row_info[k], kl, kd, ku, kf, kb);
        koff[p] = k - lo;
        for (int r2 = kd + 1; r2 < ku; r2++)
          if (col[(size_t)r2 * n + k] == i) { kslot[p] = r2; break; }
      }
    }
  }
  for (int t0 = 0; t0 < nt; t0 += NC) {
    double P[NC], aik[NPL][NC], aki[NPL][NC];
#pragma unroll
    for (int k = 0; k < NC; k++) {
      P[k] = (active && t0 + k < nt) ? aval[dg_ix(n, nt, dslot, t0 + k, i)] : 1.0;
#pragma unroll
      for (int p = 0; p < NPL; p++) {
        const bool on = koff[p] >= 0 && t0 + k < nt;
        aik[p][k] = on ? aval[dg_ix(n, nt, lfirst + p, t0 + k, i)] : 0.0;
        aki[p][k] = (on && kslot[p] >= 0) ? aval[dg_ix(n, nt, kslot[p], t0 + k, lo + koff[p])] : 0.0;
      }
    }
    for (int lev = 0; lev < nlf; lev++) {
      if (active && lf == lev) {
#pragma unroll
        for (int p = 0; p < NPL; p++) {
          if (koff[p] >= 0) {
#pragma unroll
            for (int k = 0; k < NC; k++) P[k] -= (aik[p][k] * pinv[koff[p] * NC + k]) * aki[p][k];
          }
        }
#pragma unroll
        for (int k = 0; k < NC; k++) {
          if (P[k] == 0.0) atomicMax(&flags[0], 1);
          const double inv = 1.0 / P[k];
          pinv[tid * NC + k] = inv;
          if (t0 + k < nt) fval[dg_ix(n, nt, dslot, t0 + k, i)] = inv;
        }
      }
      __syncthreads();
    }
  }
}
// L_ik = A_ik inv(p_k) on the in-subdomain lower slots (fval: a copy of A with the inverted pivots in the diagonal slots)
__global__ __launch_bounds__(TPB) void k_dg_scale_lower(int n, int nt, const int* __restrict__ row_info,
                                                        const int* __restrict__ col, double* __restrict__ fval) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  int lfirst, dslot, ulast, lf, lb;
  unpack_info(row_info[i], lfirst, dslot, ulast, lf, lb);
  for (int q = lfirst; q < dslot; q++) {
    const int k = col[(size_t)q * n + i];
    int kl, kd, ku, kf, kb;
    unpack_info(row_info[k], kl, kd, ku, kf, kb);
    for (int t = 0; t < nt; t++) fval[dg_ix(n, nt, q, t, i)] *= fval[dg_ix(n, nt, kd, t, k)];
  }
}

__global__ __launch_bounds__(TPB) void k_dg_lvl_factor(int n, int nt, int cnt, const int* __restrict__ ord,
                                                       const int* __restrict__ row_info, const int* __restrict__ col,
                                                       double* fval, int* flags) {
  const int t = blockIdx.x * TPB + threadIdx.x;
  if (t >= cnt) return;
  const int i = ord[t];
  int lfirst, dslot, ulast, lf, lb;
  dg_info<2>(row_info, nullptr, i, lfirst, dslot, ulast, lf, lb);
  dg_factor_row<2>(n, nt, i, lfirst, dslot, ulast, row_info, nullptr, col, fval, flags);
}

// forward (FWD): y_i = t_i - sum_{k < i} L_ik y_k; backward: x_i = inv(d_i) (y_i - sum_{j > i} U_ij x_j); in place, every tracer
template <bool FWD>
__global__ __launch_bounds__(TPB) void k_dg_lvl_solve(int n, int nt, int cnt, const int* __restrict__ ord,
                                                      const int* __restrict__ row_info, const int* __restrict__ col,
                                                      const double* __restrict__ fval, double* z) {
  const int t = blockIdx.x * TPB + threadIdx.x;
  if (t >= cnt) return;
  const int i = ord[t];
  int lfirst, dslot, ulast;
  unpack_info_wide(row_info[i], lfirst, dslot, ulast);
  double acc[MAX_TRACERS];
#pragma unroll
  for (int k = 0; k < MAX_TRACERS; k++) acc[k] = k < nt ? z[(size_t)i * nt + k] : 0.0;
  const int q0 = FWD ? lfirst : dslot + 1, q1 = FWD ? dslot : ulast;
  for (int q = q0; q < q1; q++) {
    const int c = col[(size_t)q * n + i];
#pragma unroll
    for (int k = 0; k < MAX_TRACERS; k++)
      if (k < nt) acc[k] -= fval[dg_ix(n, nt, q, k, i)] * z[(size_t)c * nt + k];
  }
#pragma unroll
  for (int k = 0; k < MAX_TRACERS; k++)
    if (k < nt) z[(size_t)i * nt + k] = FWD ? acc[k] : fval[dg_ix(n, nt, dslot, k, i)] * acc[k];
}

// ---- the fused preconditioned operator of a brick: z = U^-1 L^-1 (A in) (SPMV) or z = U^-1 L^-1 in ---------------------
// One workgroup per brick, one thread per row; a chunk's NC right-hand sides of the brick live in LDS ([row][NC]) and the
// two substitutions run level by level out of it between workgroup barriers -- one barrier per level for all NC tracers.
// WM 8: the factor row's 8 x NC values are pulled into registers before the first barrier (all loads in flight at once);
// WM 16 (cells with 9 .. 16 faces): they are read where they are used, sixteen slots of four would not fit the registers
// of a 1024-thread workgroup.
template <int NC, bool SPMV, int WM>
__global__ __launch_bounds__(1024) void k_dg_pc(int n, int W, int nt, int nsub, const int* __restrict__ sub_ptr,
                                                const int* __restrict__ sub_nlev, const int* __restrict__ row_info,
                                                const unsigned long long* __restrict__ row_infow,
                                                const int* __restrict__ col, const double* __restrict__ aval,
                                                const double* __restrict__ fval, const double* __restrict__ in,
                                                double* __restrict__ z, const int* __restrict__ sub_list) {
  constexpr bool PRE = WM <= WMAX;
  extern __shared__ __attribute__((aligned(16))) double ys[];  // [T][NC]
  int s = xcd_remap(blockIdx.x, nsub);
  if (s >= nsub) return;
  if (sub_list) s = sub_list[s];
  const int lo = sub_ptr[s], R = sub_ptr[s + 1] - lo;
  const int nl = sub_nlev[s];
  const int nlf = nl & 0xffff, nlb = nl >> 16;
  const int tid = threadIdx.x, i = lo + tid;
  const bool active = tid < R;
  int lfirst = 0, dslot = 0, ulast = 0, lf = -1, lb = -1;
  int cg[WM];
#pragma unroll
  for (int q = 0; q < WM; q++) cg[q] = i;
  if (active) {
    dg_info<(WM > WMAX) ? 1 : 0>(row_info, row_infow, i, lfirst, dslot, ulast, lf, lb);
#pragma unroll
    for (int q = 0; q < WM; q++)
      if (q < W) cg[q] = load_col(col, (size_t)q * n + i);
  }
  for (int t0 = 0; t0 < nt; t0 += NC) {
    double f[PRE ? WM : 1][NC];
    double dv[NC], out[NC];
#pragma unroll
    for (int k = 0; k < NC; k++) { dv[k] = 0.0; out[k] = 0.0; }
    if (active) {
      double acc[NC];
#pragma unroll
      for (int k = 0; k < NC; k++) acc[k] = 0.0;
      if constexpr (SPMV) {
#pragma unroll
        for (int q = 0; q < WM; q++) {
          if (q < W) {
#pragma unroll
            for (int k = 0; k < NC; k++)
              if (t0 + k < nt) acc[k] += aval[dg_ix(n, nt, q, t0 + k, i)] * in[(size_t)cg[q] * nt + t0 + k];
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < NC; k++)
          if (t0 + k < nt) acc[k] = in[(size_t)i * nt + t0 + k];
      }
      if constexpr (PRE) {
#pragma unroll
        for (int q = 0; q < WM; q++) {
#pragma unroll
          for (int k = 0; k < NC; k++) f[q][k] = (q < W && t0 + k < nt) ? fval[dg_ix(n, nt, q, t0 + k, i)] : 0.0;
        }
      }
#pragma unroll
      for (int k = 0; k < NC; k++) {
        if (t0 + k < nt) dv[k] = fval[dg_ix(n, nt, dslot, t0 + k, i)];
        ys[tid * NC + k] = acc[k];
      }
    }
    __syncthreads();
    // sum_q m_q y[col_q] over the in-brick lower (LOWER) or upper slots of this thread's row
    auto gather = [&](bool lower, double* sum) {
#pragma unroll
      for (int q = 0; q < WM; q++) {
        const bool take = lower ? (q >= lfirst && q < dslot) : (q > dslot && q < ulast);
        if (take) {
          const int c = cg[q] - lo;
#pragma unroll
          for (int k = 0; k < NC; k++) {
            double m;
            if constexpr (PRE) m = f[q][k];
            else m = t0 + k < nt ? fval[dg_ix(n, nt, q, t0 + k, i)] : 0.0;
            sum[k] += m * ys[c * NC + k];
          }
        }
      }
    };
    for (int lev = 1; lev < nlf; lev++) {  // level-0 rows have no lower couplings
      if (lf == lev) {
        double sum[NC];
#pragma unroll
        for (int k = 0; k < NC; k++) sum[k] = 0.0;
        gather(true, sum);
#pragma unroll
        for (int k = 0; k < NC; k++) ys[tid * NC + k] -= sum[k];
      }
      __syncthreads();
    }
    for (int lev = 0; lev < nlb; lev++) {
      if (lb == lev) {
        double sum[NC];
#pragma unroll
        for (int k = 0; k < NC; k++) sum[k] = 0.0;
        gather(false, sum);
#pragma unroll
        for (int k = 0; k < NC; k++) {
          out[k] = dv[k] * (ys[tid * NC + k] - sum[k]);
          ys[tid * NC + k] = out[k];
        }
      }
      __syncthreads();
    }
    if (active) {
#pragma unroll
      for (int k = 0; k < NC; k++)
        if (t0 + k < nt) z[(size_t)i * nt + t0 + k] = out[k];
    }
  }
}

// values on the BCSR pattern, [block][tracer] (wai_tracer_block_system)
__global__ __launch_bounds__(TPB) void k_dg_to_bcsr(int n, int W, int nt, const int* __restrict__ rowptr,
                                                    const double* __restrict__ ell, double* __restrict__ bcsr) {
  const size_t t = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= (size_t)n * W) return;
  const int s = (int)(t / n), i = (int)(t - (size_t)s * n);
  const int a = rowptr[i], cnt = rowptr[i + 1] - a;
  if (s >= cnt) return;
  for (int k = 0; k < nt; k++) bcsr[(size_t)(a + s) * nt + k] = ell[dg_ix(n, nt, s, k, i)];
}

// ---- launchers ----------------------------------------------------------------------------------------------------------
// tracers a thread works on at a time: nt itself up to four, chunks of four above
template <class F>
static void with_nc(int nt, F&& f) {
  if (nt == 2) f(std::integral_constant<int, 2>{});
  else if (nt == 3) f(std::integral_constant<int, 3>{});
  else f(std::integral_constant<int, 4>{});
}

int launch_dg_spmv(wai_ctx* c, const Bcsr& M, const double* x, double* y) {
  const int nblk = (M.n + TPB - 1) / TPB, grid = ((nblk + 7) / 8) * 8;
  with_nc(M.dg, [&](auto nc) {
    hipLaunchKernelGGL((k_dg_spmv<decltype(nc)::value>), grid, TPB, 0, c->stream, M.n, M.W, M.dg, nblk, M.col, M.val, x, y);
  });
  return 0;
}

int launch_dg_factor(wai_ctx* c, const Bcsr& M, IluSchedule& s) {
  if (hipMemcpyAsync(M.fdg, M.val, sizeof(double) * (size_t)M.W * M.dg * M.n, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return -1;
  if (s.big) {
    for (int lev = 0; lev < s.nlev_f; lev++) {
      const int a = s.lev_f_ptr[lev], cnt = s.lev_f_ptr[lev + 1] - a, g = (cnt + TPB - 1) / TPB;
      if (cnt <= 0) continue;
      hipLaunchKernelGGL(k_dg_lvl_factor, g, TPB, 0, c->stream, M.n, M.dg, cnt, s.ord_f + a, s.row_info, M.col, M.fdg, c->d_flags);
    }
  } else {
    const int grid = ((s.nsub + 7) / 8) * 8, T = pc_threads(s);
    if (s.diag_only && s.max_nl <= 4) {   // pivots only, couplings fetched ahead of the level loop; then L
      with_nc(M.dg, [&](auto nc) {
        constexpr int NC = decltype(nc)::value;
        hipLaunchKernelGGL((k_dg_pivots<NC>), grid, T, (size_t)T * NC * sizeof(double), c->stream, M.n, M.dg, s.nsub, s.sub_ptr, s.sub_nlev,
                           s.row_info, M.col, M.val, M.fdg, c->d_flags);
      });
      hipLaunchKernelGGL(k_dg_scale_lower, (M.n + TPB - 1) / TPB, TPB, 0, c->stream, M.n, M.dg, s.row_info, M.col, M.fdg);
    } else if (s.wide)
      hipLaunchKernelGGL(k_dg_factor<1>, grid, T, 0, c->stream, M.n, M.dg, s.nsub, s.sub_ptr, s.sub_nlev, s.row_info, s.row_infow, M.col, M.fdg, c->d_flags);
    else
      hipLaunchKernelGGL(k_dg_factor<0>, grid, T, 0, c->stream, M.n, M.dg, s.nsub, s.sub_ptr, s.sub_nlev, s.row_info, s.row_infow, M.col, M.fdg, c->d_flags);
  }
  return 0;
}

int launch_dg_pc(wai_ctx* c, const Bcsr& M, const IluSchedule& s, bool spmv, const double* in, double* z, const int* list, int nrun) {
  if (!list) { nrun = s.nsub; list = s.sub_order; }
  const int grid = ((nrun + 7) / 8) * 8, T = pc_threads(s);
  with_nc(M.dg, [&](auto nc) {
    constexpr int NC = decltype(nc)::value;
    const size_t lds = (size_t)T * NC * sizeof(double);
    with_flag(spmv, [&](auto sp) {
      constexpr bool SP = decltype(sp)::value;
      if (s.wide)
        hipLaunchKernelGGL((k_dg_pc<NC, SP, WMAX_WIDE>), grid, T, lds, c->stream, M.n, M.W, M.dg, nrun, s.sub_ptr, s.sub_nlev, s.row_info,
                           s.row_infow, M.col, M.val, M.fdg, in, z, list);
      else
        hipLaunchKernelGGL((k_dg_pc<NC, SP, WMAX>), grid, T, lds, c->stream, M.n, M.W, M.dg, nrun, s.sub_ptr, s.sub_nlev, s.row_info,
                           s.row_infow, M.col, M.val, M.fdg, in, z, list);
    });
  });
  return 0;
}

int launch_dg_big_solve(wai_ctx* c, const Bcsr& M, const IluSchedule& s, double* z) {
  for (int lev = 1; lev < s.nlev_f; lev++) {   // level-0 rows of the forward sweep have nothing to subtract
    const int a = s.lev_f_ptr[lev], cnt = s.lev_f_ptr[lev + 1] - a;
    if (cnt > 0) hipLaunchKernelGGL(k_dg_lvl_solve<true>, (cnt + TPB - 1) / TPB, TPB, 0, c->stream, M.n, M.dg, cnt, s.ord_f + a, s.row_info, M.col, M.fdg, z);
  }
  for (int lev = 0; lev < s.nlev_b; lev++) {
    const int a = s.lev_b_ptr[lev], cnt = s.lev_b_ptr[lev + 1] - a;
    if (cnt > 0) hipLaunchKernelGGL(k_dg_lvl_solve<false>, (cnt + TPB - 1) / TPB, TPB, 0, c->stream, M.n, M.dg, cnt, s.ord_b + a, s.row_info, M.col, M.fdg, z);
  }
  return 0;
}

int launch_dg_to_bcsr(wai_ctx* c, const Bcsr& M, double* bcsr) {
  const size_t tot = (size_t)M.n * M.W;
  hipLaunchKernelGGL(k_dg_to_bcsr, (int)((tot + TPB - 1) / TPB), TPB, 0, c->stream, M.n, M.W, M.dg, M.rowptr, M.val, bcsr);
  return 0;
}

}  // namespace wai

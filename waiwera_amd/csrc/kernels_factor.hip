// K7/K8 outside the fused launches: the ILU(0) / DILU factorisation kernels of the brick schedules, the level-per-launch
// factorisation and substitutions for subdomains of any size, the dense LU apply, and their launchers.
#include "linalg_device.hip.h"
#include "pc_lu.hip.h"

namespace wai {

// ---- K7: block ILU(0) numeric factorisation (IKJ), one workgroup per subdomain ----------------
// Works in place on fval (a copy of the matrix); rows of one dependency level are independent.
// On exit the diagonal slot of every row holds the inverted pivot block.
template <int BS>
__global__ void k_ilu_factor(int n, int nsub, const int* __restrict__ sub_ptr,
                             const int* __restrict__ sub_nlev, const int* __restrict__ row_info,
                             const int* __restrict__ col, double* fval, double* __restrict__ dinv,
                             int* flags) {
  constexpr int BB = BS * BS;
  const int s = xcd_remap(blockIdx.x, nsub);
  if (s >= nsub) return;
  const int lo = sub_ptr[s], R = sub_ptr[s + 1] - lo;
  const int nlf = sub_nlev[s] & 0xffff;
  const int i = lo + threadIdx.x;
  const bool active = (int)threadIdx.x < R;
  int lfirst = 0, dslot = 0, ulast = 0, lf = -1, lb = 0;
  if (active) unpack_info(row_info[i], lfirst, dslot, ulast, lf, lb);
  for (int lev = 0; lev < nlf; lev++) {
    if (active && lf == lev) {
      for (int q = lfirst; q < dslot; q++) {
        const int k = col[(size_t)q * n + i];
        int kl, kd, ku, kf, kb;
        unpack_info(row_info[k], kl, kd, ku, kf, kb);
        double w[BB], d[BB], t[BB];
#pragma unroll
        for (int z = 0; z < BB; z++) {
          w[z] = fval[vix<BS>(n, q, z, i)];
          d[z] = fval[vix<BS>(n, kd, z, k)];
        }
#pragma unroll
        for (int r = 0; r < BS; r++)
#pragma unroll
          for (int c = 0; c < BS; c++) {
            double acc = 0.0;
#pragma unroll
            for (int e = 0; e < BS; e++) acc += w[r * BS + e] * d[e * BS + c];
            t[r * BS + c] = acc;
          }
#pragma unroll
        for (int z = 0; z < BB; z++) fval[vix<BS>(n, q, z, i)] = t[z];
        for (int r2 = kd + 1; r2 < ku; r2++) {
          const int j = col[(size_t)r2 * n + k];
          for (int q2 = q + 1; q2 < ulast; q2++) {
            if (col[(size_t)q2 * n + i] != j) continue;
            double u[BB];
#pragma unroll
            for (int z = 0; z < BB; z++) u[z] = fval[vix<BS>(n, r2, z, k)];
#pragma unroll
            for (int r = 0; r < BS; r++)
#pragma unroll
              for (int c = 0; c < BS; c++) {
                double acc = 0.0;
#pragma unroll
                for (int e = 0; e < BS; e++) acc += t[r * BS + e] * u[e * BS + c];
                fval[vix<BS>(n, q2, r * BS + c, i)] -= acc;
              }
            break;
          }
        }
      }
      double piv[BB], inv[BB];
#pragma unroll
      for (int z = 0; z < BB; z++) piv[z] = fval[vix<BS>(n, dslot, z, i)];
      if (!block_inverse<BS>(piv, inv)) atomicMax(&flags[0], 1);
#pragma unroll
      for (int z = 0; z < BB; z++) {
        fval[vix<BS>(n, dslot, z, i)] = inv[z];
        dinv[dix<BS>(n, z, i)] = inv[z];
      }
    }
    __threadfence_block();
    __syncthreads();
  }
}

// The same for the schedules with rows of 9 .. 16 blocks, on their 64-bit row descriptor.  A copy rather than a body
// shared with k_ilu_factor: compiled through a shared inline function, k_ilu_factor<4> spilled differently.
template <int BS>
__global__ void k_ilu_factor_wide(int n, int nsub, const int* __restrict__ sub_ptr,
                                  const int* __restrict__ sub_nlev, const unsigned long long* __restrict__ row_info,
                                  const int* __restrict__ col, double* fval, double* __restrict__ dinv,
                                  int* flags) {
  constexpr int BB = BS * BS;
  const int s = xcd_remap(blockIdx.x, nsub);
  if (s >= nsub) return;
  const int lo = sub_ptr[s], R = sub_ptr[s + 1] - lo;
  const int nlf = sub_nlev[s] & 0xffff;
  const int i = lo + threadIdx.x;
  const bool active = (int)threadIdx.x < R;
  int lfirst = 0, dslot = 0, ulast = 0, lf = -1, lb = 0;
  if (active) unpack_info_w(row_info[i], lfirst, dslot, ulast, lf, lb);
  for (int lev = 0; lev < nlf; lev++) {
    if (active && lf == lev) {
      for (int q = lfirst; q < dslot; q++) {
        const int k = col[(size_t)q * n + i];
        int kl, kd, ku, kf, kb;
        unpack_info_w(row_info[k], kl, kd, ku, kf, kb);
        double w[BB], d[BB], t[BB];
#pragma unroll
        for (int z = 0; z < BB; z++) {
          w[z] = fval[vix<BS>(n, q, z, i)];
          d[z] = fval[vix<BS>(n, kd, z, k)];
        }
#pragma unroll
        for (int r = 0; r < BS; r++)
#pragma unroll
          for (int c = 0; c < BS; c++) {
            double acc = 0.0;
#pragma unroll
            for (int e = 0; e < BS; e++) acc += w[r * BS + e] * d[e * BS + c];
            t[r * BS + c] = acc;
          }
#pragma unroll
        for (int z = 0; z < BB; z++) fval[vix<BS>(n, q, z, i)] = t[z];
        for (int r2 = kd + 1; r2 < ku; r2++) {
          const int j = col[(size_t)r2 * n + k];
          for (int q2 = q + 1; q2 < ulast; q2++) {
            if (col[(size_t)q2 * n + i] != j) continue;
            double u[BB];
#pragma unroll
            for (int z = 0; z < BB; z++) u[z] = fval[vix<BS>(n, r2, z, k)];
#pragma unroll
            for (int r = 0; r < BS; r++)
#pragma unroll
              for (int c = 0; c < BS; c++) {
                double acc = 0.0;
#pragma unroll
                for (int e = 0; e < BS; e++) acc += t[r * BS + e] * u[e * BS + c];
                fval[vix<BS>(n, q2, r * BS + c, i)] -= acc;
              }
            break;
          }
        }
      }
      double piv[BB], inv[BB];
#pragma unroll
      for (int z = 0; z < BB; z++) piv[z] = fval[vix<BS>(n, dslot, z, i)];
      if (!block_inverse<BS>(piv, inv)) atomicMax(&flags[0], 1);
#pragma unroll
      for (int z = 0; z < BB; z++) {
        fval[vix<BS>(n, dslot, z, i)] = inv[z];
        dinv[dix<BS>(n, z, i)] = inv[z];
      }
    }
    __threadfence_block();
    __syncthreads();
  }
}

// ---- K7 for the diagonal-only case: pivots only ------------------------------------------------
// When ILU(0) never updates an off-diagonal block (diag_only), the factor is the pivot blocks
// P_i = A_ii - sum_{k < i in the subdomain} A_ik inv(P_k) A_ki; with the pivot-scaled rows nothing
// else of the factor is ever read.  One workgroup per subdomain, rows by dependency level, the
// inverted pivots of the subdomain in LDS; A_ki is the block of row k whose column is i (found
// among k's <= 3..4 in-subdomain upper slots, served by L2: the subdomain's rows are contiguous).
// No copy of the matrix, no in-place update of one: ~230 B per row read, 32 B written.
// PRE (rows with at most 3 in-subdomain lower blocks, BS <= 2): A_ik, A_ki and k of every lower
// coupling are fetched BEFORE the level loop, all rows of the brick at once; the loop itself then only
// reads inverted pivots from LDS.  Without it every level pays four dependent global round trips
// (column, row descriptor of k, its columns, the block) for its handful of rows.  Same arithmetic, same
// order: identical pivots.  MEASURED: 3.69 -> 0.99 ms at 216^3 (bs 2, 64 levels per brick); for 3 x 3 blocks
// (54 more doubles per thread, 80-row bricks with 13 levels) 2.98 -> 3.08 ms and 0.85 -> 1.16: not used.
template <int BS, bool PRE>
__global__ void k_dilu_pivots(int n, int nsub, const int* __restrict__ sub_ptr,
                              const int* __restrict__ sub_nlev, const int* __restrict__ row_info,
                              const int* __restrict__ col, const double* __restrict__ aval,
                              double* __restrict__ dinv, int* flags) {
  constexpr int BB = BS * BS;
  extern __shared__ double pinv[];  // [T][BB]
  const int s = xcd_remap(blockIdx.x, nsub);
  if (s >= nsub) return;
  const int lo = sub_ptr[s], R = sub_ptr[s + 1] - lo;
  const int nlf = sub_nlev[s] & 0xffff;
  const int tid = threadIdx.x, i = lo + tid;
  const bool active = tid < R;
  int lfirst = 0, dslot = 0, ulast = 0, lf = -1, lb = 0;
  double P[BB];
#pragma unroll
  for (int e = 0; e < BB; e++) P[e] = 0.0;
  if (active) {
    unpack_info(row_info[i], lfirst, dslot, ulast, lf, lb);
    load_block<BS>(aval, n, dslot, i, P);
  }
  constexpr int NP = PRE ? 3 : 1;
  double paik[NP][BB], paki[NP][BB];
  int pk_off[NP];
  if constexpr (PRE) {
#pragma unroll
    for (int p = 0; p < NP; p++) {
      pk_off[p] = -1;
#pragma unroll
      for (int e = 0; e < BB; e++) { paik[p][e] = 0.0; paki[p][e] = 0.0; }
      const int q = lfirst + p;
      if (active && q < dslot) {
        const int k = col[(size_t)q * n + i];
        int kl, kd, ku, kf, kb;
        unpack_info(row_info[k], kl, kd, ku, kf, kb);
        load_block<BS>(aval, n, q, i, paik[p]);
        for (int r2 = kd + 1; r2 < ku; r2++)
          if (col[(size_t)r2 * n + k] == i) { load_block<BS>(aval, n, r2, k, paki[p]); break; }
        pk_off[p] = (k - lo) * BB;
      }
    }
  }
  // P -= (A_ik inv(P_k)) A_ki
  auto update = [&](const double* aik, const double* pk, const double* aki) {
    double t[BB];
#pragma unroll
    for (int r = 0; r < BS; r++)
#pragma unroll
      for (int c = 0; c < BS; c++) {
        double acc = 0.0;
#pragma unroll
        for (int e = 0; e < BS; e++) acc += aik[r * BS + e] * pk[e * BS + c];
        t[r * BS + c] = acc;
      }
#pragma unroll
    for (int r = 0; r < BS; r++)
#pragma unroll
      for (int c = 0; c < BS; c++) {
        double acc = 0.0;
#pragma unroll
        for (int e = 0; e < BS; e++) acc += t[r * BS + e] * aki[e * BS + c];
        P[r * BS + c] -= acc;
      }
  };
  for (int lev = 0; lev < nlf; lev++) {
    if (active && lf == lev) {
      if constexpr (PRE) {
#pragma unroll
        for (int p = 0; p < NP; p++)
          if (pk_off[p] >= 0) update(paik[p], pinv + pk_off[p], paki[p]);
      } else {
        for (int q = lfirst; q < dslot; q++) {
          const int k = col[(size_t)q * n + i];
          int kl, kd, ku, kf, kb;
          unpack_info(row_info[k], kl, kd, ku, kf, kb);
          double aik[BB], aki[BB];
          load_block<BS>(aval, n, q, i, aik);
#pragma unroll
          for (int e = 0; e < BB; e++) aki[e] = 0.0;
          for (int r2 = kd + 1; r2 < ku; r2++)
            if (col[(size_t)r2 * n + k] == i) { load_block<BS>(aval, n, r2, k, aki); break; }
          update(aik, pinv + (size_t)(k - lo) * BB, aki);
        }
      }
      double inv[BB];
      if (!block_inverse<BS>(P, inv)) atomicMax(&flags[0], 1);
#pragma unroll
      for (int e = 0; e < BB; e++) {
        pinv[(size_t)tid * BB + e] = inv[e];
        dinv[dix<BS>(n, e, i)] = inv[e];
      }
    }
    __syncthreads();
  }
}

// The same recurrence for block sizes 3 and 4, where the lower couplings' blocks do not fit the registers
// beside the pivot and its inverse (k_dilu_pivots<3, PRE> measured no faster than the pointer-chasing loop):
// A_ik and A_ki of every lower coupling go to LDS before the level loop -- thread-private columns,
// [coupling][element][row], so neither the store nor the reload conflicts -- and A_ki is addressed through the
// transposed slot the symbolic phase recorded (row_tslot), i.e. two dependent global round trips per brick
// (column, blocks) instead of four per level.  Same products in the same order as k_dilu_pivots: identical pivots.
// RAIK (bricks of one wave, round 3): A_ik stays in registers (27 doubles per coupling set) and only A_ki and the inverted pivots
// live in LDS -- 18 instead of 32 KB per 64-row brick, eight instead of five bricks per CU.  Same products, same order.
template <int BS, int NPL, bool RAIK>
__global__ __launch_bounds__(256) void k_dilu_pivots_lds(int n, int nsub, int cap, const int* __restrict__ sub_ptr,
                                  const int* __restrict__ sub_nlev, const int* __restrict__ row_info,
                                  const int* __restrict__ row_tslot, const int* __restrict__ col,
                                  const double* __restrict__ aval, double* __restrict__ dinv, int* flags) {
  constexpr int BB = BS * BS;
  extern __shared__ double sm[];  // pinv [BB][cap], A_ik [NPL][BB][cap], A_ki [NPL][BB][cap]
  const int s = xcd_remap(blockIdx.x, nsub);
  if (s >= nsub) return;
  const int lo = sub_ptr[s], R = sub_ptr[s + 1] - lo;
  const int nlf = sub_nlev[s] & 0xffff;
  const int tid = threadIdx.x, i = lo + tid;
  const bool active = tid < R;
  double* pinv = sm;
  double* laik = sm + (size_t)BB * cap;
  double* laki = RAIK ? laik : laik + (size_t)NPL * BB * cap;
  double raik[RAIK ? NPL : 1][BB];
  int lfirst = 0, dslot = 0, ulast = 0, lf = -1, lb = 0;
  int koff[NPL];
  double P[BB];
#pragma unroll
  for (int e = 0; e < BB; e++) P[e] = 0.0;
#pragma unroll
  for (int p = 0; p < NPL; p++) koff[p] = -1;
  if (active) {
    unpack_info(row_info[i], lfirst, dslot, ulast, lf, lb);
    const int tp = row_tslot[i];
    int ks[NPL];
#pragma unroll
    for (int p = 0; p < NPL; p++) {
      ks[p] = i;
      if (lfirst + p < dslot) ks[p] = col[(size_t)(lfirst + p) * n + i];
    }
    load_block<BS>(aval, n, dslot, i, P);
#pragma unroll
    for (int p = 0; p < NPL; p++) {
      const int q = lfirst + p;
      if (q < dslot) {
        const int k = ks[p], r2 = (tp >> (4 * p)) & 15;
        koff[p] = k - lo;
#pragma unroll
        for (int e = 0; e < BB; e++) {
          if constexpr (RAIK) raik[p][e] = aval[vix<BS>(n, q, e, i)];
          else laik[(size_t)(p * BB + e) * cap + tid] = aval[vix<BS>(n, q, e, i)];
          laki[(size_t)(p * BB + e) * cap + tid] = r2 == 15 ? 0.0 : aval[vix<BS>(n, r2, e, k)];
        }
      }
    }
  }
  for (int lev = 0; lev < nlf; lev++) {
    if (active && lf == lev) {
#pragma unroll
      for (int p = 0; p < NPL; p++) {
        if (koff[p] >= 0) {   // P -= (A_ik inv(P_k)) A_ki
          double aik[BB], pk[BB], t[BB];
#pragma unroll
          for (int e = 0; e < BB; e++) {
            if constexpr (RAIK) aik[e] = raik[p][e];
            else aik[e] = laik[(size_t)(p * BB + e) * cap + tid];
            pk[e] = pinv[(size_t)e * cap + koff[p]];
          }
#pragma unroll
          for (int r = 0; r < BS; r++)
#pragma unroll
            for (int c = 0; c < BS; c++) {
              double acc = 0.0;
#pragma unroll
              for (int e = 0; e < BS; e++) acc += aik[r * BS + e] * pk[e * BS + c];
              t[r * BS + c] = acc;
            }
#pragma unroll
          for (int e = 0; e < BB; e++) aik[e] = laki[(size_t)(p * BB + e) * cap + tid];   // A_ki
#pragma unroll
          for (int r = 0; r < BS; r++)
#pragma unroll
            for (int c = 0; c < BS; c++) {
              double acc = 0.0;
#pragma unroll
              for (int e = 0; e < BS; e++) acc += t[r * BS + e] * aik[e * BS + c];
              P[r * BS + c] -= acc;
            }
        }
      }
      double inv[BB];
      if (!block_inverse<BS>(P, inv)) atomicMax(&flags[0], 1);
#pragma unroll
      for (int e = 0; e < BB; e++) {
        pinv[(size_t)e * cap + tid] = inv[e];
        dinv[dix<BS>(n, e, i)] = inv[e];
      }
    }
    __syncthreads();
  }
}

// ---- pivot scaling for the diagonal-only case --------------------------------------------------
// ILU(0) is invariant under block-diagonal row scaling: ILU(0)(S A) = (S L S^-1)(S U), so
// (L'U')^-1 (S A) = (LU)^-1 A and (L'U')^-1 (S b) = (LU)^-1 b -- the preconditioned operator and
// right-hand side PETSc's left-preconditioned Krylov methods see are unchanged.  With S = the
// inverted pivots the scaled pivots are identities: the fused kernel then reads A' = S A (one
// pass, written here after every factorisation) and no pivot blocks, 32 of ~336 bytes per row less.
template <int BS>
__global__ __launch_bounds__(TPB) void k_scale_rows(int n, int W, const double* __restrict__ aval,
                                                    const double* __restrict__ dinv, double* __restrict__ sval) {
  constexpr int BB = BS * BS;
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  double d[BB];
  load_pivot<BS>(dinv, n, i, d);
  for (int q = 0; q < W; q++) {
    double a[BB];
    load_block<BS>(aval, n, q, i, a);
#pragma unroll
    for (int r = 0; r < BS; r++)
#pragma unroll
      for (int c = 0; c < BS; c++) {
        double t = 0.0;
#pragma unroll
        for (int e = 0; e < BS; e++) t += d[r * BS + e] * a[e * BS + c];
        sval[vix<BS>(n, q, r * BS + c, i)] = t;
      }
  }
}

// ---- subdomains of any size: one launch per dependency level ------------------------------------
// Rows of equal level are independent (across all subdomains), so the ILU(0) factorisation and the
// two substitutions of PCBJACOBI / PCASM with arbitrarily large blocks -- the reference's default is
// one block per MPI rank, src/timestepper.F90:1668-1669 -- run as a sequence of launches over the
// rows of each level; kernel boundaries order the levels.  Stored factor (L multipliers, U, inverted
// pivots), unfused.  This is the general path; the brick kernels above are the fast one.
template <int BS>
__global__ __launch_bounds__(TPB) void k_lvl_factor(int n, int cnt, const int* __restrict__ ord,
                                                    const int* __restrict__ row_info, const int* __restrict__ col,
                                                    double* fval, double* __restrict__ dinv, int* flags) {
  constexpr int BB = BS * BS;
  const int t = blockIdx.x * TPB + threadIdx.x;
  if (t >= cnt) return;
  const int i = ord[t];
  int lfirst, dslot, ulast;
  unpack_info_wide(row_info[i], lfirst, dslot, ulast);
  for (int q = lfirst; q < dslot; q++) {
    const int k = col[(size_t)q * n + i];
    int kl, kd, ku;
    unpack_info_wide(row_info[k], kl, kd, ku);
    double w[BB], d[BB], tt[BB];
#pragma unroll
    for (int z = 0; z < BB; z++) { w[z] = fval[vix<BS>(n, q, z, i)]; d[z] = dinv[dix<BS>(n, z, k)]; }
#pragma unroll
    for (int r = 0; r < BS; r++)
#pragma unroll
      for (int c = 0; c < BS; c++) {
        double acc = 0.0;
#pragma unroll
        for (int e = 0; e < BS; e++) acc += w[r * BS + e] * d[e * BS + c];
        tt[r * BS + c] = acc;
      }
#pragma unroll
    for (int z = 0; z < BB; z++) fval[vix<BS>(n, q, z, i)] = tt[z];
    for (int r2 = kd + 1; r2 < ku; r2++) {
      const int j = col[(size_t)r2 * n + k];
      for (int q2 = q + 1; q2 < ulast; q2++) {
        if (col[(size_t)q2 * n + i] != j) continue;
        double u[BB];
#pragma unroll
        for (int z = 0; z < BB; z++) u[z] = fval[vix<BS>(n, r2, z, k)];
#pragma unroll
        for (int r = 0; r < BS; r++)
#pragma unroll
          for (int c = 0; c < BS; c++) {
            double acc = 0.0;
#pragma unroll
            for (int e = 0; e < BS; e++) acc += tt[r * BS + e] * u[e * BS + c];
            fval[vix<BS>(n, q2, r * BS + c, i)] -= acc;
          }
        break;
      }
    }
  }
  double piv[BB], inv[BB];
#pragma unroll
  for (int z = 0; z < BB; z++) piv[z] = fval[vix<BS>(n, dslot, z, i)];
  if (!block_inverse<BS>(piv, inv)) atomicMax(&flags[0], 1);
#pragma unroll
  for (int z = 0; z < BB; z++) dinv[dix<BS>(n, z, i)] = inv[z];
}

// forward (FWD): y_i = t_i - sum_{k < i} L_ik y_k; backward: x_i = inv(D_i) (y_i - sum_{j > i} U_ij x_j); in place
// The update of ONE row, shared by k_lvl_solve and k_tile_solve so that both do the same operations in the same order -- the
// same contraction, the same bits: acc holds the row's entry on entry; its couplings are subtracted in slot order -- `begin(k)`
// announces the coupled row, `operand(k, c)` is entry c of its value (finished by an earlier level) --; backward the result is
// multiplied by the inverted pivot; `store(r, v)` takes entry r of the result.
template <int BS, bool FWD, class Begin, class Operand, class Store>
__device__ __forceinline__ void lvl_row_update(int n, int i, int lfirst, int dslot, int ulast, const int* col, const double* fval,
                                               const double* dinv, double (&acc)[BS], Begin begin, Operand operand, Store store) {
  constexpr int BB = BS * BS;
  const int q0 = FWD ? lfirst : dslot + 1, q1 = FWD ? dslot : ulast;
  for (int q = q0; q < q1; q++) {
    const int k = col[(size_t)q * n + i];
    double m[BB];
#pragma unroll
    for (int e = 0; e < BB; e++) m[e] = fval[vix<BS>(n, q, e, i)];
    begin(k);
#pragma unroll
    for (int r = 0; r < BS; r++)
#pragma unroll
      for (int c = 0; c < BS; c++) acc[r] -= m[r * BS + c] * operand(k, c);
  }
  if constexpr (FWD) {
#pragma unroll
    for (int r = 0; r < BS; r++) store(r, acc[r]);
  } else {
    double d[BB];
#pragma unroll
    for (int e = 0; e < BB; e++) d[e] = dinv[dix<BS>(n, e, i)];
#pragma unroll
    for (int r = 0; r < BS; r++) {
      double o = 0.0;
#pragma unroll
      for (int c = 0; c < BS; c++) o += d[r * BS + c] * acc[c];
      store(r, o);
    }
  }
}

template <int BS, bool FWD>
__global__ __launch_bounds__(TPB) void k_lvl_solve(int n, int cnt, const int* __restrict__ ord,
                                                   const int* __restrict__ row_info, const int* __restrict__ col,
                                                   const double* __restrict__ fval, const double* __restrict__ dinv,
                                                   double* z) {
  const int t = blockIdx.x * TPB + threadIdx.x;
  if (t >= cnt) return;
  const int i = ord[t];
  int lfirst, dslot, ulast;
  unpack_info_wide(row_info[i], lfirst, dslot, ulast);
  double acc[BS];
#pragma unroll
  for (int r = 0; r < BS; r++) acc[r] = z[(size_t)i * BS + r];
  lvl_row_update<BS, FWD>(n, i, lfirst, dslot, ulast, col, fval, dinv, acc, [](int) {},
                          [z](int k, int c) { return z[(size_t)k * BS + c]; }, [z, i](int r, double v) { z[(size_t)i * BS + r] = v; });
}

// ---- big subdomains cut into tiles: one launch per TILE level (wai_set_pc_tiles, tile_schedule.hpp) ---------------------
// The grid is the tiles of one tile level, one workgroup per tile, one thread per row.  The tile walks its in-tile row levels
// with one barrier each, as a brick kernel does: a row at its level subtracts its couplings in slot order through
// lvl_row_update -- what k_lvl_solve does for the row, bit for bit -- taking a coupled row's entry from the tile's copy in LDS
// where the column lies in the tile and from z in global memory otherwise, where a launch of an earlier tile level finished
// it.  No flag, no polling, nothing atomic between workgroups: kernel boundaries order the tile levels.  z is read and
// written by the same launch (a plain pointer); no tile of a launch reads a row another tile of that launch writes.
// LDS: max_tile_rows * BS doubles, at most 32 KB.
template <int BS, bool FWD>
__global__ __launch_bounds__(1024) void k_tile_solve(int n, const int* __restrict__ tiles, const int* __restrict__ tile_ptr,
                                                     const int* __restrict__ tile_nin, const int* __restrict__ row_lev,
                                                     const int* __restrict__ row_info, const int* __restrict__ col,
                                                     const double* __restrict__ fval, const double* __restrict__ dinv, double* z) {
  extern __shared__ double zt[];   // [rows of the tile][BS]
  const int t = tiles[blockIdx.x];
  const int lo = tile_ptr[t], R = tile_ptr[t + 1] - lo;
  const int nin = FWD ? (tile_nin[t] & 0xffff) : (int)((unsigned)tile_nin[t] >> 16);
  const int tid = threadIdx.x, i = lo + tid;
  const bool active = tid < R;
  int lfirst = 0, dslot = 0, ulast = 0, mine = -1;
  double acc[BS];
#pragma unroll
  for (int r = 0; r < BS; r++) acc[r] = 0.0;
  if (active) {
    unpack_info_wide(row_info[i], lfirst, dslot, ulast);
    mine = FWD ? (row_lev[i] & 0xffff) : (int)((unsigned)row_lev[i] >> 16);
#pragma unroll
    for (int r = 0; r < BS; r++) acc[r] = z[(size_t)i * BS + r];
  }
  for (int lev = 0; lev < nin; lev++) {
    if (mine == lev) {
      double zk[BS];   // the coupled row's value: the tile's copy, or what an earlier launch left in z
      lvl_row_update<BS, FWD>(n, i, lfirst, dslot, ulast, col, fval, dinv, acc,
                              [&](int k) {
                                const int kt = k - lo;
                                if ((unsigned)kt < (unsigned)R) {
#pragma unroll
                                  for (int c = 0; c < BS; c++) zk[c] = zt[kt * BS + c];
                                } else {
#pragma unroll
                                  for (int c = 0; c < BS; c++) zk[c] = z[(size_t)k * BS + c];
                                }
                              },
                              [&](int, int c) { return zk[c]; },
                              [&](int r, double v) {
                                zt[tid * BS + r] = v;
                                z[(size_t)i * BS + r] = v;
                              });
    }
    __syncthreads();
  }
}

// ---- multicolour order (wai_set_pc_ordering, colour_order.hpp): one launch per COLOUR ----------------------------------------
// Every subdomain's rows are eliminated sorted by (colour, row index) and rows of one colour do not couple, so the rows of a
// colour are independent across all subdomains: the factorisation is one launch per colour, a substitution sweep one launch
// per colour too, and kernel boundaries order the colours -- the launch-per-level path above with 2 levels (hexahedral and
// MINC meshes) where the natural order has hundreds.  A row's descriptor (ColourSchedule::slots, counts) lists its
// in-subdomain slots in elimination order, the lower ones first; nothing is renumbered, the factor sits on the matrix' own
// column planes: L multipliers (already multiplied by the inverted pivot of their column's row), U, and the inverted pivot in
// the diagonal slot and in dinv.
// The general IKJ row elimination on that order: for each lower coupling k in elimination order, L_ik = A_ik inv(P_k), then
// A_ij -= L_ik U_kj for every j that follows k in row k's order and is in row i's pattern too: the diagonal (j = i), a later
// lower coupling or an upper one.  Rows k belong to earlier colours: an earlier launch finished them.
template <int BS>
__global__ __launch_bounds__(TPB) void k_colour_factor(int n, int cnt, const int* __restrict__ rows,
                                                       const unsigned long long* __restrict__ slots, const int* __restrict__ counts,
                                                       const int* __restrict__ col, double* fval, double* __restrict__ dinv, int* flags) {
  constexpr int BB = BS * BS;
  const int t = blockIdx.x * TPB + threadIdx.x;
  if (t >= cnt) return;
  const int i = rows[t];
  const unsigned long long sl = slots[i];
  const int ct = counts[i], nl = colour_nlower(ct), nu = colour_nupper(ct), dslot = colour_dslot(ct);
  for (int p = 0; p < nl; p++) {
    const int q = colour_slot(sl, p);
    const int k = col[(size_t)q * n + i];
    double w[BB], d[BB], tt[BB];
#pragma unroll
    for (int z = 0; z < BB; z++) { w[z] = fval[vix<BS>(n, q, z, i)]; d[z] = dinv[dix<BS>(n, z, k)]; }
#pragma unroll
    for (int r = 0; r < BS; r++)
#pragma unroll
      for (int c = 0; c < BS; c++) {
        double acc = 0.0;
#pragma unroll
        for (int e = 0; e < BS; e++) acc += w[r * BS + e] * d[e * BS + c];
        tt[r * BS + c] = acc;
      }
#pragma unroll
    for (int z = 0; z < BB; z++) fval[vix<BS>(n, q, z, i)] = tt[z];
    const unsigned long long ksl = slots[k];
    const int kct = counts[k], knl = colour_nlower(kct), knu = colour_nupper(kct);
    for (int p2 = knl; p2 < knl + knu; p2++) {   // row k's upper blocks U_kj
      const int r2 = colour_slot(ksl, p2);
      const int j = col[(size_t)r2 * n + k];
      int q2 = -1;                               // the slot of A_ij in row i
      if (j == i) q2 = dslot;
      else
        for (int p3 = p + 1; p3 < nl + nu; p3++) {
          const int s3 = colour_slot(sl, p3);
          if (col[(size_t)s3 * n + i] == j) { q2 = s3; break; }
        }
      if (q2 < 0) continue;
      double u[BB];
#pragma unroll
      for (int z = 0; z < BB; z++) u[z] = fval[vix<BS>(n, r2, z, k)];
#pragma unroll
      for (int r = 0; r < BS; r++)
#pragma unroll
        for (int c = 0; c < BS; c++) {
          double acc = 0.0;
#pragma unroll
          for (int e = 0; e < BS; e++) acc += tt[r * BS + e] * u[e * BS + c];
          fval[vix<BS>(n, q2, r * BS + c, i)] -= acc;
        }
    }
  }
  double piv[BB], inv[BB];
#pragma unroll
  for (int z = 0; z < BB; z++) piv[z] = fval[vix<BS>(n, dslot, z, i)];
  if (!block_inverse<BS>(piv, inv)) atomicMax(&flags[0], 1);
#pragma unroll
  for (int z = 0; z < BB; z++) {
    fval[vix<BS>(n, dslot, z, i)] = inv[z];
    dinv[dix<BS>(n, z, i)] = inv[z];
  }
}

// One colour of one substitution, in place on z.  Forward (FWD): y_i = t_i - sum over the row's lower couplings L_ik y_k;
// backward: x_i = inv(P_i) (y_i - sum over its upper couplings U_ij x_j); both in the descriptor's order.  The coupled rows
// have other colours: an earlier launch of the sweep finished them, and no row of this launch is read by another.
template <int BS, bool FWD>
__global__ __launch_bounds__(TPB) void k_colour_sweep(int n, int cnt, const int* __restrict__ rows,
                                                      const unsigned long long* __restrict__ slots, const int* __restrict__ counts,
                                                      const int* __restrict__ col, const double* __restrict__ fval,
                                                      const double* __restrict__ dinv, double* z) {
  constexpr int BB = BS * BS;
  const int t = blockIdx.x * TPB + threadIdx.x;
  if (t >= cnt) return;
  const int i = rows[t];
  const unsigned long long sl = slots[i];
  const int ct = counts[i], nl = colour_nlower(ct), nu = colour_nupper(ct);
  double acc[BS];
#pragma unroll
  for (int r = 0; r < BS; r++) acc[r] = z[(size_t)i * BS + r];
  const int p0 = FWD ? 0 : nl, p1 = FWD ? nl : nl + nu;
  for (int p = p0; p < p1; p++) {
    const int q = colour_slot(sl, p);
    const int k = col[(size_t)q * n + i];
    double m[BB], zk[BS];
#pragma unroll
    for (int e = 0; e < BB; e++) m[e] = fval[vix<BS>(n, q, e, i)];
#pragma unroll
    for (int c = 0; c < BS; c++) zk[c] = z[(size_t)k * BS + c];
#pragma unroll
    for (int r = 0; r < BS; r++)
#pragma unroll
      for (int c = 0; c < BS; c++) acc[r] -= m[r * BS + c] * zk[c];
  }
  if constexpr (FWD) {
#pragma unroll
    for (int r = 0; r < BS; r++) z[(size_t)i * BS + r] = acc[r];
  } else {
    double d[BB];
#pragma unroll
    for (int e = 0; e < BB; e++) d[e] = dinv[dix<BS>(n, e, i)];
#pragma unroll
    for (int r = 0; r < BS; r++) {
      double o = 0.0;
#pragma unroll
      for (int c = 0; c < BS; c++) o += d[r * BS + c] * acc[c];
      z[(size_t)i * BS + r] = o;
    }
  }
}

int launch_colour_factor(wai_ctx* c, const Bcsr& J, const ColourSchedule& k, IluSchedule& s) {
  if (J.dg) { c->err = "launch_colour_factor: the coupled tracer system keeps the natural order"; return -1; }
  return with_bs(J.bs, [&](auto bs) {
    constexpr int BS = decltype(bs)::value;
    // the factor starts as a copy of the matrix; colour 0 has nothing to eliminate and inverts its pivots
    hipMemcpyAsync(s.fval, J.val, sizeof(double) * ell_size(J.bs, J.n, J.W), hipMemcpyDeviceToDevice, c->stream);
    for (int col = 0; col < k.max_colours; col++) {
      const int a = k.col_ptr[col], cnt = k.col_ptr[col + 1] - a;
      if (cnt <= 0) continue;
      hipLaunchKernelGGL(k_colour_factor<BS>, (cnt + TPB - 1) / TPB, TPB, 0, c->stream, J.n, cnt, k.rows + a, k.slots, k.counts, J.col, s.fval,
                         s.dinv, c->d_flags);
    }
  });
}

// forward over colours 1 .. C - 1 (colour 0 has no lower coupling), backward over C - 1 .. 0: 2 C - 1 launches
int launch_colour_solve(wai_ctx* c, const Bcsr& J, const ColourSchedule& k, const IluSchedule& s, double* z) {
  if (J.dg) { c->err = "launch_colour_solve: the coupled tracer system keeps the natural order"; return -1; }
  return with_bs(J.bs, [&](auto bs) {
    constexpr int BS = decltype(bs)::value;
    auto sweep = [&](auto fwd, int col) {
      const int a = k.col_ptr[col], cnt = k.col_ptr[col + 1] - a;
      hipLaunchKernelGGL((k_colour_sweep<BS, decltype(fwd)::value>), (cnt + TPB - 1) / TPB, TPB, 0, c->stream, J.n, cnt, k.rows + a, k.slots,
                         k.counts, J.col, s.fval, s.dinv, z);
      c->ks.n_launch++;
    };
    for (int col = 1; col < k.max_colours; col++) sweep(std::true_type{}, col);
    for (int col = k.max_colours - 1; col >= 0; col--) sweep(std::false_type{}, col);
  });
}

// z_b = inv(A_b) r_b: one workgroup per block, one wave per output row at a time (coalesced row reads)
__global__ __launch_bounds__(256) void k_lu_apply(int nsub, int bs, const int* __restrict__ sub_ptr,
                                                  const size_t* __restrict__ inv_ptr, const double* __restrict__ inv,
                                                  const double* __restrict__ r, double* __restrict__ z) {
  const int s = blockIdx.x;
  if (s >= nsub) return;
  const int lo = sub_ptr[s] * bs, m = (sub_ptr[s + 1] - sub_ptr[s]) * bs;
  const double* A = inv + inv_ptr[s];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int i = w; i < m; i += nw) {
    double t = 0.0;
    for (int j = lane; j < m; j += 64) t += A[(size_t)i * m + j] * r[lo + j];
    t = wave_sum(t);
    if (lane == 0) z[lo + i] = t;
  }
}
int launch_lu_apply(wai_ctx* c, int bs, const double* r, double* z) {
  hipLaunchKernelGGL(k_lu_apply, c->ilu.nsub, 256, 0, c->stream, c->ilu.nsub, bs, c->ilu.sub_ptr, c->lu.inv_ptr,
                     c->lu.inv, r, z);
  return 0;
}

template <int BS>
static void ilu_factor_bs(wai_ctx* c, const Bcsr& J, IluSchedule& s) {
  if (s.sublu) {
    // sub-preconditioner lu: the complete factor of every block, one workgroup per block (pc_lu.hip.h)
    hipMemcpyAsync(s.fval, J.val, sizeof(double) * ell_size(J.bs, J.n, J.W), hipMemcpyDeviceToDevice, c->stream);
    const size_t lds = (size_t)J.W * (BS * BS * sizeof(double) + sizeof(int));
    hipLaunchKernelGGL(k_sublu_factor<BS>, s.nsub, SUBLU_FACTOR_THREADS, lds, c->stream, J.n, s.nsub, J.W, s.sub_ptr, s.row_info, J.col,
                       s.fval, s.dinv, c->d_flags);
    return;
  }
  if (s.big) {
    // one launch per forward level; the factor starts as a copy of the matrix
    hipMemcpyAsync(s.fval, J.val, sizeof(double) * ell_size(J.bs, J.n, J.W), hipMemcpyDeviceToDevice, c->stream);
    for (int lev = 0; lev < s.nlev_f; lev++) {
      const int a = s.lev_f_ptr[lev], cnt = s.lev_f_ptr[lev + 1] - a, g = (cnt + TPB - 1) / TPB;
      if (cnt <= 0) continue;
      hipLaunchKernelGGL(k_lvl_factor<BS>, g, TPB, 0, c->stream, J.n, cnt, s.ord_f + a, s.row_info, J.col, s.fval, s.dinv, c->d_flags);
    }
    return;
  }
  const int grid = ((s.nsub + 7) / 8) * 8, T = pc_threads(s);
  if (s.diag_only && s.scaled) {
    // pivots only, then the scaled rows (below): the general factor is never read in this case
    const size_t lds = (size_t)T * J.bs * J.bs * sizeof(double);
    auto pivots = [&](auto pre) {
      hipLaunchKernelGGL((k_dilu_pivots<BS, decltype(pre)::value>), grid, T, lds, c->stream, J.n, s.nsub, s.sub_ptr, s.sub_nlev,
                         s.row_info, J.col, J.val, s.dinv, c->d_flags);
    };
    if constexpr (BS <= 2) with_flag(s.fast3, pivots);
    else if constexpr (BS == 3) {
      // couplings' blocks staged in LDS when a brick's fit 64 KB (<= 130 rows with 3 lower couplings); 4 x 4
      // blocks stay on the general kernel (the staged one compiles to 256 VGPRs + scratch there: not measured)
      auto staged = [&](auto npl, auto raik, size_t lds_s) {
        hipLaunchKernelGGL((k_dilu_pivots_lds<3, decltype(npl)::value, decltype(raik)::value>), grid, T, lds_s, c->stream, J.n, s.nsub,
                           s.max_rows, s.sub_ptr, s.sub_nlev, s.row_info, s.row_tslot, J.col, J.val, s.dinv, c->d_flags);
      };
      const int npl = s.max_nl <= 3 ? 3 : 4;
      const size_t lds2 = (size_t)(1 + 2 * npl) * 9 * s.max_rows * sizeof(double);
      const std::integral_constant<int, 3> three;
      if (npl == 3 && T <= 64)   // one wave per brick: A_ik in registers
        staged(three, std::true_type{}, (size_t)(1 + npl) * 9 * s.max_rows * sizeof(double));
      else if (s.max_nl <= 4 && lds2 <= 64 * 1024 && T <= 256) {
        if (npl == 3) staged(three, std::false_type{}, lds2);
        else staged(std::integral_constant<int, 4>{}, std::false_type{}, lds2);
      } else
        pivots(std::false_type{});
    } else
      pivots(std::false_type{});
    // fval is not read in the diagonal-only case: it holds inv(P) A from here on
    hipLaunchKernelGGL(k_scale_rows<BS>, (J.n + TPB - 1) / TPB, TPB, 0, c->stream, J.n, J.W, J.val, s.dinv, s.fval);
    return;
  }
  hipMemcpyAsync(s.fval, J.val, sizeof(double) * ell_size(J.bs, J.n, J.W), hipMemcpyDeviceToDevice, c->stream);
  if (s.wide)
    hipLaunchKernelGGL(k_ilu_factor_wide<BS>, grid, T, 0, c->stream, J.n, s.nsub, s.sub_ptr, s.sub_nlev, s.row_infow, J.col, s.fval, s.dinv, c->d_flags);
  else
    hipLaunchKernelGGL(k_ilu_factor<BS>, grid, T, 0, c->stream, J.n, s.nsub, s.sub_ptr, s.sub_nlev, s.row_info, J.col, s.fval, s.dinv, c->d_flags);
}
int launch_ilu_factor_on(wai_ctx* c, const Bcsr& J, IluSchedule& s) {
  if (J.dg) return launch_dg_factor(c, J, s);   // the coupled tracer system: its own factor buffer
  return with_bs(J.bs, [&](auto bs) { ilu_factor_bs<decltype(bs)::value>(c, J, s); });
}

// the rows of each level of one sweep, a launch per level (FWD: forward)
template <int BS, bool FWD>
static void lvl_sweep(wai_ctx* c, const Bcsr& J, const IluSchedule& s, const int* ord, const std::vector<int>& ptr, int nlev, double* z) {
  for (int lev = 0; lev < nlev; lev++) {
    const int a = ptr[lev], cnt = ptr[lev + 1] - a, g = (cnt + TPB - 1) / TPB;
    if (cnt <= 0) continue;
    hipLaunchKernelGGL((k_lvl_solve<BS, FWD>), g, TPB, 0, c->stream, J.n, cnt, ord + a, s.row_info, J.col, s.fval, s.dinv, z);
    c->ks.n_launch++;
  }
}
// the tiles of each tile level of one sweep, a launch per tile level: one workgroup per tile, a thread per row of the largest
template <int BS, bool FWD>
static void tile_sweep(wai_ctx* c, const Bcsr& J, const IluSchedule& s, double* z) {
  const TileTables& t = s.tiles;
  const std::vector<int>& ptr = FWD ? t.tl_f_ptr : t.tl_b_ptr;
  const int* ord = FWD ? t.ord_f : t.ord_b;
  const int nlev = FWD ? t.ntl_f : t.ntl_b, T = ((t.max_tile_rows + 63) / 64) * 64;
  const size_t lds = (size_t)t.max_tile_rows * BS * sizeof(double);
  for (int lev = 0; lev < nlev; lev++) {
    const int a = ptr[lev], cnt = ptr[lev + 1] - a;
    if (cnt <= 0) continue;
    hipLaunchKernelGGL((k_tile_solve<BS, FWD>), cnt, T, lds, c->stream, J.n, ord + a, t.tile_ptr, t.tile_nin, t.row_lev, s.row_info, J.col,
                       s.fval, s.dinv, z);
    c->ks.n_launch++;
  }
}
// sub-preconditioner lu: both substitutions of every block in one launch, in place on z.  The block's part of the vector
// rides in LDS where the largest block's fits the 64 KB a workgroup gets without asking for more
bool sublu_vector_in_lds(const IluSchedule& s, int bs) { return (size_t)s.max_rows * bs * sizeof(double) <= 64 * 1024; }
int launch_sublu_solve(wai_ctx* c, const Bcsr& J, const IluSchedule& s, double* z) {
  if (J.dg || !s.sublu) { c->err = "launch_sublu_solve: not a sub-preconditioner lu schedule"; return -1; }
  return with_bs(J.bs, [&](auto bs) {
    constexpr int BS = decltype(bs)::value;
    const size_t lds = sublu_vector_in_lds(s, BS) ? (size_t)s.max_rows * BS * sizeof(double) : 0;
    with_flag(lds > 0, [&](auto in_lds) {
      hipLaunchKernelGGL((k_sublu_solve<BS, decltype(in_lds)::value>), s.nsub, 64 * SUBLU_SOLVE_WAVES, lds, c->stream, J.n, s.nsub, s.sub_ptr,
                         s.row_info, J.col, s.fval, s.dinv, z);
    });
  });
}

int launch_big_solve(wai_ctx* c, const Bcsr& J, const IluSchedule& s, double* z) {
  if (J.dg) return launch_dg_big_solve(c, J, s, z);
  return with_bs(J.bs, [&](auto bs) {
    constexpr int BS = decltype(bs)::value;
    if (s.tiles.serve && !s.sublu) {   // tiles set and fewer tile levels than row levels: a launch per tile level
      tile_sweep<BS, true>(c, J, s, z);
      tile_sweep<BS, false>(c, J, s, z);
      return;
    }
    lvl_sweep<BS, true>(c, J, s, s.ord_f, s.lev_f_ptr, s.nlev_f, z);   // level-0 rows of the forward sweep have nothing to subtract, but the launch is harmless
    lvl_sweep<BS, false>(c, J, s, s.ord_b, s.lev_b_ptr, s.nlev_b, z);
  });
}

}  // namespace wai

// The coarse level of the two-level preconditioner (wai_set_pc_coarse; coarse_space.hpp makes every list on the host): the
// Galerkin matrix Ac = P^T A P as a dense m x m matrix (m = nc * bs <= 1024), its explicit inverse by Gauss-Jordan
// elimination with partial pivoting, and the three launches of an application -- rc = P^T r, yc = Ac^-1 rc, z += P yc -- with
// their launchers.  Plain fp64; every sum is taken in an order fixed by the lists and the launch shape, no floating-point
// atomics: the same values give the same bits.
#include "linalg_device.hip.h"

namespace wai {

constexpr int COARSE_TPB = 256;          // one workgroup per coarse block / aggregate / four rows of Ac^-1
constexpr int COARSE_WAVES = COARSE_TPB / 64;

// the workgroup's sum of v, in thread 0: every wave's sum (wave_sum: fixed order), then the four of them in wave order
__device__ __forceinline__ double coarse_block_sum(double v, double* sh) {
  v = wave_sum(v);
  __syncthreads();   // (sh's readers of the sum before are done)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = sh[0];
#pragma unroll
  for (int w = 1; w < COARSE_WAVES; w++) t += sh[w];
  return t;
}

// Block b = (blk_row[b], blk_col[b]) of Ac: the sum of the fine blocks (ent_row, ent_slot) of list b.  Thread t takes the
// list's entries t, t + 256, ... in list order, then the workgroup's sum; Ac was zeroed before (the blocks outside the
// coarse pattern)
template <int BS>
__global__ __launch_bounds__(COARSE_TPB) void k_coarse_galerkin(int n, int nblk, int m, const int* __restrict__ blk_row,
                                                                const int* __restrict__ blk_col, const int* __restrict__ ent_ptr,
                                                                const int* __restrict__ ent_row, const int* __restrict__ ent_slot,
                                                                const double* __restrict__ val, double* __restrict__ Ac) {
  constexpr int BB = BS * BS;
  __shared__ double sh[COARSE_WAVES];
  const int b = blockIdx.x;
  if (b >= nblk) return;
  double acc[BB];
#pragma unroll
  for (int z = 0; z < BB; z++) acc[z] = 0.0;
  const int hi = ent_ptr[b + 1];
  for (int e = ent_ptr[b] + (int)threadIdx.x; e < hi; e += COARSE_TPB) {
    const int i = ent_row[e], s = ent_slot[e];
#pragma unroll
    for (int z = 0; z < BB; z++) acc[z] += val[vix<BS>(n, s, z, i)];
  }
  const size_t r0 = (size_t)blk_row[b] * BS, c0 = (size_t)blk_col[b] * BS;
#pragma unroll
  for (int z = 0; z < BB; z++) {
    const double t = coarse_block_sum(acc[z], sh);
    if (threadIdx.x == 0) Ac[(r0 + z / BS) * m + c0 + z % BS] = t;
  }
}

// rc[I] = the sum of r's blocks over aggregate I's rows: thread t takes rows t, t + 256, ... of the list, then the workgroup's sum
template <int BS>
__global__ __launch_bounds__(COARSE_TPB) void k_coarse_restrict(int nc, const int* __restrict__ agg_ptr, const int* __restrict__ agg_rows,
                                                                const double* __restrict__ r, double* __restrict__ rc) {
  __shared__ double sh[COARSE_WAVES];
  const int I = blockIdx.x;
  if (I >= nc) return;
  double acc[BS];
#pragma unroll
  for (int k = 0; k < BS; k++) acc[k] = 0.0;
  const int hi = agg_ptr[I + 1];
  for (int p = agg_ptr[I] + (int)threadIdx.x; p < hi; p += COARSE_TPB) {
    const size_t i = (size_t)agg_rows[p] * BS;
#pragma unroll
    for (int k = 0; k < BS; k++) acc[k] += r[i + k];
  }
#pragma unroll
  for (int k = 0; k < BS; k++) {
    const double t = coarse_block_sum(acc[k], sh);
    if (threadIdx.x == 0) rc[(size_t)I * BS + k] = t;
  }
}

// yc = Ainv rc: one wave per row, four rows per workgroup, m / 4 workgroups stream the matrix; lane l takes columns l, l + 64, ...
__global__ __launch_bounds__(COARSE_TPB) void k_coarse_gemv(int m, const double* __restrict__ Ainv, const double* __restrict__ rc,
                                                            double* __restrict__ yc) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * COARSE_WAVES + (threadIdx.x >> 6);
  if (i >= m) return;   // (the whole wave)
  double t = 0.0;
  for (int j = lane; j < m; j += 64) t += Ainv[(size_t)i * m + j] * rc[j];
  t = wave_sum(t);
  if (lane == 0) yc[i] = t;
}

// z_i += yc[agg[i]] (ADD) or z_i = yc[agg[i]], every component by its own constant; n = owned cells
template <bool ADD>
__global__ __launch_bounds__(COARSE_TPB) void k_coarse_prolong(int n, int bs, const int* __restrict__ agg, const double* __restrict__ yc,
                                                               double* __restrict__ z) {
  const size_t idx = (size_t)blockIdx.x * COARSE_TPB + threadIdx.x;
  if (idx >= (size_t)n * bs) return;
  const int i = (int)(idx / bs), k = (int)(idx % bs);
  const double v = yc[(size_t)agg[i] * bs + k];
  z[idx] = ADD ? z[idx] + v : v;
}

// ---- the inverse: in-place Gauss-Jordan with partial pivoting, two launches per column ------------------------------------
// Step k, first launch (ONE workgroup of 1024 threads, thread t for row t and for column t): the pivot row p is the row >= k
// with the largest |W[.][k]| (the smallest such row on a tie); rows k and p change places; the pivot row, scaled, goes to
// prow (its entry k: 1 / pivot) and to row k of W; column k of the other rows goes to pcol.  A pivot of exactly zero raises
// flags[0], as a singular ILU pivot does.
__global__ __launch_bounds__(1024) void k_coarse_pivot(int m, int k, double* __restrict__ W, double* __restrict__ prow,
                                                       double* __restrict__ pcol, int* __restrict__ perm, int* flags) {
  __shared__ double sv[1024];
  __shared__ int si[1024];
  const int t = threadIdx.x;
  double colk = 0.0;
  if (t < m) colk = W[(size_t)t * m + k];
  sv[t] = (t < m && t >= k) ? fabs(colk) : -1.0;
  si[t] = t;
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if (t < off) {
      const double a = sv[t], b = sv[t + off];
      if (b > a || (b == a && si[t + off] < si[t])) { sv[t] = b; si[t] = si[t + off]; }
    }
    __syncthreads();
  }
  const int p = si[0];
  if (t == 0) {
    perm[k] = p;
    if (!(sv[0] > 0.0)) atomicMax(&flags[0], 1);
  }
  double a = 0.0, b = 0.0, piv = 1.0, akk = 0.0;
  if (t < m) {
    a = W[(size_t)k * m + t];     // row k and row p at column t, as they stand
    b = W[(size_t)p * m + t];
    piv = W[(size_t)p * m + k];
    akk = W[(size_t)k * m + k];
  }
  __syncthreads();   // everything above is read before a row is written
  if (t < m) {
    const double s = (t == k ? 1.0 : b) / piv;
    prow[t] = s;
    W[(size_t)k * m + t] = s;
    if (p != k) W[(size_t)p * m + t] = a;
    pcol[t] = t == k ? 0.0 : (t == p ? akk : colk);
  }
}
// second launch: W[i][j] = (j == k ? 0 : W[i][j]) - pcol[i] * prow[j] for every row i != k
__global__ __launch_bounds__(COARSE_TPB) void k_coarse_eliminate(int m, int k, double* __restrict__ W, const double* __restrict__ prow,
                                                                 const double* __restrict__ pcol) {
  const int i = blockIdx.y;
  const int j = blockIdx.x * COARSE_TPB + threadIdx.x;
  if (i >= m || j >= m || i == k) return;
  const double f = pcol[i];
  const size_t at = (size_t)i * m + j;
  const double w = j == k ? 0.0 : W[at];
  W[at] = w - f * prow[j];
}
// W = (P Ac)^-1 with P the row exchanges in order, so Ac^-1 = W P: W's columns exchanged in reverse order.  src[j]: the
// column of W that column j of Ac^-1 is (one thread composes the exchanges), then a gather
__global__ void k_coarse_perm(int m, const int* __restrict__ perm, int* __restrict__ src) {
  if (blockIdx.x || threadIdx.x) return;
  for (int j = 0; j < m; j++) src[j] = j;
  for (int k = m - 1; k >= 0; k--) {
    const int p = perm[k];
    const int s = src[k]; src[k] = src[p]; src[p] = s;
  }
}
__global__ __launch_bounds__(COARSE_TPB) void k_coarse_gather(int m, const double* __restrict__ W, const int* __restrict__ src,
                                                              double* __restrict__ Ainv) {
  const int i = blockIdx.y;
  const int j = blockIdx.x * COARSE_TPB + threadIdx.x;
  if (i >= m || j >= m) return;
  Ainv[(size_t)i * m + j] = W[(size_t)i * m + src[j]];
}

// ---- launchers -------------------------------------------------------------------------------------------------------
int launch_coarse_galerkin(wai_ctx* c, const Bcsr& A, CoarseLevel& k) {
  const size_t mm = (size_t)k.m * k.m;
  HIPCHK(c, hipMemsetAsync(k.Ac, 0, mm * sizeof(double), c->stream));
  const int e = with_bs(A.bs, [&](auto bs) {
    constexpr int BS = decltype(bs)::value;
    hipLaunchKernelGGL(k_coarse_galerkin<BS>, k.nblk, COARSE_TPB, 0, c->stream, A.n, k.nblk, k.m, k.blk_row, k.blk_col, k.ent_ptr,
                       k.ent_row, k.ent_slot, A.val, k.Ac);
  });
  if (e) { c->err = "coarse level: block size"; return -1; }
  return 0;
}

int launch_coarse_invert(wai_ctx* c, CoarseLevel& k) {
  const int m = k.m;
  const size_t mm = (size_t)m * m;
  HIPCHK(c, hipMemcpyAsync(k.W, k.Ac, mm * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  const dim3 grid((m + COARSE_TPB - 1) / COARSE_TPB, m);
  for (int s = 0; s < m; s++) {
    hipLaunchKernelGGL(k_coarse_pivot, 1, 1024, 0, c->stream, m, s, k.W, k.prow, k.pcol, k.perm, c->d_flags);
    hipLaunchKernelGGL(k_coarse_eliminate, grid, COARSE_TPB, 0, c->stream, m, s, k.W, k.prow, k.pcol);
  }
  hipLaunchKernelGGL(k_coarse_perm, 1, 1, 0, c->stream, m, k.perm, k.src);
  hipLaunchKernelGGL(k_coarse_gather, grid, COARSE_TPB, 0, c->stream, m, k.W, k.src, k.Ainv);
  return 0;
}

int launch_coarse_restrict(wai_ctx* c, const CoarseLevel& k, const double* r, double* rc) {
  const int e = with_bs(k.h.bs, [&](auto bs) {
    hipLaunchKernelGGL(k_coarse_restrict<decltype(bs)::value>, k.h.nc, COARSE_TPB, 0, c->stream, k.h.nc, k.agg_ptr, k.agg_rows, r, rc);
  });
  if (e) { c->err = "coarse level: block size"; return -1; }
  c->ks.n_launch++;
  return 0;
}
int launch_coarse_gemv(wai_ctx* c, const CoarseLevel& k, const double* rc, double* yc) {
  hipLaunchKernelGGL(k_coarse_gemv, (k.m + COARSE_WAVES - 1) / COARSE_WAVES, COARSE_TPB, 0, c->stream, k.m, k.Ainv, rc, yc);
  c->ks.n_launch++;
  return 0;
}
int launch_coarse_prolong(wai_ctx* c, const CoarseLevel& k, const double* yc, double* z, bool add) {
  const size_t tot = (size_t)k.h.n * k.h.bs;
  const int grid = (int)((tot + COARSE_TPB - 1) / COARSE_TPB);
  with_flag(add, [&](auto a) {
    hipLaunchKernelGGL(k_coarse_prolong<decltype(a)::value>, grid, COARSE_TPB, 0, c->stream, k.h.n, k.h.bs, k.agg, yc, z);
  });
  c->ks.n_launch++;
  return 0;
}

}  // namespace wai

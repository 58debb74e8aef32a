// K9: the vector kernels of BiCGStab and GMRES, their reductions' kernels and the halo pack.
#pragma once
#include "reductions.hip.h"

namespace wai {

// ---- K9: fused vector kernels -----------------------------------------------------------------

__global__ __launch_bounds__(TPB) void k_dot(const double* __restrict__ a, const double* __restrict__ b,
                                             int n, double* partials, int nb_max, int slot) {
  double v[1] = {0.0};
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) v[0] += a[i] * b[i];
  const int slots[1] = {slot};
  block_reduce_store<1>(v, partials, nb_max, slots);
}

// sum the per-block partials of up to 4 reduction slots into scal[...], then derive
__global__ __launch_bounds__(1024) void k_finalize(const double* __restrict__ partials, int nb_max, int nb,
                                                   int slot0, int nslots, double* scal, int phase) {
  sum_partials(partials, nb_max, nb, slot0, nslots, scal, false);   // consumed slots are left empty (FIN_EMPTY)
  if (threadIdx.x == 0 && phase >= 0) derive_scalars(scal, phase);
}

// every partial slot of [slot0, slot0 + nslots) empty: before a solve, whatever an aborted one left
__global__ __launch_bounds__(TPB) void k_partials_clear(double* partials, double* partials2, int nb_max, int slot0, int nslots) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i < (size_t)nslots * nb_max) reinterpret_cast<unsigned long long*>(partials)[(size_t)slot0 * nb_max + i] = FIN_EMPTY;
  if (i < (size_t)nslots * FIN_MAXF) reinterpret_cast<unsigned long long*>(partials2)[(size_t)slot0 * FIN_MAXF + i] = FIN_EMPTY;
}

__global__ void k_bcgs_scalars(double* s, int phase, double* post, int seq) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    derive_scalars(s, phase);
    if (seq > 0) post_scalars(s, post, seq);
  }
}

// streaming vector accesses of the BiCGStab updates: every element is touched once per launch
__device__ __forceinline__ double ldv(const double* p) {
  return __builtin_nontemporal_load(p);
}
__device__ __forceinline__ void stv(double* p, double v) {
  __builtin_nontemporal_store(v, p);
}
// P = R + beta*(P - omega_old*V)   [VecAXPBYPCZ(P, 1, -omega*beta, beta, R, V)]
__global__ __launch_bounds__(TPB) void k_bcgs_p(double* __restrict__ P, const double* __restrict__ R,
                                                const double* __restrict__ V, int n,
                                                const double* __restrict__ s) {
  const double beta = s[S_BETA], ob = -s[S_OMEGA] * beta;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB)
    stv(P + i, __builtin_fma(beta, ldv(P + i), __builtin_fma(ob, ldv(V + i), ldv(R + i))));

}
// S = R - alpha V
__global__ __launch_bounds__(TPB) void k_bcgs_s(double* __restrict__ S, const double* __restrict__ R,
                                                const double* __restrict__ V, int n,
                                                const double* __restrict__ s) {
  const double nalpha = -s[S_ALPHA];
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) stv(S + i, __builtin_fma(nalpha, ldv(V + i), ldv(R + i)));
}
// X += alpha P + omega S ; R = S - omega T ; partial (R,R) and (R,RP) unless the caller already has
// them from the merged reductions (DOTS = false)
template <bool DOTS>
__global__ __launch_bounds__(TPB) void k_bcgs_xr(double* __restrict__ X, double* __restrict__ R,
                                                 const double* __restrict__ P, const double* __restrict__ S,
                                                 const double* __restrict__ T, const double* __restrict__ RP,
                                                 int n, const double* __restrict__ s, double* partials,
                                                 int nb_max, Fin fin) {
  if (fin_block(fin, partials, nb_max)) return;
  const int nblk = fin.count > 0 ? gridDim.x - fin.nf : gridDim.x;   // the finalisers are extra workgroups
  const double alpha = s[S_ALPHA], omega = s[S_OMEGA];
  double v[2] = {0.0, 0.0};
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += nblk * TPB) {
    const double si = ldv(S + i);
    stv(X + i, __builtin_fma(omega, si, __builtin_fma(alpha, ldv(P + i), ldv(X + i))));
    const double r = __builtin_fma(-omega, ldv(T + i), si);
    stv(R + i, r);
    if constexpr (DOTS) {
      v[0] += r * r;
      v[1] += r * ldv(RP + i);
    }
  }
  if constexpr (DOTS) {
    const int slots[2] = {S_DP2, S_RHONEW};
    block_reduce_store<2>(v, partials, nb_max, slots);
  }
}

// The iteration's vector work in ONE pass (merged reductions: omega, rho, beta are known before X and R move):
//   S = R - alpha V (re-formed, never stored)   X += alpha P + omega S   R = S - omega T   P = R + beta (P - omega V)
// -- k_bcgs_s, k_bcgs_xr and the next iteration's k_bcgs_p: reads X, P, R, V, T, writes X, R, P (8 vector passes where the
// three kernels make 14), no reduction.  Every expression is the one its separate kernel evaluates: identical bits.
// DERIVE (several ranks, round 5): the five all-reduced products have just arrived and the one-thread scalar kernel that
// used to sit between the all-reduce and this launch is gone.  Every thread forms omega, (R,R), rho, beta itself from the
// sums and the scalars of the iteration (derive_merged + derive_rotate, the same expressions in the same order: same
// bits) and uses its own copies; workgroup 0 stores them -- the rotation overwrites what the others read, so it waits
// until every workgroup of the launch has said that it has read (a counter; the grid is at most 1 024 workgroups, all
// resident) -- and posts the norm to the host.  The wait is bounded; the counter is left at zero for the next launch.
template <bool DERIVE>
__global__ __launch_bounds__(TPB) void k_bcgs_xrp(double* __restrict__ X, double* __restrict__ R, double* __restrict__ P,
                                                  const double* __restrict__ V, const double* __restrict__ T, int n,
                                                  double* s, unsigned* started, double* post, int seq) {
  double alpha, omega, beta;
  if constexpr (DERIVE) {
    double loc[8];
    // a private copy of the scalars derive_scalars' phase 6 reads and writes, the derivation on the copy
    loc[0] = s[S_D1]; loc[1] = s[S_D2]; loc[2] = s[S_DP2]; loc[3] = s[S_RHONEW]; loc[4] = s[S_W2];
    loc[5] = s[S_RHO]; loc[6] = s[S_ALPHA]; loc[7] = s[S_BREAK];
    const double st = loc[0], tt = loc[1], ss = loc[2], srp = loc[3], trp = loc[4];
    double brk = loc[7];
    if (tt == 0.0) { brk = 2.0; omega = 0.0; }
    else omega = st / tt;
    const double rr0 = (ss - 2.0 * omega * st) + omega * omega * tt;
    const double rr = rr0 > 0.0 ? rr0 : 0.0;
    const double rhonew = srp - omega * trp;
    const double rhoold = loc[5];
    alpha = loc[6];
    if (rhonew == 0.0 && brk == 0.0) brk = 3.0;
    beta = (rhonew / rhoold) * (alpha / omega);
    __syncthreads();                       // every thread of the workgroup has its copies
    if (threadIdx.x == 0) {
      __hip_atomic_fetch_add(started, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      if (blockIdx.x == 0) {
        for (int spin = 0; spin < (1 << 24) && __hip_atomic_load(started, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < gridDim.x; spin++)
          __builtin_amdgcn_s_sleep(2);
        // (a workgroup that never reported -- it cannot happen short of a lost launch -- must not pass for a valid rotation:
        // breakdown code 4, the solve ends with KSP_DIVERGED_NANORINF and a message, as for a lost partial sum)
        if (__hip_atomic_load(started, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < gridDim.x) brk = 4.0;
        s[S_OMEGA] = omega; s[S_DP2] = rr; s[S_RHONEW] = rhonew;
        s[S_RHOOLD] = rhoold; s[S_RHO] = rhonew; s[S_BETA] = beta; s[S_BREAK] = brk;
        __threadfence();
        if (seq > 0) post_scalars(s, post, seq);
        __hip_atomic_store(started, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  } else {
    alpha = s[S_ALPHA]; omega = s[S_OMEGA]; beta = s[S_BETA];
  }
  const double nalpha = -alpha, ob = -omega * beta;
  auto one = [&](double x, double r0, double p, double v, double t, double& xo, double& ro, double& po) {
    const double si = __builtin_fma(nalpha, v, r0);
    xo = __builtin_fma(omega, si, __builtin_fma(alpha, p, x));
    ro = __builtin_fma(-omega, t, si);
    po = __builtin_fma(beta, p, __builtin_fma(ob, v, ro));
  };
  // no reduction here, so the lanes are free to take two entries each (16-byte accesses; with a reduction the pairing
  // would change the order of the partial sums and with it the solver's rounding)
  const int n2 = n >> 1;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n2; i += gridDim.x * TPB) {
    const wai_d2 x = __builtin_nontemporal_load(reinterpret_cast<const wai_d2*>(X) + i);
    const wai_d2 r0 = __builtin_nontemporal_load(reinterpret_cast<const wai_d2*>(R) + i);
    const wai_d2 p = __builtin_nontemporal_load(reinterpret_cast<const wai_d2*>(P) + i);
    const wai_d2 v = __builtin_nontemporal_load(reinterpret_cast<const wai_d2*>(V) + i);
    const wai_d2 t = __builtin_nontemporal_load(reinterpret_cast<const wai_d2*>(T) + i);
    wai_d2 xo, ro, po;
    double a, b, c2;
    one(x.x, r0.x, p.x, v.x, t.x, a, b, c2); xo.x = a; ro.x = b; po.x = c2;
    one(x.y, r0.y, p.y, v.y, t.y, a, b, c2); xo.y = a; ro.y = b; po.y = c2;
    __builtin_nontemporal_store(xo, reinterpret_cast<wai_d2*>(X) + i);
    __builtin_nontemporal_store(ro, reinterpret_cast<wai_d2*>(R) + i);
    __builtin_nontemporal_store(po, reinterpret_cast<wai_d2*>(P) + i);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const int i = n - 1;
    double a, b, c2;
    one(X[i], R[i], P[i], V[i], T[i], a, b, c2);
    X[i] = a; R[i] = b; P[i] = c2;
  }
}

// halo pack of a composed vector: sendbuf[p*dof + k] = a[idx*dof + k] - alpha b[idx*dof + k] (the ghost values of
// S = R - alpha V for the fused launch that forms S on the fly; the receiver unpacks them into R's ghost entries and
// keeps V's at zero)
// DERIVE (several ranks, round 5): alpha is not there yet -- the all-reduced (V, rP) has just arrived and the one-thread
// scalar kernel that used to sit between the all-reduce and this launch is gone: every thread forms
// alpha = rho / (V, rP) itself (derive_scalars' phase 2, the same division: same bits) and thread 0 stores it -- with the
// breakdown code of (V, rP) = 0 -- for the launches behind this one, which read S_ALPHA as before.  Nobody reads S_ALPHA
// in this launch, nobody writes S_RHO / S_D1: no hazard.
template <bool DERIVE>
__global__ __launch_bounds__(TPB) void k_pack_axpy(const double* __restrict__ a, const double* __restrict__ b,
                                                   double* s, const int* __restrict__ idx,
                                                   int n, int dof, double* __restrict__ buf) {
  const int t = blockIdx.x * TPB + threadIdx.x;
  double alpha;
  if constexpr (DERIVE) {
    const double d1 = s[S_D1];
    alpha = s[S_RHO] / d1;
    if (t == 0) {
      if (d1 == 0.0) s[S_BREAK] = 1.0;
      s[S_ALPHA] = alpha;
    }
  } else alpha = s[S_ALPHA];
  if (t >= n * dof) return;
  const int p = t / dof, k = t - p * dof;
  const size_t g = (size_t)idx[p] * dof + k;
  buf[t] = __builtin_fma(-alpha, b[g], a[g]);
}

__global__ __launch_bounds__(TPB) void k_waxpy(double* w, double alpha, const double* x, const double* y, int n) {
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) w[i] = alpha * x[i] + y[i];
}

// GMRES: up to 8 dots (w, v_j) per pass.
// Round 6: the classical Gram-Schmidt passes are 3/4 of a GMRES(30) iteration's bytes (on average 16.5 + 17.5 vectors
// beside the operator's 19) and ran at 50-54 % of HBM peak (0.66 ms each per iteration at 216^3, bench_r6a_c3_gmres.json):
// scalar 8-byte loads behind a per-vector `q < cnt` branch.  Now: the vector count is a template argument (straight-line
// code: all of an element pair's CNT + 1 loads are requested together), 16-byte loads (two doubles per lane; 8-byte
// alignment is enough on gfx950, an odd leading dimension is fine), two pairs per trip, basis vectors with the streaming
// hint (each is read once per pass).  A thread's sums run over other elements than before: other rounding, same algorithm.
template <int CNT>
__global__ __launch_bounds__(TPB) void k_mdot(const double* __restrict__ w, const double* __restrict__ basis,
                                              size_t ld, int j0, int n, double* partials, int nb_max) {
  double v[CNT];
#pragma unroll
  for (int q = 0; q < CNT; q++) v[q] = 0.0;
  const size_t n2 = (size_t)n >> 1, stride = (size_t)gridDim.x * TPB;
  const wai_d2u* w2 = reinterpret_cast<const wai_d2u*>(w);
  auto one = [&](size_t i) {
    const wai_d2u wi = w2[i];
    wai_d2u b[CNT];
#pragma unroll
    for (int q = 0; q < CNT; q++) b[q] = __builtin_nontemporal_load(reinterpret_cast<const wai_d2u*>(basis + (size_t)(j0 + q) * ld) + i);
#pragma unroll
    for (int q = 0; q < CNT; q++) { v[q] += wi.x * b[q].x; v[q] += wi.y * b[q].y; }
  };
  size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  for (; i + stride < n2; i += 2 * stride) { one(i); one(i + stride); }
  if (i < n2) one(i);
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < CNT; q++) v[q] += w[n - 1] * basis[(size_t)(j0 + q) * ld + n - 1];
  }
  int slots[CNT];
#pragma unroll
  for (int q = 0; q < CNT; q++) slots[q] = S_H + j0 + q;
  block_reduce_store<CNT>(v, partials, nb_max, slots);
}
// w -= sum_j h_j v_j ; partial |w|^2   (16-byte accesses, the basis vectors eight at a time: straight-line groups)
__global__ __launch_bounds__(TPB) void k_maxpy_norm(double* __restrict__ w, const double* __restrict__ basis,
                                                    size_t ld, int k, int n, const double* __restrict__ s,
                                                    double* partials, int nb_max) {
  double v[1] = {0.0};
  const size_t n2 = (size_t)n >> 1, stride = (size_t)gridDim.x * TPB;
  wai_d2u* w2 = reinterpret_cast<wai_d2u*>(w);
  for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n2; i += stride) {
    wai_d2u wi = w2[i];
    int j = 0;
    for (; j + 8 <= k; j += 8) {
      wai_d2u b[8];
#pragma unroll
      for (int q = 0; q < 8; q++) b[q] = __builtin_nontemporal_load(reinterpret_cast<const wai_d2u*>(basis + (size_t)(j + q) * ld) + i);
#pragma unroll
      for (int q = 0; q < 8; q++) { const double h = s[S_H + j + q]; wi.x -= h * b[q].x; wi.y -= h * b[q].y; }
    }
    for (; j < k; j++) {
      const wai_d2u b = __builtin_nontemporal_load(reinterpret_cast<const wai_d2u*>(basis + (size_t)j * ld) + i);
      const double h = s[S_H + j];
      wi.x -= h * b.x; wi.y -= h * b.y;
    }
    w2[i] = wi;
    v[0] += wi.x * wi.x; v[0] += wi.y * wi.y;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    double wi = w[n - 1];
    for (int j = 0; j < k; j++) wi -= s[S_H + j] * basis[(size_t)j * ld + n - 1];
    w[n - 1] = wi;
    v[0] += wi * wi;
  }
  const int slots[1] = {S_W2};
  block_reduce_store<1>(v, partials, nb_max, slots);
}
__global__ __launch_bounds__(TPB) void k_scale_to(double* dst, const double* src, const double* __restrict__ s,
                                                  int slot, int n) {
  const double inv = 1.0 / sqrt(s[slot]);
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) dst[i] = src[i] * inv;
}
__global__ __launch_bounds__(TPB) void k_update_x(double* __restrict__ x, const double* __restrict__ basis,
                                                  size_t ld, int k, int n, const double* __restrict__ coef) {
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
    double xi = x[i];
    for (int j = 0; j < k; j++) xi += coef[j] * basis[(size_t)j * ld + i];
    x[i] = xi;
  }
}

// halo pack: sendbuf[p*dof + k] = vec[send_idx[p]*dof + k]
__global__ __launch_bounds__(TPB) void k_pack(const double* __restrict__ vec, const int* __restrict__ idx,
                                              int n, int dof, double* __restrict__ buf) {
  const int t = blockIdx.x * TPB + threadIdx.x;
  if (t >= n * dof) return;
  const int p = t / dof, k = t - p * dof;
  buf[t] = vec[(size_t)idx[p] * dof + k];
}

__global__ __launch_bounds__(TPB) void k_dots(const double* __restrict__ a1, const double* __restrict__ b1, int slot1,
                                              const double* __restrict__ a2, const double* __restrict__ b2, int slot2,
                                              int n, double* partials, int nb_max) {
  double v[2] = {0.0, 0.0};
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
    v[0] += a1[i] * b1[i];
    if (a2) v[1] += a2[i] * b2[i];
  }
  const int slots[2] = {slot1, a2 ? slot2 : slot1};
  if (a2) block_reduce_store<2>(v, partials, nb_max, slots);
  else { double v1[1] = {v[0]}; const int s1[1] = {slot1}; block_reduce_store<1>(v1, partials, nb_max, s1); }
}

}  // namespace wai

// In-launch reductions: partial sums and their finaliser workgroups, the BiCGStab scalar derivations, the start-up
// cohorts, and the inner products all five fused kernels share (pc_row_dots, pc_reduce_dots).
// ONE translation unit includes this header (kernels_fused.hip): store_partial reads the device global g_drop_partials,
// which test_drop_partials sets, and without relocatable device code every including unit would get a copy of its own.
#pragma once
#include "linalg_device.hip.h"

namespace wai {

// ---- reductions finished inside the producing kernel ---------------------------------------------
// What the host tests after an iteration -- the squared residual norm and the breakdown code -- written straight
// into pinned host memory: {(R,R), 8 * sequence number + code, check} with check = bits((R,R)) ^ bits(tag) ^ POST_KEY.
// The first two words leave as ONE aligned 16-byte store (one PCIe write on gfx942 / gfx950), the check word behind
// them; the host (wait_post, krylov.hip) spins on the tag and accepts the pair only when the check word matches, so a
// store that the fabric tears, or words that arrive in another order, can only delay the host, never pair a new
// sequence number with an old norm.  Codes: 0 none, 1-3 BiCGStab breakdowns (derive_scalars), 4 a partial sum of a
// reduction never arrived (sum_partials).
typedef unsigned wai_u4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void post_scalars(const double* scal, double* post, int seq) {
  const double v0 = scal[S_DP2], v1 = 8.0 * (double)seq + scal[S_BREAK];
  const unsigned long long chk = (unsigned long long)__double_as_longlong(v0) ^ (unsigned long long)__double_as_longlong(v1) ^ POST_KEY;
#if defined(__gfx942__) || defined(__gfx950__)
  wai_u4 w;
  w.x = (unsigned)__double2loint(v0); w.y = (unsigned)__double2hiint(v0);
  w.z = (unsigned)__double2loint(v1); w.w = (unsigned)__double2hiint(v1);
  asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" : : "v"(post), "v"(w) : "memory");
#else
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(post), (unsigned long long)__double_as_longlong(v0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(post) + 1, (unsigned long long)__double_as_longlong(v1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#endif
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(post) + 2, chk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// merged reductions (multi-rank): slots hold (S,T), (T,T), (S,S), (S,RP), (T,RP).  omega = (S,T)/(T,T) (see
// phase 3 for (T,T) = 0); then, with R = S - omega T:  (R,RP) = (S,RP) - omega (T,RP)  and
// (R,R) = (S,S) - 2 omega (S,T) + omega^2 (T,T) -- one all-reduce instead of two
__device__ __forceinline__ void derive_merged(double* s) {
  const double st = s[S_D1], tt = s[S_D2], ss = s[S_DP2], srp = s[S_RHONEW], trp = s[S_W2];
  if (tt == 0.0) { s[S_BREAK] = 2.0; s[S_OMEGA] = 0.0; }
  else s[S_OMEGA] = st / tt;
  const double om = s[S_OMEGA];
  const double rr = (ss - 2.0 * om * st) + om * om * tt;
  s[S_DP2] = rr > 0.0 ? rr : 0.0;
  s[S_RHONEW] = srp - om * trp;
}
// end of iteration: rotate rho, next beta = (rho/rhoold)*(alpha/omega)
__device__ __forceinline__ void derive_rotate(double* s) {
  s[S_RHOOLD] = s[S_RHO]; s[S_RHO] = s[S_RHONEW];
  if (s[S_RHO] == 0.0 && s[S_BREAK] == 0.0) s[S_BREAK] = 3.0;  // only matters if not converged
  s[S_BETA] = (s[S_RHO] / s[S_RHOOLD]) * (s[S_ALPHA] / s[S_OMEGA]);
}
__device__ __forceinline__ void derive_scalars(double* s, int phase) {
  switch (phase) {  // PETSc KSPSolve_BCGS order of operations
    case 0:  // after R = B^-1 b: DP2 = (R,R); rho = (R,RP) with RP = R
      s[S_RHO] = s[S_DP2]; s[S_RHOOLD] = 1.0; s[S_ALPHA] = 1.0; s[S_OMEGA] = 1.0;
      if (s[S_BREAK] != 4.0) s[S_BREAK] = 0.0;   // (4: this very reduction lost a partial sum; the driver zeroes the code before a solve)
      s[S_BETA] = (s[S_RHO] / s[S_RHOOLD]) * (s[S_ALPHA] / s[S_OMEGA]);
      if (s[S_RHO] == 0.0) s[S_BREAK] = 1.0;
      break;
    case 2:  // alpha = rho / (V,RP)
      if (s[S_D1] == 0.0) s[S_BREAK] = 1.0;
      s[S_ALPHA] = s[S_RHO] / s[S_D1];
      break;
    case 3:  // omega = (S,T)/(T,T)
      // (T,T) = 0: KSPSolve_BCGS then tests (S,S) -- zero means the half step already solved the
      // system (exact preconditioner: a single subdomain), x += alpha P and converged; otherwise
      // breakdown.  omega = 0 makes the X/R update do exactly that: X += alpha P, R = S, so the
      // (R,R) it reduces is (S,S) for the host to look at.
      if (s[S_D2] == 0.0) { s[S_BREAK] = 2.0; s[S_OMEGA] = 0.0; }
      else s[S_OMEGA] = s[S_D1] / s[S_D2];
      break;
    case 5: derive_merged(s); break;
    case 6:  // merged reductions, then the end-of-iteration rotation: the X / R update that runs between the
             // two in KSPSolve_BCGS reads alpha and omega only, which the rotation leaves alone
      derive_merged(s);
      derive_rotate(s);
      break;
    case 4: derive_rotate(s); break;
    default: break;
  }
}
// Finalisation inside the producing launch (Fin, context.hpp).  A launch that carries a Fin has a few
// workgroups more than it has work (fin_slices: one per ~1024 partials): the extra ones -- the last indices, dispatched
// after every other -- wait for the partial sums to arrive and sum them; the last one derives the BiCGStab scalars.  The working workgroups do
// nothing beyond storing their partial (agent scope: written through, coherent across the XCDs' L2s).
// Arrival is read off the data: an empty partial slot holds FIN_EMPTY (a NaN payload no sum produces), and
// whoever consumes a partial -- this workgroup or k_finalize -- leaves the slot empty again.
// INVARIANT the launchers keep (launch_pc_on, vec_dots, bcgs_update_xr): every launch that stores partials into a
// slot is followed, before the next producer of that slot, by exactly one consumer -- its own finaliser workgroup
// or a k_finalize launch -- and every Krylov driver empties the slots it uses before its first producer
// (partials_clear), so what an aborted solve or a probe left behind cannot pass for an arrival.  A partial that never
// arrives (bounded wait) or a consumer without a producer gives a NaN sum AND breakdown code 4 (KSP_DIVERGED_NANORINF
// with a message on the host).  WAI_FIN_SEPARATE=1 (run time) takes the finalisation out of the producers again --
// one-block k_finalize launches behind them, as in rounds 1-2 -- for debuggers and serialised dispatch.
// The sums are formed exactly as k_finalize forms them (virtual threads v < VT stride over the partials, a
// 64-lane shuffle tree per virtual wave, the wave sums added in order): the bits do not depend on timing
// and equal what the separate launch gave.
// MEASURED dead ends at 216^3 (k_pc_park, 0.60 ms per launch without any of this): arrival through a
// device-scope fence + counter in every workgroup, 1.435 ms (__threadfence writes back and invalidates the
// XCD's whole L2, 21 168 times: the x gathers lose their reuse); relaxed agent-scope atomics on two-level
// counters, no fence, 0.70 ms (each workgroup holds its CU slot ~2 us longer for the store acknowledgement
// and the returning atomic).
constexpr unsigned long long FIN_EMPTY = 0x7FF4DEADBEEF0001ull;
constexpr int FIN_MAXS = 5;   // reduction slots summed together (the merged BiCGStab reductions: five)
// Several finaliser workgroups (round 4).  ONE workgroup summing all partials is a serial tail that grows with the number
// of bricks: its loads are agent-scope round trips of ~2 us, a few in flight per thread -- MEASURED (bench.py --micro-only,
// fused launch with / without the in-launch finalisation): 0.015 ms of 0.563 at 216^3 (21 168 bricks of 512 rows), but
// 0.127 of 0.690 ms at C4 (78 586 one-wave bricks), 0.047 of 0.233 at C5 -- and with the five merged reductions 0.069,
// 0.537 (!) and 0.198 ms.  So the partials are cut into fin_slices(nb) slices of ~1024 (at most 64 slices), a launch carries that many extra
// workgroups, finaliser f sums slice f of every slot and stores the slice sums (second-level partials, same arrival
// protocol), and the LAST finaliser adds the slice sums in slice order, derives and posts.  k_finalize (the separate
// launch) forms the same slice sums and adds them in the same order: identical bits either way, independent of timing.
constexpr int FIN_SLICE = 1024;
__host__ __device__ __forceinline__ int fin_slices(int nb) { return nb <= FIN_SLICE ? 1 : (nb + FIN_SLICE - 1) / FIN_SLICE > FIN_MAXF ? FIN_MAXF : (nb + FIN_SLICE - 1) / FIN_SLICE; }
__host__ __device__ __forceinline__ void fin_slice_range(int nb, int nf, int f, int& lo, int& hi) {
  const int per = (nb + nf - 1) / nf;
  lo = f * per; hi = lo + per < nb ? lo + per : nb;
  if (lo > nb) lo = nb;
}
// sums of the partials [lo, hi) of ns (<= FIN_MAXS) slots starting at p0 -> res[0 .. ns) (shared memory, valid for every
// thread on return), by a workgroup of any size (multiple of 64).  A virtual thread's partials are fetched two at a time
// FOR ALL SLOTS TOGETHER -- up to 10 independent agent-scope loads in flight (one dependent round trip per entry cost 2 us
// each) -- and added per slot in ascending order; an entry that has not arrived yet is polled (bounded: a partial that
// never arrives becomes a NaN sum and breakdown code 4, KSP_DIVERGED_NANORINF, not a hung device).
__device__ __forceinline__ void sum_slice(unsigned long long* p0, int nb_max, int lo, int hi, int ns, bool wait,
                                          double* scal, double* res) {
  __shared__ __attribute__((aligned(16))) double fsm[FIN_MAXS][16];
  constexpr int CH = 2;
  const int len = hi - lo, VT = len > 256 ? 1024 : 256;
  __syncthreads();   // fsm / res of an earlier call are no longer read
  bool gave_up = false;
  for (int v = threadIdx.x; v < VT; v += blockDim.x) {   // whole waves: blockDim is a multiple of 64
    double t[FIN_MAXS];
#pragma unroll
    for (int s = 0; s < FIN_MAXS; s++) t[s] = 0.0;
    for (int i0 = lo + v; i0 < hi; i0 += VT * CH) {
      unsigned long long u[FIN_MAXS][CH];
#pragma unroll
      for (int s = 0; s < FIN_MAXS; s++)
#pragma unroll
        for (int k = 0; k < CH; k++) {
          const int i = i0 + k * VT;
          u[s][k] = (s < ns && i < hi) ? __hip_atomic_load(p0 + (size_t)s * nb_max + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
        }
      // entries that have not arrived: ALL of them asked for again together, once per round (a brick's five sums arrive
      // together; polled one after the other each cost its own round trip)
      for (int spin = 0; wait && !gave_up && spin < (1 << 22); spin++) {
        bool any = false;
#pragma unroll
        for (int s = 0; s < FIN_MAXS; s++)
#pragma unroll
          for (int k = 0; k < CH; k++) any |= (s < ns && i0 + k * VT < hi && u[s][k] == FIN_EMPTY);
        if (!any) break;
        __builtin_amdgcn_s_sleep(8);
#pragma unroll
        for (int s = 0; s < FIN_MAXS; s++)
#pragma unroll
          for (int k = 0; k < CH; k++) {
            const int i = i0 + k * VT;
            if (s < ns && i < hi && u[s][k] == FIN_EMPTY)
              u[s][k] = __hip_atomic_load(p0 + (size_t)s * nb_max + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
      }
#pragma unroll
      for (int s = 0; s < FIN_MAXS; s++)
#pragma unroll
        for (int k = 0; k < CH; k++) {
          const int i = i0 + k * VT;
          if (s < ns && i < hi) {
            // still empty: the producer never stored it (waited out above: one bounded wait per thread, a launch that lost
            // a partial ends in seconds), or -- k_finalize, wait = false -- no producer ran before this consumer.  The sum
            // is a NaN either way; say why (code 4 reaches the host with the post)
            if (u[s][k] == FIN_EMPTY) {
              // (agent scope, released: the finaliser that posts may be another workgroup on another XCD -- fin_block reads it the same way)
              gave_up = true;
              __hip_atomic_store(&scal[S_BREAK], 4.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            }
            __hip_atomic_store(p0 + (size_t)s * nb_max + i, FIN_EMPTY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // consumed: the slot is empty again
            t[s] += __longlong_as_double((long long)u[s][k]);   // FIN_EMPTY itself is a NaN
          }
        }
    }
#pragma unroll
    for (int s = 0; s < FIN_MAXS; s++) {
      const double ts = wave_sum(t[s]);
      if ((v & 63) == 0) fsm[s][v >> 6] = ts;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < ns) {
    double tot = 0.0;
    for (int w = 0; w < (VT >> 6); w++) tot += fsm[threadIdx.x][w];
    res[threadIdx.x] = tot;
  }
  __syncthreads();
}
// k_finalize's body: every slice of every slot, the slice sums added in slice order -> scal
__device__ __forceinline__ void sum_partials(const double* partials, int nb_max, int nb, int slot0, int nslots,
                                             double* scal, bool wait) {
  __shared__ __attribute__((aligned(16))) double res[8], tot[8];   // static LDS stays a multiple of 16 bytes: the kernels' dynamic arrays behind it take 16-byte accesses
  const int nf = fin_slices(nb);
  for (int sb = 0; sb < nslots; sb += FIN_MAXS) {
    const int ns = min(nslots - sb, FIN_MAXS);
    unsigned long long* p0 = reinterpret_cast<unsigned long long*>(const_cast<double*>(partials)) + (size_t)(slot0 + sb) * nb_max;
    if ((int)threadIdx.x < ns) tot[threadIdx.x] = 0.0;
    for (int f = 0; f < nf; f++) {
      int lo, hi;
      fin_slice_range(nb, nf, f, lo, hi);
      sum_slice(p0, nb_max, lo, hi, ns, wait, scal, res);
      if ((int)threadIdx.x < ns) tot[threadIdx.x] = nf == 1 ? res[threadIdx.x] : tot[threadIdx.x] + res[threadIdx.x];
    }
    if ((int)threadIdx.x < ns) scal[slot0 + sb + threadIdx.x] = tot[threadIdx.x];
    __syncthreads();
  }
}
// A workgroup's partial sum: stored at agent scope (written through to memory, coherent across the XCDs' L2s)
// so that the workgroup that finishes a reduction can read it without any cache-wide fence
// Fault injection for the tests (wai_test_drop_partials): while positive, workgroup 0 of a launch loses its partial sums
// (and counts the variable down) -- the finaliser must then run into its bounded wait, report breakdown code 4, and the
// solver must come back with KSP_DIVERGED_NANORINF instead of hanging or summing stale data.  Several waves of workgroup 0
// store at once: the count taken decides, so that a request of n drops exactly n (a store that lost the race leaves the
// variable below zero, which ends the injection as zero does).
__device__ int g_drop_partials = 0;
__device__ __forceinline__ void store_partial(double* p, double t) {
  if (blockIdx.x == 0 && __hip_atomic_load(&g_drop_partials, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 0 &&
      atomicSub(&g_drop_partials, 1) > 0)
    return;
  __hip_atomic_store(p, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// is this workgroup one of the launch's finalisers (the last f.nf workgroups)?  If so do its share (the caller returns)
__device__ __forceinline__ bool fin_block(const Fin& f, const double* partials, int nb_max) {
  if (f.count == 0 || (int)blockIdx.x < (int)gridDim.x - f.nf) return false;
  __shared__ __attribute__((aligned(16))) double res[8];   // (a multiple of 16 bytes: see sum_partials)
  const int me = (int)blockIdx.x - ((int)gridDim.x - f.nf);
  const bool last = me == f.nf - 1;
  unsigned long long* p0 = reinterpret_cast<unsigned long long*>(const_cast<double*>(partials)) + (size_t)f.slot0 * nb_max;
  unsigned long long* q0 = reinterpret_cast<unsigned long long*>(f.part2) + (size_t)f.slot0 * FIN_MAXF;
  int lo, hi;
  fin_slice_range(f.nb, f.nf, me, lo, hi);
  sum_slice(p0, nb_max, lo, hi, f.nslots, true, f.scal, res);   // nslots <= FIN_MAXS for every in-launch finalisation
  if (f.nf == 1) {
    if ((int)threadIdx.x < f.nslots) f.scal[f.slot0 + threadIdx.x] = res[threadIdx.x];
  } else {
    if ((int)threadIdx.x < f.nslots) store_partial(f.part2 + (size_t)(f.slot0 + threadIdx.x) * FIN_MAXF + me, res[threadIdx.x]);
    if (!last) return true;
    // the last finaliser, its first wave: lane t takes slice t's sums as they arrive (nf <= 64 = FIN_MAXF), every lane
    // then adds them in slice order
    if (threadIdx.x < 64) {
      const int t = (int)threadIdx.x;
      unsigned long long u[FIN_MAXS];
#pragma unroll
      for (int s2 = 0; s2 < FIN_MAXS; s2++)   // the slots' loads in flight together (one after the other they cost a round trip each)
        u[s2] = (s2 < f.nslots && t < f.nf) ? __hip_atomic_load(q0 + (size_t)s2 * FIN_MAXF + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
      for (int spin = 0; spin < (1 << 22); spin++) {   // what has not arrived asked for again, all slots together
        bool any = false;
#pragma unroll
        for (int s2 = 0; s2 < FIN_MAXS; s2++) any |= (s2 < f.nslots && t < f.nf && u[s2] == FIN_EMPTY);
        if (!any) break;
        __builtin_amdgcn_s_sleep(8);
#pragma unroll
        for (int s2 = 0; s2 < FIN_MAXS; s2++)
          if (s2 < f.nslots && t < f.nf && u[s2] == FIN_EMPTY)
            u[s2] = __hip_atomic_load(q0 + (size_t)s2 * FIN_MAXF + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
#pragma unroll
      for (int s2 = 0; s2 < FIN_MAXS; s2++) {
        if (s2 < f.nslots) {
          if (t < f.nf) {
            if (u[s2] == FIN_EMPTY) __hip_atomic_store(&f.scal[S_BREAK], 4.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(q0 + (size_t)s2 * FIN_MAXF + t, FIN_EMPTY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          const double v = __longlong_as_double((long long)u[s2]);
          double tot = 0.0;
          for (int g = 0; g < f.nf; g++) tot += __shfl(v, g);
          if (t == 0) f.scal[f.slot0 + s2] = tot;
        }
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence_block();
    // a finaliser that gave up on a partial said so at agent scope (sum_slice); it may have been another workgroup on
    // another XCD, so the code is fetched past this XCD's L2 before derive_scalars / post_scalars read it plainly
    if (__hip_atomic_load(&f.scal[S_BREAK], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 4.0) f.scal[S_BREAK] = 4.0;
    if (f.phase >= 0) derive_scalars(f.scal, f.phase);
    if (f.seq > 0) post_scalars(f.scal, f.post, f.seq);
  }
  return true;
}

// The first generation of a fused launch started in cohorts.  The workgroups that are resident together from the start
// (ncu CUs x the kernel's workgroups per CU) begin in the same phase and STAY in step -- all loading (bandwidth-bound, the
// sweeps' LDS idle), then all sweeping (the memory system idle) -- for the whole launch, 27 generations at 216^3 included:
// the slot loop's trickle that interleaves one brick's loads with its neighbours' sweeps only works once the bricks of a
// CU are out of phase.  So the k-th workgroup of a CU (blockIdx / ncu: dispatch hands the first ncu workgroups one to each
// CU) waits k x `ticks` of the 100-MHz clock before it starts, a third of a brick's period for k_pc_park's three.
// MEASURED (bench.py --micro-only, same box, profiles/stagger_r4.log): k_pc_park 0.0917 -> 0.0842 ms at 108^3, 0.0801 ->
// 0.0752 at 100^3, 0.6012 -> 0.5464 ms at 216^3 (63.5 -> 69.9 % of HBM peak) with 6 us per cohort; 3 us gives most of it,
// 9 us nothing; a second box: 0.0899 -> 0.0840 at 108^3, 0.556-0.561 -> 0.546-0.551 at 216^3.  k_pc_wave (ten-odd one-wave
// bricks per CU, in workgroups of four) gains 1.5 % with 4 us per cohort (C5 0.1981-0.1993 -> 0.1954-0.1959, C4's quarter
// 0.1687-0.1695 -> 0.1661-0.1666).  (Round 3 tried the same on the all-loads-at-once experiment k_pc_rows3 and saw no
// change: there a brick's loads ARE one burst.)
// A workgroup barrier that orders LDS accesses only: what the waves wrote to LDS before it is what they read after it, and
// nothing waits for vector memory -- global loads requested in front of it are still in flight behind it.  The fences name
// the local address space, so the only counter the compiler may wait on here is lgkmcnt.
// (__syncthreads() fences every address space.  With only plain global loads outstanding this compiler emits the same
// `s_waitcnt lgkmcnt(0); s_barrier` for it -- profiles/stage_kernel_asm_r10.log -- but nothing promises that; this form says
// what is meant.)
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

struct Stagger { int ticks = 0, ncu = 256, per_cu = 3; };
static_assert(std::is_trivially_copyable<Stagger>::value, "a kernel argument holds views, never an owner");
__device__ __forceinline__ void stagger_start(const Stagger& st) {
  if (st.ticks > 0 && (int)blockIdx.x < st.ncu * st.per_cu) {
    const unsigned long long t0 = wall_clock64(), wait = (unsigned long long)((int)blockIdx.x / st.ncu) * (unsigned long long)st.ticks;
    while (wall_clock64() - t0 < wait) __builtin_amdgcn_s_sleep(32);
  }
}

// the workgroup's sums of v[0 .. NS) into the partials of the consecutive slots slot0, slot0 + 1, ... (entry blk)
template <int NS>
__device__ __forceinline__ void wg_reduce_store(double (&v)[NS], double* red, double* partials,
                                                int nb_max, int slot0, int blk) {
  // red: LDS scratch of NS * 16 doubles (up to 16 waves per workgroup)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int s = 0; s < NS; s++) {
    const double t = wave_sum(v[s]);
    if (lane == 0) red[s * 16 + w] = t;
  }
  __syncthreads();
  // Round 6, one WAVE per slot: wave s's first lane adds the waves' sums of slot s (w = 0, 1, ... in order: same bits), the NS chains
  // side by side; slot = slot0 + wave (an indexed or selected table of slot numbers went to scratch).
  // MEASURED (profiles/epiw_ab_r6_*.log, alternating same-box rounds): the composed launch with its five sums 0.6889 -> 0.6836 ms at
  // 216^3, 0.0977 -> 0.0961 at 108^3 (three rounds each, every round the same sign); one-sum launches and k_pc_wave unchanged.
  // (Before: thread 0 added all slots, rounds 1-5.)
  if (nw >= NS) {      // (a workgroup of fewer waves than slots: the one-lane form below)
    if (lane == 0 && w < NS) {
      double t = 0.0;
      for (int q = 0; q < nw; q++) t += red[w * 16 + q];
      store_partial(partials + (size_t)(slot0 + w) * nb_max + blk, t);
    }
    return;
  }
  // MEASURED AND REMOVED (round 6): one lane per slot for these NS sums (side by side instead of one after the other, same
  // order inside each) -- the lane-indexed slot number sent the slot table to scratch memory (32 bytes per lane) and every
  // fused launch ran 10 % slower (0.533 -> 0.586 ms at 216^3, 0.083 -> 0.089 at 108^3: profiles/exp_ab_r6_*.log).
  if (threadIdx.x == 0) {
#pragma unroll
    for (int s = 0; s < NS; s++) {
      double t = 0.0;
      for (int q = 0; q < nw; q++) t += red[s * 16 + q];
      store_partial(partials + (size_t)(slot0 + s) * nb_max + blk, t);
    }
  }
}
// the workgroup's partial sums of dot mode `mode`'s products (v: pc_row_dots), one per slot, into entry blk
__device__ __forceinline__ void pc_reduce_dots(int mode, double (&v)[5], double* red, double* partials, int nb_max, int blk) {
  const int slot0 = pc_dot_slot0(mode);
  if (mode == PC_DOT_MERGED) wg_reduce_store<5>(v, red, partials, nb_max, slot0, blk);
  else if (mode == PC_DOT_XZ) { double v2[2] = {v[0], v[1]}; wg_reduce_store<2>(v2, red, partials, nb_max, slot0, blk); }
  else { double v1[1] = {v[0]}; wg_reduce_store<1>(v1, red, partials, nb_max, slot0, blk); }
}

// The same for a workgroup that several bricks share (k_pc_park<.., PACK>): the sums over the waves [w0, w0 + nwm) of the
// calling wave's brick into entry blk, the brick's own index; blk < 0: a wave without a brick, which only takes part in
// the barrier.  The brick's waves are added in ascending order from +0.0, as wg_reduce_store adds them in the brick's own
// workgroup (whose further waves, all inactive, add +0.0): the same bits.  One wave per slot where the brick has that many
// waves (its k-th wave takes slot slot0 + k), else the brick's first wave takes the slots one after the other.
template <int NS>
__device__ __forceinline__ void wg_reduce_store_waves(double (&v)[NS], double* red, double* partials, int nb_max, int slot0,
                                                      int blk, int w0, int nwm) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < NS; s++) {
    const double t = wave_sum(v[s]);
    if (lane == 0) red[s * 16 + w] = t;
  }
  __syncthreads();
  if (blk < 0 || lane != 0) return;
  const int k = w - w0;
  if (nwm >= NS) {
    if (k < NS) {
      double t = 0.0;
      for (int q = w0; q < w0 + nwm; q++) t += red[k * 16 + q];
      store_partial(partials + (size_t)(slot0 + k) * nb_max + blk, t);
    }
    return;
  }
  if (k == 0) {
#pragma unroll
    for (int s = 0; s < NS; s++) {
      double t = 0.0;
      for (int q = w0; q < w0 + nwm; q++) t += red[s * 16 + q];
      store_partial(partials + (size_t)(slot0 + s) * nb_max + blk, t);
    }
  }
}
__device__ __forceinline__ void pc_reduce_dots_waves(int mode, double (&v)[5], double* red, double* partials, int nb_max, int blk,
                                                     int w0, int nwm) {
  const int slot0 = pc_dot_slot0(mode);
  if (mode == PC_DOT_MERGED) wg_reduce_store_waves<5>(v, red, partials, nb_max, slot0, blk, w0, nwm);
  else if (mode == PC_DOT_XZ) { double v2[2] = {v[0], v[1]}; wg_reduce_store_waves<2>(v2, red, partials, nb_max, slot0, blk, w0, nwm); }
  else { double v1[1] = {v[0]}; wg_reduce_store_waves<1>(v1, red, partials, nb_max, slot0, blk, w0, nwm); }
}

// One row's (k_pc_rows, k_pc_wave: one scalar's) terms of dot mode `mode`'s products (context.hpp, PcDot), for a mode
// other than none: v[0 .. pc_dot_nslots(mode)) gain x.o, o.o, ... over N components, with o the result z, x the operand
// and a the partner aux.  get_x(x) / get_a(a) fill in the operand and the partner inside the branch of a mode that
// needs them, so that each kernel's loads stay where they were.  Modes 1 and 4 skip inactive rows; mode 2 skips them
// where GUARD2, and mode 3 never does.  Each kernel keeps the arithmetic it always had, because the two forms round apart
// once the compiler contracts them into FMAs:
//   SUM = false (k_pc, k_pc_wave): term by term, v[q] += x[0] o[0]; v[q] += x[1] o[1]; ...
//   SUM = true (k_pc_park, k_pc_rows): one sum per product, v[q] = x[0] o[0] + x[1] o[1] + ...
template <int N, bool SUM, bool GUARD2, class GetX, class GetA>
__device__ __forceinline__ void pc_row_dots(int mode, double (&v)[5], const double (&o)[N], bool active, GetX get_x,
                                            GetA get_a) {
  auto dot = [&](int q, const double (&p)[N], const double (&r)[N]) {
    if constexpr (SUM) {
      double t = p[0] * r[0];
#pragma unroll
      for (int k = 1; k < N; k++) t += p[k] * r[k];
      v[q] = t;
    } else {
#pragma unroll
      for (int k = 0; k < N; k++) v[q] += p[k] * r[k];
    }
  };
  double x[N], a[N];
  if (mode == PC_DOT_ZA) {
    if (active) { get_a(a); dot(0, o, a); }
  } else if (mode == PC_DOT_XZ) {
    if (active || !GUARD2) { get_x(x); dot(0, x, o); dot(1, o, o); }
  } else if (mode == PC_DOT_MERGED) {
    if (active) { get_x(x); get_a(a); dot(0, x, o); dot(1, o, o); dot(2, x, x); dot(3, x, a); dot(4, o, a); }
  } else {
    dot(0, o, o);
  }
}

template <int NS>
__device__ __forceinline__ void block_reduce_store(double (&v)[NS], double* partials, int nb_max,
                                                   const int* slots) {
  __shared__ double sm[NS][TPB / 64];
#pragma unroll
  for (int s = 0; s < NS; s++) {
    const double t = wave_sum(v[s]);
    if ((threadIdx.x & 63) == 0) sm[s][threadIdx.x >> 6] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int s = 0; s < NS; s++) {
      double t = 0.0;
#pragma unroll
      for (int w = 0; w < TPB / 64; w++) t += sm[s][w];
      store_partial(partials + (size_t)slots[s] * nb_max + blockIdx.x, t);
    }
  }
}

}  // namespace wai

// The fused kernel with one wave per brick of <= 64 block rows, k_pc_wave.
#pragma once
#include "reductions.hip.h"

namespace wai {

// ---- K6+K8 fused, one WAVE per brick of <= 64 block rows (block sizes 3, 4; pivot-scaled DILU) ------
// k_pc_rows spreads a brick over BS x R threads and pays a workgroup barrier per substitution level, with most
// of its waves idle at every one of them.  A brick of at most 64 block rows fits ONE wave, one lane per block
// row, and then no barrier is needed at all: the LDS executes a wave's instructions in order, so a level's
// writes are seen by the next level's reads.  The lower blocks of a row stay in registers (3 x BS^2 doubles),
// the upper ones are parked in LDS as the row streams in (k_pc_park's idea) and read back from there in the
// backward sweep; four independent bricks share a 256-thread workgroup (no barrier through the sweeps; one at the very end,
// where the four bricks' inner-product sums become the workgroup's one partial sum per slot: round 4), ~13 bricks
// are resident per CU, and the latency of one brick's sweeps hides behind the loads of the others.
// Serves the 8 x 4 x 2 bricks of 3 x 3 blocks and the 4 x 4 x 2 (32 + 32 rows) MINC bricks.
// MEASURED and not kept (round 4, C5 = MINC bricks of 32 eight-block + 32 two-block rows):
//  * the matrix rows' lanes, idle through six of the eight streaming rounds, taking over the trailing (upper / out-of-brick)
//    slots of the fracture rows -- five full rounds instead of eight half-empty ones; the SpMV ALONE gains 10 % from full
//    load instructions (tools/micro/spmv_minc_rows.hip: 64.3 -> 70.9 % of HBM peak; the holes the short rows leave in the
//    value planes cost nothing), but this kernel does not: application without the product 0.169 -> 0.165 ms, with it
//    0.171 -> 0.190 (141-147 VGPRs: three waves per SIMD).  A brick lives ~18 us -- column indices, blocks + gathers, ~20
//    levels through LDS, epilogue: a chain of latencies -- and 16 are resident per CU: the launch is
//    bricks / (16 x 256) generations of that, whatever the rounds hold (profiles/wave_help_ab_r4.log);
//  * two bricks per workgroup instead of four (C4's bricks park 11.3 KB each: 7 x 2 = 14 per CU instead of 3 x 4 = 12; the
//    registers allow 16): no difference at C4 (0.4995-0.5028 against 0.5018-0.5028 ms without a reduction), the finalisers'
//    128 threads 1-2 % slower with one (profiles/wave_bpw_ab_r4.log) -- more resident bricks do not help either;
//  * the slots' loads overlapped.  In the slot loop below every slot sits behind its own `q < cnt` branch and the compiler
//    ends each with s_waitcnt vmcnt(0): W dependent round trips per brick with ~11 loads in flight per lane.  A variant for
//    rows of exactly seven slots, known at compile time (C4), has no branch between the slots; unfenced, all 77 loads of a
//    row are requested up front: 193-233 VGPRs, two waves per SIMD, fused launch 0.574 against 0.500 ms at C4 -- but the
//    application WITHOUT the product (151 VGPRs, three waves per SIMD = what the LDS allows anyway) 0.528 against 0.549.
//    Holding the product variant to two or three slots in flight (the streams are read-only __restrict__ data that no
//    compiler barrier holds back; the next request's offset made to depend on the consumed slot's sum through an empty
//    asm does) bounds the loads but not the registers: the lower-coupling selects and the gathers are then put off to the
//    end of the row and keep all seven blocks alive (195-251 VGPRs).  Not kept (profiles/wave_pipe_ab_r4.log);
//  * (first attempt at what is now in: see pav below) the epilogue's dot-product partners requested before the backward sweep,
//    behind per-lane conditions: the epilogue 20 us shorter with five
//    products, the rest of the kernel 2 % longer, nothing per iteration (profiles/wave_prefetch_ab_r4.log).
template <int BS, bool SPMV, bool AX>
__global__ __launch_bounds__(256) void k_pc_wave(
    int n, int W, int nsub, const int* __restrict__ sub_ptr, const int* __restrict__ sub_nlev,
    const int* __restrict__ row_info, const int* __restrict__ row_uoffw, const int* __restrict__ col,
    const double* __restrict__ sval, const double* __restrict__ dinv, const double* __restrict__ in,
    const double* __restrict__ in2, const double* __restrict__ scal, double* __restrict__ z, const double* __restrict__ aux, double* partials, int nb_max, int dot,
    const int* __restrict__ sub_list, const int* __restrict__ rowptr, const int* __restrict__ sub_split, int lds_per_brick, int pbase, Fin fin, Stagger stagger) {
  constexpr int BB = BS * BS, NL = 3, NU = 4;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ __attribute__((aligned(16))) double wred[FIN_MAXS][4];   // the four bricks' sums of a workgroup (160 bytes: a multiple of 16)
  if (fin_block(fin, partials, nb_max)) return;
  stagger_start(stagger);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (dot != 0 && lane < FIN_MAXS) wred[lane][wave] = 0.0;   // (a wave without a brick leaves zeros behind)
  const int ngrp = (nsub + 3) >> 2;
  const int g = xcd_remap(blockIdx.x, ngrp);
  if (g >= ngrp) return;
  int s = g * 4 + wave;
  // wave-uniform exit of a WHOLE wave ahead of the workgroup barriers of the reduction epilogue: s_barrier counts only
  // the waves that have not terminated (CDNA ISA, "S_BARRIER": ended waves are not waited for), which this relies on;
  // the epilogue reads the zeros such a wave left in wred above
  if (s >= nsub) return;
  if (sub_list) s = sub_list[s];
  const int lo = sub_ptr[s], R = sub_ptr[s + 1] - lo;
  const int nl = sub_nlev[s];
  const int spl = sub_split ? sub_split[s] : 0;   // (with the brick's other scalars: no round trip of its own)
  const int nlf = nl & 0xffff, nlb = nl >> 16;
  const int i = lo + lane;
  const bool active = lane < R;
  const double nalpha = AX ? -scal[S_ALPHA] : 0.0;   // input = in - alpha in2
  // The epilogue's dot-product partner (block order, lane-linear) is requested HERE, before anything else of the brick: at
  // the end of the brick nothing of this wave is left to hide the round trip behind, and a brick lives only ~20-30 us.
  // One uniform branch, inside it straight-line loads with a clamped index (per-lane conditions around the requests made
  // the compiler wait between them: the first attempt, profiles/wave_prefetch_ab_r4.log, gained nothing).  MEASURED
  // (profiles/wave_early_aux_ab_r4.log, alternating builds, three runs): the launch with one product 0.5686 -> 0.5475 ms at
  // C4, 0.1889 -> 0.1826 at C5; an iteration -2.1 % / -1.9 %.
  double pav[BS];
#pragma unroll
  for (int j = 0; j < BS; j++) pav[j] = 0.0;
  if (dot == PC_DOT_ZA || dot == PC_DOT_MERGED) {
    const int totp = R * BS;
#pragma unroll
    for (int j = 0; j < BS; j++) pav[j] = __builtin_nontemporal_load(aux + (size_t)lo * BS + min(lane + 64 * j, totp - 1));
  }
  double* ys = lds + (size_t)wave * lds_per_brick;   // [64 * BS] solution in block order
  double* upark = ys + 64 * BS;                      // parked upper blocks, row-major BS x BS each
  double Lf[NL][BB];
  int Lc[NL], ucpack = 0, lf = -1, lb = -1, uo = 0, nU = 0;   // ucpack: local columns of the <= 4 upper couplings, 8 bits each
#pragma unroll
  for (int p = 0; p < NL; p++) {
    Lc[p] = lane;
#pragma unroll
    for (int e = 0; e < BB; e++) Lf[p][e] = 0.0;
  }
  if (active) {
    int lfirst, dslot, ulast;
    unpack_info(row_info[i], lfirst, dslot, ulast, lf, lb);
    uo = row_uoffw[i];
    nU = ulast - dslot - 1;
    // slots to stream: all W on uniform rows; with short rows (MINC matrix cells) the brick's record tells -- the long
    // rows first, all W slots each (padding = a zero block on the own column), then the short ones -- unless the brick
    // mixes them (15): then, and without a record, the row pointers do, one dependent round trip before the first block
    int cnt = W;
    if (rowptr) cnt = (sub_split && (spl >> 16) != 15) ? (lane < (spl & 0xffff) ? W : (spl >> 16)) : rowptr[i + 1] - rowptr[i];
    int cgs[WMAX];
#pragma unroll
    for (int q = 0; q < WMAX; q++) {
      cgs[q] = i;
      if (q < cnt) cgs[q] = load_col(col, (size_t)q * n + i);
    }
    double acc[BS];
#pragma unroll
    for (int r = 0; r < BS; r++) acc[r] = 0.0;
#pragma unroll
    for (int q = 0; q < WMAX; q++) {
      if (q < cnt) {
        const int cg = cgs[q];
        double blk[BB];
#pragma unroll
        for (int e = 0; e < BB; e++) blk[e] = __builtin_nontemporal_load(sval + vix<BS>(n, q, e, i));
        if constexpr (SPMV) {
          double xv[BS];
          load_xs<BS, AX>(in, in2, nalpha, cg, xv);
#pragma unroll
          for (int r = 0; r < BS; r++)
#pragma unroll
            for (int k = 0; k < BS; k++) acc[r] += blk[r * BS + k] * xv[k];
        }
        const bool isl = (q >= lfirst) && (q < dslot), isu = (q > dslot) && (q < ulast);
#pragma unroll
        for (int p = 0; p < NL; p++) {
          const bool tl = isl && (q - lfirst == p);
          Lc[p] = tl ? cg - lo : Lc[p];
#pragma unroll
          for (int e = 0; e < BB; e++) Lf[p][e] = tl ? blk[e] : Lf[p][e];
        }
        if (isu) {
          const int pu = q - dslot - 1;
          ucpack |= (cg - lo) << (8 * pu);
          double* dst = upark + (size_t)(uo + pu) * BB;
#pragma unroll
          for (int e = 0; e < BB; e++) dst[e] = blk[e];
        }
      }
    }
    if constexpr (!SPMV) {  // plain application to an unscaled vector: scale it by the inverted pivot
#pragma unroll
      for (int r = 0; r < BS; r++)
#pragma unroll
        for (int k = 0; k < BS; k++) acc[r] += dinv[dix<BS>(n, r * BS + k, i)] * in[(size_t)i * BS + k];
    }
#pragma unroll
    for (int r = 0; r < BS; r++) ys[lane * BS + r] = acc[r];
  }
  __builtin_amdgcn_wave_barrier();
  for (int lev = 1; lev < nlf; lev++) {  // forward: y_i = t_i - sum A'_ik y_k
    if (lf == lev) {
      double a[BS];
#pragma unroll
      for (int r = 0; r < BS; r++) a[r] = ys[lane * BS + r];
#pragma unroll
      for (int p = 0; p < NL; p++) {
        double yk[BS];
#pragma unroll
        for (int k = 0; k < BS; k++) yk[k] = ys[Lc[p] * BS + k];
#pragma unroll
        for (int r = 0; r < BS; r++)
#pragma unroll
          for (int k = 0; k < BS; k++) a[r] -= Lf[p][r * BS + k] * yk[k];
      }
#pragma unroll
      for (int r = 0; r < BS; r++) ys[lane * BS + r] = a[r];
    }
    __builtin_amdgcn_wave_barrier();
  }
  // ... and the operand's own entries (block order) for the merged products a backward sweep early: the lower blocks'
  // registers are free now (requested at the start too they would cost the fourth wave per SIMD).  MEASURED on top of the
  // partner vector (profiles/wave_early_xi_ab_r4.log): the five-product launch 0.6177 -> 0.6015 ms at C4; an iteration
  // against everything in the epilogue 1.477 -> 1.429 ms at C4 (-3.3 %), 0.503 -> 0.496 at C5, 0.413 -> 0.399 at C4's share
  double pxi[BS], pi2[BS];
#pragma unroll
  for (int j = 0; j < BS; j++) { pxi[j] = 0.0; pi2[j] = 0.0; }
  if (dot == PC_DOT_XZ || dot == PC_DOT_MERGED) {
    const int totp = R * BS;
#pragma unroll
    for (int j = 0; j < BS; j++) {
      const size_t gp = (size_t)lo * BS + min(lane + 64 * j, totp - 1);
      pxi[j] = in[gp];
      if constexpr (AX) pi2[j] = in2[gp];
    }
  }
  for (int lev = 0; lev < nlb; lev++) {  // backward: x_i = y_i - sum A'_ij x_j, upper blocks from LDS
    if (lb == lev) {
      double a[BS];
#pragma unroll
      for (int r = 0; r < BS; r++) a[r] = ys[lane * BS + r];
#pragma unroll
      for (int p = 0; p < NU; p++) {
        if (p < nU) {
          const double* ub = upark + (size_t)(uo + p) * BB;
          double xk[BS];
          const int uc = (ucpack >> (8 * p)) & 63;
#pragma unroll
          for (int k = 0; k < BS; k++) xk[k] = ys[uc * BS + k];
#pragma unroll
          for (int r = 0; r < BS; r++)
#pragma unroll
            for (int k = 0; k < BS; k++) a[r] -= ub[r * BS + k] * xk[k];
        }
      }
#pragma unroll
      for (int r = 0; r < BS; r++) ys[lane * BS + r] = a[r];
    }
    __builtin_amdgcn_wave_barrier();
  }
  // block-order, lane-linear epilogue: the wave's R * BS results leave coalesced; dot products on the way
  double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  const int tot = R * BS;
#pragma unroll
  for (int j = 0; j < BS; j++) {
    const int t = lane + 64 * j;
    if (t < tot) {
      const size_t gi = (size_t)lo * BS + t;
      const double out = ys[t];
      __builtin_nontemporal_store(out, z + gi);
      if (dot != 0)
        pc_row_dots<1, false, false>(dot, v, {out}, true, [&](double (&x)[1]) { x[0] = AX ? __builtin_fma(nalpha, pi2[j], pxi[j]) : pxi[j]; },
                                     [&](double (&a)[1]) { a[0] = pav[j]; });
    }
  }
  if (dot != 0) {
    // ONE partial sum per workgroup and slot, not one per brick: what the in-launch finalisation costs over storing the
    // partials goes with their number -- MEASURED 9 us + 0.27 us per 1000 partials of five slots (2 646 at 108^3: 9 us,
    // 21 168 at 216^3: 15, 31 250 at C5: 20, 78 586 at C4: 30), whatever the finalisers' count, batching or polling
    // interval (profiles/fin_jv_ab_r4.log, fin_sleep_ab_r4.log).  The workgroup's LDS is held until its last brick ends
    // anyway, so the barrier costs no residency.  Index: the workgroup's position in the launch's list + pbase (the
    // face bricks' launch continues where the interior bricks' ended)
    const int ns = pc_dot_nslots(dot), slot0 = pc_dot_slot0(dot);
#pragma unroll
    for (int q = 0; q < 5; q++) {
      if (q < ns) {
        const double t = wave_sum(v[q]);
        if (lane == 0) wred[q][wave] = t;
      }
    }
    __syncthreads();   // (waves that left without a brick do not count)
    if (wave == 0 && lane < ns)
      store_partial(partials + (size_t)(slot0 + lane) * nb_max + pbase + g, ((wred[lane][0] + wred[lane][1]) + wred[lane][2]) + wred[lane][3]);
  }
}

}  // namespace wai

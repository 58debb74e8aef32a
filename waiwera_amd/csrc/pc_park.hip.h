// The fused kernel for 2 x 2 blocks with the upper blocks parked in LDS, k_pc_park.
#pragma once
#include "reductions.hip.h"

namespace wai {

// ---- K6+K8 fused, upper blocks parked in LDS (bs = 2, pivot-scaled DILU, <= 3+3 couplings) -----
// k_pc holds a row's three lower and three upper blocks in registers through both sweeps (~100
// VGPRs: two workgroups per CU), although the upper blocks are only needed once the forward sweep
// is over and the lower ones are dead by then.  Here the upper blocks go to LDS as the row is
// loaded (compactly: a brick has ~2.6 in-brick upper couplings per row, 43 KB for 8x8x8) and come
// back into the lower blocks' registers for the backward sweep.  ~75 VGPRs, 6 waves per SIMD:
// three resident workgroups per CU (3 x 51 KB of the 160 KB LDS), so one more brick's loads are in
// flight to cover the latency-bound sweeps of the others.
// MEASURED (216^3, MI355X, same box): 0.604 ms against k_pc's 0.709 ms; 68 VGPRs, no spills.
// MEASURED AND REMOVED (round 4): wave-staged sweeps.  With a brick's rows in dependency-level order a wave's 64 rows
// span a contiguous range of levels and need no barrier among themselves (the LDS executes a wave's instructions in
// order), so the workgroup barrier can shrink to the hand-over from one wave to the next -- 8 per sweep instead of 32.
// Same bits, and SLOWER on every size: fused launch 0.6175 against 0.5904 ms at 216^3, 0.0960 / 0.0892 at 108^3,
// 0.0839 / 0.0766 at 100^3 (same box, profiles/bench_r4_wavestage_ab.log): a level's cost is its LDS round trip and FMA
// chain, not the barrier, and the per-level barriers let the two waves that share a level run it side by side.
// C16 (round 5): the column indices come as brick-local 16-bit (segment, offset) pairs (IluSchedule::col16, sub_seg), a
// row's eight together: ONE 16-byte load per row instead of seven 4-byte loads from seven planes (16 instead of 28 bytes,
// and six vector-memory instructions fewer of a row's ~28); the eight segment bases of the brick are wave-uniform (scalar
// loads) and the lane's pick among them a chain of selects.  Same columns, same order, same bits.
// (First form, one 16-bit plane per slot: 2 bytes less per block but the same seven loads -- MEASURED no faster: fused
// launch 0.0845 -> 0.0859 ms at 108^3, 0.584 -> 0.581 at 216^3, profiles/col16_planes_ab_r5.log.)
// MEASURED AND NOT KEPT (round 6, profiles/persist_ab_r6_*.log; the variant was never committed -- this note is its record: the body
// below inside `for (bpos = blockIdx.x; bpos < padded count; bpos += G)`, G = gridDim.x - finalisers, a barrier at the loop's end,
// grid = 3 x CUs rounded to a multiple of 8): the launch as 768 PERSISTENT
// workgroups (3 per CU), each walking the brick positions w, w + 768, ... of its XCD's eighth in a loop instead of giving its
// slot back after one brick (the verdict's "no re-dispatch gap, bricks handed out by a cursor").  Same bits.  Two findings:
// (i) the loop form alone costs registers -- 80 VGPRs and 20-36 bytes of scratch where the straight-line body has 73 and
// none (loop-carried kernel arguments: 41-53 SGPR spills) -- 0.545 -> 0.627 ms first launch, 0.674 -> 0.769 composed at 216^3;
// (ii) on that same code the persistent grid is SLOWER again than one workgroup per brick: 0.685 / 0.836 ms at 216^3, equal at
// 108^3 and 100^3.  Re-dispatch is not a gap worth closing (a fresh workgroup is in its slot within the time a brick's
// epilogue drains), and the dispatcher's hand-out -- whichever slot frees first -- decorrelates the bricks of a CU, which a
// fixed stride never does: workgroups that started together stay in step, all loading, then all sweeping (the effect the
// start-up cohorts were introduced against in round 4, now for the whole launch).
// STAGE (round 10; the operator on the 16-bit column indices only): the brick's own operand segment staged in LDS.  Each
// thread requests its row's own entry beside the descriptors, stores S_i = R_i - alpha V_i (the fma of load_xs; one vector:
// the entry) to the idle solution area, and behind a barrier the in-brick columns -- the sweeps' couplings, slots
// [lfirst, ulast), 79 % of a 16 x 16 x 2 brick's -- are 16-byte LDS reads at the brick-local number the sweeps use; far
// columns keep their gathers, the products and their order are unchanged, a second barrier gives the area back to t = A S.
// Same bits (tests/test_hip_park_stage.py).  Round 6 built this once (profiles/stage_ab_r6_*.log: composed launch 0.651 ->
// 0.673 ms, first 0.529 -> 0.571) and blamed the two barriers.  The barriers were not it: __syncthreads() with plain loads
// outstanding is `s_waitcnt lgkmcnt(0); s_barrier` on this compiler too, it never drained vmcnt.  What that form paid was the
// ORDER -- own entry requested, waited for, stored, barrier, and only then slot 0's loads: one whole exposed round trip per
// brick.  Here slot 0's block and, for a far slot 0, its gather are requested BEFORE the store and are in flight across the
// barrier (lds_barrier: fences on the local address space only), so the round trip the brick waits for behind the barrier is
// the one it waited for anyway.  Three things the compiler needed telling (profiles/stage_kernel_asm_r10.log): the explicit
// vmcnt(0) behind the barrier (else every later reuse of a register drains the dot product's partner, which is meant to fly
// through the sweeps), the opaque copy of the far slot 0's pair (else S is formed of it, and waited for, in front of the
// barrier), and the inner products' FMAs written out (else (S, S) is contracted the other way round: one ulp).
// MEASURED (profiles/stage_ab_r10_*.log, alternating same-box rounds, two boxes): composed launch 0.600-0.606 -> 0.578-0.582
// ms at C3 in all seven rounds (-3.7 %), 0.0783 -> 0.0768-0.0775 at C2, 0.0929 -> 0.0918 at the 108^3 share; L1 -> L2 read
// requests 42.1 M -> 32.2 M per launch, memory reads unchanged at 22.67 M lines (pmc_stage_r10_c3.txt).  The FIRST launch,
// which gathers one vector where the composed one gathers two, LOSES: 0.505-0.507 -> 0.519 ms at C3, 0.0662 -> 0.0675 at C2
// -- so the compiled-in default stages the composed launch only (kernels_fused.hip: park_staged; WAI_PARK_STAGE=0|1 forces
// both kinds).  80 / 76 VGPRs (composed / first), no scratch, three workgroups per CU as before.
// PACK (round 9): short bricks share a workgroup (ilu_schedule.hpp, phase 10).  The workgroup's position selects a GROUP of
// 1 .. 8 bricks and `sub_list` is the groups' table: each wave reads its record -- its brick (or none: the wave only takes part
// in the barriers), the brick's thread offset in the workgroup, its base in the park, the group's level counts -- with one
// 16-byte scalar load, and runs its brick as the brick's own workgroup would: the same rows on the same lanes of whole waves,
// the same sums, one partial per brick at the brick's own index, the brick's waves added in ascending order (what its own
// workgroup does, where the absent waves add +0.0).  Same bits.  nsub is then the number of groups.
template <bool SPMV, bool AX, bool C16, bool PACK = false, bool STAGE = false>   // (PACK && STAGE: brick-local numbers are tid - toff, a wave without a brick only takes part in the barriers)
__global__ __launch_bounds__(512, 6) void k_pc_park(
    int n, int W, int nsub, const int* __restrict__ sub_ptr, const int* __restrict__ sub_nlev,
    const int* __restrict__ sub_desc, const int* __restrict__ row_info, const int* __restrict__ row_uoff, const int* __restrict__ col,
    const unsigned short* __restrict__ col16, const int* __restrict__ sub_seg,
    const double* __restrict__ sval, const double* __restrict__ dinv, const double* __restrict__ in,
    const double* __restrict__ in2, const double* __restrict__ scal,
    double* __restrict__ z, const double* __restrict__ aux, double* partials, int nb_max, int dot,
    const int* __restrict__ sub_list, Fin fin, Stagger stagger) {
  constexpr int BS = 2, BB = 4, MLU = 3;
  static_assert(!STAGE || (SPMV && C16), "the staged operand is the operator's, on the 16-bit column indices");
  extern __shared__ __attribute__((aligned(16))) double lds[];  // [T*2] solution, [80] reduction scratch, then parked U blocks
  // nsub subdomains to run: all of them, or (sub_list) the listed ones -- the bricks that touch no
  // partition ghost while the halo exchange is in flight, the others after it
  if (fin_block(fin, partials, nb_max)) return;
  int s = xcd_remap(blockIdx.x, nsub);
  if (s >= nsub) return;
  int toff = 0, ubase = 0, nl_grp = 0;   // PACK: the wave's member of the group (all wave-uniform)
  if constexpr (PACK) {
    const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int4 rec = reinterpret_cast<const int4*>(sub_list)[(size_t)s * 8 + w];
    s = rec.x; toff = rec.y; ubase = rec.z; nl_grp = rec.w;
  } else {
    if (sub_list) s = sub_list[s];
  }
  const bool member = !PACK || s >= 0;
  const int lo = member ? sub_ptr[s] : 0, R = member ? sub_ptr[s + 1] - lo : 0;
  // C16: row_info, row_uoff and col16 are the descriptor templates, the brick's rows from sub_desc[s] on (requested beside
  // sub_ptr, not behind it); otherwise the per-row arrays
  int dlo = lo;
  if constexpr (C16) dlo = member ? sub_desc[s] : 0;
  const int nl = PACK ? nl_grp : sub_nlev[s];
  const int nlf = nl & 0xffff, nlb = nl >> 16;
  // a member's rows sit on the threads from its offset on: brick-local numbers are thread numbers less the offset
  const int tid = threadIdx.x, lob = lo - toff, i = lob + tid, di = dlo - toff + tid;
  const bool active = tid - toff < R;
  const double nalpha = AX ? -scal[S_ALPHA] : 0.0;   // input = in - alpha in2 (uniform: a scalar load)
  stagger_start(stagger);
  double* ys = lds;
  double* upark = lds + (size_t)blockDim.x * BS + 80 + (size_t)ubase * BB;
  double Lf[MLU][BB];
  int Lc[MLU], Uc[MLU], lf = -1, lb = -1, uo = 0, nU = 0;
  double xin[BS] = {0.0, 0.0}, avp[BS] = {0.0, 0.0};
#pragma unroll
  for (int p = 0; p < MLU; p++) {
    Lc[p] = tid; Uc[p] = tid;
#pragma unroll
    for (int e = 0; e < BB; e++) Lf[p][e] = 0.0;
  }
  int lfirst = 0, dslot = 0, ulast = 0;
  int cgs[WMAX];
  // STAGE: the own entry's second operand, slot 0's block and, for a far column, its operand entry, requested in front of the barrier
  [[maybe_unused]] double own2[BS], blk0[BB], xr0[BS], xv0[BS];
  [[maybe_unused]] bool far0 = false;
  if (active) {
    unpack_info(row_info[di], lfirst, dslot, ulast, lf, lb);
    uo = row_uoff[di];
    nU = ulast - dslot - 1;
    // STAGE: the row's own operand entry, requested beside the descriptors (S_i is formed where it is stored, below)
    if constexpr (STAGE) {
      load_x<BS>(in, i, xin);
      if constexpr (AX) load_x<BS>(in2, i, own2);
    }
    // (MEASURED AND REMOVED, round 6: slot 0's block -- which needs nothing but the row number -- requested here, together with
    // the descriptors and the index record, one dependent round trip less per brick: 77 VGPRs, no scratch, same bits, and
    // 3 % SLOWER at 108^3 and 100^3 (first launch 0.0840 -> 0.0868, 0.0741 -> 0.0764 ms), no better at 216^3:
    // profiles/hoist_ab_r6_*.log.  Like every earlier form that put more of a brick's loads in flight at once.)
    // all column indices first: one round trip instead of one per slot (MEASURED at 216^3, same box:
    // 0.6196 -> 0.6018 ms).  A branch-free 7-slot loop, which lets the compiler keep every slot's loads
    // in flight, needs more than the 80 registers of 6 waves per SIMD: 188 bytes of scratch, 0.965 ms;
    // fetching the next slot's block while the current one is used (80 registers, no scratch): 0.626 against 0.614
    if constexpr (C16) {
      const int* sg = sub_seg + (size_t)s * 8;     // wave-uniform
      const int g0 = sg[0], g1 = sg[1], g2 = sg[2], g3 = sg[3], g4 = sg[4], g5 = sg[5], g6 = sg[6], g7 = sg[7];
      typedef unsigned wai_u4v __attribute__((ext_vector_type(4)));
      const wai_u4v pk = reinterpret_cast<const wai_u4v*>(col16)[di];   // the row's eight 16-bit entries (no streaming hint: a template's lines are meant to stay cached)
      const unsigned pw[4] = {pk.x, pk.y, pk.z, pk.w};
      unsigned cu[WMAX];
#pragma unroll
      for (int q = 0; q < WMAX; q++) cu[q] = (pw[q >> 1] >> (16 * (q & 1))) & 0xffffu;
#pragma unroll
      for (int q = 0; q < WMAX; q++) {
        const unsigned code = cu[q] >> 13;
        int b = g0;
        b = code == 1 ? g1 : b; b = code == 2 ? g2 : b; b = code == 3 ? g3 : b; b = code == 4 ? g4 : b;
        b = code == 5 ? g5 : b; b = code == 6 ? g6 : b; b = code == 7 ? g7 : b;
        cgs[q] = q < W ? b + (int)(cu[q] & 8191u) : i;
      }
    } else {
#pragma unroll
      for (int q = 0; q < WMAX; q++) {
        cgs[q] = i;
        if (q < W) cgs[q] = load_col(col, (size_t)q * n + i);
      }
    }
    if constexpr (STAGE) {
      // slot 0's block (a row has its diagonal: W >= 1) goes out first, then the wait for the OLDER own-entry loads alone
      // -- loads return in order, the block stays in flight -- and S_i = R_i - alpha V_i, the fma of load_xs, into the idle
      // solution area, where the brick's other rows find it.  A far slot 0's gather follows the store.
      load_block<BS>(sval, n, 0, i, blk0);
      if constexpr (AX) {
#pragma unroll
        for (int k = 0; k < BS; k++) xin[k] = __builtin_fma(nalpha, own2[k], xin[k]);
      }
      *reinterpret_cast<double2*>(ys + tid * 2) = make_double2(xin[0], xin[1]);
      far0 = lfirst > 0;
      if (far0) {
        load_x<BS>(in, cgs[0], xr0);
        if constexpr (AX) load_x<BS>(in2, cgs[0], xv0);
      }
    }
  }
  if constexpr (STAGE) {
    lds_barrier();   // S is in place; slot 0's loads are still in flight
    // Slot 0's loads are waited for HERE, by every wave, and not at their first use inside `if (active)`: a wave could --
    // for all the compiler knows -- skip that region with them pending, and it then drains vmcnt in front of the next
    // register it reuses, with the dot product's partner (requested at the end of the slot loop, meant to stay in flight
    // through the sweeps) among what is drained.
    __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0) alone (gfx9 encoding: expcnt 7 and lgkmcnt 15 wait for nothing)
  }
  double acc[BS] = {0.0, 0.0};
  if (active) {
#pragma unroll
    for (int q = 0; q < WMAX; q++) {
      if (q < W) {
        const int cg = cgs[q];
        double blk[BB];
        if constexpr (STAGE) {
          if (q == 0) {
#pragma unroll
            for (int e = 0; e < BB; e++) blk[e] = blk0[e];
          } else load_block<BS>(sval, n, q, i, blk);
          // in-brick columns -- the sweeps' couplings, slots [lfirst, ulast) -- read S from the solution area at the
          // brick-local number the sweeps use (a far column: the own entry, unused); the diagonal slot has it in registers
          const bool inb = (q >= lfirst) && (q < ulast);
          const double2 sv = *reinterpret_cast<const double2*>(ys + ((inb && q != dslot) ? cg - lob : tid) * 2);
          double xv[BS] = {q == dslot ? xin[0] : sv.x, q == dslot ? xin[1] : sv.y};
          if (!inb) {
            if (q == 0) {
              // (the compiler must not form S of the gathered pair where the pair was requested, in front of the barrier)
              asm volatile("" : "+v"(xr0[0]), "+v"(xr0[1]));
              xv[0] = xr0[0]; xv[1] = xr0[1];
              if constexpr (AX) { xv[0] = __builtin_fma(nalpha, xv0[0], xv[0]); xv[1] = __builtin_fma(nalpha, xv0[1], xv[1]); }
            } else load_xs<BS, AX>(in, in2, nalpha, cg, xv);
          }
          acc[0] += blk[0] * xv[0] + blk[1] * xv[1];
          acc[1] += blk[2] * xv[0] + blk[3] * xv[1];
        } else load_block<BS>(sval, n, q, i, blk);
        if constexpr (SPMV && !STAGE) {
          double xv[BS];
          load_xs<BS, AX>(in, in2, nalpha, cg, xv);
          acc[0] += blk[0] * xv[0] + blk[1] * xv[1];
          acc[1] += blk[2] * xv[0] + blk[3] * xv[1];
          // the diagonal slot gathered the row's own operand entry: kept for the inner products (the slot, not cg == i --
          // the padding slots of a short row carry the own column too)
          xin[0] = q == dslot ? xv[0] : xin[0];
          xin[1] = q == dslot ? xv[1] : xin[1];
        }
        const bool isl = (q >= lfirst) && (q < dslot), isu = (q > dslot) && (q < ulast);
#pragma unroll
        for (int p = 0; p < MLU; p++) {
          const bool tl = isl && (q - lfirst == p), tu = isu && (q - dslot - 1 == p);
          Lc[p] = tl ? cg - lob : Lc[p];
          Uc[p] = tu ? cg - lob : Uc[p];
#pragma unroll
          for (int e = 0; e < BB; e++) Lf[p][e] = tl ? blk[e] : Lf[p][e];
        }
        if (isu) {
          double* dst = upark + (size_t)(uo + (q - dslot - 1)) * BB;
          *reinterpret_cast<double2*>(dst) = make_double2(blk[0], blk[1]);
          *reinterpret_cast<double2*>(dst + 2) = make_double2(blk[2], blk[3]);
        }
      }
    }
    if constexpr (!SPMV) {  // plain application to an unscaled vector: scale it by the inverted pivot
      double r[BS], dv[BB];
      load_x<BS>(in, i, r);
      load_pivot<BS>(dinv, n, i, dv);
      acc[0] = dv[0] * r[0] + dv[1] * r[1];
      acc[1] = dv[2] * r[0] + dv[3] * r[1];
      xin[0] = r[0]; xin[1] = r[1];
    }
    // (xin: no load of its own -- until round 7 a second fetch of the row's entry here, waited for in front of the first
    // barrier)
    if (dot == PC_DOT_ZA || dot == PC_DOT_MERGED) load_x_stream<BS>(aux, i, avp);   // the dot product's partner: in flight through the sweeps
  }
  if constexpr (STAGE) lds_barrier();   // every row has read the S it needs: the area is the solution's again
  if (active) *reinterpret_cast<double2*>(ys + tid * 2) = make_double2(acc[0], acc[1]);
  __syncthreads();
  auto gather3 = [&](const int (&cc)[MLU], const double (&ff)[MLU][BB], double* sum) {
    double2 yk[MLU];
#pragma unroll
    for (int p = 0; p < MLU; p++) yk[p] = *reinterpret_cast<const double2*>(ys + cc[p] * 2);
#pragma unroll
    for (int r = 0; r < BS; r++) {
      double part[MLU];
#pragma unroll
      for (int p = 0; p < MLU; p++) part[p] = ff[p][r * BS] * yk[p].x + ff[p][r * BS + 1] * yk[p].y;
      sum[r] = (part[0] + part[1]) + part[2];
    }
  };
  // (The sweeps at raised wave priority, s_setprio 3, measured slower: 0.6663 -> 0.6741 ms composed at 216^3, profiles/exp_ab_r6_*.log.)
  for (int lev = 1; lev < nlf; lev++) {  // forward: y_i = t_i - sum A'_ik y_k
    if (lf == lev) {
      const double2 a = *reinterpret_cast<const double2*>(ys + tid * 2);
      double sum[BS];
      gather3(Lc, Lf, sum);
      *reinterpret_cast<double2*>(ys + tid * 2) = make_double2(a.x - sum[0], a.y - sum[1]);
    }
    __syncthreads();
  }
  // the lower blocks are dead: their registers take the parked upper blocks
#pragma unroll
  for (int p = 0; p < MLU; p++) {
    const bool have = p < nU;
    const double* src = upark + (size_t)(uo + (have ? p : 0)) * BB;
    const double2 u0 = *reinterpret_cast<const double2*>(src), u1 = *reinterpret_cast<const double2*>(src + 2);
    Lf[p][0] = have ? u0.x : 0.0; Lf[p][1] = have ? u0.y : 0.0;
    Lf[p][2] = have ? u1.x : 0.0; Lf[p][3] = have ? u1.y : 0.0;
  }
  double out[BS] = {0.0, 0.0};
  for (int lev = 0; lev < nlb; lev++) {  // backward: x_i = y_i - sum A'_ij x_j
    if (lb == lev) {
      const double2 a = *reinterpret_cast<const double2*>(ys + tid * 2);
      double sum[BS];
      gather3(Uc, Lf, sum);
      out[0] = a.x - sum[0];
      out[1] = a.y - sum[1];
      *reinterpret_cast<double2*>(ys + tid * 2) = make_double2(out[0], out[1]);
    }
    if (lev + 1 < nlb) __syncthreads();
  }
  if (active) store_z2(z, (size_t)i, out[0], out[1]);
  if (dot != 0) {
    double* red = lds + (size_t)blockDim.x * BS;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if constexpr (STAGE) {
      // The products of pc_row_dots<BS, true, false>, with the FMA each is contracted into written out.  The compiler is free
      // to fuse either multiplication of p0 r0 + p1 r1 into the addition, the two choices round apart, and what it chooses
      // depends on where the operands come from: with xin a plain fma's result instead of the slot loop's select it chose
      // otherwise for (x, x), and the staged launch's (S, S) was one ulp off the unstaged one's.  These are the forms the
      // unstaged instantiations compile to (profiles/stage_kernel_asm_r10.log); tests/test_hip_park_stage.py holds the two
      // kernels to the same bits.
      auto hi = [](const double (&p)[BS], const double (&r)[BS]) { return __builtin_fma(p[0], r[0], p[1] * r[1]); };
      auto lo = [](const double (&p)[BS], const double (&r)[BS]) { return __builtin_fma(p[1], r[1], p[0] * r[0]); };
      if (dot == PC_DOT_ZA) {
        if (active) v[0] = hi(out, avp);
      } else if (dot == PC_DOT_XZ) {
        v[0] = hi(xin, out); v[1] = hi(out, out);
      } else if (dot == PC_DOT_MERGED) {
        if (active) { v[0] = hi(xin, out); v[1] = hi(out, out); v[2] = lo(xin, xin); v[3] = lo(xin, avp); v[4] = hi(out, avp); }
      } else {
        v[0] = hi(out, out);
      }
    } else
    pc_row_dots<BS, true, false>(dot, v, out, active, [&](double (&x)[BS]) { x[0] = xin[0]; x[1] = xin[1]; },
                                 [&](double (&a)[BS]) { a[0] = avp[0]; a[1] = avp[1]; });
    // the reduction scratch is touched by nothing before this point; dropping the barrier was not felt (0.5704 / 0.6942
    // against 0.5714 / 0.6924 ms at 216^3, profiles/nobar_ab_r6_c3.log), so it stays
    __syncthreads();
    if constexpr (PACK) pc_reduce_dots_waves(dot, v, red, partials, nb_max, s, toff >> 6, (R + 63) >> 6);
    else pc_reduce_dots(dot, v, red, partials, nb_max, s);
  }
}

}  // namespace wai

// Every kernel that stores or finalises a partial sum -- the five fused preconditioned-operator kernels and the K9 vector
// kernels -- with their launchers, the run-time switches and the tests' fault-injection hook (reductions.hip.h says why
// they share one translation unit); the multicolour ordering's k_pc_colour is the sixth fused kernel.
#include "pc_generic.hip.h"
#include "pc_wide.hip.h"
#include "pc_park.hip.h"
#include "pc_rows.hip.h"
#include "pc_wave.hip.h"
#include "pc_colour.hip.h"
#include "krylov_vec.hip.h"

namespace wai {

// ---- launchers -------------------------------------------------------------------------------
static inline int vgrid(int n) {
  int g = (n + TPB - 1) / TPB;
  return g > 1024 ? 1024 : (g < 1 ? 1 : g);
}

// the fused launches' run-time switches: read once per solve / set-up / probe (tests switch them between solves of one process)
void read_env(wai_ctx* c) {
  c->env.fin_separate = getenv("WAI_FIN_SEPARATE") != nullptr;
  c->env.no_col16 = getenv("WAI_NO_COL16") != nullptr;
  c->env.scalar_kernels = getenv("WAI_BCGS_SCALAR_KERNELS") != nullptr;   // several ranks: the one-thread kernels behind the all-reduces (rounds 3-4)
  c->env.iluk_level_path = getenv("WAI_ILUK_LEVEL_PATH") != nullptr;
  c->env.asm_unfused = getenv("WAI_ASM_UNFUSED") != nullptr;
  c->env.no_desc_share = getenv("WAI_NO_DESC_SHARE") != nullptr;
  c->env.no_pack = getenv("WAI_NO_PACK") != nullptr;
  c->env.colour_sweeps = getenv("WAI_COLOUR_SWEEPS") != nullptr;
  c->env.pc_unfused = getenv("WAI_PC_UNFUSED") != nullptr;
  const char* st = getenv("WAI_PARK_STAGE");
  c->env.park_stage = st && (st[0] == '0' || st[0] == '1') ? st[0] - '0' : -1;
}

// k_pc_park<.., STAGE> (pc_park.hip.h): is the brick's own operand segment staged in LDS?  Per launch kind -- the composed
// second launch of a BiCGStab iteration (its operand formed from two vectors) and the first launch (one vector) -- as
// MEASURED (profiles/stage_ab_r10_*.log); WAI_PARK_STAGE=0|1 forces both kinds off or on.
#ifndef WAI_PARK_STAGE_COMPOSED
#define WAI_PARK_STAGE_COMPOSED 1
#endif
#ifndef WAI_PARK_STAGE_FIRST
#define WAI_PARK_STAGE_FIRST 0
#endif
static bool park_staged(const wai_ctx* c, bool composed) {
  if (c->env.park_stage >= 0) return c->env.park_stage == 1;
  return composed ? WAI_PARK_STAGE_COMPOSED != 0 : WAI_PARK_STAGE_FIRST != 0;
}

// which fused kernel serves (matrix, schedule; context.hpp).  Kinds 1 .. 3 can form their input on the fly (in - alpha in2:
// launch_pc_on's in2)
int pc_kernel_kind(const wai_ctx* c, const Bcsr& J, const IluSchedule& s) {
  if (J.dg) return -1;    // the coupled tracer system: k_dg_pc (kernels_tracer_block.hip)
  if (s.wide) return 4;   // rows of 9 .. 16 blocks: no other fused kernel reads their descriptor
  if (c->dbg) return 0;
  if (s.wave_kernel && J.bs >= 3) return 3;
  if (s.rows_kernel) return 2;
  if (park_serves(s, J.bs)) return 1;   // (ilu_schedule.hpp: the rule the col16 tables are built by)
  return 0;
}
static bool kind_composes(int kind) { return kind >= 1 && kind <= 3; }
bool pc_axpy_capable(const wai_ctx* c, const Bcsr& M) { return !c->ilu.big && kind_composes(pc_kernel_kind(c, M, c->ilu)); }
bool pc_axpy_default(const wai_ctx* c, const Bcsr& M) {
  if (c->ilu.big) return false;
  const int kind = pc_kernel_kind(c, M, c->ilu);
  return (kind == 1 && c->ilu.col16 && !c->env.no_col16) || kind == 3;   // k_pc_park on col16, k_pc_wave: measured faster end to end
}

template <int BS>
static void launch_pc_bs(wai_ctx* c, const Bcsr& J, const IluSchedule& s, bool spmv, const double* in, double* z,
                         int dot_mode, const double* aux, const int* list, int nrun, const Fin* finp, const double* in2,
                         const Bcsr* F, const int* row_map) {
  // the launch list asked for, as the packed groups number them (0 all subdomains, 1 sub_int, 2 sub_bnd; -1: some other list)
  const int which = !list ? 0 : (list == s.sub_int ? 1 : (list == s.sub_bnd ? 2 : -1));
  if (!list) { nrun = s.nsub; list = s.sub_order; }   // all subdomains: in the schedule's launch order, if it has one
  const bool with_fin = finp && dot_mode != 0;
  Fin fin;
  if (finp && dot_mode != 0) { fin = *finp; fin.count = nrun; fin.nb = s.nsub; fin.nf = fin_slices(s.nsub); }   // all subdomains' partials are summed
  c->ks.n_launch++;
  const int grid = ((nrun + 7) / 8) * 8 + (with_fin ? fin.nf : 0), T = pc_threads(s);   // + the finalisers (fin_block)
  const size_t lds = ((size_t)T * BS + 80) * sizeof(double);
  // the (SPMV, AX) pairs the composing kernels are built for: (true, true), (true, false), (false, false)
  auto sp_ax = [&](auto&& go) {
    if (spmv) with_flag(in2 != nullptr, [&](auto ax) { go(std::true_type{}, ax); });
    else go(std::false_type{}, std::false_type{});
  };
  const int kind = pc_kernel_kind(c, J, s);
  const double* scal = c->ks.scal;
  const int* rp = (size_t)J.nnzb * 10 < (size_t)J.n * J.W * 9 ? J.rowptr : nullptr;   // > 10 % padding
  if (kind == 4) {
    // the filled ILU(k) factor of 1 x 1 and 2 x 2 blocks whose rows have at most NSB lower and NSB upper in-brick blocks (ILU(1)
    // of a 7-point stencil: 6 + 6): both sweeps on blocks staged in registers, nothing parked
    constexpr int NSB = BS == 1 ? 8 : (BS == 2 ? 6 : 0);
    // PCASM's extended ILU(0) factor of 2 x 2 blocks has 3 + 3 in-block couplings per row: staged on 3 slots it keeps two
    // 1024-thread workgroups on a CU where the 6-slot form's registers allow one
    if constexpr (BS == 2) {
      if (F && row_map && s.max_nlu <= 3) {
        with_flag(spmv, [&](auto sp) {
          hipLaunchKernelGGL((k_pc_wide<2, decltype(sp)::value, true, 3, true>), grid, T, lds, c->stream, J.n, J.W, nrun, s.sub_ptr,
                             s.sub_nlev, s.row_infow, s.row_uoffw, J.col, rp, J.val, s.fval, in, z, aux, c->ks.partials, c->ks.nb_max,
                             dot_mode, 0, list, fin, F->col, F->n, row_map);
        });
        return;
      }
    }
    if constexpr (NSB > 0) {
      if (F && s.max_nlu <= NSB) {
        with_flag(spmv, [&](auto sp) {
          with_flag(row_map != nullptr, [&](auto map) {
            hipLaunchKernelGGL((k_pc_wide<BS, decltype(sp)::value, true, NSB, decltype(map)::value>), grid, T, lds, c->stream, J.n, J.W,
                               nrun, s.sub_ptr, s.sub_nlev, s.row_infow, s.row_uoffw, J.col, rp, J.val, s.fval, in, z, aux,
                               c->ks.partials, c->ks.nb_max, dot_mode, 0, list, fin, F->col, F->n, row_map);
          });
        });
        return;
      }
    }
    // rows of 9 .. 16 blocks (or the unstaged filled factor): parked upper blocks within the 64 KB a workgroup may ask for
    const size_t room = (size_t)64 * 1024 > lds ? (size_t)64 * 1024 - lds : 0;
    const int ucap = (int)std::min((size_t)s.max_ublocks_w, room / ((size_t)BS * BS * sizeof(double)));
    const size_t lds_w = lds + (size_t)ucap * BS * BS * sizeof(double);
    // (F: the filled ILU(k) factor on its own column planes, the operator on J's narrow rows; row_map: PCASM's extended
    // system -- F's rows are the overlapped blocks', mapped to the operator's by row_map)
    auto wide = [&](auto sp, auto fill, auto map) {
      hipLaunchKernelGGL((k_pc_wide<BS, decltype(sp)::value, decltype(fill)::value, 0, decltype(map)::value>), grid, T, lds_w, c->stream,
                         J.n, J.W, nrun, s.sub_ptr, s.sub_nlev, s.row_infow, s.row_uoffw, J.col, rp, J.val, s.fval, in, z, aux,
                         c->ks.partials, c->ks.nb_max, dot_mode, ucap, list, fin, F ? F->col : J.col, F ? F->n : J.n, row_map);
    };
    with_flag(spmv, [&](auto sp) {
      if (F && row_map) wide(sp, std::true_type{}, std::true_type{});
      else with_flag(F != nullptr, [&](auto fill) { wide(sp, fill, std::false_type{}); });
    });
    return;
  }
  // one wave per brick of <= 64 block rows (block sizes 3 and 4), four bricks per workgroup
  if (kind == 3) {
    if constexpr (BS >= 3) {
      // one partial sum per WORKGROUP (four bricks) and slot: the face bricks' launch of the overlapped halo exchange
      // continues the interior bricks' indices, and its finalisers sum both
      const int ngrp = (nrun + 3) / 4;
      const int pbase = (list && list == s.sub_bnd) ? (s.n_int + 3) / 4 : 0, nb_w = pbase + ngrp;
      if (with_fin) { fin.nb = nb_w; fin.nf = fin_slices(nb_w); }
      c->ks.nb_pc = nb_w;
      const int gridw = ((ngrp + 7) / 8) * 8 + (with_fin ? fin.nf : 0);
      const int per = 64 * BS + s.max_ublocks_w * BS * BS;            // doubles per brick: solution + parked upper blocks
      const size_t lds_w = (size_t)4 * per * sizeof(double);
      Stagger stagger;
      stagger.ncu = c->n_cu;
      stagger.per_cu = std::max(1, (int)((size_t)160 * 1024 / (lds_w + 864)));
      stagger.ticks = 400;   // ticks of the 100-MHz clock between the cohorts (stagger_start)
      sp_ax([&](auto sp, auto ax) {
        hipLaunchKernelGGL((k_pc_wave<BS, decltype(sp)::value, decltype(ax)::value>), gridw, 256, lds_w, c->stream, J.n, J.W, nrun,
                           s.sub_ptr, s.sub_nlev, s.row_info, s.row_uoffw, J.col, s.fval, s.dinv, in, in2, scal, z, aux, c->ks.partials,
                           c->ks.nb_max, dot_mode, list, rp, s.sub_split, per, pbase, fin, stagger);
      });
      return;
    }
  }
  // one thread per scalar row: block sizes 3 and 4 (and 2 when asked for: WAI_PC_ROWS=1)
  if (kind == 2) {
    const int TR = ((s.max_rows * BS + 63) / 64) * 64;
    const size_t lds_r = ((size_t)s.max_rows * BS + BS + 5 * 16 + 8) * sizeof(double);
    auto rows = [&](auto nlu) {   // couplings per sweep held in registers: 3 or 4
      sp_ax([&](auto sp, auto ax) {
        constexpr int NLU = decltype(nlu)::value;
        hipLaunchKernelGGL((k_pc_rows<BS, decltype(sp)::value, NLU, NLU, decltype(ax)::value>), grid, TR, lds_r, c->stream, J.n, J.W,
                           nrun, s.sub_ptr, s.sub_nlev, s.row_info, J.col, s.fval, s.dinv, in, in2, scal, z, aux, c->ks.partials,
                           c->ks.nb_max, dot_mode, list, rp, s.sub_split, fin);
      });
    };
    if (s.max_nlu <= 3) rows(std::integral_constant<int, 3>{});
    else rows(std::integral_constant<int, 4>{});
    return;
  }
  if constexpr (BS == 2) {
    // upper blocks parked in LDS: three resident workgroups per CU
    if (kind == 1) {
      const size_t lds_park = lds + (size_t)s.max_ublocks * 4 * sizeof(double);
      Stagger stagger;
      stagger.ncu = c->n_cu;
      stagger.per_cu = std::max(1, std::min(3, (int)((size_t)160 * 1024 / (lds_park + 704))));
      stagger.ticks = 600;
      const bool on16 = s.col16 && !c->env.no_col16;
      // on col16 the descriptors come from the shared templates (IluSchedule::sub_desc), or -- WAI_NO_DESC_SHARE -- from the
      // per-row arrays through the same indexing: a brick's first row is its template's
      const bool shared = on16 && s.sub_desc && !c->env.no_desc_share;
      const int* d_info = shared ? s.t_info.get() : s.row_info.get();
      const int* d_uoff = shared ? s.t_uoff.get() : s.row_uoff.get();
      const unsigned short* d_c16 = shared ? s.t_col16.get() : s.col16.get();
      const int* d_desc = shared ? s.sub_desc.get() : s.sub_ptr.get();
      // the operator on col16 with shared descriptors may stage its operand (park_staged); the plain application never does
      const bool stage = shared && spmv && park_staged(c, in2 != nullptr);
      auto staged = [&](auto pack, int g, int count, const int* lst) {
        with_flag(in2 != nullptr, [&](auto ax) {
          hipLaunchKernelGGL((k_pc_park<true, decltype(ax)::value, true, decltype(pack)::value, true>), g, T, lds_park, c->stream,
                             J.n, J.W, count, s.sub_ptr, s.sub_nlev, d_desc, d_info, d_uoff, J.col, d_c16, s.sub_seg, s.fval, s.dinv,
                             in, in2, scal, z, aux, c->ks.partials, c->ks.nb_max, dot_mode, lst, fin, stagger);
        });
      };
      // short bricks sharing workgroups (col16 with shared descriptors only): the list's groups instead of its bricks.  Each
      // brick still leaves its own partial, so the finalisers and fin.nb stay what they are; WAI_NO_PACK: one workgroup per brick
      if (shared && which >= 0 && s.pack_tab[which] && !c->env.no_pack) {
        const int ngrp = s.n_groups[which], gridp = ((ngrp + 7) / 8) * 8 + (with_fin ? fin.nf : 0);
        if (stage) { staged(std::true_type{}, gridp, ngrp, s.pack_tab[which].get()); return; }
        sp_ax([&](auto sp, auto ax) {
          hipLaunchKernelGGL((k_pc_park<decltype(sp)::value, decltype(ax)::value, true, true>), gridp, T, lds_park, c->stream,
                             J.n, J.W, ngrp, s.sub_ptr, s.sub_nlev, d_desc, d_info, d_uoff, J.col, d_c16, s.sub_seg, s.fval, s.dinv,
                             in, in2, scal, z, aux, c->ks.partials, c->ks.nb_max, dot_mode, s.pack_tab[which].get(), fin, stagger);
        });
        return;
      }
      if (stage) { staged(std::false_type{}, grid, nrun, list); return; }
      with_flag(on16, [&](auto c16) {
        sp_ax([&](auto sp, auto ax) {
          hipLaunchKernelGGL((k_pc_park<decltype(sp)::value, decltype(ax)::value, decltype(c16)::value>), grid, T, lds_park, c->stream,
                             J.n, J.W, nrun, s.sub_ptr, s.sub_nlev, d_desc, d_info, d_uoff, J.col, d_c16, s.sub_seg, s.fval, s.dinv,
                             in, in2, scal, z, aux, c->ks.partials, c->ks.nb_max, dot_mode, list, fin, stagger);
        });
      });
      return;
    }
  }
  auto generic = [&](auto di) {   // 0 stored factor, 1 DILU, 2 DILU on rows pre-scaled by the inverted pivots
    with_flag(spmv, [&](auto sp) {
      with_flag(s.fast3, [&](auto fast) {
        hipLaunchKernelGGL((k_pc<BS, decltype(sp)::value, decltype(di)::value, decltype(fast)::value>), grid, T, lds, c->stream,
                           J.n, J.W, nrun, s.sub_ptr, s.sub_nlev, s.row_info, J.col, J.val, s.fval, s.dinv, in, z, aux,
                           c->ks.partials, c->ks.nb_max, dot_mode, c->dbg, list, fin);
      });
    });
  };
  if (s.diag_only && s.scaled) generic(std::integral_constant<int, 2>{});
  else if (s.diag_only) generic(std::integral_constant<int, 1>{});
  else generic(std::integral_constant<int, 0>{});
}

int launch_pc_on(wai_ctx* c, const Bcsr& M, const IluSchedule& s, bool spmv, const double* in, double* z,
                 int dot_mode, const double* aux, const int* list, int nrun, const Fin* fin, const double* in2, const Bcsr* F,
                 const int* row_map) {
  if (F && (!s.wide || M.dg || M.W > WMAX || (!row_map && F->n != M.n) || F->bs != M.bs)) { c->err = "a factor pattern of its own asked of a kernel that has none"; return -1; }
  if (row_map && !F) { c->err = "a row map without a factor pattern of its own"; return -1; }
  if (row_map && z == in) { c->err = "the fused PCASM application cannot run in place: a block reads rows another block writes"; return -1; }
  if (in2 && (!spmv || !kind_composes(pc_kernel_kind(c, M, s)))) { c->err = "composed input asked of a kernel that cannot form it"; return -1; }
  const Fin* fin_later = nullptr;
  if (fin && dot_mode != 0 && c->env.fin_separate) { fin_later = fin; fin = nullptr; }
  if (M.dg) {
    // the coupled tracer system: the brick kernel reduces nothing; the dot mode's products of the result come from the vector
    // kernels (their partial sums in ks.nb_pc blocks per slot) and are finished as the general path finishes them
    c->ks.n_launch++;
    if (launch_dg_pc(c, M, s, spmv, in, z, list, nrun)) return -1;
    if (dot_mode == PC_DOT_NONE) return 0;
    const int n = M.dg * M.n, s0 = pc_dot_slot0(dot_mode);
    if (dot_mode == PC_DOT_ZA || dot_mode == PC_DOT_ZZ) vec_dots(c, z, dot_mode == PC_DOT_ZA ? aux : z, s0, nullptr, nullptr, 0, n);
    else {
      vec_dots(c, in, z, s0, z, z, s0 + 1, n);
      if (dot_mode == PC_DOT_MERGED) { vec_dots(c, in, in, s0 + 2, in, aux, s0 + 3, n); vec_dots(c, z, aux, s0 + 4, nullptr, nullptr, 0, n); }
    }
    if (const Fin* f = fin ? fin : fin_later) {   // separate launches either way (WAI_FIN_SEPARATE changes nothing here)
      if (dot_mode == PC_DOT_MERGED) { vec_finalize(c, c->ks.nb_pc, s0, 4, -1); vec_finalize(c, c->ks.nb_pc, s0 + 4, 1, f->phase); }
      else vec_finalize(c, c->ks.nb_pc, s0, pc_dot_nslots(dot_mode), f->phase);
      if (f->seq > 0) bcgs_post(c, f->seq);
    }
    return 0;
  }
  c->ks.nb_pc = s.nsub;   // partial sums per slot this application leaves: one per brick (k_pc_wave: per workgroup, set there)
  if (with_bs(M.bs, [&](auto bs) { launch_pc_bs<decltype(bs)::value>(c, M, s, spmv, in, z, dot_mode, aux, list, nrun, fin, in2, F, row_map); }) != 0)
    return -1;
  if (fin_later) {
    vec_finalize(c, c->ks.nb_pc, fin_later->slot0, fin_later->nslots, fin_later->phase);
    if (fin_later->seq > 0) bcgs_post(c, fin_later->seq);
  }
  return 0;
}
// The multicolour ordering's fused launch (k_pc_colour; ColourSchedule::fused says whether it serves): one workgroup per
// subdomain on the matrix' own planes, the inverted pivots from s.dinv; partial sums and finalisers as launch_pc_on's
bool pc_colour_serves(const wai_ctx* c, const Bcsr& M, const ColourSchedule& k, bool one_rank) {
  const int T = ((k.max_rows + 63) / 64) * 64;
  return k.built && k.diag_only && !M.dg && M.W <= WMAX && k.max_blocks <= WMAX && M.bs >= 1 && M.bs <= 4 && T <= pc_colour_threads(M.bs) &&
         one_rank && !c->env.colour_sweeps;
}
int launch_pc_colour(wai_ctx* c, const Bcsr& M, const ColourSchedule& k, const IluSchedule& s, bool spmv, const double* in, double* z,
                     int dot_mode, const double* aux, const Fin* finp) {
  if (!k.fused) { c->err = "launch_pc_colour: the colour schedule is not served by the fused launch"; return -1; }
  const Fin* fin_later = nullptr;
  if (finp && dot_mode != 0 && c->env.fin_separate) { fin_later = finp; finp = nullptr; }
  const bool with_fin = finp && dot_mode != 0;
  Fin fin;
  if (with_fin) { fin = *finp; fin.count = k.nsub; fin.nb = k.nsub; fin.nf = fin_slices(k.nsub); }
  c->ks.nb_pc = k.nsub;   // one partial sum per subdomain and slot
  c->ks.n_launch++;
  const int grid = ((k.nsub + 7) / 8) * 8 + (with_fin ? fin.nf : 0), T = ((k.max_rows + 63) / 64) * 64;
  if (with_bs(M.bs, [&](auto bs) {
        constexpr int BS = decltype(bs)::value;
        const size_t lds = ((size_t)T * BS + 80) * sizeof(double);
        with_flag(spmv, [&](auto sp) {
          hipLaunchKernelGGL((k_pc_colour<BS, decltype(sp)::value>), grid, T, lds, c->stream, M.n, M.W, k.nsub, k.sub_ptr, k.sub_ncol,
                             k.slots, k.counts, M.col, M.val, s.dinv, in, z, aux, c->ks.partials, c->ks.nb_max, dot_mode, nullptr, fin);
        });
      }) != 0)
    return -1;
  if (fin_later) {
    vec_finalize(c, c->ks.nb_pc, fin_later->slot0, fin_later->nslots, fin_later->phase);
    if (fin_later->seq > 0) bcgs_post(c, fin_later->seq);
  }
  return 0;
}

int launch_pc(wai_ctx* c, const Bcsr& M, bool spmv, const double* in, double* z, int dot_mode, const double* aux,
              const int* list, int nrun, const Fin* fin, const double* in2) {
  return launch_pc_on(c, M, c->ilu, spmv, in, z, dot_mode, aux, list, nrun, fin, in2);
}
Fin make_fin(wai_ctx* c, int slot0, int nslots, int phase, bool post) {
  Fin f;   // count / nb: filled in by the launcher
  f.slot0 = slot0; f.nslots = nslots; f.phase = phase;
  f.scal = c->ks.scal; f.post = c->ks.d_post; f.part2 = c->ks.partials2;
  f.seq = post ? ++c->ks.seq : 0;
  return f;
}

int vec_finalize(wai_ctx* c, int nb, int slot0, int nslots, int phase) {
  const int T = nb > 256 ? 1024 : 256;
  c->ks.n_launch++;
  hipLaunchKernelGGL(k_finalize, 1, T, 0, c->stream, c->ks.partials, c->ks.nb_max, nb, slot0, nslots, c->ks.scal, phase);
  return 0;
}

int vec_dot(wai_ctx* c, const double* a, const double* b, int n, int slot) {
  const int g = vgrid(n);
  c->ks.n_launch++;
  hipLaunchKernelGGL(k_dot, g, TPB, 0, c->stream, a, b, n, c->ks.partials, c->ks.nb_max, slot);
  return vec_finalize(c, g, slot, 1, -1);
}
int vec_dots(wai_ctx* c, const double* a1, const double* b1, int slot1, const double* a2, const double* b2,
             int slot2, int n) {
  const int g = vgrid(n);
  c->ks.n_launch++;
  hipLaunchKernelGGL(k_dots, g, TPB, 0, c->stream, a1, b1, slot1, a2, b2, slot2, n, c->ks.partials, c->ks.nb_max);
  c->ks.nb_pc = g;
  return 0;
}
int partials_clear(wai_ctx* c, int slot0, int nslots) {
  const size_t tot = (size_t)nslots * std::max(c->ks.nb_max, (int)FIN_MAXF);   // both arrays: the slices' sums too
  c->ks.n_launch++;
  hipLaunchKernelGGL(k_partials_clear, (int)((tot + TPB - 1) / TPB), TPB, 0, c->stream, c->ks.partials, c->ks.partials2, c->ks.nb_max, slot0, nslots);
  return 0;
}
int vec_copy(wai_ctx* c, double* dst, const double* src, size_t n) {
  c->ks.n_copy++;
  return hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream) == hipSuccess ? 0 : -1;
}
int vec_zero(wai_ctx* c, double* dst, size_t n) {
  return hipMemsetAsync(dst, 0, n * sizeof(double), c->stream) == hipSuccess ? 0 : -1;
}
int vec_waxpy(wai_ctx* c, double* w, double alpha, const double* x, const double* y, int n) {
  c->ks.n_launch++;
  hipLaunchKernelGGL(k_waxpy, vgrid(n), TPB, 0, c->stream, w, alpha, x, y, n);
  return 0;
}
int bcgs_scalars(wai_ctx* c, int phase, bool post) {
  c->ks.n_launch++;
  hipLaunchKernelGGL(k_bcgs_scalars, 1, 64, 0, c->stream, c->ks.scal, phase, c->ks.d_post, post ? ++c->ks.seq : 0);
  return 0;
}
int test_drop_partials(wai_ctx* c, int n) {
  return hipMemcpyToSymbolAsync(HIP_SYMBOL(g_drop_partials), &n, sizeof(int), 0, hipMemcpyHostToDevice, c->stream) == hipSuccess &&
         hipStreamSynchronize(c->stream) == hipSuccess ? 0 : -1;
}
int bcgs_post(wai_ctx* c, int seq) {   // the device scalars as they stand, under a sequence number already handed out
  c->ks.n_launch++;
  hipLaunchKernelGGL(k_bcgs_scalars, 1, 64, 0, c->stream, c->ks.scal, -1, c->ks.d_post, seq);
  return 0;
}

int bcgs_update_p(wai_ctx* c, const KrylovVecs& k, int n) {
  c->ks.n_launch++;
  hipLaunchKernelGGL(k_bcgs_p, vgrid(n), TPB, 0, c->stream, k.P, k.R, k.V, n, c->ks.scal);
  return 0;
}
int bcgs_update_s(wai_ctx* c, const KrylovVecs& k, int n) {
  c->ks.n_launch++;
  hipLaunchKernelGGL(k_bcgs_s, vgrid(n), TPB, 0, c->stream, k.S, k.R, k.V, n, c->ks.scal);
  return 0;
}
int bcgs_update_xr(wai_ctx* c, const KrylovVecs& k, int n, bool dots, int fin_phase, bool post) {
  const int g = vgrid(n);
  Fin fin;
  if (dots && fin_phase >= -1) { fin = make_fin(c, S_DP2, 2, fin_phase, post); fin.count = g; fin.nb = g; fin.nf = fin_slices(g); }
  c->ks.n_launch++;
  if (dots && fin.count > 0 && c->env.fin_separate) {
    Fin none;
    hipLaunchKernelGGL(k_bcgs_xr<true>, g, TPB, 0, c->stream, k.X, k.R, k.P, k.S, k.T,
                       k.RP, n, c->ks.scal, c->ks.partials, c->ks.nb_max, none);
    c->ks.nblocks = g;
    vec_finalize(c, g, S_DP2, 2, fin_phase);
    if (fin.seq > 0) bcgs_post(c, fin.seq);
    return 0;
  }
  if (dots)
    hipLaunchKernelGGL(k_bcgs_xr<true>, g + (fin.count > 0 ? fin.nf : 0), TPB, 0, c->stream, k.X, k.R, k.P, k.S, k.T,
                       k.RP, n, c->ks.scal, c->ks.partials, c->ks.nb_max, fin);
  else
    hipLaunchKernelGGL(k_bcgs_xr<false>, g, TPB, 0, c->stream, k.X, k.R, k.P, k.S, k.T,
                       k.RP, n, c->ks.scal, c->ks.partials, c->ks.nb_max, fin);
  c->ks.nblocks = g;
  return 0;
}
int bcgs_update_xrp(wai_ctx* c, const KrylovVecs& k, int n) {
  c->ks.n_launch++;
  hipLaunchKernelGGL(k_bcgs_xrp<false>, vgrid(n), TPB, 0, c->stream, k.X, k.R, k.P, k.V, k.T, n,
                     c->ks.scal, nullptr, nullptr, 0);
  return 0;
}
// the same launch deriving omega, (R,R), rho, beta from the all-reduced sums itself and posting the norm (several ranks)
int bcgs_update_xrp_derive(wai_ctx* c, const KrylovVecs& k, int n) {
  c->ks.n_launch++;
  hipLaunchKernelGGL(k_bcgs_xrp<true>, vgrid(n), TPB, 0, c->stream, k.X, k.R, k.P, k.V, k.T, n,
                     c->ks.scal, c->ks.started, c->ks.d_post, ++c->ks.seq);
  return 0;
}
int gmres_mdot(wai_ctx* c, const double* basis, size_t ld, int n, const double* w, int k) {
  const int g = vgrid(n);
  for (int j0 = 0; j0 < k; j0 += 8) {
    const int cnt = (k - j0) < 8 ? (k - j0) : 8;
#define MD(CNT) hipLaunchKernelGGL(k_mdot<CNT>, g, TPB, 0, c->stream, w, basis, ld, j0, n, c->ks.partials, c->ks.nb_max)
    c->ks.n_launch++;
    switch (cnt) { case 1: MD(1); break; case 2: MD(2); break; case 3: MD(3); break; case 4: MD(4); break;
                   case 5: MD(5); break; case 6: MD(6); break; case 7: MD(7); break; default: MD(8); break; }
#undef MD
    vec_finalize(c, g, S_H + j0, cnt, -1);   // k_finalize sums any number of slots (five at a time) in one launch
  }
  return 0;
}
int gmres_maxpy_norm(wai_ctx* c, const double* basis, size_t ld, int n, double* w, int k) {
  const int g = vgrid(n);
  hipLaunchKernelGGL(k_maxpy_norm, g, TPB, 0, c->stream, w, basis, ld, k, n,
                     c->ks.scal, c->ks.partials, c->ks.nb_max);
  return vec_finalize(c, g, S_W2, 1, -1);
}
int gmres_scale_to(wai_ctx* c, double* dst, const double* src, int slot_norm2, int n) {
  hipLaunchKernelGGL(k_scale_to, vgrid(n), TPB, 0, c->stream, dst, src, c->ks.scal, slot_norm2, n);
  return 0;
}
int gmres_update_x(wai_ctx* c, const double* basis, size_t ld, int n, double* x, const double* ycoef_host, int k) {
  double* dcoef = c->ks.scal + 64;  // coefficients travel through the tail of the scalar buffer
  hipMemcpyAsync(dcoef, ycoef_host, sizeof(double) * k, hipMemcpyHostToDevice, c->stream);
  hipLaunchKernelGGL(k_update_x, vgrid(n), TPB, 0, c->stream, x, basis, ld, k, n, dcoef);
  return 0;
}
int pack_halo(wai_ctx* c, const double* vec, int dof, hipStream_t stream) {
  const int n = c->send_total;
  if (n <= 0) return 0;
  c->ks.n_launch++;
  hipLaunchKernelGGL(k_pack, (n * dof + TPB - 1) / TPB, TPB, 0, stream ? stream : c->stream, vec, c->d_send_idx, n,
                     dof, c->d_sendbuf);
  return 0;
}
int pack_halo_axpy(wai_ctx* c, const double* a, const double* b, int dof, hipStream_t stream) {
  const int n = c->send_total;
  if (n <= 0) return 0;
  c->ks.n_launch++;
  with_flag(c->ks.alpha_pending, [&](auto derive) {
    hipLaunchKernelGGL(k_pack_axpy<decltype(derive)::value>, (n * dof + TPB - 1) / TPB, TPB, 0, stream ? stream : c->stream, a, b,
                       c->ks.scal, c->d_send_idx, n, dof, c->d_sendbuf);
  });
  c->ks.alpha_pending = false;
  return 0;
}
int unpack_halo(wai_ctx* c, double* vec, int dof, hipStream_t stream) {
  // halo cells are contiguous after the owned cells and the receive buffer is in halo order
  const size_t n = (size_t)c->mesh.n_halo * dof;
  if (n == 0) return 0;
  c->ks.n_copy++;
  return hipMemcpyAsync(vec + (size_t)c->mesh.n_owned * dof, c->d_recvbuf, n * sizeof(double),
                        hipMemcpyDeviceToDevice, stream ? stream : c->stream) == hipSuccess ? 0 : -1;
}

}  // namespace wai

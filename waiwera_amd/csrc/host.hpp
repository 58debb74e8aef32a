// Host-side internals of libwaiwera_hip.so shared by its translation units (capi.hip: the ode_type hooks and the Newton
// iteration; context.hip: the context and its set-up; sources.hip: sources and their controls; tracers.hip: the tracer
// problem; pc_setup.hip: symbolic phases -- made on the host alone by ilu_schedule.hpp and asm_pattern.hpp, which
// tests/pc_setup_host runs without a device, and uploaded there -- and factorisations; krylov.hip: the Krylov drivers and
// the preconditioned operator; network.hip: the source network; measure.hip: measurement entry points).  Not part of the ABI.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <numeric>
#include "comm.hpp"
#include "context.hpp"
#include "../../include/waiwera_hip_bench.h"

namespace wai {

constexpr int NSLOTS = 64;
constexpr int NSCAL = 128;

// GMRES / LGMRES basis: restart vectors, at least 3 (LGMRES: one Krylov direction + 2 error approximations),
// at most MAX_RESTART (the Hessenberg column travels through the scalar / partial-sum slots S_H ..)
constexpr int MAX_RESTART = 40;
constexpr int BCGSL_VECS = 7;   // BiCGStab(2): r_0..r_2, u_0..u_2, r~ (KrylovVecs::bl)
inline int basis_vectors(int restart) { return std::max(3, std::min(restart > 0 ? restart : 30, MAX_RESTART)); }

inline bool is_device_ptr(const void* p) {
  hipPointerAttribute_t a;
  hipError_t e = hipPointerGetAttributes(&a, p);
  if (e != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

// The one place that decides a copy's direction.  One side is the caller's vector -- device or host memory, asked of the
// runtime -- the other the library's device memory: n doubles on the context's stream, not synchronised.
enum CopyDir { FROM_CALLER, TO_CALLER };
inline int copy_vec(wai_ctx* c, double* dst, const double* src, size_t n, CopyDir dir, bool caller_on_device) {
  const hipMemcpyKind kind = caller_on_device ? hipMemcpyDeviceToDevice : (dir == TO_CALLER ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice);
  HIPCHK(c, hipMemcpyAsync(dst, src, n * sizeof(double), kind, c->stream));
  return 0;
}
inline int copy_vec(wai_ctx* c, double* dst, const double* src, size_t n, CopyDir dir) {
  return copy_vec(c, dst, src, n, dir, is_device_ptr(dir == TO_CALLER ? dst : src));
}

// the device flags' rest state (fetch_flags): flag 1 is a minimum
inline constexpr int FLAGS_RESET[4] = {0, 0x7fffffff, 0, 0};

// vector argument handling: device pointers pass through, host arrays are staged (asked once: the staged side is host memory)
struct VecArg {
  wai_ctx* c; double* dev = nullptr; double* host = nullptr; size_t n = 0; bool staged = false;
  int in(const double* p, size_t n_, int slot) {
    n = n_;
    if (!p) { dev = nullptr; return 0; }
    if (is_device_ptr(p)) { dev = const_cast<double*>(p); return 0; }
    if (n > c->stage_len) { c->err = "vector longer than staging buffer"; return -1; }
    host = const_cast<double*>(p); dev = c->stage[slot]; staged = true;
    return copy_vec(c, dev, p, n, FROM_CALLER, false);
  }
  int out_only(double* p, size_t n_, int slot) {
    n = n_;
    if (!p) { dev = nullptr; return 0; }
    if (is_device_ptr(p)) { dev = p; return 0; }
    if (n > c->stage_len) { c->err = "vector longer than staging buffer"; return -1; }
    host = p; dev = c->stage[slot]; staged = true;
    return 0;
  }
  int back() {
    if (staged && host) {
      if (copy_vec(c, host, dev, n, TO_CALLER, false)) return -1;
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return 0;
  }
};

struct Prof {
  wai_ctx* c; int k;
  Prof(wai_ctx* c_, int k_) : c(c_), k(k_) {
    if (c->prof_on) (void)hipEventRecord(c->pev0, c->stream);
  }
  ~Prof() {
    if (c->prof_on) {
      (void)hipEventRecord(c->pev1, c->stream);
      (void)hipEventSynchronize(c->pev1);
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, c->pev0, c->pev1);
      c->prof_ms[k] += ms;
      c->prof_n[k] += 1;
    }
  }
};

// the source network's blocks E are part of the system's operator in force: A + E (the flow Jacobian's only)
inline bool net_in_operator(const wai_ctx* c, const LinSys& sys) { return sys.net_blocks && c->net.cp_valid; }
// which preconditioner path is in force for a system: the fused brick kernels (block Jacobi, every subdomain
// <= 1024 rows) or the general one (PCASM's extended system, subdomains of any size, PCNONE)
// the source network's blocks are part of the operator in force AND go into the factor's pattern (one rank)
inline bool pc_with_net(const wai_ctx* c, const LinSys& sys) { return net_in_operator(c, sys) && c->net.cp_in_pc && !c->net.cp_span; }
// the preconditioner settings in force for a system: its own (wai_set_aux_pc) or, when it follows, the flow solver's
inline PcOpts pc_of(const wai_ctx* c, const LinSys& sys) {
  if (sys.pc.type != WAI_AUX_PC_FOLLOW) return sys.pc;
  PcOpts p;
  p.type = c->opts.pc_type; p.asm_overlap = c->opts.asm_overlap; p.ilu_levels = c->opts.ilu_levels; p.sub = c->sub_pc;
  return p;
}
// sub-preconditioner lu is in force (wai_set_sub_pc; it acts under bjacobi and asm alone, and ilu_levels is ignored then)
inline bool pc_sub_lu(const PcOpts& p) { return p.sub == WAI_SUB_LU && (p.type == WAI_PC_BJACOBI || p.type == WAI_PC_ASM); }
// block-Jacobi ILU(k), k > 0, on the flow system, applied by ONE launch: the set-up in force built the filled factor on a
// wide schedule (AsmSystem::fused -- fill of <= 16 blocks per row, subdomains of <= 1024 rows, one rank, no network
// blocks); k_pc_wide's two-pattern form then serves pc_amul / pc_solve (launch_pc_sys, krylov.hip)
inline bool pc_fill_fused(const wai_ctx* c, const LinSys& sys) {
  const PcOpts p = pc_of(c, sys);
  const AsmSystem& a = sys.as;
  return &sys == &c->flow && p.type == WAI_PC_BJACOBI && p.ilu_levels > 0 && !pc_with_net(c, sys) && !pc_sub_lu(p) &&
         a.fused && a.overlap == 0 && a.levels == p.ilu_levels && a.sched.wide;
}
// PCASM (any overlap, sub-preconditioner ILU(k), k >= 0) on the flow system, applied by ONE launch: the set-up in force put
// the extended system on a wide schedule (AsmSystem::fused -- extended blocks of <= 1024 rows, rows of E of <= 16 blocks,
// one rank, no network blocks, WAI_ASM_UNFUSED unset); k_pc_wide's two-pattern form with a row map serves it
inline bool pc_asm_fused(const wai_ctx* c, const LinSys& sys) {
  const PcOpts p = pc_of(c, sys);
  const AsmSystem& a = sys.as;
  return &sys == &c->flow && p.type == WAI_PC_ASM && !pc_with_net(c, sys) && !pc_sub_lu(p) && a.fused && a.overlap > 0 &&
         a.overlap == (p.asm_overlap > 0 ? p.asm_overlap : 1) && a.levels == (p.ilu_levels > 0 ? p.ilu_levels : 0) &&
         !a.cross && a.sched.wide;
}
// either: the factor has a pattern of its own (sys.as.E on sys.as.sched) -- no composed operand, no interior / face split
inline bool pc_own_factor(const wai_ctx* c, const LinSys& sys) { return pc_fill_fused(c, sys) || pc_asm_fused(c, sys); }
// block-Jacobi ILU(0) in multicolour order is in force for `sys` (wai_set_pc_ordering): the flow system's alone, where the
// set-up does not refuse the combination (do_pc_setup); the tracer systems keep the natural order.  Its factor is the stored
// one on the matrix' own planes (wai_ctx::ilu's buffers), its tables wai_ctx::colour's; one fused launch (k_pc_colour) applies it
// where ColourSchedule::fused says so, pc_solve's launch-per-colour sweeps everywhere else
inline bool pc_colour(const wai_ctx* c, const LinSys& sys) {
  const PcOpts p = pc_of(c, sys);
  return c->pc_ordering == WAI_PC_ORDER_MULTICOLOUR && &sys == &c->flow && p.type == WAI_PC_BJACOBI && p.ilu_levels <= 0 &&
         !pc_sub_lu(p) && !pc_with_net(c, sys);
}
inline bool pc_fused(const wai_ctx* c, const LinSys& sys) {
  const PcOpts p = pc_of(c, sys);
  if (pc_colour(c, sys)) return c->colour.fused;   // k_pc_colour, or the launch-per-colour path: the unfused branches of pc_amul and pc_solve
  if (pc_own_factor(c, sys)) return true;
  return p.type == WAI_PC_BJACOBI && !c->ilu.big && p.ilu_levels <= 0 && !pc_with_net(c, sys) && !pc_sub_lu(p);
}
// the extended-system path: PCASM's overlapped row sets and / or ILU(k)'s filled pattern and / or the network's blocks
inline bool pc_extended(const wai_ctx* c, const LinSys& sys) {
  const PcOpts p = pc_of(c, sys);
  return p.type == WAI_PC_ASM || (p.type == WAI_PC_BJACOBI && (p.ilu_levels > 0 || pc_with_net(c, sys) || pc_sub_lu(p)));
}
// the two-level preconditioner's coarse level is in force for `sys` (wai_set_pc_coarse): the flow system's alone.  The system
// then takes the unfused route -- pc_amul computes t = A x and calls pc_solve, which applies the one-level preconditioner and
// the coarse correction and reduces the inner products of the final z; no composed operand (pc_axpy_ok)
inline bool pc_coarse(const wai_ctx* c, const LinSys& sys) { return c->coarse.mode != WAI_PC_COARSE_OFF && &sys == &c->flow; }
// the preconditioner set up for `sys` no longer stands (its values changed); without a system: nobody's does
inline void pc_invalidate(wai_ctx* c, const LinSys& sys) { if (c->ilu.owner == &sys) c->ilu.owner = nullptr; }
inline void pc_invalidate(wai_ctx* c) { c->ilu.owner = nullptr; }

// ---- pc_setup.hip ------------------------------------------------------------------------------------------------
int build_schedule(wai_ctx* c, IluSchedule& s, const std::vector<int>& rowptr, const std::vector<int>& colidx,
                   const std::vector<int>& sub, int N, int W, int np, bool ghosts, bool allow_wide = true, bool sublu = false,
                   bool fill = false, const std::vector<int>* row_tile = nullptr);
int ensure_halo_dof(wai_ctx* c, int dof);   // halo buffers wide enough for `dof` doubles per cell
int do_pc_setup(wai_ctx* c, LinSys& sys);
// what the coarse level does not combine with, from the settings alone: null, or the party it met
const char* coarse_refusal(const wai_ctx* c, bool at_setup);
int coarse_upload(wai_ctx* c);    // the lists of c->coarse.h to the device, the matrices and work vectors allocated
// ---- krylov.hip --------------------------------------------------------------------------------------------------
int halo_exchange(wai_ctx* c, double* vec, int dof);
// the two launches of the overlapped halo exchange on the compute stream: interior bricks, then face bricks behind `after`
// (null: behind what the compute stream held when called)
int launch_pc_split(wai_ctx* c, const Bcsr& M, const double* x, double* z, int dot_mode, const double* aux, const Fin* fp, const double* x2,
                    hipEvent_t after);
int allreduce_scal(wai_ctx* c, int slot, int count);
int read_scal(wai_ctx* c, int first, int count);
int wait_post(wai_ctx* c, int seq);   // the scalars a launch posted under `seq`: h_scal[S_DP2], h_scal[S_BREAK]
// z = B^-1 r; dot_mode as launch_pc, with `x` the partner of mode 2.  fin_phase >= -1: the partial sums of the dot
// products are summed into the device scalars (and the BiCGStab scalars of that phase derived); -2: left as partials
int pc_solve(wai_ctx* c, LinSys& sys, const double* r, double* z, int dot_mode, const double* x, const double* aux, int fin_phase = -2);
// z = B^-1 A x (x has halo room); x2: the operand is x - alpha x2 (fused kernels); post: the scalars to the host
int pc_amul(wai_ctx* c, LinSys& sys, double* x, double* z, int dot_mode = PC_DOT_NONE, const double* aux = nullptr, int fin_phase = -2,
            const double* x2 = nullptr, bool post = false);
// launch_pc for a system on the fused path: the brick schedule's factor, the filled ILU(k) factor of pc_fill_fused, or
// PCASM's extended factor through its row map (pc_asm_fused)
int launch_pc_sys(wai_ctx* c, const LinSys& sys, bool spmv, const double* in, double* z, int dot_mode, const double* aux,
                  const int* list = nullptr, int nrun = 0, const Fin* fin = nullptr, const double* in2 = nullptr);
int do_ksp(wai_ctx* c, LinSys& sys, const double* b, double* x, int* its, int* reason, double* rnorm);
int bcgs_mode(const wai_ctx* c);
bool pc_axpy_ok(const wai_ctx* c, const LinSys& sys);
struct BcgsPlan { int mode; bool fused3, merged, axpy, multi; };
BcgsPlan bcgs_plan(const wai_ctx* c, const LinSys& sys);
int bcgs_first_half(wai_ctx* c, LinSys& sys, const BcgsPlan& pl);
int bcgs_second_half(wai_ctx* c, LinSys& sys, const BcgsPlan& pl);
// ---- network.hip -------------------------------------------------------------------------------------------------
// a control record's separator as the pass reads it: hf, hg of stage 1, then (hf, hg) of stages 2..4
inline void src_separator(const SrcCtl& k, double* sep8) {
  sep8[0] = k.sep_hf; sep8[1] = k.sep_hg;
  for (int q = 0; q < 6; q++) sep8[2 + q] = k.sep_more[q];
}
// the pass on the device is in force (wai_set_network_pass): asked for, one rank -- by the communicator's size alone, so
// every rank decides alike -- and a network whose description and state fit a workgroup's LDS
// The wave-wide walk (wai_set_network_walk) can run: asked for, one rank, and a network its schedule accepts.  It holds
// networks of up to 160 KiB on the device, where the lane walk stops at NET_LDS_DOUBLES
inline bool net_wave_usable(const wai_ctx* c) {
  return c->net_walk == WAI_NETWORK_WALK_WAVE && c->net.on && c->net.wave_ok && !(c->comm && c->comm->nranks > 1);
}
inline bool net_on_device(const wai_ctx* c) {
  return c->net_pass == WAI_NETWORK_PASS_DEVICE && c->net.on && (c->net.flat_fits || net_wave_usable(c)) &&
         !(c->comm && c->comm->nranks > 1);
}
// ... is in force: where the device pass is
inline bool net_walk_wave(const wai_ctx* c) { return net_wave_usable(c) && net_on_device(c); }
// Is the batched coupling build (wai_set_coupling_build) in force: asked for, the device pass in force, the couplings on
inline bool cp_batched(const wai_ctx* c) {
  return c->cp_build == WAI_COUPLING_BUILD_BATCHED && net_on_device(c) && c->net.coupling;
}
constexpr long long COUPLING_BATCH_BYTES = 256LL << 20;   // the most scratch one chunk of its columns takes (coupling_batch.hpp)
int network_update(wai_ctx* c);
int network_fetch_state(wai_ctx* c);       // what the last device pass kept to Network::h_state
int network_fetch_couplings(wai_ctx* c);   // the device-built coupling blocks to h_cp_val
int network_couplings(wai_ctx* c, double dt, double* y, const double* lhs_old);
int apply_operator(wai_ctx* c, const LinSys& sys, const double* x, double* t);   // t = A x, + E x where the source network's blocks belong to sys
// ---- context.hip -------------------------------------------------------------------------------------------------
int alloc_krylov_vecs(wai_ctx* c, KrylovVecs& k, size_t nl);
int ensure_basis(wai_ctx* c, LinSys& sys, int m);
int ensure_bcgsl_vecs(wai_ctx* c, KrylovVecs& k, size_t nl);
Bcsr matrix_on(const Pattern& p, int bs, double* val);
// ---- capi.hip ----------------------------------------------------------------------------------------------------
int fetch_flags(wai_ctx* c, int out[4]);
int do_pre_eval(wai_ctx* c, double* y);
int do_residual(wai_ctx* c, double dt, double* y, const double* lhs_old, double* f);
int do_jacobian(wai_ctx* c, double dt, const double* y, const double* lhs_old);

}  // namespace wai

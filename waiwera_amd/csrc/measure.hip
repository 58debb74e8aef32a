// Measurement and reporting entry points of libwaiwera_hip.so (include/waiwera_hip_bench.h; wai_pc_kernel_name and
// wai_comm_size of include/waiwera_hip.h): kernel micro-benchmarks, HIP-event timers, launch and collective counters.
#include "host.hpp"

using namespace wai;

namespace {
// What the memory system gives a plain stream on this box, for the bench line's roofline.copy_ceiling / read_ceiling:
// 16-byte streaming loads (and stores), two per thread and trip, enough workgroups to fill the chip.
typedef double stream_d2 __attribute__((ext_vector_type(2)));
__global__ __launch_bounds__(256) void k_stream_copy(const stream_d2* __restrict__ src, stream_d2* __restrict__ dst, size_t n2) {
  const size_t stride = (size_t)gridDim.x * 256;
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + stride < n2; i += 2 * stride) {
    const stream_d2 a = __builtin_nontemporal_load(src + i), b = __builtin_nontemporal_load(src + i + stride);
    __builtin_nontemporal_store(a, dst + i);
    __builtin_nontemporal_store(b, dst + i + stride);
  }
  if (i < n2) __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
}
__global__ __launch_bounds__(256) void k_stream_read(const stream_d2* __restrict__ src, size_t n2, double* sink) {
  const size_t stride = (size_t)gridDim.x * 256;
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  double t = 0.0;
  for (; i + stride < n2; i += 2 * stride) {
    const stream_d2 a = __builtin_nontemporal_load(src + i), b = __builtin_nontemporal_load(src + i + stride);
    t += (a.x + a.y) + (b.x + b.y);
  }
  if (i < n2) { const stream_d2 a = __builtin_nontemporal_load(src + i); t += a.x + a.y; }
  if (t == 1.2345678e300) *sink = t;   // never: keeps the loads
}
// can pc_amul form its operand x - alpha x2 inside the launch?  (pc_axpy_ok without the switch and the default)
bool pc_operand_composable(const wai_ctx* c) {
  return pc_fused(c, c->flow) && !pc_own_factor(c, c->flow) && !pc_colour(c, c->flow) && !net_in_operator(c, c->flow) && !pc_coarse(c, c->flow) &&
         !c->env.pc_unfused && pc_axpy_capable(c, c->flow.A);
}
}  // namespace

extern "C" {

// Micro-benchmark of one kernel on the library's stream, HIP-event timed: which 0 = block SpMV,
// 1 = ILU(0) apply z = B^-1 r, 2 = fused z = B^-1 (A x) with the (z, aux) reduction finished in the kernel,
// 3/4 = probes of 1/2 with the substitution sweeps skipped (load/compute phase split), 5 = the five launches
// of a whole BiCGStab iteration (overwrites the Krylov work vectors), 6 = its vector updates alone,
// 9 / 10 = the fused kernel on the interior / face bricks only (all on the flow system), 23 = z = B^-1 (A x) by the launch-per-level path on the
// factor in force (k_spmv + k_lvl_solve per level: the path k_pc_wide replaces, on the same system).
int wai_bench_kernel(wai_ctx* c, int which, int reps, float* ms_per_launch) {
  if (!c || !ms_per_launch || reps <= 0) return -2;
  read_env(c);
  LinSys& sys = c->flow;
  KrylovVecs& k = *sys.kv;
  if ((which == 20 || which == 21) && !k.basis) { c->err = "wai_bench_kernel 20 / 21: no Krylov basis (ksp_type gmres)"; return -2; }
  if (which > 0 && c->ilu.owner != &sys) { const int e = do_pc_setup(c, sys); if (e) return e < 0 ? -1 : e; }
  // the probes launch the natural order's kernels on the brick schedule: the multicolour factor is not theirs to read
  if (which > 0 && pc_colour(c, sys)) { c->err = "wai_bench_kernel: the natural order's kernels, not the multicolour ordering (tools/pc_colour_timing.py times it)"; return -2; }
  const bool fill = pc_fill_fused(c, sys);   // the filled ILU(k) factor: its own pattern and schedule (sys.as)
  if (which == 23 && (!pc_fused(c, sys) || !(fill ? sys.as.sched.ord_f : c->ilu.ord_f))) {
    c->err = "wai_bench_kernel 23: no level sets (a block-Jacobi schedule of a wide mesh, or fused ILU(k))";
    return -2;
  }
  // PCASM's fused form: the factor's rows are the extended system's (n_ext > N), the probes of one kernel class work on
  // vectors of the system's own length
  if (pc_asm_fused(c, sys) && (which == 9 || which == 10 || which == 16 || which == 23)) {
    c->err = "wai_bench_kernel 9 / 10 / 16 / 23: the brick schedule's kernels and the level sets of a factor on the system's own rows, not fused PCASM";
    return -2;
  }
  if (fill && (which == 9 || which == 10 || which == 16)) { c->err = "wai_bench_kernel 9 / 10 / 16: the brick schedule's kernels, not fused ILU(k)"; return -2; }
  const size_t copy_n = (size_t)c->np * c->df * c->mesh.n_prim / 2;   // modes 18 / 19 (the scratch is rewritten by every Jacobian)
  auto run = [&]() {
    switch (which) {
      case 0: launch_spmv(c, sys.A, k.P, k.tmp); break;
      case 1: case 3: pc_solve(c, sys, k.P, k.V, PC_DOT_NONE, nullptr, nullptr); break;
      case 23:   // the launch-per-level path on the schedule in force (wide schedules: the factor k_pc_wide applies), for comparison
        launch_spmv(c, sys.A, k.P, k.V);
        if (fill) launch_big_solve(c, sys.as.E, sys.as.sched, k.V);   // (no overlap: E's rows are the system's own, in order)
        else launch_big_solve(c, sys.A, c->ilu, k.V);
        break;
      case 9: if (c->ilu.n_int > 0) launch_pc(c, sys.A, true, k.P, k.V, PC_DOT_ZA, k.RP, c->ilu.sub_int, c->ilu.n_int); break;   // interior bricks only
      case 10: if (c->ilu.n_bnd > 0) launch_pc(c, sys.A, true, k.P, k.V, PC_DOT_ZA, k.RP, c->ilu.sub_bnd, c->ilu.n_bnd); break;  // face bricks only
      case 16:  // interior + face bricks as the overlapped halo exchange launches them (no halo here): the split's cost against case 2
        if (c->ilu.n_int > 0 && c->ilu.n_bnd > 0) {
          const Fin fin = make_fin_dots(c, PC_DOT_ZA, 2);
          launch_pc_split(c, sys.A, k.P, k.V, PC_DOT_ZA, k.RP, &fin, nullptr, nullptr);
        }
        break;
      case 5: {  // the launches (and, on several ranks, collectives) of one BiCGStab iteration back to back, no host in
                 // the loop: the iteration's floor
        const BcgsPlan pl = bcgs_plan(c, sys);
        bcgs_first_half(c, sys, pl); bcgs_second_half(c, sys, pl);
        break;
      }
      case 6:   // its vector updates alone
        if (bcgs_mode(c) == 2) { if (!pc_axpy_ok(c, sys)) bcgs_update_s(c, k, sys.n); bcgs_update_xrp(c, k, sys.n); }
        else { bcgs_update_p(c, k, sys.n); bcgs_update_s(c, k, sys.n); bcgs_update_xr(c, k, sys.n, true, 4, false); }
        break;
      case 17: {  // the second fused launch of the iteration exactly as bcgs_second_half issues it on one rank: operand S (or
                  // R - alpha V formed in the launch), five inner products, omega / (R,R) / rho / beta + the post in the finaliser
        const BcgsPlan pl = bcgs_plan(c, sys);
        pc_amul(c, sys, pl.axpy ? k.R : k.S, k.T, PC_DOT_MERGED, k.RP, 6, pl.axpy ? k.V : nullptr, true);
        break;
      }
      case 18:   // what a copy achieves on this box: hipMemcpy device to device, half of the perturbed-fluid scratch onto the other
        hipMemcpyAsync(c->flu_pert + copy_n, c->flu_pert, copy_n * sizeof(double), hipMemcpyDeviceToDevice, c->stream);
        break;
      case 19:   // the same bytes through a streaming copy kernel (16-byte non-temporal loads and stores)
        hipLaunchKernelGGL(k_stream_copy, 8192, 256, 0, c->stream, reinterpret_cast<const stream_d2*>(c->flu_pert.get()),
                           reinterpret_cast<stream_d2*>(c->flu_pert + (copy_n & ~(size_t)1)), copy_n / 2);
        break;
      case 22:   // read-only stream over the whole scratch (2 x copy_n doubles)
        hipLaunchKernelGGL(k_stream_read, 8192, 256, 0, c->stream, reinterpret_cast<const stream_d2*>(c->flu_pert.get()), copy_n & ~(size_t)1,
                           c->ks.scal + 60);
        break;
      case 20: {  // GMRES: the classical Gram-Schmidt inner products (w, v_0 .. v_j) of a whole restart cycle, j = 0 .. m - 1,
                  // as ksp_gmres issues them (k_mdot passes + their finalisations); ms_per_launch = per Krylov iteration
        const int m = std::min(std::max(sys.ksp.restart, 1), k.basis_m);
        for (int j = 0; j < m; j++) gmres_mdot(c, k.basis, (size_t)sys.nl, sys.n, k.T, j + 1);
        break;
      }
      case 21: {  // GMRES: w -= sum h_j v_j + |w|^2 of a whole restart cycle (k_maxpy_norm + finalisation), per iteration
        const int m = std::min(std::max(sys.ksp.restart, 1), k.basis_m);
        for (int j = 0; j < m; j++) gmres_maxpy_norm(c, k.basis, (size_t)sys.nl, sys.n, k.T, j + 1);
        break;
      }
      case 7:   // the second fused launch of the "fused" iteration: z = B^-1 A (R - alpha V) with the five inner products
        pc_amul(c, sys, k.R, k.T, PC_DOT_MERGED, k.RP, -1, pc_axpy_ok(c, sys) ? k.V : nullptr, false);
        break;
      // the fused launch by reduction mode: 11 none; 12 (z,aux) left as partials; 13 (x,z),(z,z) + omega in the launch;
      // 14 the five merged products left as partials; 15 the five + omega, (R,R), rho, beta in the launch
      case 11: pc_amul(c, sys, k.P, k.V, PC_DOT_NONE, nullptr, -2); break;
      case 12: pc_amul(c, sys, k.P, k.V, PC_DOT_ZA, k.RP, -2); break;
      case 13: pc_amul(c, sys, k.P, k.V, PC_DOT_XZ, nullptr, 3); break;
      case 14: pc_amul(c, sys, k.P, k.V, PC_DOT_MERGED, k.RP, -2); break;
      case 15: pc_amul(c, sys, k.P, k.V, PC_DOT_MERGED, k.RP, 6); break;
      default: pc_amul(c, sys, k.P, k.V, PC_DOT_ZA, k.RP, 2); break;   // what a BiCGStab half-iteration runs (no halo on one rank)
    }
  };
  c->dbg = (which == 3 || which == 4) && pc_fused(c, sys) && !(sys.A.bs == 2 && c->ilu.park) ? 1 : 0;
  partials_clear(c, S_D1, 5);
  // Warm-up by TIME, not by count: the probes run behind host-side work (the bench's checks, a Jacobian), and the first
  // launches after such a pause run below the clocks the real iteration sees -- MEASURED (round 6, one box, same process
  // order): k_spmv 0.516 ms in the bench line's probe against 0.442 ms average over the traced run's 205 launches.  So:
  // launches until 25 ms have gone by (at least 5, at most twice the timed repetitions: a counter-collection pass pays
  // tens of milliseconds of host time per dispatch and asks for few repetitions), then the timed repetitions.
  // On several ranks the probes contain collectives: every rank must issue the same number of launches, so the count
  // cannot depend on a rank's own clock -- five launches there, as in rounds 1-5 (the first form of this warm-up hung the
  // multi-rank bench tests: the ranks' loop counts differed).
  if (c->comm && c->comm->nranks > 1) {
    for (int i = 0; i < 5; i++) run();
  } else {
    float warm = 0.f;
    int n = 0;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    do {
      for (int i = 0; i < 5; i++) run();
      n += 5;
      HIPCHK(c, hipEventRecord(c->ev1, c->stream));
      HIPCHK(c, hipEventSynchronize(c->ev1));
      HIPCHK(c, hipEventElapsedTime(&warm, c->ev0, c->ev1));
    } while (warm < 25.f && n < std::max(10, 2 * reps));
  }
  HIPCHK(c, hipEventRecord(c->ev0, c->stream));
  for (int i = 0; i < reps; i++) run();
  HIPCHK(c, hipEventRecord(c->ev1, c->stream));
  HIPCHK(c, hipEventSynchronize(c->ev1));
  c->dbg = 0;
  partials_clear(c, S_D1, 5);   // the interior- / face-only launches leave partials nobody sums
  float ms = 0.f;
  HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
  *ms_per_launch = ms / reps;
  if (which == 20 || which == 21) *ms_per_launch /= (float)std::min(std::max(sys.ksp.restart, 1), k.basis_m);
  return 0;
}

// name of the kernel (or path) a preconditioned-operator application runs on, for reports
const char* wai_pc_kernel_name(wai_ctx* c) {
  if (!c) return "";
  const IluSchedule& s = c->ilu;
  const LinSys& sys = c->flow;
  const int bs = sys.A.bs;
  const PcOpts pc = pc_of(c, sys);
  if (pc.type == WAI_PC_NONE) return "k_spmv (no preconditioner)";
  if (pc.type == WAI_PC_LU) return "k_spmv + k_lu_apply (dense block inverses)";
  static thread_local char buf[96];
  if (pc_sub_lu(pc)) {
    snprintf(buf, sizeof(buf), "k_spmv + k_sublu_solve on the extended system (%s, sub-preconditioner lu)",
             pc.type == WAI_PC_ASM ? "ASM" : "block Jacobi");
    return buf;
  }
  if (pc_colour(c, sys)) {
    if (!c->colour.fused) return "k_spmv + k_colour_sweep per colour (block Jacobi, multicolour ILU(0))";
    snprintf(buf, sizeof(buf), "k_pc_colour<%d,spmv>", bs);
    return buf;
  }
  if (pc_fill_fused(c, sys)) {   // one launch: A on the Jacobian's planes, the sweeps on the filled factor's
    snprintf(buf, sizeof(buf), "k_pc_wide<%d,spmv> on the filled factor (block Jacobi, ILU(%d))", bs, pc.ilu_levels);
    return buf;
  }
  if (pc_asm_fused(c, sys)) {   // one launch: A on the Jacobian's planes by the row map, the sweeps on the extended factor's
    snprintf(buf, sizeof(buf), "k_pc_wide<%d,spmv,map> on the extended system (ASM, ILU(%d))", bs, std::max(pc.ilu_levels, 0));
    return buf;
  }
  if (pc_extended(c, sys)) {
    snprintf(buf, sizeof(buf), "k_spmv + %s on the extended system (%s, ILU(%d))",
             sys.as.sched.big ? (sys.as.sched.tiles.serve && !sys.as.sched.sublu ? "k_tile_solve per tile level" : "k_lvl_solve per level")
                              : (sys.as.sched.wide ? "k_pc_wide" : "k_pc"),
             pc.type == WAI_PC_ASM ? "ASM" : "block Jacobi", std::max(pc.ilu_levels, 0));
    return buf;
  }
  if (s.big) return s.tiles.serve ? "k_spmv + k_tile_solve per tile level" : "k_spmv + k_lvl_solve per level";
  switch (pc_kernel_kind(c, sys.A, s)) {   // the launcher's own rule (kernels_fused.hip)
    case 4: snprintf(buf, sizeof(buf), "k_pc_wide<%d,spmv>", bs); break;
    case 3: snprintf(buf, sizeof(buf), "k_pc_wave<%d,spmv>", bs); break;
    case 2: snprintf(buf, sizeof(buf), "k_pc_rows<%d,spmv,%d+%d>", bs, s.max_nlu <= 3 ? 3 : 4, s.max_nlu <= 3 ? 3 : 4); break;
    case 1: return s.col16 && !getenv("WAI_NO_COL16") ? "k_pc_park<spmv,col16>" : "k_pc_park<spmv>";
    default:
      snprintf(buf, sizeof(buf), "k_pc<%d,spmv,%s,%s>", bs, s.diag_only ? (s.scaled ? "dilu-scaled" : "dilu") : "ilu",
               s.fast3 ? "compact3" : "generic");
  }
  return buf;
}
int wai_comm_size(wai_ctx* c) { return c ? comm_count(c->comm) : -2; }
// does a BiCGStab iteration's second fused launch form its operand S = R - alpha V itself (three launches per iteration)?
int wai_bcgs_composed(wai_ctx* c) {
  if (!c) return -2;
  read_env(c);
  const BcgsPlan pl = bcgs_plan(c, c->flow);
  return pl.axpy ? 1 : 0;
}
int wai_launch_stats(wai_ctx* c, long long* kernels, long long* copies) {
  if (!c) return -2;
  if (kernels) *kernels = c->ks.n_launch;
  if (copies) *copies = c->ks.n_copy;
  return 0;
}
int wai_tracer_stats(wai_ctx* c, long long* assembly_sweeps) {
  if (!c) return -2;
  if (assembly_sweeps) *assembly_sweeps = c->tr.n_sweeps;
  return 0;
}
int wai_test_drop_partials(wai_ctx* c, int n) { return c ? test_drop_partials(c, n) : -2; }
int wai_test_device_memory(long long* allocations, long long* bytes) {
  if (!allocations || !bytes) return -2;
  *allocations = dev_live_allocs; *bytes = dev_live_bytes;
  return 0;
}
// one preconditioned-operator application as the drivers issue it (waiwera_hip_bench.h): the inputs into the Krylov work
// vectors (halo room), the scalars seeded, the partial slots emptied as a driver empties them before its first producer,
// then pc_amul / pc_solve / launch_pc_split unchanged
int wai_test_pc_operator(wai_ctx* c, int spmv, const double* x, const double* x2, double alpha, int dot_mode, const double* aux,
                         int split, int fin_phase, const double* scal_in, double* z, double* scal_out) {
  if (!c || !x || !z || !scal_in || !scal_out || dot_mode < PC_DOT_NONE || dot_mode > PC_DOT_MERGED || fin_phase < -2) return -2;
  if ((dot_mode == PC_DOT_ZA || dot_mode == PC_DOT_MERGED) && !aux) { c->err = "wai_test_pc_operator: dot modes 1 and 4 need aux"; return -2; }
  read_env(c);
  LinSys& sys = c->flow;
  if (c->ilu.owner != &sys) { const int e = do_pc_setup(c, sys); if (e) return e < 0 ? -1 : e; }
  if (x2 && (!spmv || !pc_operand_composable(c))) { c->err = "wai_test_pc_operator: composed operand asked of a kernel that cannot form it"; return -1; }
  if (split && (!spmv || !pc_fused(c, sys) || pc_own_factor(c, sys) || pc_colour(c, sys) || net_in_operator(c, sys) || pc_coarse(c, sys) || c->ilu.n_int <= 0 || c->ilu.n_bnd <= 0 ||
                !c->ilu.sub_int)) {
    c->err = "wai_test_pc_operator: no interior / face brick lists to split the launch over";
    return -1;
  }
  KrylovVecs& k = *sys.kv;
  const size_t n = (size_t)sys.n;
  double s[16];
  for (int i = 0; i < 16; i++) s[i] = scal_in[i];
  s[S_ALPHA] = alpha;
  HIPCHK(c, hipMemcpyAsync(k.R, x, n * sizeof(double), hipMemcpyDefault, c->stream));
  if (x2) HIPCHK(c, hipMemcpyAsync(k.V, x2, n * sizeof(double), hipMemcpyDefault, c->stream));
  if (aux) HIPCHK(c, hipMemcpyAsync(k.RP, aux, n * sizeof(double), hipMemcpyDefault, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->ks.scal, s, sizeof(s), hipMemcpyHostToDevice, c->stream));
  partials_clear(c, S_D1, 5);
  const double* a = aux ? k.RP : nullptr;
  const double* v = x2 ? k.V : nullptr;
  int e = 0;
  if (split) {
    Fin fin;
    const Fin* fp = nullptr;
    if (fin_phase >= -1 && dot_mode) {
      fin = make_fin_dots(c, dot_mode, fin_phase);
      fp = &fin;
    }
    e = launch_pc_split(c, sys.A, k.R, k.T, dot_mode, a, fp, v, nullptr);
  } else if (spmv) {
    e = pc_amul(c, sys, k.R, k.T, dot_mode, a, fin_phase, v, false);
  } else {
    e = pc_solve(c, sys, k.R, k.T, dot_mode, k.R, a, fin_phase);
  }
  if (e) return e;
  if (fin_phase == -2 && dot_mode)   // the partial sums left behind, summed by k_finalize as the general path sums them
    vec_finalize(c, c->ks.nb_pc, pc_dot_slot0(dot_mode), pc_dot_nslots(dot_mode), -1);
  HIPCHK(c, hipMemcpyAsync(z, k.T, n * sizeof(double), hipMemcpyDefault, c->stream));
  HIPCHK(c, hipMemcpyAsync(s, c->ks.scal, sizeof(s), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < 16; i++) scal_out[i] = s[i];
  return 0;
}
// one launch of the coarse level through the launcher pc_solve itself uses, or a download of its matrices
// (waiwera_hip_bench.h).  Vectors are host or device memory; a device vector is handed to the launcher as it is
int wai_test_coarse(wai_ctx* c, int what, const double* in, double* out) {
  if (!c || !out || what < WAI_COARSE_RESTRICT || what > WAI_COARSE_TIMES) return -2;
  if (!in && what <= WAI_COARSE_PROLONG_SET) return -2;
  LinSys& sys = c->flow;
  CoarseLevel& k = c->coarse;
  if (!pc_coarse(c, sys)) { c->err = "wai_test_coarse: no coarse level is in force (wai_set_pc_coarse)"; return -2; }
  read_env(c);
  if (what == WAI_COARSE_GEMV || what == WAI_COARSE_AC || what == WAI_COARSE_AINV || what == WAI_COARSE_TIMES)
    if (c->ilu.owner != &sys) { const int e = do_pc_setup(c, sys); if (e) return e < 0 ? -1 : e; }
  const size_t n = (size_t)sys.n, m = (size_t)k.m;
  if (what == WAI_COARSE_TIMES) { out[0] = k.ms_galerkin; out[1] = k.ms_inverse; return 0; }
  if (what == WAI_COARSE_AC || what == WAI_COARSE_AINV) {
    HIPCHK(c, hipMemcpyAsync(out, what == WAI_COARSE_AC ? k.Ac.get() : k.Ainv.get(), m * m * sizeof(double), hipMemcpyDefault, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
  }
  VecArg vi{c}, vo{c};
  int e = 0;
  switch (what) {
    case WAI_COARSE_RESTRICT:
      if (vi.in(in, n, 0) || vo.out_only(out, m, 1)) return -1;
      e = launch_coarse_restrict(c, k, vi.dev, vo.dev);
      break;
    case WAI_COARSE_GEMV:
      if (vi.in(in, m, 0) || vo.out_only(out, m, 1)) return -1;
      e = launch_coarse_gemv(c, k, vi.dev, vo.dev);
      break;
    default:
      if (vi.in(in, m, 0) || vo.in(out, n, 1)) return -1;
      e = launch_coarse_prolong(c, k, vi.dev, vo.dev, what == WAI_COARSE_PROLONG_ADD);
  }
  if (e) return e;
  if (vo.back()) return -1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
int wai_pc_axpy_capable(wai_ctx* c) { return c ? (pc_operand_composable(c) ? 1 : 0) : -2; }
int wai_test_partial_count(wai_ctx* c) { return c ? c->ks.nb_pc : -2; }
int wai_test_desc_templates(wai_ctx* c, int* bricks, int* rows) {
  if (!c) return -2;
  const bool have = c->ilu.sub_desc != nullptr;
  if (bricks) *bricks = c->ilu.nsub;
  if (rows) *rows = have ? c->ilu.template_rows : 0;
  return have ? c->ilu.n_templates : 0;
}
int wai_test_pack_groups(wai_ctx* c, int list, int* shared, int* table, int cap) {
  if (!c || list < 0 || list > 2 || cap < 0 || (cap > 0 && !table)) return -2;
  read_env(c);
  const IluSchedule& s = c->ilu;
  // the launcher's own condition (launch_pc_bs): k_pc_park on col16 with shared descriptors, a table for the list, no WAI_NO_PACK
  const bool packed = !s.big && pc_kernel_kind(c, c->flow.A, s) == 1 && s.col16 && !c->env.no_col16 && s.sub_desc &&
                      !c->env.no_desc_share && s.pack_tab[list] && !c->env.no_pack;
  if (shared) *shared = packed ? s.n_shared[list] : 0;
  if (!packed) return 0;
  const int n = std::min(cap, s.n_groups[list] * 32);
  if (n > 0) HIPCHK(c, hipMemcpy(table, s.pack_tab[list].get(), sizeof(int) * n, hipMemcpyDeviceToHost));
  return s.n_groups[list];
}
int wai_test_tile_schedule(wai_ctx* c, int extended, int* facts) {
  if (!c || !facts) return -2;
  read_env(c);
  LinSys& sys = c->flow;
  if (c->ilu.owner != &sys) { const int e = do_pc_setup(c, sys); if (e) return e < 0 ? -1 : e; }
  if (extended && !pc_extended(c, sys)) { c->err = "wai_test_tile_schedule: the preconditioner in force has no extended system"; return -1; }
  const IluSchedule& s = extended ? sys.as.sched : c->ilu;
  const TileFacts& t = s.tiles;
  const int f[8] = {t.n_tiles, t.ntl_f, t.ntl_b, t.max_tile_rows, t.max_in_levels, t.serve ? 1 : 0, s.nlev_f, s.nlev_b};
  std::copy(f, f + 8, facts);
  return t.n_tiles;
}
// one vector / reduction step of the Krylov drivers through the drivers' own launchers (waiwera_hip_bench.h): temporaries of
// the caller's padded lengths, all NSCAL scalars seeded, every partial slot emptied as ksp_gmres empties them before its
// first producer, the launchers unchanged, everything back to the caller -- guard elements included
int wai_test_krylov_vec(wai_ctx* c, int op, int variant, int n, int k, long long ld, long long len, double alpha, double* vecs,
                        double* basis, const double* coef, double* scal, double* post) {
  if (!c || !vecs || !scal || !post) return -2;
  const bool gmres = op == WAI_KV_MDOT || op == WAI_KV_MAXPY_NORM || op == WAI_KV_UPDATE_X;
  auto refuse = [&](const char* why) { c->err = std::string("wai_test_krylov_vec: ") + why; return -2; };
  if (op < WAI_KV_DOT || op > WAI_KV_UPDATE_X) return refuse("no such op");
  if (n < 1) return refuse("n < 1");
  if (k < 0 || k > MAX_RESTART || (gmres && k < 1)) return refuse("basis count out of range");
  if (len < (long long)n) return refuse("len < n");
  if (gmres && (ld < (long long)n || !basis)) return refuse("ld < n, or no basis");
  if (op == WAI_KV_UPDATE_X && !coef) return refuse("no coefficients");
  const int vmax[] = {0, 1, 2, 0, 0, 3, 0, 0, 6, 0, 0, 1, 0};   // per op: the largest variant
  if (variant < 0 || variant > vmax[op] || (op == WAI_KV_SCALARS && variant == 1)) return refuse("no such variant");
  read_env(c);
  enum { X, R, RP, P, V, S, T, NV };
  KrylovVecs kv;   // owners of this call's temporaries: returned when it ends, whichever way
  DevBuf<double>* own[NV] = {&kv.X_own, &kv.R, &kv.RP, &kv.P, &kv.V, &kv.S, &kv.T};
  const size_t L = (size_t)len, nbasis = gmres ? (size_t)(k + 1) * (size_t)ld : 0;
  for (int i = 0; i < NV; i++) {
    if (own[i]->alloc(c, L)) return -1;
    HIPCHK(c, hipMemcpyAsync(own[i]->get(), vecs + (size_t)i * L, L * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  kv.X = kv.X_own;
  if (gmres) {
    if (kv.basis.alloc(c, nbasis)) return -1;
    HIPCHK(c, hipMemcpyAsync(kv.basis.get(), basis, nbasis * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, hipMemcpyAsync(c->ks.scal, scal, NSCAL * sizeof(double), hipMemcpyHostToDevice, c->stream));
  partials_clear(c, 0, NSLOTS);
  int seq = 0;   // > 0: the launch posts to the host under this sequence number
  switch (op) {
    case WAI_KV_DOT: vec_dot(c, kv.X, kv.R, n, S_W2); break;
    case WAI_KV_DOTS:   // host_dots
      vec_dots(c, kv.X, kv.R, S_D1, variant ? nullptr : kv.P.get(), variant ? nullptr : kv.V.get(), S_D2, n);
      vec_finalize(c, c->ks.nb_pc, S_D1, variant ? 1 : 2, -1);
      break;
    case WAI_KV_WAXPY:
      vec_waxpy(c, variant == 0 ? kv.T.get() : (variant == 1 ? kv.X : kv.R.get()), alpha, kv.X, kv.R, n);
      break;
    case WAI_KV_BCGS_P: bcgs_update_p(c, kv, n); break;
    case WAI_KV_BCGS_S: bcgs_update_s(c, kv, n); break;
    case WAI_KV_BCGS_XR:
      if (variant == 0) bcgs_update_xr(c, kv, n, false);
      else if (variant == 1) bcgs_update_xr(c, kv, n, true, -1, false);
      else if (variant == 2) { bcgs_update_xr(c, kv, n, true, 4, true); seq = c->ks.seq; }
      else { bcgs_update_xr(c, kv, n, true, -2, false); vec_finalize(c, c->ks.nblocks, S_DP2, 2, -1); }
      break;
    case WAI_KV_BCGS_XRP: bcgs_update_xrp(c, kv, n); break;
    case WAI_KV_BCGS_XRP_DERIVE: bcgs_update_xrp_derive(c, kv, n); seq = c->ks.seq; break;
    case WAI_KV_SCALARS:
      bcgs_scalars(c, variant, variant == 6);
      if (variant == 6) seq = c->ks.seq;
      break;
    case WAI_KV_MDOT: gmres_mdot(c, kv.basis, (size_t)ld, n, kv.T, k); break;
    case WAI_KV_MAXPY_NORM: gmres_maxpy_norm(c, kv.basis, (size_t)ld, n, kv.T, k); break;
    case WAI_KV_SCALE_TO: gmres_scale_to(c, variant ? kv.X : kv.T.get(), kv.X, S_W2, n); break;
    default: gmres_update_x(c, kv.basis, (size_t)ld, n, kv.X, coef, k); break;
  }
  if (seq > 0) {
    if (wait_post(c, seq)) return -1;
    post[0] = c->ks.h_scal[S_DP2]; post[1] = c->ks.h_scal[S_BREAK];
  }
  for (int i = 0; i < NV; i++)
    HIPCHK(c, hipMemcpyAsync(vecs + (size_t)i * L, own[i]->get(), L * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (gmres) HIPCHK(c, hipMemcpyAsync(basis, kv.basis.get(), nbasis * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(scal, c->ks.scal, NSCAL * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
int wai_test_drop_stream_wait(wai_ctx* c, int which) { if (!c) return -2; c->test_drop_wait = which; return 0; }
int wai_bench_mute_comm(wai_ctx* c, int on) {
  if (!c) return -2;
  if (c->comm) c->comm->mute = on != 0;
  return 0;
}
int wai_halo_size(wai_ctx* c, int dof, long long* bytes_sent, int* n_neighbours) {
  if (!c) return -2;
  if (bytes_sent) *bytes_sent = (long long)c->send_total * dof * (long long)sizeof(double);
  if (n_neighbours) *n_neighbours = c->n_nbr;
  return 0;
}
int wai_comm_stats(wai_ctx* c, long long* allreduces, long long* exchanges) {
  if (!c) return -2;
  if (allreduces) *allreduces = c->comm ? c->comm->n_allreduce : 0;
  if (exchanges) *exchanges = c->comm ? c->comm->n_exchange : 0;
  return 0;
}

int wai_timer_start(wai_ctx* c) { if (!c) return -2; HIPCHK(c, hipEventRecord(c->ev0, c->stream)); return 0; }
int wai_timer_stop(wai_ctx* c, float* ms) {
  if (!c || !ms) return -2;
  HIPCHK(c, hipEventRecord(c->ev1, c->stream));
  HIPCHK(c, hipEventSynchronize(c->ev1));
  HIPCHK(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
  return 0;
}
int wai_synchronize(wai_ctx* c) { if (!c) return -2; HIPCHK(c, hipStreamSynchronize(c->stream)); return 0; }
int wai_profile_enable(wai_ctx* c, int on) { if (!c) return -2; c->prof_on = on != 0; return 0; }
int wai_profile_get(wai_ctx* c, int kclass, double* ms, long long* launches) {
  if (!c || kclass < 0 || kclass >= KC_COUNT) return -2;
  if (ms) *ms = c->prof_ms[kclass];
  if (launches) *launches = c->prof_n[kclass];
  return 0;
}
int wai_profile_reset(wai_ctx* c) {
  if (!c) return -2;
  for (int i = 0; i < KC_COUNT; i++) { c->prof_ms[i] = 0.0; c->prof_n[i] = 0; }
  return 0;
}

}  // extern "C"

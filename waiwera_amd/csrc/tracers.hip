// Passive tracers behind the C ABI of libwaiwera_hip.so (include/waiwera_hip.h): the auxiliary linear problem's set-up,
// its solver and preconditioner settings, its systems (per tracer and coupled) and its solve.
#include "host.hpp"

using namespace wai;

namespace wai {

// the coupled system's own buffers (values, factor, right-hand side), on first use after wai_set_tracers
static int coupled_system_buffers(wai_ctx* c) {
  Tracers& t = c->tr;
  Bcsr& A = c->coupled.A;
  const size_t nv = (size_t)A.W * t.nt * A.n;
  LinSys& cp = c->coupled;
  if (!cp.val && cp.val.alloc(c, nv)) return -1;
  if (!cp.fdg && cp.fdg.alloc(c, nv)) return -1;
  if (!c->tr_rhsb && c->tr_rhsb.alloc(c, (size_t)cp.nl + 16)) return -1;
  A.val = cp.val; A.fdg = cp.fdg; t.rhsb = c->tr_rhsb;
  return 0;
}

// ... and what a coupled SOLVE needs beside them: the Krylov vectors of nt * n_prim entries, the GMRES basis, halo buffers
// of nt values per cell.  What the mode does not cover is refused by name
static int coupled_prepare(wai_ctx* c) {
  LinSys& sys = c->coupled;
  const char* what = nullptr;
  const PcOpts pc = pc_of(c, sys);   // the auxiliary systems' own preconditioner, or the flow solver's where they follow
  if (pc_sub_lu(pc)) what = "the lu sub-preconditioner (WAI_SUB_LU)";
  else if (pc.type == WAI_PC_ASM) what = "the asm preconditioner";
  else if (pc.type == WAI_PC_LU) what = "the lu preconditioner";
  else if (pc.ilu_levels > 0) what = "ILU(k) with k > 0";
  else if (pc.type != WAI_PC_BJACOBI && pc.type != WAI_PC_NONE) what = "this preconditioner";
  if (what) {
    c->err = std::string("coupled tracer solve (WAI_TRACER_COUPLED) does not cover ") + what +
             ": block Jacobi ILU(0) or none only; use WAI_TRACER_PER_TRACER";
    return -2;
  }
  if (sys.ksp.type == WAI_KSP_LGMRES || sys.ksp.type == WAI_KSP_BCGSL) {
    c->err = std::string("coupled tracer solve (WAI_TRACER_COUPLED) does not cover the ") +
             (sys.ksp.type == WAI_KSP_LGMRES ? "lgmres" : "bcgsl") + " solver: gmres or bcgs only; use WAI_TRACER_PER_TRACER";
    return -2;
  }
  if (coupled_system_buffers(c) || alloc_krylov_vecs(c, *sys.kv, (size_t)sys.nl)) return -1;
  if (sys.ksp.type == WAI_KSP_GMRES && ensure_basis(c, sys, basis_vectors(sys.ksp.restart))) return -1;
  if (c->comm && c->mesh.n_halo && ensure_halo_dof(c, c->tr.nt)) return -1;
  return 0;
}

// what wai_tracer_system (tracer: its index), wai_tracer_block_system and wai_tracer_solve (tracer: null; ratio: the solve
// checks it with the BDF2 history) refuse alike
static int tracer_args(wai_ctx* c, const int* tracer, int method, const double* alx_last, const double* alx_last2,
                       const double* ratio = nullptr) {
  if (tracer && (*tracer < 0 || *tracer >= c->tr.nt)) { c->err = "tracer index out of range"; return -1; }
  if (!tracer && !c->tr.nt) { c->err = "no tracers set"; return -1; }
  if (method < WAI_METHOD_BEULER || method > WAI_METHOD_DIRECTSS) { c->err = "unknown time stepping method"; return -1; }
  if (method != WAI_METHOD_DIRECTSS && !alx_last) return -2;
  if (method == WAI_METHOD_BDF2 && ratio && (!alx_last2 || !(*ratio > 0.0))) { c->err = "BDF2 needs a step size ratio > 0 and Al o X two steps back"; return -1; }
  if (method == WAI_METHOD_BDF2 && !alx_last2) return -2;
  return 0;
}

static TracerForm tracer_form(const Tracers& t, int it, int method, double dt, double ratio) {
  TracerForm tf;
  tf.method = method; tf.it = it; tf.nt = t.nt; tf.phase = t.phase[it];
  tf.dt = dt; tf.ratio = ratio; tf.decay = t.decay[it]; tf.activation = t.activation[it];
  tf.diffusion = t.diffusion[it];
  return tf;
}

}  // namespace wai

extern "C" {

// ---- passive tracers: the auxiliary linear problem -------------------------------------------
int wai_set_tracers(wai_ctx* c, int n, const int* phase, const double* decay, const double* activation,
                    const double* diffusion) {
  if (!c || n < 0 || (n > 0 && !phase)) return -2;
  if (n > wai::MAX_TRACERS) { c->err = "too many tracers (at most 8)"; return -1; }
  Tracers& t = c->tr;
  for (int i = 0; i < n; i++) {
    if (phase[i] < 0 || phase[i] >= c->nmob) { c->err = "tracer phase index out of range"; return -1; }
    t.phase[i] = phase[i];
    t.decay[i] = decay ? decay[i] : 0.0;
    t.activation[i] = activation ? activation[i] : 0.0;
    t.diffusion[i] = diffusion ? diffusion[i] : 0.0;
  }
  t.nt = n;
  c->tr_bc.reset(); c->tr_inj.reset(); c->tr_rhsb.reset();
  t.bc = t.inj = t.rhsb = nullptr;
  // the scalar system: block size 1 on the mesh's pattern, the flow's work vectors and basis (LinSys: the alias and the clamp)
  LinSys& aux = c->aux;
  aux.val.reset(); aux.A.val = nullptr;
  aux.n = c->mesh.n_owned; aux.nl = c->mesh.n_prim; aux.kv = &c->kv;
  // the coupled system's buffers are sized by nt: rebuilt on first use (coupled_system_buffers, coupled_prepare)
  LinSys& cp = c->coupled;
  cp.val.reset(); cp.fdg.reset(); cp.A.val = cp.A.fdg = nullptr;
  c->kv_coupled = KrylovVecs();
  cp.n = c->mesh.n_owned * n; cp.nl = c->mesh.n_prim * n; cp.kv = &c->kv_coupled;
  pc_invalidate(c, cp);
  if (n == 0) return 0;
  const size_t nbc = (size_t)std::max(c->mesh.n_bc, 1) * n, nsrc = (size_t)std::max(c->src.n, 1) * n;
  if (c->tr_bc.alloc_zeroed(c, nbc) || c->tr_inj.alloc_zeroed(c, nsrc) || aux.val.alloc(c, (size_t)c->pat.W * c->pat.n)) return -1;
  t.bc = c->tr_bc; t.inj = c->tr_inj;
  aux.A = matrix_on(c->pat, 1, aux.val);
  cp.A = matrix_on(c->pat, n, nullptr);
  cp.A.dg = n;
  return 0;
}

int wai_set_tracer_bc(wai_ctx* c, const double* x_bc) {
  if (!c || !x_bc) return -2;
  if (!c->tr.nt) { c->err = "no tracers set"; return -1; }
  if (c->mesh.n_bc)
    HIPCHK(c, hipMemcpy(c->tr.bc, x_bc, sizeof(double) * (size_t)c->mesh.n_bc * c->tr.nt, hipMemcpyDefault));
  return 0;
}

int wai_set_tracer_injection(wai_ctx* c, const double* rate) {
  if (!c || !rate) return -2;
  if (!c->tr.nt) { c->err = "no tracers set"; return -1; }
  // sized by the sources in force now: wai_set_sources first
  c->tr.inj = nullptr;
  if (c->tr_inj.alloc_zeroed(c, (size_t)std::max(c->src.n, 1) * c->tr.nt)) return -1;
  c->tr.inj = c->tr_inj;
  if (c->src.n)
    HIPCHK(c, hipMemcpy(c->tr.inj, rate, sizeof(double) * (size_t)c->src.n * c->tr.nt, hipMemcpyDefault));
  return 0;
}

int wai_set_aux_solver(wai_ctx* c, int ksp_type, int gmres_restart, double rtol, double atol, int max_its) {
  if (!c) return -2;
  if (ksp_type < WAI_KSP_BCGS || ksp_type > WAI_KSP_LGMRES) { c->err = "unknown KSP type"; return -1; }
  if (gmres_restart > MAX_RESTART) { c->err = "gmres restart above 40 is not supported"; return -1; }
  KspOpts& k = c->aux.ksp;
  k.type = ksp_type;
  if (gmres_restart > 0) k.restart = gmres_restart;
  if (rtol > 0.0) k.rtol = rtol;
  if (atol > 0.0) k.atol = atol;
  if (max_its > 0) k.max_its = max_its;
  c->coupled.ksp = k;   // one setting for the auxiliary problem, whichever way it is solved
  return 0;
}

int wai_set_tracer_solve_mode(wai_ctx* c, int mode) {
  if (!c) return -2;
  if (mode != WAI_TRACER_PER_TRACER && mode != WAI_TRACER_COUPLED) { c->err = "unknown tracer solve mode"; return -2; }
  c->tr.mode = mode;
  return 0;
}

// The auxiliary systems' own preconditioner (both of them: per tracer and coupled, as wai_set_aux_solver's settings), or
// WAI_AUX_PC_FOLLOW: the flow solver's.  Their set-up alone is invalidated; the extended systems they cached are rebuilt
// by the next set-up where the settings differ (do_pc_setup)
int wai_set_aux_pc(wai_ctx* c, int pc_type, int asm_overlap, int ilu_levels, int sub_pc) {
  if (!c) return -2;
  if (pc_type != WAI_AUX_PC_FOLLOW && (pc_type < WAI_PC_BJACOBI || pc_type > WAI_PC_LU)) {
    c->err = "unknown auxiliary preconditioner type (a WAI_PC_* value or WAI_AUX_PC_FOLLOW)";
    return -2;
  }
  if (ilu_levels < 0 || ilu_levels > 8) { c->err = "auxiliary preconditioner: ILU(k) levels 0..8"; return -2; }
  if (sub_pc != WAI_SUB_ILU && sub_pc != WAI_SUB_LU) { c->err = "unknown auxiliary sub-preconditioner (WAI_SUB_ILU or WAI_SUB_LU)"; return -2; }
  PcOpts p;
  p.type = pc_type; p.asm_overlap = asm_overlap; p.ilu_levels = ilu_levels; p.sub = sub_pc;
  c->aux.pc = c->coupled.pc = p;
  pc_invalidate(c, c->aux);
  pc_invalidate(c, c->coupled);
  return 0;
}

int wai_get_aux_pc(wai_ctx* c, int* pc_type, int* asm_overlap, int* ilu_levels, int* sub_pc) {
  if (!c) return -2;
  const PcOpts& p = c->aux.pc;
  if (pc_type) *pc_type = p.type;
  if (asm_overlap) *asm_overlap = p.asm_overlap;
  if (ilu_levels) *ilu_levels = p.ilu_levels;
  if (sub_pc) *sub_pc = p.sub;
  return 0;
}

int wai_tracer_lhs(wai_ctx* c, double* Al) {
  if (!c || !Al) return -2;
  if (!c->tr.nt) { c->err = "no tracers set"; return -1; }
  VecArg o{c};
  if (o.out_only(Al, (size_t)c->mesh.n_owned * c->tr.nt, 0)) return -1;
  launch_tracer_lhs(c, o.dev);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return o.back();
}

int wai_tracer_block_system(wai_ctx* c, int method, double dt, double ratio, const double* alx_last,
                            const double* alx_last2, double* val, double* b) {
  if (!c || !val || !b) return -2;
  if (int e = tracer_args(c, nullptr, method, alx_last, alx_last2)) return e;
  Tracers& t = c->tr;
  if (coupled_system_buffers(c)) return -1;   // the system alone: no solver buffers, whatever the preconditioner
  const Bcsr& A = c->coupled.A;
  const size_t nx = (size_t)c->mesh.n_owned * t.nt;
  VecArg a1{c}, a2{c};
  if (a1.in(alx_last, nx, 0) || a2.in(alx_last2, nx, 1)) return -1;
  if (launch_tracer_assemble_all(c, method, dt, ratio, a1.dev, a2.dev, t.rhsb)) return -1;
  launch_dg_to_bcsr(c, A, A.fdg);   // the factor buffer as scratch: nnzb * nt <= W * nt * n
  pc_invalidate(c);   // (as it always has: the next solve of any system sets up again)
  HIPCHK(c, hipMemcpyAsync(val, A.fdg, sizeof(double) * (size_t)A.nnzb * t.nt, hipMemcpyDefault, c->stream));
  HIPCHK(c, hipMemcpyAsync(b, t.rhsb, sizeof(double) * nx, hipMemcpyDefault, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int wai_tracer_system(wai_ctx* c, int tracer, int method, double dt, double ratio, const double* alx_last,
                      const double* alx_last2, double* val, double* b) {
  if (!c || !val || !b) return -2;
  if (int e = tracer_args(c, &tracer, method, alx_last, alx_last2)) return e;
  Tracers& t = c->tr;
  const size_t nx = (size_t)c->mesh.n_owned * t.nt;
  VecArg a1{c}, a2{c};
  if (a1.in(alx_last, nx, 0) || a2.in(alx_last2, nx, 1)) return -1;
  if (launch_tracer_assemble(c, tracer_form(t, tracer, method, dt, ratio), a1.dev, a2.dev, c->w_a)) return -1;
  double* tmp = c->stage[2];  // nnzb scalars fit the staging buffer (>= 23 doubles per cell)
  launch_ell_to_bcsr(c, c->aux.A, tmp);
  pc_invalidate(c);   // (as it always has: the next solve of any system sets up again)
  HIPCHK(c, hipMemcpyAsync(val, tmp, sizeof(double) * c->pat.nnzb, hipMemcpyDefault, c->stream));
  HIPCHK(c, hipMemcpyAsync(b, c->w_a, sizeof(double) * c->mesh.n_owned, hipMemcpyDefault, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int wai_tracer_solve(wai_ctx* c, int method, double dt, double ratio, const double* alx_last,
                     const double* alx_last2, double* X, double* alx_new, int* its, int* reason) {
  if (!c || !X || !alx_new || !its || !reason) return -2;
  if (int e = tracer_args(c, nullptr, method, alx_last, alx_last2, &ratio)) return e;
  Tracers& t = c->tr;
  const size_t nx = (size_t)c->mesh.n_owned * t.nt;
  VecArg a1{c}, a2{c}, xx{c}, an{c};
  if (a1.in(alx_last, nx, 0) || a2.in(alx_last2, nx, 1) || xx.in(X, nx, 2) || an.out_only(alx_new, nx, 3)) return -1;
  *its = 0;
  *reason = 100;
  if (t.mode == WAI_TRACER_COUPLED && t.nt > 1) {
    // one assembly sweep, one factorisation, ONE Krylov solve on the [cell][tracer] vector (timestepper.F90:2345-2355):
    // its iteration count, its reason, the combined preconditioned residual norm against rtol / atol
    LinSys& sys = c->coupled;
    if (int e = coupled_prepare(c)) return e;
    if (launch_tracer_assemble_all(c, method, dt, ratio, a1.dev, a2.dev, t.rhsb)) return -1;
    pc_invalidate(c, sys);
    double rn = 0.0;
    vec_zero(c, xx.dev, sys.n);  // a failed factorisation returns before the solver zeroes it
    if (do_ksp(c, sys, t.rhsb, xx.dev, its, reason, &rn)) return -1;
  } else {
    LinSys& sys = c->aux;
    // the flow solver may never have needed a basis: the one it would have
    if ((sys.ksp.type == WAI_KSP_GMRES || sys.ksp.type == WAI_KSP_LGMRES) && !c->kv.basis && ensure_basis(c, c->flow, c->kv.basis_m)) return -1;
    // ... nor BiCGStab(L)'s vectors: they are shared like the rest, so sized for the flow's vectors, not for a tracer's
    if (sys.ksp.type == WAI_KSP_BCGSL && ensure_bcgsl_vecs(c, c->kv, (size_t)c->flow.nl)) return -1;
    double* b = c->w_a;
    double* x = c->w_c;
    for (int it = 0; it < t.nt; it++) {
      if (launch_tracer_assemble(c, tracer_form(t, it, method, dt, ratio), a1.dev, a2.dev, b)) return -1;
      pc_invalidate(c, sys);   // new values: one factorisation per tracer
      int k = 0, r = 0;
      double rn = 0.0;
      vec_zero(c, x, sys.n);  // a failed factorisation returns before the solver zeroes it
      if (do_ksp(c, sys, b, x, &k, &r, &rn)) return -1;
      *its += k;
      if (r < *reason) *reason = r;
      launch_tracer_put(c, x, it, xx.dev);
    }
  }
  launch_tracer_alx(c, xx.dev, an.dev);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (xx.back() || an.back()) return -1;
  return 0;
}

}  // extern "C"

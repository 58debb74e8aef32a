// The ode_type hooks and the Newton iteration of the reference's SNES callbacks (src/timestepper.F90:587-735, 1898-1951)
// behind the C ABI of libwaiwera_hip.so (include/waiwera_hip.h).  Host code here only orders kernel launches and RCCL
// calls on one HIP stream and reads back a handful of scalars per Krylov iteration; all vectors and matrices stay in HBM.
// The context and its set-up live in context.hip, sources and their controls in sources.hip, the tracer problem in
// tracers.hip, the Krylov drivers in krylov.hip, the preconditioner set-up in pc_setup.hip, the source network in
// network.hip, measurement entry points in measure.hip; host.hpp declares what they share.
#include "host.hpp"

using namespace wai;

namespace wai {

// read and clear the device flags; collective over ranks
int fetch_flags(wai_ctx* c, int out[4]) {
  if (c->comm && c->comm->nranks > 1) {
    // flags -> doubles -> allreduce max (flag 1 is a min: send its negation)
    HIPCHK(c, hipMemcpyAsync(c->h_flags, c->d_flags, 4 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double v[4] = {(double)c->h_flags[0], -(double)c->h_flags[1], (double)c->h_flags[2], (double)c->h_flags[3]};
    HIPCHK(c, hipMemcpyAsync(c->d_red + 2048, v, sizeof(v), hipMemcpyHostToDevice, c->stream));
    if (comm_allreduce(c->comm, c->d_red + 2048, 4, 1, c->stream, c->err)) return -1;
    HIPCHK(c, hipMemcpyAsync(c->h_red + 8, c->d_red + 2048, sizeof(v), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out[0] = (int)c->h_red[8]; out[1] = c->h_flags[1]; out[2] = (int)c->h_red[10]; out[3] = (int)c->h_red[11];
  } else {
    HIPCHK(c, hipMemcpyAsync(c->h_flags, c->d_flags, 4 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < 4; i++) out[i] = c->h_flags[i];
  }
  HIPCHK(c, hipMemcpyAsync(c->d_flags, FLAGS_RESET, sizeof(FLAGS_RESET), hipMemcpyHostToDevice, c->stream));
  return 0;
}

// ---- fluid_properties / pre_eval on device vectors -------------------------------------------
int do_pre_eval(wai_ctx* c, double* y /* nl, device */) {
  if (c->comm && c->mesh.n_halo) {
    if (halo_exchange(c, y, c->np)) return -1;
    launch_region_get(c, c->w_c);
    if (halo_exchange(c, c->w_c, 1)) return -1;
    launch_region_set(c, c->w_c, c->mesh.n_owned, c->mesh.n_halo);
  }
  {
    Prof p(c, KC_EOS);
    launch_eos(c, y, 0, c->mesh.n_prim, false);
  }
  int fl[4];
  if (fetch_flags(c, fl)) return -1;
  return fl[0] ? 1 : 0;
}

int do_residual(wai_ctx* c, double dt, double* y, const double* lhs_old, double* f) {
  int e = do_pre_eval(c, y);
  if (e) return e;
  if (c->net.on && network_update(c)) return -1;
  Prof p(c, KC_RESIDUAL);
  launch_residual(c, dt, lhs_old, f, nullptr, nullptr);
  return 0;
}

int do_jacobian(wai_ctx* c, double dt, const double* y, const double* lhs_old) {
  {
    Prof p(c, KC_EOS);
    launch_eos(c, y, 0, c->mesh.n_prim, true);
  }
  int fl[4];
  if (fetch_flags(c, fl)) return -1;
  if (fl[0]) return 1;
  Prof p(c, KC_JACOBIAN);
  if (launch_jacobian(c, dt, lhs_old)) return -1;
  pc_invalidate(c, c->flow);
  return network_couplings(c, dt, const_cast<double*>(y), lhs_old);   // y is perturbed and restored in place
}

int do_norm2(wai_ctx* c, const double* v, double* out) {
  vec_dot(c, v, v, c->flow.n, S_W2);
  if (allreduce_scal(c, S_W2, 1)) return -1;
  if (read_scal(c, S_W2, 1)) return -1;
  *out = std::sqrt(c->ks.h_scal[S_W2]);
  return 0;
}

int do_max_scaled(wai_ctx* c, const double* v, const double* scale, double tol, double* val, int* idx) {
  if (launch_max_scaled(c, v, scale, tol, val, idx)) return -1;
  if (c->comm && c->comm->nranks > 1) {
    HIPCHK(c, hipMemcpyAsync(c->d_red + 2048, val, sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (comm_allreduce(c->comm, c->d_red + 2048, 1, 1, c->stream, c->err)) return -1;
    HIPCHK(c, hipMemcpyAsync(val, c->d_red + 2048, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return 0;
}

// SNES_convergence (timestepper.F90:1898-1951) + SNESConvergedDefault [PETSc]
int snes_convergence(wai_ctx* c, int it, const double* f, const double* lhs_old, const double* y,
                     const double* update, double fnorm, double* max_residual, int* reason) {
  int loc;
  if (do_max_scaled(c, f, lhs_old, c->opts.ftol_abs, max_residual, &loc)) return -1;
  int r = 0;
  if (std::isnan(fnorm)) r = -4;
  else if (it == 0) { if (fnorm < 1.e-50) r = 3; }
  else if (fnorm <= 1.e-8 * c->fnorm0) r = 4;
  else if (fnorm > 1.e8 * c->fnorm0) r = -9;
  if (it < c->opts.min_newton_its) r = 0;  // nonlinear_solver_minimum_iterations (:1930-1932)
  else if (*max_residual < c->opts.ftol_rel) r = 1;
  else if (it > 0) {
    double mu;
    if (do_max_scaled(c, update, y, c->opts.utol_abs, &mu, &loc)) return -1;
    if (mu <= c->opts.utol_rel) r = 2;
  }
  *reason = r;
  return 0;
}

// one Newton iteration on device vectors y (nl), lhs_old (n), f (n)
int do_newton_step(wai_ctx* c, double dt, int iter, double* y, const double* lhs_old, double* f,
                   int* ksp_its, int* reason, double* max_residual) {
  const int n = c->flow.n;
  *ksp_its = 0;
  if (iter == 0 && do_norm2(c, f, &c->fnorm0)) return -1;
  // SNES_pre_iteration_update (flow_simulation.F90:2120): last_iteration_fluid = fluid.  Inside the device-resident Newton
  // step its only reader is the transition sweep, which reads temperature, region and old region of it (k_transitions) --
  // three consecutive planes of the 23 (F_T, F_REGION, F_OLD_REGION): 0.24 GB instead of 1.85 GB per iteration at 10 M
  // cells.  (wai_pre_iteration, the callback of the boundary, copies the whole record.)
  static_assert(F_REGION == F_T + 1 && F_OLD_REGION == F_T + 2, "the transition sweep's planes are consecutive");
  HIPCHK(c, hipMemcpyAsync(c->flu_last_iter + (size_t)F_T * c->mesh.n_local, c->flu + (size_t)F_T * c->mesh.n_local,
                           sizeof(double) * (size_t)3 * c->mesh.n_local, hipMemcpyDeviceToDevice, c->stream));
  c->last_iter_partial = true;   // wai_get_fluid(ctx, 1, ..) refuses until wai_pre_iteration makes the whole record again
  int e = do_jacobian(c, dt, y, lhs_old);
  if (e < 0) return -1;
  if (e > 0) { *reason = -3; return 0; }
  int kreason = 0;
  double rn = 0.0;
  if (do_ksp(c, c->flow, f, c->w_delta, ksp_its, &kreason, &rn)) return -1;
  if (kreason < 0) { *reason = -3; return 0; }
  // SNES_linesearch, lambda = 1
  vec_copy(c, c->w_yold, y, c->flow.nl);
  vec_waxpy(c, y, -1.0, c->w_delta, c->w_yold, n);
  {
    Prof p(c, KC_TRANSITIONS);
    launch_transitions(c, c->w_yold, c->w_delta, y);
  }
  int fl[4];
  if (fetch_flags(c, fl)) return -1;
  if (fl[0]) { *reason = -3; return 0; }
  if (iter < c->opts.max_newton_its - 1) {
    e = do_residual(c, dt, y, lhs_old, f);
    if (e < 0) return -1;
    if (e > 0) { *reason = -3; return 0; }
  }
  double fnorm;
  if (do_norm2(c, f, &fnorm)) return -1;
  if (snes_convergence(c, iter + 1, f, lhs_old, y, c->w_delta, fnorm, max_residual, reason)) return -1;
  if (!*reason && iter + 1 >= c->opts.max_newton_its) *reason = -5;
  return 0;
}

int snapshot_step(wai_ctx* c) {
  HIPCHK(c, hipMemcpyAsync(c->flu_last_step, c->flu, sizeof(double) * (size_t)c->df * c->mesh.n_local,
                           hipMemcpyDeviceToDevice, c->stream));
  return 0;
}
int restore_step(wai_ctx* c) {
  HIPCHK(c, hipMemcpyAsync(c->flu, c->flu_last_step, sizeof(double) * (size_t)c->df * c->mesh.n_local,
                           hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

}  // namespace wai

extern "C" {

// the flux vector of the reference (flow_simulation.F90:156-205): per face np component fluxes + nmob
// phase fluxes per unit area, positive from cell 1 to cell 2, on the fluid state in force
int wai_get_fluxes(wai_ctx* c, double* out) {
  if (!c || !out) return -2;
  const size_t n = (size_t)c->mesh.n_faces * (c->np + c->nmob);
  if (!n) return 0;
  DevBuf<double> tmp;
  if (tmp.alloc(c, n)) return -1;
  launch_face_fluxes(c, c->mesh.face_cells, tmp);
  HIPCHK(c, hipMemcpyAsync(out, tmp, n * sizeof(double), hipMemcpyDefault, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
int wai_num_flux_dof(wai_ctx* c) { return c ? c->np + c->nmob : -2; }

int wai_get_fluid(wai_ctx* c, int which, double* out) {
  if (!c || !out) return -2;
  if (which == 1 && c->last_iter_partial) {
    // wai_newton_step snapshots only the planes its transition sweep reads: the rest of the record is stale (advisor, round 5)
    c->err = "wai_get_fluid(1): the last-iteration record is partial after wai_newton_step (temperature, region, old region); "
             "call wai_pre_iteration for the whole record";
    return -2;
  }
  const double* src = which == 0 ? c->flu : (which == 1 ? c->flu_last_iter : c->flu_last_step);
  const size_t tot = (size_t)c->df * c->mesh.n_local;
  launch_fluid_aos(c, src, c->stage[0]);
  if (copy_vec(c, out, c->stage[0], tot, TO_CALLER)) return -1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int wai_halo_exchange(wai_ctx* c, double* vec, int dof) {
  if (!c || !vec) return -2;
  VecArg v{c};
  const size_t n = (size_t)dof * c->mesh.n_prim;
  if (v.in(vec, n, 0)) return -1;
  if (halo_exchange(c, v.dev, dof)) return -1;
  return v.back();
}

int wai_pre_timestep(wai_ctx* c) { return c ? snapshot_step(c) : -2; }
int wai_pre_retry_timestep(wai_ctx* c) {
  if (!c) return -2;
  if (c->can_reject) {  // a converged step the adaptor turned down (TIMESTEP_TOO_BIG, :1339,1468-1470)
    std::swap(c->w_hist, c->w_hist_prev);
    c->dt_last = c->dt_last_prev;
    c->taken--;
    c->can_reject = false;
  }
  return restore_step(c);
}
int wai_pre_iteration(wai_ctx* c) {
  if (!c) return -2;
  HIPCHK(c, hipMemcpyAsync(c->flu_last_iter, c->flu, sizeof(double) * (size_t)c->df * c->mesh.n_local,
                           hipMemcpyDeviceToDevice, c->stream));
  c->last_iter_partial = false;
  return 0;
}

// copy the owned part of a caller vector into an nl-sized work vector (halo room)
static int to_work(wai_ctx* c, const double* y, double* work) {
  return copy_vec(c, work, y, c->flow.n, FROM_CALLER);
}
static int from_work(wai_ctx* c, const double* work, double* y) {
  if (copy_vec(c, y, work, c->flow.n, TO_CALLER)) return -1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int wai_pre_eval(wai_ctx* c, double t, const double* y) {
  (void)t;
  if (!c || !y) return -2;
  if (to_work(c, y, c->w_y)) return -1;
  return do_pre_eval(c, c->w_y);
}

int wai_lhs(wai_ctx* c, double t, const double* y, double* lhs) {
  (void)t; (void)y;
  if (!c || !lhs) return -2;
  VecArg o{c};
  if (o.out_only(lhs, c->flow.n, 0)) return -1;
  {
    Prof p(c, KC_RESIDUAL);
    launch_residual(c, 0.0, nullptr, nullptr, o.dev, nullptr);
  }
  return o.back();
}

int wai_rhs(wai_ctx* c, double t, const double* y, double* rhs) {
  (void)t; (void)y;
  if (!c || !rhs) return -2;
  VecArg o{c};
  if (o.out_only(rhs, c->flow.n, 0)) return -1;
  if (c->net.on && network_update(c)) return -1;
  {
    Prof p(c, KC_RESIDUAL);
    launch_residual(c, 0.0, nullptr, nullptr, nullptr, o.dev);
  }
  return o.back();
}

int wai_set_residual_form(wai_ctx* c, int method, double ratio, const double* lhs_last2) {
  if (!c) return -2;
  if (method < WAI_METHOD_BEULER || method > WAI_METHOD_DIRECTSS) { c->err = "unknown time stepping method"; return -1; }
  if (method == WAI_METHOD_BDF2) {
    if (!lhs_last2 || !(ratio > 0.0)) { c->err = "BDF2 needs a step size ratio > 0 and the lhs two steps back"; return -1; }
    if (lhs_last2 != c->w_lhs2) {
      HIPCHK(c, hipMemcpyAsync(c->w_lhs2, lhs_last2, sizeof(double) * c->flow.n, hipMemcpyDefault, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
  }
  c->method = method;
  c->ratio = ratio;
  return 0;
}

int wai_set_timestep_method(wai_ctx* c, int method) {
  if (!c) return -2;
  if (method < WAI_METHOD_BEULER || method > WAI_METHOD_DIRECTSS) { c->err = "unknown time stepping method"; return -1; }
  c->scheme = method;
  c->taken = 0;
  c->dt_last = 0.0;
  c->can_reject = false;
  c->method = method == WAI_METHOD_DIRECTSS ? WAI_METHOD_DIRECTSS : WAI_METHOD_BEULER;
  return 0;
}

int wai_residual(wai_ctx* c, double t, double dt, const double* y, const double* lhs_old, double* f) {
  (void)t;
  if (!c || !y || !lhs_old || !f) return -2;
  VecArg lo{c}, fo{c};
  if (to_work(c, y, c->w_y) || lo.in(lhs_old, c->flow.n, 1) || fo.out_only(f, c->flow.n, 2)) return -1;
  const int e = do_residual(c, dt, c->w_y, lo.dev, fo.dev);
  if (e) return e;
  return fo.back();
}

int wai_jacobian(wai_ctx* c, double t, double dt, const double* y, const double* lhs_old) {
  (void)t;
  if (!c || !y || !lhs_old) return -2;
  VecArg lo{c};
  if (to_work(c, y, c->w_y) || lo.in(lhs_old, c->flow.n, 1)) return -1;
  if (c->comm && c->mesh.n_halo && halo_exchange(c, c->w_y, c->np)) return -1;
  return do_jacobian(c, dt, c->w_y, lo.dev);
}

int wai_jacobian_nnzb(wai_ctx* c) { return c ? c->pat.nnzb : -2; }

int wai_jacobian_pattern(wai_ctx* c, int* rowptr, int* colidx) {
  if (!c || !rowptr || !colidx) return -2;
  std::memcpy(rowptr, c->pat.h_rowptr.data(), sizeof(int) * (c->pat.n + 1));
  std::memcpy(colidx, c->pat.h_colidx.data(), sizeof(int) * c->pat.nnzb);
  return 0;
}

int wai_jacobian_get_values(wai_ctx* c, double* val) {
  if (!c || !val) return -2;
  const size_t n = (size_t)c->pat.nnzb * c->np * c->np;
  DevBuf<double> tmp;
  if (tmp.alloc(c, n)) return -1;
  launch_ell_to_bcsr(c, c->flow.A, tmp);
  if (copy_vec(c, val, tmp, n, TO_CALLER)) return -1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int wai_jacobian_set_values(wai_ctx* c, const double* val) {
  if (!c || !val) return -2;
  const size_t n = (size_t)c->pat.nnzb * c->np * c->np;
  DevBuf<double> tmp;
  if (tmp.alloc(c, n)) return -1;
  if (copy_vec(c, tmp, val, n, FROM_CALLER)) return -1;
  launch_bcsr_to_ell(c, tmp, c->flow.A);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  pc_invalidate(c, c->flow);
  c->net.cp_valid = false;   // values from outside: the network's blocks of the last wai_jacobian no longer belong
  return 0;
}

int wai_spmv(wai_ctx* c, const double* x, double* y) {
  if (!c || !x || !y) return -2;
  VecArg yo{c};
  double* xd;
  if (is_device_ptr(x) && (!c->comm || c->mesh.n_halo == 0)) xd = const_cast<double*>(x);
  else { if (to_work(c, x, c->w_a)) return -1; xd = c->w_a; if (halo_exchange(c, xd, c->np)) return -1; }
  if (yo.out_only(y, c->flow.n, 1)) return -1;
  {
    Prof p(c, KC_SPMV);
    if (apply_operator(c, c->flow, xd, yo.dev)) return -1;
  }
  return yo.back();
}

int wai_pc_setup(wai_ctx* c) { return c ? do_pc_setup(c, c->flow) : -2; }

int wai_pc_apply(wai_ctx* c, const double* r, double* z) {
  if (!c || !r || !z) return -2;
  read_env(c);
  if (c->ilu.owner != &c->flow) { const int e = do_pc_setup(c, c->flow); if (e) return e; }
  VecArg ri{c}, zo{c};
  if (ri.in(r, c->flow.n, 0) || zo.out_only(z, c->flow.n, 1)) return -1;
  {
    Prof p(c, KC_PC_APPLY);
    if (pc_solve(c, c->flow, ri.dev, zo.dev, PC_DOT_NONE, nullptr, nullptr)) return -1;
  }
  return zo.back();
}

int wai_ksp_solve(wai_ctx* c, const double* b, double* x, int* its, int* reason, double* rnorm) {
  if (!c || !b || !x || !its || !reason || !rnorm) return -2;
  VecArg bi{c}, xo{c};
  if (bi.in(b, c->flow.n, 0) || xo.out_only(x, c->flow.n, 1)) return -1;
  if (do_ksp(c, c->flow, bi.dev, xo.dev, its, reason, rnorm)) return -1;
  return xo.back();
}

int wai_max_scaled(wai_ctx* c, const double* v, const double* scale, double tol, double* val, int* idx) {
  if (!c || !v || !scale || !val || !idx) return -2;
  VecArg a{c}, b{c};
  if (a.in(v, c->flow.n, 0) || b.in(scale, c->flow.n, 1)) return -1;
  return do_max_scaled(c, a.dev, b.dev, tol, val, idx);
}

int wai_post_linesearch(wai_ctx* c, const double* y_old, double* search, double* y, int* changed_search,
                        int* changed_y) {
  if (!c || !y_old || !search || !y) return -2;
  VecArg a{c}, s{c}, yy{c};
  if (a.in(y_old, c->flow.n, 0) || s.in(search, c->flow.n, 1) || yy.in(y, c->flow.n, 2)) return -1;
  {
    Prof p(c, KC_TRANSITIONS);
    launch_transitions(c, a.dev, s.dev, yy.dev);
  }
  int fl[4];
  if (fetch_flags(c, fl)) return -1;
  if (changed_y) *changed_y = fl[2];
  if (changed_search) *changed_search = fl[3];
  if (s.back() || yy.back()) return -1;
  return fl[0] ? 1 : 0;
}

int wai_newton_step(wai_ctx* c, double t, double dt, int iter, double* y, const double* lhs_old, double* f,
                    int* ksp_its, int* reason, double* max_residual) {
  (void)t;
  if (!c || !y || !lhs_old || !f || !ksp_its || !reason || !max_residual) return -2;
  VecArg lo{c}, ff{c};
  if (to_work(c, y, c->w_y) || lo.in(lhs_old, c->flow.n, 1) || ff.in(f, c->flow.n, 2)) return -1;
  if (c->comm && c->mesh.n_halo && halo_exchange(c, c->w_y, c->np)) return -1;
  if (do_newton_step(c, dt, iter, c->w_y, lo.dev, ff.dev, ksp_its, reason, max_residual)) return -1;
  if (from_work(c, c->w_y, y)) return -1;
  return ff.back();
}

int wai_timestep(wai_ctx* c, double t, double dt, double* y, int* newton_its, int* ksp_its, int* reason) {
  (void)t;
  if (!c || !y || !newton_its || !ksp_its || !reason) return -2;
  const int n = c->flow.n;
  *newton_its = 0; *ksp_its = 0; *reason = 0;
  if (to_work(c, y, c->w_y)) return -1;
  if (snapshot_step(c)) return -1;
  vec_copy(c, c->w_b, c->w_y, n);  // saved solution for a failed step
  int e = do_pre_eval(c, c->w_y);
  if (e < 0) return -1;
  int r = 0;
  if (e > 0) r = -3;
  if (!r) {
    launch_residual(c, 0.0, nullptr, nullptr, c->w_lhs, nullptr);  // L(y_old)
    if (c->scheme == WAI_METHOD_BDF2 && c->taken > 0) {
      c->method = WAI_METHOD_BDF2;
      c->ratio = dt / c->dt_last;
      vec_copy(c, c->w_lhs2, c->w_hist, n);
    } else {
      c->method = c->scheme == WAI_METHOD_DIRECTSS ? WAI_METHOD_DIRECTSS : WAI_METHOD_BEULER;
    }
    e = do_residual(c, dt, c->w_y, c->w_lhs, c->w_f);
    if (e < 0) return -1;
    if (e > 0) r = -3;
  }
  if (!r) {
    double fnorm, mr;
    if (do_norm2(c, c->w_f, &fnorm)) return -1;
    c->fnorm0 = fnorm;
    if (snes_convergence(c, 0, c->w_f, c->w_lhs, c->w_y, nullptr, fnorm, &mr, &r)) return -1;
    int it = 0;
    while (!r) {
      int kits = 0;
      if (do_newton_step(c, dt, it, c->w_y, c->w_lhs, c->w_f, &kits, &r, &mr)) return -1;
      *ksp_its += kits;
      it++;
    }
    *newton_its = it;
  }
  *reason = r;
  if (r < 0) {
    vec_copy(c, c->w_y, c->w_b, n);
    if (restore_step(c)) return -1;
    c->can_reject = false;
  } else {
    // accepted: this step's starting lhs is the next step's two-steps-back vector
    std::swap(c->w_hist, c->w_hist_prev);
    vec_copy(c, c->w_hist, c->w_lhs, n);
    c->dt_last_prev = c->dt_last;
    c->dt_last = dt;
    c->taken++;
    c->can_reject = true;
  }
  return from_work(c, c->w_y, y);
}

}  // extern "C"

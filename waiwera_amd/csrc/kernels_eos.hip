// Assembly kernels, pointwise in the cells: EOS evaluation for the state and for the FD Jacobian's perturbed states (K1),
// phase transitions (K11), the separator's saturation enthalpies.  Shared pieces: assembly_device.hip.h.
#include "assembly_device.hip.h"

namespace wai {

// ---- K1: EOS ---------------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(TPB) void k_eos(EosParams ep, const double* __restrict__ y,
                                             double* __restrict__ flu, size_t stride, int first,
                                             int count, int* flags) {
  using E = EosT<KIND>;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const size_t c = (size_t)first + t;
  double yc[E::np];
#pragma unroll
  for (int k = 0; k < E::np; k++) yc[k] = y[c * E::np + k];
  const int region = (int)flu[F_REGION * stride + c];
  CellState<KIND> s;
  if (eos_eval<KIND>(ep, yc, region, s)) { flag_error(flags, (int)c); return; }
  store_state<KIND>(flu, stride, c, s);
}

// perturbed states for the FD Jacobian: thread (k, cell); state k of cell c has primary k
// incremented by h = fd_step(y_ck); region held fixed
template <int KIND>
__global__ __launch_bounds__(TPB) void k_eos_pert(EosParams ep, const double* __restrict__ y,
                                                  const double* __restrict__ flu, size_t stride,
                                                  double* __restrict__ flu_pert,
                                                  double* __restrict__ hstep, int n_prim,
                                                  double eps, double umin, int* flags) {
  using E = EosT<KIND>;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)n_prim * E::np) return;
  const int k = (int)(t / n_prim);
  const size_t c = t - (size_t)k * n_prim;
  double yc[E::np];
#pragma unroll
  for (int q = 0; q < E::np; q++) yc[q] = y[c * E::np + q];
  double h = 0.0;
#pragma unroll
  for (int q = 0; q < E::np; q++)
    if (q == k) { h = fd_step(yc[q], eps, umin); yc[q] += h; }
  hstep[c * E::np + k] = h;
  const int region = (int)flu[F_REGION * stride + c];
  CellState<KIND> s;
  if (eos_eval<KIND>(ep, yc, region, s)) { flag_error(flags, (int)c); return; }
  store_state<KIND>(flu_pert + (size_t)k * E::df * n_prim, (size_t)n_prim, c, s);
}

// ---- K11: transitions ------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(TPB) void k_transitions(EosParams ep, int n_owned,
                                                     double* __restrict__ flu, size_t stride,
                                                     const double* __restrict__ flu_old,
                                                     const double* __restrict__ y_old,
                                                     double* __restrict__ search,
                                                     double* __restrict__ y, int* flags) {
  using E = EosT<KIND>;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_owned) return;
  int region = (int)flu[F_REGION * stride + c];
  const int old_region = (int)flu_old[F_REGION * stride + c];
  const double old_t = flu_old[F_T * stride + c];
  double prim[E::np], oldp[E::np], yo[E::np], yn[E::np];
#pragma unroll
  for (int k = 0; k < E::np; k++) {
    yo[k] = y_old[(size_t)c * E::np + k];
    yn[k] = y[(size_t)c * E::np + k];
  }
  eos_unscale<KIND>(ep, yn, region, prim);
  eos_unscale<KIND>(ep, yo, old_region, oldp);
  flu[F_OLD_REGION * stride + c] = (double)region;
  bool transition = false, changed = false;
  int err;
  if constexpr (is_salt<KIND>)
    err = eos_transition_wse<is_wsge<KIND>>(ep.thermo, oldp, prim, old_region, old_t, region,
                             (int)flu_old[F_OLD_REGION * stride + c], region, transition);
  else
    err = eos_transition<KIND>(ep.thermo, oldp, prim, old_region, old_t, region, transition);
  if (!err) err = eos_check_primary<KIND>(prim, region, changed);
  if (err) { flag_error(flags, c); return; }
  if (transition || changed) {
    if (transition) flu[F_REGION * stride + c] = (double)region;
    eos_scale<KIND>(ep, prim, region, yn);
#pragma unroll
    for (int k = 0; k < E::np; k++) {
      y[(size_t)c * E::np + k] = yn[k];
      search[(size_t)c * E::np + k] = yo[k] - yn[k];
    }
    flags[2] = 1;
    flags[3] = 1;
  }
}

// separator_stage_init (separator.F90:108-136): enthalpies of saturated water and steam at the
// separator pressure; out = {hf, hg, err}
__global__ void k_separator(int thermo, double t1_max, double pressure, double* __restrict__ out) {
  double ts = 0.0, rho = 0.0, u = 0.0;
  int err = th::sat_temperature(thermo, pressure, ts);
  if (!err) err = th::props(thermo, t1_max, 1, pressure, ts, rho, u);
  out[0] = u + pressure / rho;
  if (!err) err = th::props(thermo, t1_max, 2, pressure, ts, rho, u);
  out[1] = u + pressure / rho;
  out[2] = (double)err;
}

// ---- launchers -------------------------------------------------------------------------------
int launch_eos(wai_ctx* c, const double* y, int first, int count, bool perturbed) {
  if (count <= 0) return 0;
  const size_t stride = c->mesh.n_local;
  const int n_prim = c->mesh.n_prim;
  if (with_eos(c->kind, [&](auto k) {
        constexpr int K = decltype(k)::value;
        if (!perturbed)
          hipLaunchKernelGGL(k_eos<K>, grid_for(count), TPB, 0, c->stream, c->ep, y, c->flu, stride, first, count, c->d_flags);
        else
          hipLaunchKernelGGL(k_eos_pert<K>, grid_for((size_t)n_prim * c->np), TPB, 0, c->stream, c->ep, y, c->flu, stride,
                             c->flu_pert, c->hstep, n_prim, c->opts.fd_eps, c->opts.fd_umin, c->d_flags);
      })) return -1;
  return launched(c, perturbed ? "k_eos_pert" : "k_eos");
}

int launch_transitions(wai_ctx* c, const double* y_old, double* search, double* y) {
  const int n = c->mesh.n_owned;
  const size_t stride = c->mesh.n_local;
  if (with_eos(c->kind, [&](auto k) {
        constexpr int K = decltype(k)::value;
        hipLaunchKernelGGL(k_transitions<K>, grid_for(n), TPB, 0, c->stream, c->ep, n, c->flu, stride, c->flu_last_iter, y_old,
                           search, y, c->d_flags);
      })) return -1;
  return launched(c, "k_transitions");
}

int launch_separator(wai_ctx* c, double pressure, double* out) {
  hipLaunchKernelGGL(k_separator, 1, 1, 0, c->stream, c->ep.thermo, c->ep.t1_max, pressure, out);
  return launched(c, "k_separator");
}

}  // namespace wai

// Assembly kernels of the passive tracers: one scalar system per tracer (k_tracer_assemble) or every tracer's system in
// one sweep (k_tracer_assemble_all, the coupled solve), the accumulation coefficients, and the copies between the
// tracer-interleaved and the per-tracer vectors.  Shared pieces: assembly_device.hip.h.
#include "assembly_device.hip.h"

namespace wai {

// ---- tracers: the auxiliary linear problem ------------------------------------------------------
// One scalar system per tracer on the flow Jacobian's sparsity, one thread per owned cell (row):
// aux_lhs (flow_simulation.F90:1489-1556), aux_rhs (:1560-1833: advection with the phase flux,
// upstream by its sign; diffusion with the harmonic porosity*density*saturation factor;
// production / injection; Arrhenius decay), the method's setup_linear (timestepper.F90:458-581)
// and aux_pre_solve (:1837-1959) fused.  The phase fluxes are recomputed from the converged
// fluid state rather than read from a flux store.  Dirichlet boundary cells are
// eliminated into the right-hand side.
template <int KIND>
__device__ __forceinline__ double tracer_coef(const CellState<KIND>& s, const RockState& r, int p) {
  double sat = 0.0, rho = 0.0;
#pragma unroll
  for (int q = 0; q < EosT<KIND>::nph; q++)
    if (q == p) { sat = s.sat[q]; rho = s.rho[q]; }
  return r.phi * sat * rho;  // cell_tracer_balance_coefs, cell.F90:146-164
}

// Arithmetic that k_tracer_assemble and k_tracer_assemble_all share, written once (tests/test_hip_tracer_coupled.py holds
// the two entry points bit-identical).  The source component selection and setup_linear's diagonal / right-hand side are
// NOT among it: behind a helper, in any of the shapes tried, both kernels come out of hipcc with another register
// allocation, so those two stay written out in each kernel and must be edited together.
// apply_tracer_decay (:1776-1831), tracer_decay (tracer.F90:48-61): what Arrhenius decay adds to the row's diagonal
__device__ __forceinline__ double tracer_decay_term(double decay, double activation, double T, double al) {
  return -(decay * exp(-activation / (8.3144598 * (T + 273.15)))) * al;
}
// setup_linear (timestepper.F90:458-581): the factor of Ar in A = cA Ar + cL Al; r1 = ratio + 1
__device__ __forceinline__ double tracer_cA(int method, double dt, double r1) {
  return method == WAI_METHOD_DIRECTSS ? 1.0 : (method == WAI_METHOD_BDF2 ? -dt * r1 : -dt);
}

// WM: the most slots of a row (MAXDEG; MAXDEG_WIDE for cells with 9 .. 16 faces)
template <int KIND, int WM = MAXDEG>
__global__ __launch_bounds__(TPB) void k_tracer_assemble(MeshView m, const double* __restrict__ flu,
                                                         size_t stride, TracerForm tf, int n_prim, int W,
                                                         const double* __restrict__ alx1,
                                                         const double* __restrict__ alx2,
                                                         const double* __restrict__ xbc,
                                                         const double* __restrict__ inj,
                                                         double* __restrict__ aval,
                                                         double* __restrict__ b) {
  using E = EosT<KIND>;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= m.n_owned) return;
  const int p = tf.phase;
  CellState<KIND> own;
  RockState rown;
  load_state<KIND>(flu, stride, c, own);
  load_rock(m.rock, m.n_local, c, rown);
  const double vol = m.vol[c];
  const int dslot = m.diag_blk[c];
  double row[WM];  // Ar by ELL slot
#pragma unroll
  for (int q = 0; q < WM; q++) row[q] = 0.0;
  double diag = 0.0, br = 0.0;
  const double cf_own = tracer_coef<KIND>(own, rown, p);  // cell_diffusion_factor: the same product
  for (int s = 0; s < m.max_deg; s++) {
    const int fs = m.adj_face[(size_t)s * m.n_owned + c];
    if (fs < 0) continue;
    const int o = m.adj_other[(size_t)s * m.n_owned + c];
    const int blk = m.adj_blk[(size_t)s * m.n_owned + c];
    const int side = fs & 1;
    FaceGeom g;
    load_face(m, fs >> 1, g);
    CellState<KIND> oth;
    RockState roth;
    load_state<KIND>(flu, stride, o, oth);
    load_rock(m.rock, m.n_local, o, roth);
    const double pf = side == 0 ? face_phase_flux<KIND>(g, own, rown, oth, roth, p)
                                : face_phase_flux<KIND>(g, oth, roth, own, rown, p);
    const double sign = side ? 1.0 : -1.0;
    // advective: at the upstream cell's column (phase flux >= 0: the face's first cell)
    const bool up_is_own = (pf >= 0.0) == (side == 0);
    const double fa = sign * (pf * g.area) / vol;
    // diffusive: face_diffusion_factor (face.F90:519-536), cell factors porosity*density*saturation
    const double cf_oth = tracer_coef<KIND>(oth, roth, p);
    const double dfac = side == 0 ? harmonic(g, cf_own, cf_oth) : harmonic(g, cf_oth, cf_own);
    const double fd = g.area * dfac * tf.diffusion / (g.d12 * vol);
    double to_own = -fd, to_oth = fd;
    if (up_is_own) to_own += fa; else to_oth += fa;
    diag += to_own;
    if (blk >= 0) {
#pragma unroll
      for (int q = 0; q < WM; q++) row[q] += (q == blk) ? to_oth : 0.0;
    } else {
      br += to_oth * xbc[(size_t)(o - n_prim) * tf.nt + tf.it];
    }
  }
  // sources (tracer_source_iterator, flow_simulation.F90:1722-1772)
  for (int si = m.cell_src[c]; si >= 0; si = m.src_next[si]) {
    const double rate = source_rate<KIND>(own, m.src_ctl, si, m.src_rate[si], m.src_net);
    const int component = source_component(rate, m.src_comp[si], m.src_pcomp[si]);
    if (!(component < E::np)) continue;
    if (rate < 0.0) {
      const int ph = (int)own.phases;
      double frac = 0.0, sum = 0.0;
#pragma unroll
      for (int q = 0; q < E::nph; q++)
        if (ph & (1 << q)) {
          const double mob = own.kr[q] * own.rho[q] / own.mu[q];
          sum += mob;
          if (q == p) frac = mob;
        }
      diag += (frac / sum) * rate / vol;
    } else {
      br += inj[(size_t)si * tf.nt + tf.it] / vol;
    }
  }
  const double al = tracer_coef<KIND>(own, rown, p);
  diag += tracer_decay_term(tf.decay, tf.activation, own.T, al);
  // setup_linear: A = cA Ar + cL Al, b from the history
  const double r = tf.ratio, r1 = r + 1.0;
  const double cA = tracer_cA(tf.method, tf.dt, r1);
  const size_t ix = (size_t)c * tf.nt + tf.it;
  // direct steady state: A = Ar, b = -br.  (Initialised here and overwritten below: leaving it
  // uninitialised with a trailing `else rhs = -br` came out of hipcc 7.2 -O3 as rhs = r1.)
  double rhs = -br;
  diag *= cA;
  if (tf.method == WAI_METHOD_BEULER) {
    diag += al;
    rhs = alx1[ix] + tf.dt * br;
  } else if (tf.method == WAI_METHOD_BDF2) {
    diag += al * (1.0 + 2.0 * r);
    rhs = (alx1[ix] * (r1 * r1) + (-r * r) * alx2[ix]) + (tf.dt * r1) * br;
  }
  // aux_pre_solve: phase absent -> identity row, zero right-hand side
  const bool absent = !(((int)own.phases) & (1 << p));
  const size_t n = m.n_owned;
#pragma unroll
  for (int q = 0; q < WM; q++) {
    if (q < W) {
      double v = (q == dslot) ? diag : cA * row[q];
      if (absent) v = (q == dslot) ? 1.0 : 0.0;
      aval[(size_t)q * n + c] = v;
    }
  }
  b[c] = absent ? 0.0 : rhs;
}

// Every tracer's system in ONE sweep over the faces (the coupled solve, kernels_tracer_block.hip): a face's geometry, the
// two cells' states, each mobile phase's flux, upstream choice and diffusion factor are formed once and serve every tracer
// of that phase; per tracer remain its diffusion coefficient, decay, history and aux_pre_solve's identity row.  The same
// expressions in the same order as k_tracer_assemble, tracer by tracer: identical values.  Two cells share at most one
// face (wai_ctx_create refuses duplicate connections), so a row's off-diagonal entries are stored where their face is met
// (after the row's slots are given their empty value) instead of being collected in registers -- nt rows of up to 16 slots
// would not fit them.  The empty value: k_tracer_assemble writes cA * 0.0 into a slot no face fills, which is -0.0 for the
// transient methods (cA = -dt); the same product here keeps the two entry points bit-identical, sign of zero included; values: aval[(slot * nt + t) * n + cell],
// right-hand side b[cell * nt + t].
template <int KIND>
__global__ __launch_bounds__(TPB) void k_tracer_assemble_all(MeshView m, const double* __restrict__ flu, size_t stride,
                                                             Tracers tr, int method, double dt, double ratio, int n_prim,
                                                             int W, const double* __restrict__ alx1,
                                                             const double* __restrict__ alx2, double* __restrict__ aval,
                                                             double* __restrict__ b) {
  using E = EosT<KIND>;
  constexpr int NT = MAX_TRACERS, NPH = 2;   // tracers live in the mobile phases: liquid, vapour
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= m.n_owned) return;
  const int nt = tr.nt;
  const size_t n = m.n_owned;
  CellState<KIND> own;
  RockState rown;
  load_state<KIND>(flu, stride, c, own);
  load_rock(m.rock, m.n_local, c, rown);
  const double vol = m.vol[c];
  const int dslot = m.diag_blk[c];
  int used = 0;
  for (int t = 0; t < nt; t++) used |= 1 << tr.phase[t];
  const double r = ratio, r1 = r + 1.0;
  const double cA = tracer_cA(method, dt, r1);
  double cf_own[NPH];
#pragma unroll
  for (int p = 0; p < NPH; p++) cf_own[p] = (used >> p) & 1 ? tracer_coef<KIND>(own, rown, p) : 0.0;
  bool absent[NT];
  double diag[NT], br[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) {
    diag[t] = 0.0; br[t] = 0.0;
    absent[t] = t < nt ? !(((int)own.phases) & (1 << tr.phase[t])) : true;
  }
  for (int q = 0; q < W; q++)
    for (int t = 0; t < nt; t++) aval[((size_t)q * nt + t) * n + c] = absent[t] ? 0.0 : cA * 0.0;   // (the sign k_tracer_assemble's empty slots carry)
  for (int s = 0; s < m.max_deg; s++) {
    const int fs = m.adj_face[(size_t)s * m.n_owned + c];
    if (fs < 0) continue;
    const int o = m.adj_other[(size_t)s * m.n_owned + c];
    const int blk = m.adj_blk[(size_t)s * m.n_owned + c];
    const int side = fs & 1;
    FaceGeom g;
    load_face(m, fs >> 1, g);
    CellState<KIND> oth;
    RockState roth;
    load_state<KIND>(flu, stride, o, oth);
    load_rock(m.rock, m.n_local, o, roth);
    const double sign = side ? 1.0 : -1.0;
    double fa[NPH], dfac[NPH];
    bool up_is_own[NPH];
#pragma unroll
    for (int p = 0; p < NPH; p++) {
      fa[p] = 0.0; dfac[p] = 0.0; up_is_own[p] = false;
      if ((used >> p) & 1) {
        const double pf = side == 0 ? face_phase_flux<KIND>(g, own, rown, oth, roth, p)
                                    : face_phase_flux<KIND>(g, oth, roth, own, rown, p);
        up_is_own[p] = (pf >= 0.0) == (side == 0);
        fa[p] = sign * (pf * g.area) / vol;
        const double cf_oth = tracer_coef<KIND>(oth, roth, p);
        dfac[p] = side == 0 ? harmonic(g, cf_own[p], cf_oth) : harmonic(g, cf_oth, cf_own[p]);
      }
    }
#pragma unroll
    for (int t = 0; t < NT; t++) {
      if (t < nt) {
        const int p = tr.phase[t];
        const double fap = p ? fa[1] : fa[0], dfp = p ? dfac[1] : dfac[0];
        const bool up = p ? up_is_own[1] : up_is_own[0];
        const double fd = g.area * dfp * tr.diffusion[t] / (g.d12 * vol);
        double to_own = -fd, to_oth = fd;
        if (up) to_own += fap; else to_oth += fap;
        diag[t] += to_own;
        if (blk >= 0) aval[((size_t)blk * nt + t) * n + c] = absent[t] ? 0.0 : cA * (0.0 + to_oth);
        else br[t] += to_oth * tr.bc[(size_t)(o - n_prim) * nt + t];
      }
    }
  }
  // sources (tracer_source_iterator, flow_simulation.F90:1722-1772)
  for (int si = m.cell_src[c]; si >= 0; si = m.src_next[si]) {
    const double rate = source_rate<KIND>(own, m.src_ctl, si, m.src_rate[si], m.src_net);
    const int component = source_component(rate, m.src_comp[si], m.src_pcomp[si]);
    if (!(component < E::np)) continue;
    if (rate < 0.0) {
      const int ph = (int)own.phases;
      double mobq[NPH] = {0.0, 0.0}, sum = 0.0;
#pragma unroll
      for (int q = 0; q < E::nph; q++)
        if (ph & (1 << q)) {
          const double mob = own.kr[q] * own.rho[q] / own.mu[q];
          sum += mob;
          if (q < NPH) mobq[q] = mob;
        }
#pragma unroll
      for (int t = 0; t < NT; t++)
        if (t < nt) diag[t] += ((tr.phase[t] ? mobq[1] : mobq[0]) / sum) * rate / vol;
    } else {
#pragma unroll
      for (int t = 0; t < NT; t++)
        if (t < nt) br[t] += tr.inj[(size_t)si * nt + t] / vol;
    }
  }
#pragma unroll
  for (int t = 0; t < NT; t++) {
    if (t < nt) {
      const double al = tr.phase[t] ? cf_own[1] : cf_own[0];
      double d = diag[t];
      d += tracer_decay_term(tr.decay[t], tr.activation[t], own.T, al);
      // setup_linear: A = cA Ar + cL Al, b from the history
      const size_t ix = (size_t)c * nt + t;
      double rhs = -br[t];
      d *= cA;
      if (method == WAI_METHOD_BEULER) {
        d += al;
        rhs = alx1[ix] + dt * br[t];
      } else if (method == WAI_METHOD_BDF2) {
        d += al * (1.0 + 2.0 * r);
        rhs = (alx1[ix] * (r1 * r1) + (-r * r) * alx2[ix]) + (dt * r1) * br[t];
      }
      // aux_pre_solve: phase absent -> identity row, zero right-hand side
      aval[((size_t)dslot * nt + t) * n + c] = absent[t] ? 1.0 : d;
      b[ix] = absent[t] ? 0.0 : rhs;
    }
  }
}

template <int KIND>
__global__ __launch_bounds__(TPB) void k_tracer_lhs(MeshView m, const double* __restrict__ flu, size_t stride,
                                                    Tracers tr, double* __restrict__ Al) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= m.n_owned) return;
  CellState<KIND> own;
  RockState rown;
  load_state<KIND>(flu, stride, c, own);
  load_rock(m.rock, m.n_local, c, rown);
  for (int it = 0; it < tr.nt; it++) Al[(size_t)c * tr.nt + it] = tracer_coef<KIND>(own, rown, tr.phase[it]);
}

__global__ __launch_bounds__(TPB) void k_tracer_pick(const double* __restrict__ X, int n, int nt, int it,
                                                     double* __restrict__ x) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < n) x[c] = X[(size_t)c * nt + it];
}
__global__ __launch_bounds__(TPB) void k_tracer_put(const double* __restrict__ x, int n, int nt, int it,
                                                    double* __restrict__ X) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < n) X[(size_t)c * nt + it] = x[c];
}
__global__ __launch_bounds__(TPB) void k_tracer_alx(const double* __restrict__ Al, const double* __restrict__ X,
                                                    size_t n, double* __restrict__ alx) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) alx[i] = Al[i] * X[i];
}

// ---- launchers -------------------------------------------------------------------------------
int launch_tracer_assemble(wai_ctx* c, const TracerForm& tf, const double* alx_last,
                           const double* alx_last2, double* b) {
  const MeshView m = view(c);
  c->tr.n_sweeps++;
  if (with_eos(c->kind, [&](auto k) {
        constexpr int K = decltype(k)::value;
        // rows indexed by ELL slot: up to W of them (wai_ctx_create refuses rows of more than MAXDEG_WIDE blocks)
        if (c->pat.W > MAXDEG)
          hipLaunchKernelGGL((k_tracer_assemble<K, MAXDEG_WIDE>), grid_for(m.n_owned), TPB, 0, c->stream, m, c->flu,
                             (size_t)c->mesh.n_local, tf, c->mesh.n_prim, c->pat.W, alx_last, alx_last2, c->tr.bc, c->tr.inj,
                             c->aux.A.val, b);
        else
          hipLaunchKernelGGL((k_tracer_assemble<K>), grid_for(m.n_owned), TPB, 0, c->stream, m, c->flu,
                             (size_t)c->mesh.n_local, tf, c->mesh.n_prim, c->pat.W, alx_last, alx_last2, c->tr.bc, c->tr.inj,
                             c->aux.A.val, b);
      })) return -1;
  return launched(c, "k_tracer_assemble");
}

int launch_tracer_assemble_all(wai_ctx* c, int method, double dt, double ratio, const double* alx_last,
                               const double* alx_last2, double* b) {
  const MeshView m = view(c);
  c->tr.n_sweeps++;
  if (with_eos(c->kind, [&](auto k) {
        constexpr int K = decltype(k)::value;
        hipLaunchKernelGGL(k_tracer_assemble_all<K>, grid_for(m.n_owned), TPB, 0, c->stream, m, c->flu,
                           (size_t)c->mesh.n_local, c->tr, method, dt, ratio, c->mesh.n_prim, c->pat.W, alx_last, alx_last2,
                           c->coupled.A.val, b);
      })) return -1;
  return launched(c, "k_tracer_assemble_all");
}

int launch_tracer_lhs(wai_ctx* c, double* Al) {
  const MeshView m = view(c);
  if (with_eos(c->kind, [&](auto k) {
        constexpr int K = decltype(k)::value;
        hipLaunchKernelGGL(k_tracer_lhs<K>, grid_for(m.n_owned), TPB, 0, c->stream, m, c->flu, (size_t)c->mesh.n_local, c->tr, Al);
      })) return -1;
  return launched(c, "k_tracer_lhs");
}

int launch_tracer_pick(wai_ctx* c, const double* X, int it, double* x) {
  const int n = c->mesh.n_owned;
  hipLaunchKernelGGL(k_tracer_pick, grid_for(n), TPB, 0, c->stream, X, n, c->tr.nt, it, x);
  return launched(c, "k_tracer_pick");
}
int launch_tracer_put(wai_ctx* c, const double* x, int it, double* X) {
  const int n = c->mesh.n_owned;
  hipLaunchKernelGGL(k_tracer_put, grid_for(n), TPB, 0, c->stream, x, n, c->tr.nt, it, X);
  return launched(c, "k_tracer_put");
}
int launch_tracer_alx(wai_ctx* c, const double* X, double* alx) {
  const size_t n = (size_t)c->mesh.n_owned * c->tr.nt;
  if (launch_tracer_lhs(c, alx)) return -1;  // Al of the current fluid, multiplied in place
  hipLaunchKernelGGL(k_tracer_alx, grid_for(n), TPB, 0, c->stream, alx, X, n, alx);
  return launched(c, "k_tracer_alx");
}

}  // namespace wai

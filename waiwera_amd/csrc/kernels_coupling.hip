// The batched coupling build (wai_set_coupling_build, WAI_COUPLING_BUILD_BATCHED): all m * bs columns of the source
// network's Jacobian blocks E at once, each on private scratch (coupling_batch.hpp), in five launches whatever m is --
// where the column loop (network_couplings, network.hip) borrows y, the fluid record and Sources::net / enth for one column
// at a time and spends about thirteen launches on it.  Nothing global is written but the blocks and their flag.
//   k_cb_states   per column: h, and the record of cell j on y_jk + h (k_cp_perturb + k_eos)
//   k_cb_raw      per (column, source): the sources' own rates and enthalpies on it (k_source_rates, factors off)
//   k_cb_rows<0>  per (column, network row): g0, the residual with the global factors held (k_residual's row list)
//   k_cb_pass     per column, one wave: the network pass in LDS on the private raw rates (k_network_pass)
//   k_cb_rows<1>  per (column, network row): g1 with the column's factors, and E = (g1 - g0) / h (k_cp_diff)
// The same device functions, the same operations in the same order as the column loop's kernels, no FMA contraction (an
// assembly unit, waiwera_amd/build.py): the column loop is the oracle, bit for bit.
#include "assembly_device.hip.h"
#include "network_pass.hpp"
#include "network_wave.hpp"

namespace wai {

// one chunk's columns: scratch as CouplingBatch lays it out, column q of the chunk being column col0 + q of E
struct CbView {
  double* scratch;
  const int* cells;     // the network's cells [m], rows and columns alike (one rank)
  long long per_col;
  int off_rec, off_raw, off_net, off_enth, off_g0;
  int col0, ncol, m, ml, n_src;
};
static_assert(std::is_trivially_copyable<CbView>::value, "a kernel argument holds views, never an owner");

// the record of cell c as column `col` sees it: its own where c is the column's cell, the global one otherwise
template <int KIND>
__device__ __forceinline__ void cb_load_state(const double* __restrict__ flu, size_t stride, const double* col, int off_rec, int cj,
                                              int c, CellState<KIND>& s) {
  if (c == cj) load_state<KIND>(col + off_rec, 1, 0, s);
  else load_state<KIND>(flu, stride, c, s);
}

template <int KIND>
__global__ __launch_bounds__(TPB) void k_cb_states(EosParams ep, CbView v, const double* __restrict__ y,
                                                   const double* __restrict__ flu, size_t stride, double umin, double eps) {
  using E = EosT<KIND>;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= v.ncol) return;
  const int q = v.col0 + t, j = q / E::np, k = q % E::np;
  const size_t c = (size_t)v.cells[j];
  double* col = v.scratch + (size_t)t * v.per_col;
  double yc[E::np];
#pragma unroll
  for (int i = 0; i < E::np; i++) yc[i] = y[c * E::np + i];
  double h = 0.0;
#pragma unroll
  for (int i = 0; i < E::np; i++)
    if (i == k) {   // k_cp_perturb's rule
      const double y0 = yc[i];
      double dx = y0;
      if (fabs(dx) < umin) dx = dx >= 0.0 ? umin : -umin;
      h = dx * eps;
      yc[i] = y0 + h;
    }
  col[0] = h;
  double* rec = col + v.off_rec;
  for (int f = 0; f < E::df; f++) rec[f] = flu[(size_t)f * stride + c];
  const int region = (int)flu[F_REGION * stride + c];
  CellState<KIND> s;
  // a perturbed state outside the EOS's range: the column keeps the unperturbed record (k_eos returns without storing),
  // and no flag is raised -- the perturbed-state sweep of A reported it
  if (eos_eval<KIND>(ep, yc, region, s)) return;
  store_state<KIND>(rec, 1, 0, s);
}

// m.src_net is null: the sources' own controls, before the network pass.  enth: the column's copy of the global array
template <int KIND>
__global__ __launch_bounds__(TPB) void k_cb_raw(MeshView m, CbView v, const int* __restrict__ src_cell,
                                                const double* __restrict__ flu, size_t stride) {
  using E = EosT<KIND>;
  const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (size_t)v.ncol * v.n_src) return;
  const int t = (int)(id / v.n_src), si = (int)(id % v.n_src), n_src = v.n_src;
  double* col = v.scratch + (size_t)t * v.per_col;
  const int cj = v.cells[(v.col0 + t) / E::np];
  CellState<KIND> s;
  cb_load_state<KIND>(flu, stride, col, v.off_rec, cj, src_cell[si], s);
  const double q = source_rate<KIND>(s, m.src_ctl, si, m.src_rate[si], m.src_net);
  double h = m.src_enth[si];
  col[v.off_enth + si] = h;
  if (!(q > 0.0)) {
    const int phases = (int)s.phases;
    double sum = 0.0;
    h = 0.0;
#pragma unroll
    for (int p = 0; p < E::nph; p++) if (phases & (1 << p)) sum += s.kr[p] * s.rho[p] / s.mu[p];
    if constexpr (!E::isothermal) {
      if (m.src_pcomp[si] < E::np) {   // a production component np produces heat alone: no enthalpy is formed (source.F90:419-425)
#pragma unroll
        for (int p = 0; p < E::nph; p++)
          if (phases & (1 << p)) h += (s.kr[p] * s.rho[p] / s.mu[p] / sum) * s.h[p];
      }
    }
  }
  col[v.off_raw + si] = q;
  col[v.off_raw + n_src + si] = h;
}

// SECOND 0: g0 -> scratch; 1: the column's factors stand in for Sources::net / enth, E[i][j][:][k] = (g1 - g0) / h -> val
template <int KIND, int SECOND>
__global__ __launch_bounds__(TPB) void k_cb_rows(MeshView m, CbView v, const double* __restrict__ flu, size_t stride, ResForm rf,
                                                 double* __restrict__ val, int* __restrict__ flag) {
  using E = EosT<KIND>;
  const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (size_t)v.ncol * v.ml) return;
  const int t = (int)(id / v.ml), i = (int)(id % v.ml);
  double* col = v.scratch + (size_t)t * v.per_col;
  const int q = v.col0 + t, j = q / E::np, kq = q % E::np;
  const int cj = v.cells[j], c = v.cells[i];
  if constexpr (SECOND != 0) { m.src_net = col + v.off_net; m.src_enth = col + v.off_enth; }
  CellState<KIND> own;
  RockState rown;
  cb_load_state<KIND>(flu, stride, col, v.off_rec, cj, c, own);
  load_rock(m.rock, m.n_local, c, rown);
  const double vol = m.vol[c];
  double L[E::np], R[E::np];
  cell_balance<KIND>(own, rown, L);
#pragma unroll
  for (int k = 0; k < E::np; k++) R[k] = 0.0;
  for (int s = 0; s < m.max_deg; s++) {
    const int fs = m.adj_face[(size_t)s * m.n_owned + c];
    if (fs < 0) continue;
    const int o = m.adj_other[(size_t)s * m.n_owned + c];
    FaceGeom g;
    load_face(m, fs >> 1, g);
    CellState<KIND> oth;
    RockState roth;
    cb_load_state<KIND>(flu, stride, col, v.off_rec, cj, o, oth);
    load_rock(m.rock, m.n_local, o, roth);
    double term[E::np];
    slot_term<KIND>(g, fs & 1, own, rown, oth, roth, vol, term);
#pragma unroll
    for (int k = 0; k < E::np; k++) R[k] += term[k];
  }
  source_terms<KIND>(m, c, own, vol, R, false);
  double* g0 = col + v.off_g0 + (size_t)i * E::np;
#pragma unroll
  for (int r = 0; r < E::np; r++) {
    const size_t ix = (size_t)c * E::np + r;
    const double fv = res_form(rf, L[r], R[r], rf.last[ix], rf.method == WAI_METHOD_BDF2 ? rf.last2[ix] : 0.0);
    if constexpr (SECOND == 0) g0[r] = fv;
    else {
      const double e = (fv - g0[r]) / col[0];
      val[(((size_t)i * v.m + j) * E::np + r) * E::np + kq] = e;
      if (e != 0.0) atomicOr(flag, 1);
    }
  }
}

// k_network_pass on one column's raw rates: a workgroup of one wave per column, description and state in (dynamic) LDS --
//   [ dw | raw 2n | state (net_state_carve) | iw ]   net_lds_doubles(h) doubles
// -- the factors and the fed sources' enthalpies into the column's scratch, the node states nowhere
__global__ __launch_bounds__(64) void k_cb_pass(NetFlat h, const int* __restrict__ iw, const double* __restrict__ dw, CbView v) {
  extern __shared__ double lds[];
  if ((int)blockIdx.x >= v.ncol) return;
  double* col = v.scratch + (size_t)blockIdx.x * v.per_col;
  const double* raw = col + v.off_raw;
  const int t = threadIdx.x, n = h.n_src;
  double* sdw = lds;
  double* sraw = sdw + h.n_dw;
  double* sstate = sraw + 2 * n;
  int* siw = reinterpret_cast<int*>(sstate + net_state_doubles(h));
  for (int i = t; i < h.n_dw; i += 64) sdw[i] = dw[i];
  for (int i = t; i < 2 * n; i += 64) sraw[i] = raw[i];
  for (int i = t; i < h.n_iw; i += 64) siw[i] = iw[i];
  __syncthreads();
  const NetFlatView fv{h, siw, sdw};
  NetState s;
  net_state_carve(h, sstate, s);
  s.net = col + v.off_net; s.enth = col + v.off_enth;
  network_pass_sources(fv, sraw, s, t, 64);
  __syncthreads();
  if (t == 0) network_pass_serial(fv, sraw, s);
  __syncthreads();
  network_pass_final(fv, sraw, s, t, 64);
}

// k_cb_pass with the wave-wide walk (wai_set_network_walk; network_wave.hpp), as k_network_pass_wave:
//   [ dw | raw 2n | state | staging | iw | ww ]   net_wave_lds_doubles(h, w) doubles, up to 160 KiB
__global__ __launch_bounds__(64) void k_cb_pass_wave(NetFlat h, NetWave w, const int* __restrict__ iw, const double* __restrict__ dw,
                                                     const int* __restrict__ ww, CbView v) {
  extern __shared__ double lds[];
  if ((int)blockIdx.x >= v.ncol) return;   // (the whole workgroup alike)
  double* col = v.scratch + (size_t)blockIdx.x * v.per_col;
  NetState s;
  net_wave_pass_lds(h, w, iw, dw, ww, col + v.off_raw, col + v.off_net, col + v.off_enth, lds, s);
}

// wave: k_cb_pass_wave stands in for k_cb_pass (net_wave_usable, host.hpp); the scratch plan is the same
int launch_coupling_batch(wai_ctx* c, const CouplingBatch& b, int col0, int ncol, double dt, const double* y, const double* lhs_old,
                          long long* launches, bool wave) {
  const Network& nw = c->net;
  const int ml = (int)nw.cp_cells.size(), n = c->src.n;
  if (ncol <= 0 || ncol > b.chunk || col0 < 0 || col0 + ncol > b.ncol || (long long)ncol * b.per_col > nw.cb_doubles ||
      nw.flat.h.n_src != n || ml * c->np != b.ncol) {
    c->err = "coupling batch: a chunk outside its scratch plan";
    return -1;
  }
  CbView v;
  v.scratch = nw.d_cb_scratch; v.cells = nw.d_cp_cells; v.per_col = b.per_col;
  v.off_rec = b.off_rec; v.off_raw = b.off_raw; v.off_net = b.off_net; v.off_enth = b.off_enth; v.off_g0 = b.off_g0;
  v.col0 = col0; v.ncol = ncol; v.m = ml; v.ml = ml; v.n_src = n;
  const MeshView m = view(c);
  MeshView mraw = m;
  mraw.src_net = nullptr;
  const size_t stride = c->mesh.n_local;
  const ResForm rf = res_form_of(c, dt, lhs_old);
  size_t lds = sizeof(double) * (size_t)net_lds_doubles(nw.flat.h);
  if (wave && net_wave_allow_lds(c, reinterpret_cast<const void*>(&k_cb_pass_wave), 2, &lds)) return -1;
  const char* kernel = "k_cb_states";
  int e = with_eos(c->kind, [&](auto k) {
    constexpr int K = decltype(k)::value;
    hipLaunchKernelGGL(k_cb_states<K>, grid_for(ncol), TPB, 0, c->stream, c->ep, v, y, (const double*)c->flu, stride, c->opts.fd_umin,
                       c->opts.fd_eps);
    if (launched(c, kernel)) return;
    kernel = "k_cb_raw";
    hipLaunchKernelGGL(k_cb_raw<K>, grid_for((size_t)ncol * n), TPB, 0, c->stream, mraw, v, (const int*)c->src.cell,
                       (const double*)c->flu, stride);
    if (launched(c, kernel)) return;
    kernel = "k_cb_rows";
    hipLaunchKernelGGL((k_cb_rows<K, 0>), grid_for((size_t)ncol * ml), TPB, 0, c->stream, m, v, (const double*)c->flu, stride, rf,
                       (double*)nw.d_cp_val, (int*)nw.d_cp_flag);
    if (launched(c, kernel)) return;
    kernel = "k_cb_pass";
    if (wave)
      hipLaunchKernelGGL(k_cb_pass_wave, ncol, 64, lds, c->stream, nw.flat.h, nw.wave.w, (const int*)nw.d_flat_iw,
                         (const double*)nw.d_flat_dw, (const int*)nw.d_wave_ww, v);
    else
      hipLaunchKernelGGL(k_cb_pass, ncol, 64, lds, c->stream, nw.flat.h, (const int*)nw.d_flat_iw, (const double*)nw.d_flat_dw, v);
    if (launched(c, kernel)) return;
    kernel = "k_cb_rows";
    hipLaunchKernelGGL((k_cb_rows<K, 1>), grid_for((size_t)ncol * ml), TPB, 0, c->stream, m, v, (const double*)c->flu, stride, rf,
                       (double*)nw.d_cp_val, (int*)nw.d_cp_flag);
    if (launched(c, kernel)) return;
    kernel = nullptr;
  });
  if (e || kernel) return -1;
  if (launches) *launches += 5;
  return 0;
}

}  // namespace wai

// Assembly kernels: accumulation + cell-centric flux gather + residual form in one sweep (K2-K4) -- k_residual_tile with
// the workgroup's cells staged in LDS (the default) and k_residual --, the source-rate and face-flux outputs evaluated
// with the same terms, the scaled max-norm (K10) and the layout copies.  Shared pieces: assembly_device.hip.h.
#include "assembly_device.hip.h"

namespace wai {

// ---- K2-K4: residual -------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(TPB) void k_residual(MeshView m, const double* __restrict__ flu,
                                                  size_t stride, ResForm rf,
                                                  double* __restrict__ f, double* __restrict__ lhs_out,
                                                  double* __restrict__ rhs_out,
                                                  const int* __restrict__ only, int n_only) {
  using E = EosT<KIND>;
  int c;
  if (only) {   // the listed rows alone (the source network's cells, network_couplings in network.hip)
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= n_only) return;
    c = only[t];
  } else {
    c = xcd_cell(m.n_owned);
    if (c < 0) return;
  }
  CellState<KIND> own;
  RockState rown;
  load_state<KIND>(flu, stride, c, own);
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
    load_state<KIND>(flu, stride, o, oth);
    load_rock(m.rock, m.n_local, o, roth);
    double term[E::np];
    slot_term<KIND>(g, fs & 1, own, rown, oth, roth, vol, term);
#pragma unroll
    for (int k = 0; k < E::np; k++) R[k] += term[k];
  }
  source_terms<KIND>(m, c, own, vol, R, only == nullptr);   // a full sweep is an unperturbed evaluation (the row list: network_couplings)
#pragma unroll
  for (int k = 0; k < E::np; k++) {
    if (lhs_out) lhs_out[(size_t)c * E::np + k] = L[k];
    if (rhs_out) rhs_out[(size_t)c * E::np + k] = R[k];
    if (f) {
      const size_t i = (size_t)c * E::np + k;
      f[i] = res_form(rf, L[k], R[k], rf.last[i], rf.method == WAI_METHOD_BDF2 ? rf.last2[i] : 0.0);
    }
  }
}

// ---- K2-K4 with the workgroup's own cells staged in LDS -----------------------------------------------
// k_residual gathers a neighbour's record (state + rock: 26 doubles for eos we) from memory for every face, in-brick
// neighbours included, and NONE of these gathers hits a cache: the XCD's 32 CUs stream ~14 MB of records through its
// 4 MB L2 while a workgroup lives, so a line fetched as one wave's own record is gone when another wave asks for it as
// a neighbour's (PMC, 216^3: 1.6 KB of L2-miss traffic per cell = every load of the kernel, 3.4 x the algorithmic
// bytes).  Here a workgroup's T = 256 consecutive cells (half a 16 x 16 x 2 brick) park the records they have loaded
// anyway -- state as park_state lays it out, and the rock fields the flux reads -- in LDS, field-major (a wave
// instruction reads or writes 64 consecutive doubles of one plane: conflict-free), and a neighbour inside the tile is
// read from there; only neighbours outside the tile (the brick above / below, the other half) are gathered from memory.
// Same loads of the same doubles, same arithmetic in the same order: bit-identical residuals.
template <int KIND> struct ResTile {
  using E = EosT<KIND>;
  static constexpr int nld = ParkT<KIND>::npark, nrk = 5;     // parked state record, rock: k1 k2 k3 wet dry
  static constexpr int lds_bytes = (nld + nrk) * 8 * TPB;
  // the tile needs up to 72 KB (eos wsce / wsae): fine on gfx950's 160 KB, above the 64 KB a workgroup may have on older
  // parts -- launch_residual then falls back to k_residual (as ParkT<>::use does for the Jacobian)
  static bool use(const wai_ctx* c) { return (size_t)lds_bytes <= c->lds_per_block; }
};
template <int KIND>
__global__ __launch_bounds__(TPB) void k_residual_tile(MeshView m, const double* __restrict__ flu,
                                                       size_t stride, ResForm rf,
                                                       double* __restrict__ f, double* __restrict__ lhs_out,
                                                       double* __restrict__ rhs_out) {
  using E = EosT<KIND>;
  constexpr int nld = ResTile<KIND>::nld;
  extern __shared__ double tile[];
  const int st = (int)blockDim.x;
  // the tile: cells c0 .. c1 - 1 (xcd_cell's block mapping)
  const int nblk = (m.n_owned + st - 1) / st, per = (nblk + 7) >> 3;
  const int b = ((int)blockIdx.x & 7) * per + ((int)blockIdx.x >> 3);
  if (((int)blockIdx.x >> 3) >= per || b >= nblk) return;   // padding workgroup (uniform)
  const int c0 = b * st, c1 = min(c0 + st, m.n_owned);
  const int c = c0 + (int)threadIdx.x;
  const bool active = c < c1;
  CellState<KIND> own;
  RockState rown;
  double* rk = tile + (size_t)nld * st + threadIdx.x;
  if (active) {
    load_state<KIND>(flu, stride, c, own);
    load_rock(m.rock, m.n_local, c, rown);
    park_state<KIND>(own, tile + threadIdx.x, st);
    rk[0] = rown.k[0]; rk[st] = rown.k[1]; rk[2 * st] = rown.k[2]; rk[3 * st] = rown.wet; rk[4 * st] = rown.dry;
  }
  __syncthreads();
  if (!active) return;
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
    if (o >= c0 && o < c1) {   // a cell of this tile: its record is in LDS
      const int lo = o - c0;
      unpark_state<KIND>(tile + lo, st, oth);
      const double* ro = tile + (size_t)nld * st + lo;
      roth.k[0] = ro[0]; roth.k[1] = ro[st]; roth.k[2] = ro[2 * st]; roth.wet = ro[3 * st]; roth.dry = ro[4 * st];
      roth.phi = 0.0; roth.rho = 0.0; roth.cp = 0.0;   // the flux reads permeabilities and conductivities only
    } else {
      load_state<KIND>(flu, stride, o, oth);
      load_rock(m.rock, m.n_local, o, roth);
    }
    double term[E::np];
    slot_term<KIND>(g, fs & 1, own, rown, oth, roth, vol, term);
#pragma unroll
    for (int k = 0; k < E::np; k++) R[k] += term[k];
  }
  source_terms<KIND>(m, c, own, vol, R, true);   // a full sweep is an unperturbed evaluation
#pragma unroll
  for (int k = 0; k < E::np; k++) {
    if (lhs_out) lhs_out[(size_t)c * E::np + k] = L[k];
    if (rhs_out) rhs_out[(size_t)c * E::np + k] = R[k];
    if (f) {
      const size_t i = (size_t)c * E::np + k;
      f[i] = res_form(rf, L[k], R[k], rf.last[i], rf.method == WAI_METHOD_BDF2 ? rf.last2[i] : 0.0);
    }
  }
}

// rate and (flowing or injection) enthalpy of every source on the current fluid: the source_rate /
// source_enthalpy output fields
template <int KIND>
__global__ __launch_bounds__(TPB) void k_source_rates(MeshView m, const int* __restrict__ src_cell, int n_src,
                                                      const double* __restrict__ flu, size_t stride,
                                                      double* __restrict__ out) {
  using E = EosT<KIND>;
  const int si = blockIdx.x * blockDim.x + threadIdx.x;
  if (si >= n_src) return;
  CellState<KIND> s;
  load_state<KIND>(flu, stride, src_cell[si], s);
  const double q = source_rate<KIND>(s, m.src_ctl, si, m.src_rate[si], m.src_net);
  double h = m.src_enth[si];
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
  out[si] = q;
  out[n_src + si] = h;
}

// the reference's flux store (flow_simulation.F90:156-205, 1436-1440): per face the np component
// fluxes (mass components, then energy) and the nmob phase fluxes, from cell 1 to cell 2, per unit area
template <int KIND>
__global__ __launch_bounds__(TPB) void k_face_fluxes(MeshView m, const int* __restrict__ face_cells,
                                                     const double* __restrict__ flu, size_t stride,
                                                     double* __restrict__ out) {
  using E = EosT<KIND>;
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= m.n_faces) return;
  const int c1 = face_cells[2 * f], c2 = face_cells[2 * f + 1];
  FaceGeom g;
  load_face(m, f, g);
  CellState<KIND> a, b;
  RockState ra, rb;
  load_state<KIND>(flu, stride, c1, a);
  load_state<KIND>(flu, stride, c2, b);
  load_rock(m.rock, m.n_local, c1, ra);
  load_rock(m.rock, m.n_local, c2, rb);
  double flux[E::np];
  face_flux<KIND>(g, a, ra, b, rb, flux);
  constexpr int nf = E::np + E::nmob;
#pragma unroll
  for (int k = 0; k < E::np; k++) out[(size_t)f * nf + k] = flux[k];
#pragma unroll
  for (int p = 0; p < E::nmob; p++) out[(size_t)f * nf + E::np + p] = face_phase_flux<KIND>(g, a, ra, b, rb, p);
}

// ---- K10: max_i |v_i| / max(|s_i|, tol) with first-index argmax ------------------------------
__global__ __launch_bounds__(TPB) void k_max_scaled(const double* __restrict__ v,
                                                    const double* __restrict__ scale, double tol,
                                                    int n, double* __restrict__ pval,
                                                    int* __restrict__ pidx) {
  double best = -1.0;
  int bi = 0x7fffffff;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const double sc = fmax(fabs(scale[i]), tol);
    double r = fabs(v[i]) / sc;
    if (r != r) r = __builtin_huge_val();  // NaN counts as the maximum
    if (r > best) { best = r; bi = i; }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double ob = __shfl_down(best, off);
    const int oi = __shfl_down(bi, off);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  __shared__ double sb[TPB / 64];
  __shared__ int si[TPB / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) { sb[w] = best; si[w] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int q = 1; q < TPB / 64; q++)
      if (sb[q] > best || (sb[q] == best && si[q] < bi)) { best = sb[q]; bi = si[q]; }
    pval[blockIdx.x] = best;
    pidx[blockIdx.x] = bi;
  }
}

// one wave: lanes scan the per-block results strided, then the same first-index tie-break across lanes (a single
// thread walking ~1000 dependent loads took 100 us -- 6 % of a Newton step's fixed part at a rank's share of 216^3)
__global__ void k_max_scaled_final(int nb, double* pval, int* pidx) {
  if (blockIdx.x != 0 || threadIdx.x >= 64) return;
  double best = -1.0;
  int bi = 0x7fffffff;
  for (int q = threadIdx.x; q < nb; q += 64) {
    const double v = pval[q];
    const int i = pidx[q];
    if (v > best || (v == best && i < bi)) { best = v; bi = i; }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double ob = __shfl_down(best, off);
    const int oi = __shfl_down(bi, off);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  if (threadIdx.x == 0) { pval[0] = best; pidx[0] = bi; }
}

// ---- layout helpers --------------------------------------------------------------------------
__global__ void k_soa_to_aos(const double* __restrict__ soa, double* __restrict__ aos, int n, int df) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)n * df) return;
  const int f = (int)(t / n);
  const size_t c = t - (size_t)f * n;
  aos[c * df + f] = soa[t];
}
__global__ void k_copy_strided(const double* __restrict__ src, double* __restrict__ dst, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) dst[t] = src[t];
}

// ---- launchers -------------------------------------------------------------------------------
int launch_residual(wai_ctx* c, double dt, const double* lhs_old, double* f, double* lhs_out,
                    double* rhs_out, const int* only, int n_only) {
  const MeshView m = view(c);
  const size_t stride = c->mesh.n_local;
  const ResForm rf = res_form_of(c, dt, lhs_old);
  const char* et = getenv("WAI_RES_TILE");   // read per call: tests compare the two kernels in one process
  const bool tile = !only && !(et && et[0] == '0');   // a full sweep: the workgroup's own cells staged in LDS
  const char* kernel = "k_residual";
  if (with_eos(c->kind, [&](auto k) {
        constexpr int K = decltype(k)::value;
        if (tile && ResTile<K>::use(c)) {
          kernel = "k_residual_tile";
          hipLaunchKernelGGL(k_residual_tile<K>, grid8_for(m.n_owned), TPB, ResTile<K>::lds_bytes, c->stream, m, c->flu, stride,
                             rf, f, lhs_out, rhs_out);
        } else {
          hipLaunchKernelGGL(k_residual<K>, only ? grid_for(n_only) : grid8_for(m.n_owned), TPB, 0, c->stream, m, c->flu, stride,
                             rf, f, lhs_out, rhs_out, only, n_only);
        }
      })) return -1;
  return launched(c, kernel);   // a refused launch must not leave f / lhs / rhs stale in silence
}

int launch_source_rates(wai_ctx* c, double* out, bool raw) {
  MeshView m = view(c);
  if (raw) m.src_net = nullptr;   // rates of the sources' own controls, before the network pass
  if (with_eos(c->kind, [&](auto k) {
        constexpr int K = decltype(k)::value;
        hipLaunchKernelGGL(k_source_rates<K>, grid_for(c->src.n), TPB, 0, c->stream, m, c->src.cell, c->src.n, c->flu,
                           (size_t)c->mesh.n_local, out);
      })) return -1;
  return launched(c, "k_source_rates");
}

int launch_face_fluxes(wai_ctx* c, const int* face_cells, double* out) {
  const MeshView m = view(c);
  if (with_eos(c->kind, [&](auto k) {
        constexpr int K = decltype(k)::value;
        hipLaunchKernelGGL(k_face_fluxes<K>, grid_for(c->mesh.n_faces), TPB, 0, c->stream, m, face_cells, c->flu,
                           (size_t)c->mesh.n_local, out);
      })) return -1;
  return launched(c, "k_face_fluxes");
}

int launch_max_scaled(wai_ctx* c, const double* v, const double* scale, double tol, double* val,
                      int* idx) {
  const int n = c->np * c->mesh.n_owned;
  int nb = grid_for(n);
  if (nb > 1024) nb = 1024;
  double* pval = c->d_red;
  int* pidx = reinterpret_cast<int*>(c->d_red + 1024);
  hipLaunchKernelGGL(k_max_scaled, nb, TPB, 0, c->stream, v, scale, tol, n, pval, pidx);
  if (launched(c, "k_max_scaled")) return -1;
  hipLaunchKernelGGL(k_max_scaled_final, 1, 64, 0, c->stream, nb, pval, pidx);
  if (launched(c, "k_max_scaled_final")) return -1;
  hipMemcpyAsync(c->h_red, pval, sizeof(double), hipMemcpyDeviceToHost, c->stream);
  hipMemcpyAsync(c->h_red + 1, pidx, sizeof(int), hipMemcpyDeviceToHost, c->stream);
  if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
  *val = c->h_red[0];
  *idx = *reinterpret_cast<int*>(c->h_red + 1);
  return 0;
}

int launch_fluid_aos(wai_ctx* c, const double* flu_soa, double* out_aos) {
  const size_t tot = (size_t)c->mesh.n_local * c->df;
  hipLaunchKernelGGL(k_soa_to_aos, grid_for(tot), TPB, 0, c->stream, flu_soa, out_aos,
                     c->mesh.n_local, c->df);
  return launched(c, "k_soa_to_aos");
}

int launch_region_get(wai_ctx* c, double* out) {
  hipLaunchKernelGGL(k_copy_strided, grid_for(c->mesh.n_prim), TPB, 0, c->stream,
                     c->flu + (size_t)F_REGION * c->mesh.n_local, out, c->mesh.n_prim);
  return launched(c, "k_copy_strided");
}

int launch_region_set(wai_ctx* c, const double* in, int first, int count) {
  if (count <= 0) return 0;
  double* reg = c->flu + (size_t)F_REGION * c->mesh.n_local;
  hipLaunchKernelGGL(k_copy_strided, grid_for(count), TPB, 0, c->stream, in + first, reg + first, count);
  return launched(c, "k_copy_strided");
}

}  // namespace wai

// The source network on the device (wai_set_network_pass, WAI_NETWORK_PASS_DEVICE): k_network_pass runs the pass of
// network_pass.hpp -- the text the host runs too -- in one wave on LDS, and three small kernels keep the coupling build's
// column loop (network_couplings, network.hip) on the stream: perturb y, difference the gathered rows into the blocks,
// restore y.  Built without FMA contraction, like the assembly units: the host pass gives the same bits.
#include "context.hpp"
#include "network_pass.hpp"
#include "network_wave.hpp"

namespace wai {

// One workgroup of one wave.  The description (dw, iw), the raw rates and the whole state live in LDS:
//   [ dw | raw 2n | state (net_state_carve) | iw ]          net_lds_doubles(h) <= NET_LDS_DOUBLES, decided by the builder
// The per-source parts are strided over the 64 lanes; lane 0 walks groups and reinjectors.
// raw: launch_source_rates(c, raw, true); net, enth: Sources::net, Sources::enth (enth: fed sources only);
// state_out: sources 6 each, groups 6 each, reinjectors 8 each (net_state_keep)
__global__ __launch_bounds__(64) void k_network_pass(NetFlat h, const int* __restrict__ iw, const double* __restrict__ dw,
                                                     const double* __restrict__ raw, double* __restrict__ net,
                                                     double* __restrict__ enth, double* __restrict__ state_out) {
  __shared__ double lds[NET_LDS_DOUBLES];
  const int t = threadIdx.x, n = h.n_src;
  double* sdw = lds;
  double* sraw = sdw + h.n_dw;
  double* sstate = sraw + 2 * n;
  int* siw = reinterpret_cast<int*>(sstate + net_state_doubles(h));
  for (int i = t; i < h.n_dw; i += 64) sdw[i] = dw[i];
  for (int i = t; i < 2 * n; i += 64) sraw[i] = raw[i];
  for (int i = t; i < h.n_iw; i += 64) siw[i] = iw[i];
  __syncthreads();
  const NetFlatView v{h, siw, sdw};
  NetState s;
  net_state_carve(h, sstate, s);
  s.net = net; s.enth = enth;
  network_pass_sources(v, sraw, s, t, 64);
  __syncthreads();
  if (t == 0) network_pass_serial(v, sraw, s);
  __syncthreads();
  network_pass_final(v, sraw, s, t, 64);
  __syncthreads();
  net_state_keep(h, s, state_out, t, 64);
}

// The same pass with the wave-wide walk (wai_set_network_walk, WAI_NETWORK_WALK_WAVE; network_wave.hpp): one wave, dynamic
// LDS of the network's own size plus the staging run and the schedule (ww), up to 160 KiB
__global__ __launch_bounds__(64) void k_network_pass_wave(NetFlat h, NetWave w, const int* __restrict__ iw, const double* __restrict__ dw,
                                                          const int* __restrict__ ww, const double* __restrict__ raw,
                                                          double* __restrict__ net, double* __restrict__ enth,
                                                          double* __restrict__ state_out) {
  extern __shared__ double lds[];
  const int t = threadIdx.x;
  NetState s;
  net_wave_pass_lds(h, w, iw, dw, ww, raw, net, enth, lds, s);   // (ends with a barrier)
  net_state_keep(h, s, state_out, t, 64);
}

// y_jk + h, with h by the Jacobian's rule (MatFDColoring "ds", as fd_step of the assembly sweeps); yh keeps y_jk and h
__global__ void k_cp_perturb(double* __restrict__ p, double* __restrict__ yh, double umin, double eps) {
  if (threadIdx.x || blockIdx.x) return;
  const double y0 = *p;
  double dx = y0;
  if (fabs(dx) < umin) dx = dx >= 0.0 ? umin : -umin;
  const double h = dx * eps;
  yh[0] = y0; yh[1] = h;
  *p = y0 + h;
}
__global__ void k_cp_restore(double* __restrict__ p, const double* __restrict__ yh) {
  if (threadIdx.x || blockIdx.x) return;
  *p = yh[0];
}
// E[i][j][r][k] = (g1 - g0) / h for the ml x bs gathered rows: g = [g0 (factors held) | g1 (pass redone)]; flag |= 1
// where an entry is nonzero
__global__ void k_cp_diff(int ml, int m, int bs, int j, int k, const double* __restrict__ g, const double* __restrict__ yh,
                          double* __restrict__ val, int* __restrict__ flag) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, mb = ml * bs;
  if (t >= mb) return;
  const int i = t / bs, r = t % bs;
  const double e = (g[mb + t] - g[t]) / yh[1];
  val[((size_t)(i * m + j) * bs + r) * bs + k] = e;
  if (e != 0.0) atomicOr(flag, 1);
}

// the wave kernels take dynamic LDS of the network's own size; above 64 KB a kernel has to be allowed it, once (bit: which)
int net_wave_allow_lds(wai_ctx* c, const void* kernel, int bit, size_t* bytes) {
  const Network& nw = c->net;
  *bytes = sizeof(double) * (size_t)net_wave_lds_doubles(nw.flat.h, nw.wave.w);
  if (!nw.wave_ok || !nw.d_wave_ww || !nw.d_flat_iw || *bytes > sizeof(double) * (size_t)NET_WAVE_LDS_DOUBLES) { c->err = "network wave walk: a network its schedule refused"; return -1; }
  if (c->net_wave_attr & bit) return 0;
  HIPCHK(c, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * NET_WAVE_LDS_DOUBLES)));
  c->net_wave_attr |= bit;
  return 0;
}
// wave: the wave-wide walk (net_wave_usable, host.hpp)
int launch_network_pass(wai_ctx* c, const double* raw, double* net, double* enth, double* state_out, bool wave) {
  const Network& nw = c->net;
  if (wave) {
    size_t lds = 0;
    if (net_wave_allow_lds(c, reinterpret_cast<const void*>(&k_network_pass_wave), 1, &lds)) return -1;
    hipLaunchKernelGGL(k_network_pass_wave, 1, 64, lds, c->stream, nw.flat.h, nw.wave.w, (const int*)nw.d_flat_iw,
                       (const double*)nw.d_flat_dw, (const int*)nw.d_wave_ww, raw, net, enth, state_out);
    return 0;
  }
  hipLaunchKernelGGL(k_network_pass, 1, 64, 0, c->stream, nw.flat.h, (const int*)nw.d_flat_iw, (const double*)nw.d_flat_dw, raw, net,
                     enth, state_out);
  return 0;
}
int launch_cp_perturb(wai_ctx* c, double* p, double* yh) {
  hipLaunchKernelGGL(k_cp_perturb, 1, 1, 0, c->stream, p, yh, c->opts.fd_umin, c->opts.fd_eps);
  return 0;
}
int launch_cp_restore(wai_ctx* c, double* p, const double* yh) {
  hipLaunchKernelGGL(k_cp_restore, 1, 1, 0, c->stream, p, yh);
  return 0;
}
int launch_cp_diff(wai_ctx* c, int ml, int m, int bs, int j, int k, const double* g, const double* yh, double* val, int* flag) {
  hipLaunchKernelGGL(k_cp_diff, (ml * bs + 63) / 64, 64, 0, c->stream, ml, m, bs, j, k, g, yh, val, flag);
  return 0;
}

}  // namespace wai

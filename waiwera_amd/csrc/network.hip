// The source network (groups, reinjectors: src/source_network*.F90) of libwaiwera_hip.so: its host pass between the EOS
// sweep and the residual kernel, the Jacobian blocks it couples cells with (src/flow_simulation.F90:3023-3084), the
// operator (A + E) x, and the ABI entry points that describe and inspect it.
#include "host.hpp"

using namespace wai;

namespace wai {

// ---- source network: groups and reinjectors, one pass --------------------------------------------
// source_network%update (src/source_network.F90:90-130) after the sources' own controls: group sums
// (source_network_group.F90:239-287) and limiters with uniform (:479-534) or progressive (:652-763;
// array_progressive_limit, utils.F90:607-647) scaling, reinjector capacities
// (source_network_reinjector.F90:1014-1112) and distribution with overflow (:1115-1292, :970-1010): network_pass of
// network_pass.hpp, here on the host.  raw: rates, then enthalpies of the sources' own controls; work: the pass' scratch;
// net, enth (null: not wanted): what the residual kernel is handed, per source of the description; kept: net_state_keep.
// Returns the working state (is_out: the sources a reinjector feeds)
static NetState network_pass_host(const NetFlatHost& F, const double* raw, std::vector<double>& work, double* net, double* enth,
                                  double* kept) {
  work.resize((size_t)net_state_doubles(F.h));
  NetState s;
  net_state_carve(F.h, work.data(), s);
  s.net = net; s.enth = enth;
  network_pass(F.view(), raw, s);
  net_state_keep(F.h, s, kept, 0, 1);
  return s;
}

// a stream wait of network_update / network_couplings, counted (wai_test_network_stats)
#define NET_WAIT(c) do { (c)->net_waits++; HIPCHK(c, hipStreamSynchronize((c)->stream)); } while (0)

// the sources' separators and specified enthalpies as they stand now, in the description's doubles
static void network_flat_refresh(Network& nw) {
  if (nw.flat_host_gen == nw.flat_gen) return;
  const NetFlat& h = nw.flat.h;
  for (int i = 0; i < h.n_src; i++) {
    nw.flat.dw[h.src_enth0 + i] = i < (int)nw.h_enth0.size() ? nw.h_enth0[i] : 0.0;
    src_separator(i < (int)nw.h_ctl.size() ? nw.h_ctl[i] : SrcCtl{}, &nw.flat.dw[h.src_sep + 8 * i]);
  }
  nw.flat_host_gen = nw.flat_gen;
}
// ... and the description on the device, where that is older
static int network_flat_upload(wai_ctx* c) {
  Network& nw = c->net;
  if (nw.flat_dev_gen == nw.flat_gen) return 0;
  network_flat_refresh(nw);
  const NetFlat& h = nw.flat.h;
  if (!nw.d_flat_iw && (nw.d_flat_iw.alloc(c, (size_t)h.n_iw) || nw.d_flat_dw.alloc(c, (size_t)h.n_dw) ||
                        nw.d_state.alloc(c, (size_t)net_kept_doubles(h))))
    return -1;
  if (nw.wave_ok && !nw.d_wave_ww) {   // the wave walk's schedule: it changes with the description alone
    if (nw.d_wave_ww.alloc(c, (size_t)std::max(nw.wave.w.n_ww, 1))) return -1;
    HIPCHK(c, hipMemcpyAsync(nw.d_wave_ww, nw.wave.ww.data(), sizeof(int) * (size_t)nw.wave.w.n_ww, hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, hipMemcpyAsync(nw.d_flat_iw, nw.flat.iw.data(), sizeof(int) * (size_t)h.n_iw, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(nw.d_flat_dw, nw.flat.dw.data(), sizeof(double) * (size_t)h.n_dw, hipMemcpyHostToDevice, c->stream));
  NET_WAIT(c);   // (only after the description changed: the host arrays are free again)
  nw.flat_dev_gen = nw.flat_gen;
  return 0;
}

int network_update(wai_ctx* c) {
  Network& nw = c->net;
  const int n = c->src.n;           // local sources
  if (!nw.on) return 0;
  const bool span = nw.n_global > 0;   // (not "gidx is not empty": a rank WITHOUT sources takes part in the gather too)
  const int ng = span ? nw.n_global : n;
  if (ng == 0) return 0;
  c->net_passes++;
  if (net_on_device(c)) {   // k_network_pass: nothing comes to the host and nobody waits
    if (network_flat_upload(c)) return -1;
    launch_source_rates(c, nw.d_raw, true);
    if (launch_network_pass(c, nw.d_raw, c->src.net, c->src.enth, nw.d_state, net_wave_usable(c))) return -1;
    nw.state_on_device = true;
    nw.enth_stale = true;
    return 0;
  }
  nw.state_on_device = false;
  // the sources' own (controlled) rates and flowing enthalpies on the current fluid
  if (n) {
    launch_source_rates(c, nw.d_raw, true);
    HIPCHK(c, hipMemcpyAsync(span ? nw.h_loc.data() : nw.h_raw.data(), nw.d_raw, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, c->stream));
    NET_WAIT(c);
  }
  if (span) {   // all ranks' sources: every rank fills its own entries, the sum is the gather (collective)
    std::fill(nw.h_raw.begin(), nw.h_raw.end(), 0.0);
    for (int i = 0; i < n; i++) { nw.h_raw[nw.gidx[i]] = nw.h_loc[i]; nw.h_raw[ng + nw.gidx[i]] = nw.h_loc[n + i]; }
    HIPCHK(c, hipMemcpyAsync(nw.d_all, nw.h_raw.data(), sizeof(double) * 2 * ng, hipMemcpyHostToDevice, c->stream));
    if (comm_allreduce(c->comm, nw.d_all, 2 * (size_t)ng, 0, c->stream, c->err)) return -1;
    HIPCHK(c, hipMemcpyAsync(nw.h_raw.data(), nw.d_all, sizeof(double) * 2 * ng, hipMemcpyDeviceToHost, c->stream));
    NET_WAIT(c);
  }
  network_flat_refresh(nw);
  const NetState s = network_pass_host(nw.flat, nw.h_raw.data(), nw.h_work, nw.h_net.data(), nw.h_enth.data(), nw.h_state.data());
  if (!n) return 0;
  // hand the result to the device: this rank's (mode, value) pairs -- scale factors of group members, rates of reinjection
  // sources -- and the enthalpies of the sources a reinjector feeds
  bool enth_changed = false;
  const bool stale = nw.enth_stale;   // device passes wrote the fed sources' enthalpies since l_enth was handed over
  nw.enth_stale = false;
  for (int i = 0; i < n; i++) {
    const int g = span ? nw.gidx[i] : i;
    nw.l_net[2 * i] = nw.h_net[2 * g]; nw.l_net[2 * i + 1] = nw.h_net[2 * g + 1];
    if (s.is_out[g] != 0.0 && (nw.h_enth[g] != nw.l_enth[i] || stale)) { nw.l_enth[i] = nw.h_enth[g]; enth_changed = true; }
  }
  HIPCHK(c, hipMemcpyAsync(c->src.net, nw.l_net.data(), sizeof(double) * 2 * n, hipMemcpyHostToDevice, c->stream));
  if (enth_changed)
    HIPCHK(c, hipMemcpyAsync(c->src.enth, nw.l_enth.data(), sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  NET_WAIT(c);   // l_net / l_enth are reused by the next pass
  return 0;
}

int network_fetch_state(wai_ctx* c) {
  Network& nw = c->net;
  if (!nw.state_on_device || !nw.d_state) return 0;
  HIPCHK(c, hipMemcpyAsync(nw.h_state.data(), nw.d_state, sizeof(double) * nw.h_state.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  nw.state_on_device = false;
  return 0;
}
int network_fetch_couplings(wai_ctx* c) {
  Network& nw = c->net;
  if (!nw.cp_on_device || !nw.d_cp_val || nw.h_cp_val.empty()) return 0;
  HIPCHK(c, hipMemcpyAsync(nw.h_cp_val.data(), nw.d_cp_val, sizeof(double) * nw.h_cp_val.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  nw.cp_on_device = false;
  return 0;
}

// ---- Jacobian couplings through the source network ---------------------------------------------
// flow_simulation_modify_jacobian (src/flow_simulation.F90:3023-3084) widens the Jacobian's pattern by the
// network's dependencies and MatFDColoring then differences the whole residual function -- network pass
// included -- into it.  Here the 7-point part A is differenced with the network's factors held
// (k_jacobian), and the rest, E = dR/dy *through the network pass*, is differenced separately on the cells
// of the network's sources: for every such cell j and primary k, with y_jk + h (the same h as A's
// columns), E[:, j][:, k] = (R(network pass redone) - R(factors held)) / h on the rows of those cells.
// Two residual launches on the network's rows alone (k_residual's row list: the same code path per row, so
// the same bits as a full sweep) and three host passes per column: the cost does not grow with the mesh.
// wai_set_coupling_build, WAI_COUPLING_BUILD_BATCHED (where the device pass is in force): the columns are independent, so
// all of them run at once on private scratch in five launches (kernels_coupling.hip; the plan: coupling_batch.hpp, its byte
// cap COUPLING_BATCH_BYTES or, for the tests, the environment's WAI_COUPLING_BATCH_BYTES) -- the same bits.
__global__ void k_gather_rows(int m, int bs, const int* __restrict__ cells, const double* __restrict__ f,
                              double* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m * bs) return;
  out[t] = f[(size_t)cells[t / bs] * bs + t % bs];
}

// t += E x on the network's rows: thread (i, r) sums its row over the mc column cells (cells are distinct: no race).
// xg != null: x at the column cells, gathered over the ranks ([mc][bs]); else the columns are the row cells themselves
__global__ void k_coupling_apply(int mr, int mc, int bs, const int* __restrict__ cells, const double* __restrict__ val,
                                 const double* __restrict__ x, const double* __restrict__ xg, double* __restrict__ t) {
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= mr * bs) return;
  const int i = id / bs, r = id % bs;
  double s = 0.0;
  for (int j = 0; j < mc; j++) {
    const double* e = val + ((size_t)(i * mc + j) * bs + r) * bs;
    const double* xj = xg ? xg + (size_t)j * bs : x + (size_t)cells[j] * bs;
    for (int k = 0; k < bs; k++) s += e[k] * xj[k];
  }
  t[(size_t)cells[i] * bs + r] += s;
}

int network_couplings(wai_ctx* c, double dt, double* y, const double* lhs_old) {
  Network& nw = c->net;
  nw.cp_valid = false;
  c->cp_launches = c->cp_columns = c->cp_chunks = 0;
  const bool span = nw.cp_span;
  const int ml = (int)nw.cp_cells.size(), m = span ? nw.cp_m : ml, j0 = span ? nw.cp_j0 : 0;
  if (!nw.on || !nw.coupling || m == 0) return 0;
  const int bs = c->np, mb = ml * bs, me = span ? c->comm->rank : 0;
  if (!nw.d_cp_val) {
    std::vector<int> cells = nw.cp_cells;
    if (cells.empty()) cells.push_back(0);
    if (nw.d_cp_cells.upload(c, cells) || nw.d_cp_val.alloc(c, (size_t)std::max(ml, 1) * m * bs * bs) ||
        nw.d_cp_f.alloc(c, (size_t)c->mesh.n_local * bs) || nw.d_cp_g.alloc(c, (size_t)2 * std::max(mb, 1)) ||
        nw.d_cp_x.alloc(c, (size_t)m * bs + 2))
      return -1;
  }
  nw.h_cp_val.assign((size_t)ml * m * bs * bs, 0.0);
  nw.cp_on_device = false;
  const int grid = (mb + 63) / 64;
  if (net_on_device(c)) {
    // the same columns with nothing read back inside the loop: y_jk and h stay in device scratch, the differences go
    // straight into d_cp_val, and the host waits once, for the flag
    if (!nw.d_cp_yh && (nw.d_cp_yh.alloc(c, 2) || nw.d_cp_flag.alloc(c, 1))) return -1;
    if (network_update(c)) return -1;   // the factors A was differenced with
    HIPCHK(c, hipMemsetAsync(nw.d_cp_flag, 0, sizeof(int), c->stream));
    c->cp_columns = (long long)m * bs;
    c->cp_launches = 2;   // network_update above: k_source_rates and k_network_pass
    const bool batched = cp_batched(c);
    if (batched) {
      // all columns at once, each on private scratch (kernels_coupling.hip): y, the fluid record and the factors are read
      // and never written, so nothing is perturbed, restored or passed again -- five launches per chunk whatever m is
      CouplingBatch b;
      long long cap = COUPLING_BATCH_BYTES;
      if (const char* ev = getenv("WAI_COUPLING_BATCH_BYTES")) cap = atoll(ev);   // read per build: the tests force several chunks
      if (int e = coupling_batch_plan(m, ml, bs, c->df, c->src.n, cap, b, c->err)) return e;
      if (b.doubles > nw.cb_doubles) {
        if (nw.d_cb_scratch.alloc(c, (size_t)b.doubles)) return -1;
        nw.cb_doubles = b.doubles;
      }
      for (int ch = 0; ch < b.n_chunks; ch++)
        if (launch_coupling_batch(c, b, ch * b.chunk, ch + 1 < b.n_chunks ? b.chunk : b.last, dt, y, lhs_old, &c->cp_launches,
                                  net_wave_usable(c)))
          return -1;
      c->net_passes += b.ncol;   // one pass per column, in k_cb_pass
      c->cp_chunks = b.n_chunks;
    } else c->cp_launches += 13 * c->cp_columns;   // counted from the loop below (each network_update in it: two launches)
    for (int j = 0; j < m && !batched; j++) {
      const int cell = nw.cp_cells[j];
      for (int k = 0; k < bs; k++) {
        double* p = y + (size_t)cell * bs + k;
        launch_cp_perturb(c, p, nw.d_cp_yh);
        launch_eos(c, y, cell, 1, false);
        launch_residual(c, dt, lhs_old, nw.d_cp_f, nullptr, nullptr, nw.d_cp_cells, ml);   // factors held
        hipLaunchKernelGGL(k_gather_rows, grid, 64, 0, c->stream, ml, bs, nw.d_cp_cells, nw.d_cp_f, nw.d_cp_g);
        if (network_update(c)) return -1;
        launch_residual(c, dt, lhs_old, nw.d_cp_f, nullptr, nullptr, nw.d_cp_cells, ml);   // network pass redone
        hipLaunchKernelGGL(k_gather_rows, grid, 64, 0, c->stream, ml, bs, nw.d_cp_cells, nw.d_cp_f, nw.d_cp_g + mb);
        launch_cp_diff(c, ml, m, bs, j, k, nw.d_cp_g, nw.d_cp_yh, nw.d_cp_val, nw.d_cp_flag);
        launch_cp_restore(c, p, nw.d_cp_yh);
        launch_eos(c, y, cell, 1, false);
        if (network_update(c)) return -1;
      }
    }
    HIPCHK(c, hipMemsetAsync(c->d_flags, 0, sizeof(int), c->stream));
    int any_dev = 0;
    HIPCHK(c, hipMemcpyAsync(&any_dev, nw.d_cp_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    NET_WAIT(c);
    nw.cp_on_device = true;
    nw.cp_valid = any_dev != 0;
    return 0;
  }
  std::vector<double> g((size_t)2 * mb), yc((size_t)bs);
  auto set_y = [&](int cell, int k, double v) -> int {
    HIPCHK(c, hipMemcpyAsync(y + (size_t)cell * bs + k, &v, sizeof(double), hipMemcpyHostToDevice, c->stream));
    NET_WAIT(c);
    launch_eos(c, y, cell, 1, false);
    return 0;
  };
  // one double from its owner to every rank (the sum over the ranks of {value on the owner, 0 elsewhere})
  auto from_owner = [&](double& v, bool mine) -> int {
    if (!span) return 0;
    const double mineval = mine ? v : 0.0;
    HIPCHK(c, hipMemcpyAsync(nw.d_cp_x, &mineval, sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (comm_allreduce(c->comm, nw.d_cp_x, 1, 0, c->stream, c->err)) return -1;
    HIPCHK(c, hipMemcpyAsync(&v, nw.d_cp_x, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    NET_WAIT(c);
    return 0;
  };
  if (network_update(c)) return -1;   // the factors A was differenced with
  c->cp_columns = (long long)m * bs;
  // counted from the loop below: per column two residuals and gathers, two k_source_rates, and two k_eos on its owner
  c->cp_launches = (c->src.n ? 1 : 0) + ((ml ? 4 : 0) + (c->src.n ? 2 : 0)) * c->cp_columns + 2LL * ml * bs;
  bool any = false;
  for (int j = 0; j < m; j++) {       // every rank walks the same columns: the network passes are collective
    const bool mine = !span || nw.cp_owner[j] == me;
    const int cell = mine ? nw.cp_cells[j - j0] : -1;
    if (mine) {
      HIPCHK(c, hipMemcpyAsync(yc.data(), y + (size_t)cell * bs, sizeof(double) * bs, hipMemcpyDeviceToHost, c->stream));
      NET_WAIT(c);
    }
    for (int k = 0; k < bs; k++) {
      double h = 0.0;
      if (mine) {
        double dx = yc[k];   // MatFDColoring "ds" increment, as fd_step of the assembly sweeps
        if (std::fabs(dx) < c->opts.fd_umin) dx = dx >= 0.0 ? c->opts.fd_umin : -c->opts.fd_umin;
        h = dx * c->opts.fd_eps;
      }
      if (from_owner(h, mine)) return -1;
      if (mine && set_y(cell, k, yc[k] + h)) return -1;
      if (ml) {
        launch_residual(c, dt, lhs_old, nw.d_cp_f, nullptr, nullptr, nw.d_cp_cells, ml);   // factors held; the network's rows alone
        hipLaunchKernelGGL(k_gather_rows, grid, 64, 0, c->stream, ml, bs, nw.d_cp_cells, nw.d_cp_f, nw.d_cp_g);
      }
      if (network_update(c)) return -1;
      if (ml) {
        launch_residual(c, dt, lhs_old, nw.d_cp_f, nullptr, nullptr, nw.d_cp_cells, ml);   // network pass redone
        hipLaunchKernelGGL(k_gather_rows, grid, 64, 0, c->stream, ml, bs, nw.d_cp_cells, nw.d_cp_f, nw.d_cp_g + mb);
        HIPCHK(c, hipMemcpyAsync(g.data(), nw.d_cp_g, sizeof(double) * 2 * mb, hipMemcpyDeviceToHost, c->stream));
        NET_WAIT(c);
        for (int i = 0; i < ml; i++)
          for (int r = 0; r < bs; r++) {
            const double e = (g[(size_t)mb + i * bs + r] - g[(size_t)i * bs + r]) / h;
            nw.h_cp_val[((size_t)(i * m + j) * bs + r) * bs + k] = e;
            any = any || e != 0.0;
          }
      }
      if (mine && set_y(cell, k, yc[k])) return -1;   // back to the unperturbed state and its network factors
      if (network_update(c)) return -1;
    }
  }
  // a perturbed state outside the EOS's range was already reported by the perturbed-state sweep of A
  HIPCHK(c, hipMemsetAsync(c->d_flags, 0, sizeof(int), c->stream));
  if (any) {
    HIPCHK(c, hipMemcpyAsync(nw.d_cp_val, nw.h_cp_val.data(), sizeof(double) * nw.h_cp_val.size(), hipMemcpyHostToDevice,
                             c->stream));
    NET_WAIT(c);
  }
  double flag = any ? 1.0 : 0.0;   // every rank applies E (a collective gather of x) or none does
  if (span) {
    HIPCHK(c, hipMemcpyAsync(nw.d_cp_x, &flag, sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (comm_allreduce(c->comm, nw.d_cp_x, 1, 1, c->stream, c->err)) return -1;
    HIPCHK(c, hipMemcpyAsync(&flag, nw.d_cp_x, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    NET_WAIT(c);
  }
  nw.cp_valid = flag != 0.0;
  return 0;
}

// t = (A + E) x: the block-ELL SpMV and, when the network couples cells, its blocks on top.  A network on several
// ranks: x at the network's cells is gathered first (one all-reduce of m * bs doubles per application)
int apply_operator(wai_ctx* c, const LinSys& sys, const double* x, double* t) {
  launch_spmv(c, sys.A, x, t);
  const Network& nw = c->net;
  if (!net_in_operator(c, sys)) return 0;
  const int ml = (int)nw.cp_cells.size(), bs = sys.A.bs;
  if (!nw.cp_span) {
    hipLaunchKernelGGL(k_coupling_apply, (ml * bs + 63) / 64, 64, 0, c->stream, ml, ml, bs, nw.d_cp_cells, nw.d_cp_val, x,
                       (const double*)nullptr, t);
    return 0;
  }
  const int m = nw.cp_m;
  HIPCHK(c, hipMemsetAsync(nw.d_cp_x, 0, sizeof(double) * (size_t)m * bs, c->stream));
  if (ml) hipLaunchKernelGGL(k_gather_rows, (ml * bs + 63) / 64, 64, 0, c->stream, ml, bs, nw.d_cp_cells, x, nw.d_cp_x + (size_t)nw.cp_j0 * bs);
  if (comm_allreduce(c->comm, nw.d_cp_x, (size_t)m * bs, 0, c->stream, c->err)) return -1;
  if (ml) hipLaunchKernelGGL(k_coupling_apply, (ml * bs + 63) / 64, 64, 0, c->stream, ml, m, bs, nw.d_cp_cells, nw.d_cp_val, x,
                             (const double*)nw.d_cp_x, t);
  return 0;
}

// the cells whose equations and unknowns the network ties together: every source a group, a reinjector input,
// output or overflow names (source_network_identify_source_dependencies, source_network.F90:359-498, walks the
// same lists: production cells of a reinjector's input x cells of the sources it -- or the reinjectors
// it delivers or overflows to -- feeds; the members of a limited group among each other).  The coupling
// blocks E cover all pairs of these cells, a superset of the reference's dependency list.
// key[i]: what stands for source i's cell; the distinct keys of the named sources, ascending
template <class T>
static std::vector<T> network_cells(const NetFlatHost& F, const T* key, int n_key) {
  const NetFlat& h = F.h;
  const int* iw = F.iw.data();
  std::vector<char> in_net((size_t)h.n_src, 0);
  auto mark = [&](int kind, int index) { if (kind == NET_SOURCE && index >= 0 && index < h.n_src) in_net[index] = 1; };
  for (int q = 0; q < h.n_in; q++) mark(iw[h.in_kind + q], iw[h.in_index + q]);
  for (int r = 0; r < h.n_rj; r++) { mark(iw[h.rj_in_kind + r], iw[h.rj_in + r]); mark(iw[h.rj_over_kind + r], iw[h.rj_over + r]); }
  for (int q = 0; q < h.n_out; q++) mark(iw[h.out_kind + q], iw[h.out_node + q]);
  std::vector<T> u;
  for (int i = 0; i < h.n_src && i < n_key; i++) if (in_net[i]) u.push_back(key[i]);
  std::sort(u.begin(), u.end());
  u.erase(std::unique(u.begin(), u.end()), u.end());
  return u;
}
// the same over several ranks: the network's cells of all ranks (id: rank * 2^32 + local cell, per global source), so
// ordered by (owner rank, local cell); this rank's own are then one contiguous run of the columns and, in that order, the
// rows it differences and applies
static void network_cells_span(Network& nw, const std::vector<double>& id, int rank) {
  const std::vector<double> u = network_cells(nw.flat, id.data(), (int)id.size());
  nw.cp_span = true;
  nw.cp_m = (int)u.size();
  nw.cp_owner.resize(u.size());
  nw.cp_cells.clear();
  nw.cp_j0 = 0;
  for (size_t j = 0; j < u.size(); j++) {
    const int owner = (int)(u[j] / 4294967296.0);
    nw.cp_owner[j] = owner;
    if (owner == rank) {
      if (nw.cp_cells.empty()) nw.cp_j0 = (int)j;
      nw.cp_cells.push_back((int)(u[j] - (double)owner * 4294967296.0));
    }
  }
}

}  // namespace wai

extern "C" {

// Source network (src/source_network_group.F90, source_network_reinjector.F90; input "network.group",
// "network.reinject").  Node references are (kind, index) pairs: kind 0 none, 1 source, 2 group,
// 3 reinjector.  Groups in dependency order (a group after the groups it takes in).
int wai_set_source_network(wai_ctx* c, const int* rate_specified, const int* enthalpy_specified, int n_groups,
                           const int* grp_ptr, const int* grp_in_kind, const int* grp_in, const int* grp_scaling,
                           const int* grp_limit_type, const double* grp_limit, const double* grp_sep, int n_reinj,
                           const int* rj_in_kind, const int* rj_in, const int* rj_out_ptr, const int* out_flow,
                           const int* out_kind, const int* out_node, const double* out_rate,
                           const double* out_proportion, const double* out_enthalpy, const int* rj_overflow_kind,
                           const int* rj_overflow) {
  if (!c) return -2;
  Network& nw = c->net;
  const int n = c->src.n;
  auto ctl = nw.h_ctl; auto e0 = nw.h_enth0; auto cells = nw.h_cell;
  // a network set AGAIN on several ranks (its time tables, once per step): the copies above are numbered globally by now
  const std::vector<int> was = nw.gidx;
  const bool coupling = nw.coupling;
  c->src.net.reset();
  nw = Network();
  nw.h_ctl = ctl; nw.h_enth0 = e0; nw.h_cell = cells; nw.coupling = coupling;
  if (n_groups <= 0 && n_reinj <= 0) return 0;
  const bool span = c->comm && c->comm->nranks > 1;
  int ng = n;
  std::vector<double> span_id;   // several ranks: every source's cell as (owner rank, local cell)
  if (span) {
    // the description is numbered by global source index (wai_set_source_global_index); what the pass needs of
    // the other ranks' sources -- separator enthalpies, specified injection enthalpies -- is gathered once, here
    if ((int)c->src_gidx.size() != n || c->src_nglobal < n) { c->err = "source network on several ranks: wai_set_source_global_index first"; return -2; }
    ng = c->src_nglobal;
    for (int g : c->src_gidx) if (g < 0 || g >= ng) { c->err = "global source index out of range"; return -2; }
    nw.gidx = c->src_gidx;
    nw.n_global = ng;
    const int NG = 10;   // per source: 8 separator enthalpies, the specified enthalpy, the cell's identity (rank * 2^32 + cell)
    std::vector<double> all((size_t)NG * ng, 0.0);
    for (int i = 0; i < n; i++) {
      const int g = nw.gidx[i];
      const int k = (int)was.size() == n ? was[i] : i;   // source i in ctl and e0
      if (k < (int)ctl.size()) src_separator(ctl[k], &all[(size_t)NG * g]);
      all[(size_t)NG * g + 8] = k < (int)e0.size() ? e0[k] : 0.0;
      all[(size_t)NG * g + 9] = (double)c->comm->rank * 4294967296.0 + (double)(i < (int)cells.size() ? cells[i] : 0);
    }
    DevBuf<double> tmp;
    if (tmp.upload(c, all) || comm_allreduce(c->comm, tmp, all.size(), 0, c->stream, c->err)) return -1;
    HIPCHK(c, hipMemcpyAsync(all.data(), tmp, sizeof(double) * all.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    nw.h_ctl.assign((size_t)ng, SrcCtl{});
    nw.h_enth0.assign((size_t)ng, 0.0);
    span_id.assign((size_t)ng, 0.0);
    for (int g = 0; g < ng; g++) {
      nw.h_ctl[g].sep_hf = all[(size_t)NG * g]; nw.h_ctl[g].sep_hg = all[(size_t)NG * g + 1];
      for (int q = 0; q < 6; q++) nw.h_ctl[g].sep_more[q] = all[(size_t)NG * g + 2 + q];
      nw.h_enth0[g] = all[(size_t)NG * g + 8];
      span_id[g] = all[(size_t)NG * g + 9];
    }
  }
  // the description (every refusal is the builder's); the sources' separators and specified enthalpies come into it from
  // h_ctl and h_enth0, now and whenever they change (network_flat_refresh)
  if (int e = build_net_flat(nw.flat, ng, rate_specified, enthalpy_specified, nullptr, nullptr, n_groups, grp_ptr, grp_in_kind, grp_in,
                             grp_scaling, grp_limit_type, grp_limit, grp_sep, n_reinj, rj_in_kind, rj_in, rj_out_ptr, out_flow,
                             out_kind, out_node, out_rate, out_proportion, out_enthalpy, rj_overflow_kind, rj_overflow, c->err))
    return e;
  const NetFlat& h = nw.flat.h;
  nw.h_raw.assign(2 * (size_t)ng, 0.0);
  if (nw.h_enth0.size() != (size_t)ng) nw.h_enth0.assign((size_t)ng, 0.0);
  nw.h_net.assign(2 * (size_t)ng, 0.0);
  nw.h_enth.assign((size_t)ng, 0.0);
  nw.h_state.assign((size_t)net_kept_doubles(h), 0.0);
  if (nw.d_raw.alloc(c, 2 * (size_t)std::max(n, 1)) || c->src.net.alloc(c, 2 * (size_t)std::max(n, 1))) return -1;
  if (span && nw.d_all.alloc(c, 2 * (size_t)ng)) return -1;
  HIPCHK(c, hipMemset(c->src.net, 0, sizeof(double) * 2 * std::max(n, 1)));
  nw.h_loc.assign(2 * (size_t)n, 0.0);
  nw.l_net.assign(2 * (size_t)n, 0.0);
  nw.l_enth.assign((size_t)n, 0.0);
  for (int i = 0; i < n; i++) nw.l_enth[i] = nw.h_enth0[span ? nw.gidx[i] : i];
  nw.on = true;
  if (!span) {   // the pass on the device (wai_set_network_pass) and its wave walk (wai_set_network_walk): one rank only
    nw.flat_fits = net_lds_doubles(h) <= NET_LDS_DOUBLES;
    // the wave walk's schedule, whatever walk is asked for now: it may be asked for later
    nw.wave_ok = build_net_wave(nw.flat, nw.wave, nw.wave_err) == 0;
    nw.wave_built = nw.wave_ok || nw.wave.w.n_ww > 0;
    nw.cp_cells = network_cells(nw.flat, nw.h_cell.data(), (int)nw.h_cell.size());
  } else network_cells_span(nw, span_id, c->comm->rank);
  c->flow.as.overlap = -1;   // the factor's pattern carries the network's cell pairs: built again at the next set-up
  return 0;
}

// Global index of every local source, for a source network whose sources live on several ranks: the network
// description handed to wai_set_source_network then refers to sources by these indices (0 .. n_global - 1), the same
// description on every rank.  After wai_set_sources, before wai_set_source_network.
int wai_set_source_global_index(wai_ctx* c, int n_global, const int* global_index) {
  if (!c || n_global < 0 || (c->src.n > 0 && !global_index)) return -2;
  c->src_gidx.assign(global_index, global_index + c->src.n);
  c->src_nglobal = n_global;
  return 0;
}

int wai_set_network_couplings(wai_ctx* c, int on) {
  if (!c) return -2;
  const bool was = pc_with_net(c, c->flow);
  c->net.coupling = on != 0;
  c->net.cp_in_pc = on != 1;      // 1: in the operator only (rounds 2-3); 2 (and any other non-zero value): in the factor's pattern too
  if (!on) c->net.cp_valid = false;
  // pc_fused() / pc_extended() follow pc_with_net(): a set-up made for the other path (the extended system factored and
  // c->ilu not, or the other way round) must not be applied -- the next solve sets up again, the extended pattern included
  if (pc_with_net(c, c->flow) != was) {
    pc_invalidate(c);
    c->flow.as.overlap = -1;
  }
  return 0;
}

// Where the source network's pass runs (include/waiwera_hip.h)
int wai_set_network_pass(wai_ctx* c, int where) {
  if (!c) return -2;
  if (where != WAI_NETWORK_PASS_HOST && where != WAI_NETWORK_PASS_DEVICE) {
    c->err = "unknown place for the source network's pass (WAI_NETWORK_PASS_HOST or WAI_NETWORK_PASS_DEVICE)";
    return -2;
  }
  if (where != c->net_pass && network_fetch_state(c)) return -1;   // the host's copy of the node states stays the last pass'
  c->net_pass = where;
  return 0;
}
int wai_get_network_pass(wai_ctx* c, int* requested, int* in_force) {
  if (!c) return -2;
  if (requested) *requested = c->net_pass;
  if (in_force) *in_force = net_on_device(c) ? WAI_NETWORK_PASS_DEVICE : WAI_NETWORK_PASS_HOST;
  return 0;
}
// How the device pass walks groups and reinjectors (include/waiwera_hip.h)
int wai_set_network_walk(wai_ctx* c, int how) {
  if (!c) return -2;
  if (how != WAI_NETWORK_WALK_LANE && how != WAI_NETWORK_WALK_WAVE) {
    c->err = "unknown walk of the source network's device pass (WAI_NETWORK_WALK_LANE or WAI_NETWORK_WALK_WAVE)";
    return -2;
  }
  // a network only the wave walk holds on the device goes back to the host pass: its copy of the node states stays the last pass'
  if (how != c->net_walk && network_fetch_state(c)) return -1;
  c->net_walk = how;
  return 0;
}
int wai_get_network_walk(wai_ctx* c, int* requested, int* in_force) {
  if (!c) return -2;
  if (requested) *requested = c->net_walk;
  if (in_force) *in_force = net_walk_wave(c) ? WAI_NETWORK_WALK_WAVE : WAI_NETWORK_WALK_LANE;
  return 0;
}
// How the network's Jacobian blocks are built (include/waiwera_hip.h)
int wai_set_coupling_build(wai_ctx* c, int how) {
  if (!c) return -2;
  if (how != WAI_COUPLING_BUILD_COLUMNS && how != WAI_COUPLING_BUILD_BATCHED) {
    c->err = "unknown way to build the source network's coupling blocks (WAI_COUPLING_BUILD_COLUMNS or WAI_COUPLING_BUILD_BATCHED)";
    return -2;
  }
  c->cp_build = how;
  return 0;
}
int wai_get_coupling_build(wai_ctx* c, int* requested, int* in_force) {
  if (!c) return -2;
  if (requested) *requested = c->cp_build;
  if (in_force) *in_force = cp_batched(c) ? WAI_COUPLING_BUILD_BATCHED : WAI_COUPLING_BUILD_COLUMNS;
  return 0;
}
int wai_test_coupling_build_stats(wai_ctx* c, long long* launches, long long* columns, long long* chunks) {
  if (!c) return -2;
  if (launches) *launches = c->cp_launches;
  if (columns) *columns = c->cp_columns;
  if (chunks) *chunks = c->cp_chunks;
  return 0;
}
// one pass on the device for the given raw rates (include/waiwera_hip_bench.h)
int wai_test_network_pass(wai_ctx* c, const double* raw2n, double* sources6, double* groups6, double* reinjectors8, double* net2n,
                          double* enth_n) {
  if (!c || !raw2n) return -2;
  Network& nw = c->net;
  const int n = c->src.n;
  const bool wave = net_wave_usable(c);
  if (!nw.on || !(nw.flat_fits || wave) || (c->comm && c->comm->nranks > 1)) {
    c->err = "wai_test_network_pass: a source network on one rank that fits a workgroup's LDS";
    if (c->net_walk == WAI_NETWORK_WALK_WAVE && !nw.wave_err.empty()) c->err += " (" + nw.wave_err + ")";
    return -2;
  }
  if (network_flat_upload(c)) return -1;
  const NetFlat& h = nw.flat.h;
  HIPCHK(c, hipMemcpyAsync(nw.d_raw, raw2n, sizeof(double) * 2 * n, hipMemcpyHostToDevice, c->stream));
  if (launch_network_pass(c, nw.d_raw, c->src.net, c->src.enth, nw.d_state, wave)) return -1;
  nw.state_on_device = true;
  nw.enth_stale = true;
  const size_t ns = (size_t)NET_NODE * h.n_src, ngd = (size_t)NET_NODE * h.n_grp;
  if (sources6) HIPCHK(c, hipMemcpyAsync(sources6, nw.d_state, sizeof(double) * ns, hipMemcpyDeviceToHost, c->stream));
  if (groups6 && ngd) HIPCHK(c, hipMemcpyAsync(groups6, nw.d_state + ns, sizeof(double) * ngd, hipMemcpyDeviceToHost, c->stream));
  if (reinjectors8 && h.n_rj)
    HIPCHK(c, hipMemcpyAsync(reinjectors8, nw.d_state + ns + ngd, sizeof(double) * 8 * h.n_rj, hipMemcpyDeviceToHost, c->stream));
  if (net2n) HIPCHK(c, hipMemcpyAsync(net2n, c->src.net, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, c->stream));
  if (enth_n) HIPCHK(c, hipMemcpyAsync(enth_n, c->src.enth, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
int wai_test_network_stats(wai_ctx* c, long long* passes, long long* host_waits) {
  if (!c) return -2;
  if (passes) *passes = c->net_passes;
  if (host_waits) *host_waits = c->net_waits;
  return 0;
}
// the most doubles of LDS a network's description and state may take for the pass on the device, and what the
// context's network takes (0: none set, or one on several ranks)
int wai_test_network_lds(wai_ctx* c, int* limit, int* needed) {
  if (!c) return -2;
  const Network& nw = c->net;
  const bool have = nw.on && !nw.n_global;
  if (c->net_walk == WAI_NETWORK_WALK_WAVE && have && nw.wave_built) {   // the wave walk's own limit and need
    if (limit) *limit = NET_WAVE_LDS_DOUBLES;
    if (needed) *needed = net_wave_lds_doubles(nw.flat.h, nw.wave.w);
    return 0;
  }
  if (limit) *limit = NET_LDS_DOUBLES;
  if (needed) *needed = have ? net_lds_doubles(nw.flat.h) : 0;
  return 0;
}

int wai_get_network_couplings(wai_ctx* c, int* n_cells, int* cells, double* values) {
  if (!c || !n_cells) return -2;
  const Network& nw = c->net;
  const bool on = nw.on && nw.coupling && nw.cp_valid;
  const int ml = on ? (int)nw.cp_cells.size() : 0, m = on ? (nw.cp_span ? nw.cp_m : ml) : 0;
  *n_cells = m;
  if (cells)
    for (int j = 0; j < m; j++) {
      const bool mine = !nw.cp_span || (j >= nw.cp_j0 && j < nw.cp_j0 + ml);
      cells[j] = mine ? nw.cp_cells[j - (nw.cp_span ? nw.cp_j0 : 0)] : -1 - nw.cp_owner[j];
    }
  if (values && ml) {
    if (network_fetch_couplings(c)) return -1;
    std::memcpy(values, nw.h_cp_val.data(), sizeof(double) * nw.h_cp_val.size());
  }
  return 0;
}
// The network pass without a context or a device (the host pass of network_update; tests): the sources' own rates
// and enthalpies and their separators (8 doubles per source: hf, hg of stage 1, then (hf, hg) of stages
// 2..4, hg = 0: no separator / no further stage) in, node states out -- sources and groups 6 doubles each
// (rate, enthalpy, water_rate, water_enthalpy, steam_rate, steam_enthalpy), reinjectors 8 each as
// wai_get_source_network.
int wai_network_evaluate(int n_sources, const double* rate, const double* enthalpy, const double* src_sep,
                         const int* rate_specified, const int* enthalpy_specified, int n_groups,
                         const int* grp_ptr, const int* grp_in_kind, const int* grp_in, const int* grp_scaling,
                         const int* grp_limit_type, const double* grp_limit, const double* grp_sep, int n_reinj,
                         const int* rj_in_kind, const int* rj_in, const int* rj_out_ptr, const int* out_flow,
                         const int* out_kind, const int* out_node, const double* out_rate,
                         const double* out_proportion, const double* out_enthalpy, const int* rj_overflow_kind,
                         const int* rj_overflow, double* sources_out, double* groups_out, double* reinjectors_out) {
  if (!rate || !enthalpy || n_sources <= 0) return -2;
  NetFlatHost F;
  std::string err;
  if (int e = build_net_flat(F, n_sources, rate_specified, enthalpy_specified, src_sep, enthalpy, n_groups, grp_ptr, grp_in_kind, grp_in,
                             grp_scaling, grp_limit_type, grp_limit, grp_sep, n_reinj, rj_in_kind, rj_in, rj_out_ptr, out_flow,
                             out_kind, out_node, out_rate, out_proportion, out_enthalpy, rj_overflow_kind, rj_overflow, err))
    return e;
  std::vector<double> raw(rate, rate + n_sources), work, kept((size_t)net_kept_doubles(F.h));
  raw.insert(raw.end(), enthalpy, enthalpy + n_sources);
  network_pass_host(F, raw.data(), work, nullptr, nullptr, kept.data());
  const size_t ns = (size_t)NET_NODE * F.h.n_src, ngd = (size_t)NET_NODE * F.h.n_grp;
  if (sources_out) std::memcpy(sources_out, kept.data(), sizeof(double) * ns);
  if (groups_out) std::memcpy(groups_out, kept.data() + ns, sizeof(double) * ngd);
  if (reinjectors_out) std::memcpy(reinjectors_out, kept.data() + ns + ngd, sizeof(double) * 8 * (size_t)F.h.n_rj);
  return 0;
}
// The cells between which wai_jacobian forms the network's coupling blocks, for the given sources' cells and
// network description -- no context, no device (tests pin it on the reference's dependency list).
// cells: room for n_sources entries; *n_cells: how many were written (ascending, distinct)
int wai_network_cells(int n_sources, const int* source_cell, const int* rate_specified, const int* enthalpy_specified,
                      int n_groups, const int* grp_ptr, const int* grp_in_kind, const int* grp_in, const int* grp_scaling,
                      const int* grp_limit_type, const double* grp_limit, const double* grp_sep, int n_reinj,
                      const int* rj_in_kind, const int* rj_in, const int* rj_out_ptr, const int* out_flow,
                      const int* out_kind, const int* out_node, const double* out_rate, const double* out_proportion,
                      const double* out_enthalpy, const int* rj_overflow_kind, const int* rj_overflow, int* n_cells,
                      int* cells) {
  if (!source_cell || !n_cells || !cells || n_sources <= 0) return -2;
  NetFlatHost F;
  std::string err;
  if (int e = build_net_flat(F, n_sources, rate_specified, enthalpy_specified, nullptr, nullptr, n_groups, grp_ptr, grp_in_kind, grp_in,
                             grp_scaling, grp_limit_type, grp_limit, grp_sep, n_reinj, rj_in_kind, rj_in, rj_out_ptr, out_flow,
                             out_kind, out_node, out_rate, out_proportion, out_enthalpy, rj_overflow_kind, rj_overflow, err))
    return e;
  const std::vector<int> u = network_cells(F, source_cell, n_sources);
  *n_cells = (int)u.size();
  std::copy(u.begin(), u.end(), cells);
  return 0;
}
// state of the network after the last pass: groups 6 doubles each (rate, enthalpy, water_rate,
// water_enthalpy, steam_rate, steam_enthalpy); reinjectors 8 each (output water / steam rate, overflow
// rate, enthalpy, water rate, water enthalpy, steam rate, steam enthalpy)
int wai_get_source_network(wai_ctx* c, double* groups, double* reinjectors) {
  if (!c) return -2;
  if (network_fetch_state(c)) return -1;   // a pass on the device: its node states are downloaded when asked for
  const Network& nw = c->net;
  if (nw.h_state.empty()) return 0;   // no network
  const NetFlat& h = nw.flat.h;
  const double* kept = nw.h_state.data() + (size_t)NET_NODE * h.n_src;
  if (groups) std::memcpy(groups, kept, sizeof(double) * NET_NODE * (size_t)h.n_grp);
  if (reinjectors) std::memcpy(reinjectors, kept + (size_t)NET_NODE * h.n_grp, sizeof(double) * 8 * (size_t)h.n_rj);
  return 0;
}

}  // extern "C"

// Sources and their controls behind the C ABI of libwaiwera_hip.so (include/waiwera_hip.h): the source list, its rates
// and enthalpies, the state-dependent control records and what is read back of them.  The network over the sources is
// network.hip.
#include "host.hpp"

using namespace wai;

extern "C" {

int wai_set_sources(wai_ctx* c, int n, const int* cell, const double* rate, const double* enthalpy,
                    const int* component) {
  if (!c || n < 0) return -2;
  Sources& s = c->src;
  s = Sources();
  s.n = n;
  const int N = c->mesh.n_owned;
  std::vector<int> head(N, -1), next(std::max(n, 1), -1), vc(std::max(n, 1), 0), vk(std::max(n, 1), 0);
  std::vector<double> vr(std::max(n, 1), 0.0), ve(std::max(n, 1), 0.0);
  // chain sources of a cell in input order
  for (int i = n - 1; i >= 0; i--) {
    if (cell[i] < 0 || cell[i] >= N) { c->err = "source cell not owned"; return -2; }
    next[i] = head[cell[i]];
    head[cell[i]] = i;
    vc[i] = cell[i]; vk[i] = component ? component[i] : 0; vr[i] = rate[i]; ve[i] = enthalpy ? enthalpy[i] : 0.0;
  }
  HIPCHK(c, hipMemcpy(c->mesh.cell_src, head.data(), N * sizeof(int), hipMemcpyHostToDevice));
  if (s.cell.upload(c, vc) || s.comp.upload(c, vk) || s.pcomp.upload(c, std::vector<int>(std::max(n, 1), 0)) || s.next.upload(c, next) || s.rate.upload(c, vr) || s.enth.upload(c, ve)) return -1;
  const bool coupling = c->net.coupling, cp_in_pc = c->net.cp_in_pc;
  c->net = Network();   // a network refers to sources by index: set it again after the sources
  c->net.h_enth0 = ve;
  c->net.h_cell.assign(vc.begin(), vc.begin() + n);
  c->net.coupling = coupling; c->net.cp_in_pc = cp_in_pc;
  c->flow.as.overlap = -1;   // an extended system built for another network's cells is stale
  return 0;
}

int wai_update_sources(wai_ctx* c, const double* rate, const double* enthalpy) {
  if (!c) return -2;
  const size_t nb = sizeof(double) * (size_t)c->src.n;
  if (!c->src.n) return 0;
  if (rate) HIPCHK(c, hipMemcpyAsync(c->src.rate, rate, nb, hipMemcpyDefault, c->stream));
  if (enthalpy) HIPCHK(c, hipMemcpyAsync(c->src.enth, enthalpy, nb, hipMemcpyDefault, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (enthalpy && !is_device_ptr(enthalpy)) {   // the network's host copies of the specified injection enthalpies
    Network& nw = c->net;
    const bool span = !nw.gidx.empty();
    for (int i = 0; i < c->src.n; i++) {
      const size_t g = span ? (size_t)nw.gidx[i] : (size_t)i;
      if (g < nw.h_enth0.size()) nw.h_enth0[g] = enthalpy[i];
      if ((size_t)i < nw.l_enth.size()) nw.l_enth[i] = enthalpy[i];
    }
    nw.flat_gen++;   // the pass' copies of the specified enthalpies, host and device
  }
  return 0;
}

// production components beside wai_set_sources' `component` (source.F90:340-366, 403-453): a producing source with c > 0
// puts its whole rate into component c -- c = np: heat alone, and no enthalpy is formed -- instead of `component`'s
int wai_set_source_production_component(wai_ctx* c, const int* component) {
  if (!c) return -2;
  Sources& s = c->src;
  std::vector<int> v(std::max(s.n, 1), 0);
  for (int i = 0; i < s.n && component; i++) {
    if (component[i] > c->np) { c->err = "production component above the number of primary variables"; return -2; }
    v[i] = std::max(component[i], 0);
  }
  if (!s.pcomp) return component && s.n ? (c->err = "production components: wai_set_sources first", -2) : 0;
  HIPCHK(c, hipMemcpyAsync(s.pcomp, v.data(), sizeof(int) * v.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

static_assert(sizeof(wai_source_control) == sizeof(SrcCtl), "wai_source_control and the device record differ");

int wai_set_source_controls(wai_ctx* c, const wai_source_control* controls) {
  if (!c) return -2;
  Sources& s = c->src;
  if (!controls || !s.n) {
    s.ctl.reset();
    return 0;
  }
  for (int i = 0; i < s.n; i++) {
    const wai_source_control& k = controls[i];
    if (k.kind < 0 || k.kind > 2 || k.direction < 0 || k.direction > 2 || k.limiter < 0 || k.limiter > 3 ||
        k.table_coord < 0 || k.table_coord > 2 || (k.table_coord && (k.n_table < 1 || k.n_table > 8))) {
      c->err = "bad source control record";
      return -1;
    }
  }
  // threshold deliverability: the index the device noted so far survives a new set of records (they are set again
  // before every try for their time tables) unless the record brings one (threshold_pi >= 0)
  std::vector<SrcCtl> recs(reinterpret_cast<const SrcCtl*>(controls), reinterpret_cast<const SrcCtl*>(controls) + s.n);
  {
    std::vector<SrcCtl> old;
    if (s.ctl) {
      old.resize((size_t)s.n);
      HIPCHK(c, hipMemcpyAsync(old.data(), s.ctl, sizeof(SrcCtl) * (size_t)s.n, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    for (int i = 0; i < s.n; i++)
      if (recs[i].threshold > 0.0 && recs[i].threshold_pi < 0.0)   // inherited only from a record that HAD a threshold and a noted index
        recs[i].threshold_pi = (!old.empty() && old[i].threshold > 0.0 && old[i].threshold_pi >= 0.0) ? old[i].threshold_pi : recs[i].coef;
  }
  controls = reinterpret_cast<const wai_source_control*>(recs.data());
  if (!s.ctl && s.ctl.alloc(c, (size_t)s.n)) return -1;
  if (c->net.gidx.empty()) c->net.h_ctl.assign(reinterpret_cast<const SrcCtl*>(controls), reinterpret_cast<const SrcCtl*>(controls) + s.n);
  else   // a network across ranks numbers its control records globally: this rank's own entries
    for (int i = 0; i < s.n; i++) c->net.h_ctl[c->net.gidx[i]] = reinterpret_cast<const SrcCtl*>(controls)[i];
  c->net.flat_gen++;   // the pass' copies of the separators, host and device
  HIPCHK(c, hipMemcpyAsync(s.ctl, controls, sizeof(SrcCtl) * (size_t)s.n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int wai_separator_enthalpies(wai_ctx* c, double pressure, double* hf, double* hg) {
  if (!c || !hf || !hg) return -2;
  DevBuf<double> tmp;
  double host[3];
  if (tmp.alloc(c, 3)) return -1;
  launch_separator(c, pressure, tmp);
  HIPCHK(c, hipMemcpyAsync(host, tmp, sizeof host, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (host[2] != 0.0) { c->err = "separator pressure outside the saturation line"; return -1; }
  *hf = host[0];
  *hg = host[1];
  return 0;
}

int wai_get_source_rates(wai_ctx* c, double* rate, double* enthalpy) {
  if (!c || !rate) return -2;
  const size_t n = (size_t)c->src.n;
  // on the fluid state in force, like the residual's pass.  A network across ranks gathers every rank's sources in it: a
  // rank without sources takes part before it returns
  if (c->net.on && network_update(c)) return -1;
  if (!n) return 0;
  DevBuf<double> tmp;
  if (tmp.alloc(c, 2 * n)) return -1;
  launch_source_rates(c, tmp);
  HIPCHK(c, hipMemcpyAsync(rate, tmp, n * sizeof(double), hipMemcpyDefault, c->stream));
  if (enthalpy) HIPCHK(c, hipMemcpyAsync(enthalpy, tmp + n, n * sizeof(double), hipMemcpyDefault, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

// separated water / steam flows of every source (source_network_node_type: water_rate, water_enthalpy,
// steam_rate, steam_enthalpy; separator.F90:212-260) for the rates and enthalpies in force; zero for
// sources without a separator and for injection
int wai_get_source_separated(wai_ctx* c, double* out4) {
  if (!c || !out4) return -2;
  const int n = c->src.n;
  std::vector<double> q(std::max(n, 1)), h(std::max(n, 1));
  if (int e = wai_get_source_rates(c, q.data(), h.data())) return e;   // (the network pass in it: made without sources too)
  for (int i = 0; i < n; i++) {
    double nd[NET_NODE] = {q[i], h[i], 0.0, 0.0, 0.0, 0.0}, sep[8];
    const int g = c->net.gidx.empty() ? i : c->net.gidx[i];   // the network's control records are numbered globally
    if (q[i] < 0.0 && g < (int)c->net.h_ctl.size() && c->net.h_ctl[g].sep_hg > 0.0) {
      src_separator(c->net.h_ctl[g], sep);
      netpass::separate(sep, q[i], h[i], nd);
    }
    for (int k = 0; k < 4; k++) out4[4 * i + k] = nd[2 + k];
  }
  return 0;
}

}  // extern "C"

// The source network's pass with the walk of groups and reinjectors spread over the lanes of one wave
// (wai_set_network_walk, WAI_NETWORK_WALK_WAVE): a schedule built on the host from the flat description of
// network_pass.hpp, and the walk written once over a small executor -- "every lane runs f(lane)", "one lane runs f",
// "barrier" -- so that the same text runs in a kernel (threadIdx.x, a lane-0 guard, __syncthreads()) and in a host program
// that loops over 64 emulated lanes (tests/network_wave_host).  Host-only compatible, like network_pass.hpp: no HIP header.
//
// THE SAME BITS as network_pass_serial.  The serial text is slow because every term of every sum is reached through two
// dependent reads (iw -> node address -> node), not because its additions are serial.  Here the lanes GATHER the terms into a
// contiguous staging run -- every product rounded once, as there -- and the additions are then CHAINED in input order over
// contiguous, index-free data, each sum on one lane: the same sequence of roundings.  Work that is independent per source (scaling what is below a
// limited group, delivering to distinct injection sources) is strided over the lanes.  No contraction of a product and a sum.
//
// What keeps a one-wave kernel from hanging: every executor call starts and ends with a barrier and none stands inside a
// lane-dependent branch; every trip count and decision between two calls (over, scale, the stack pointer, a frame's fields)
// is computed by every lane from words that a finished call left behind, so all lanes take the same way.
#pragma once
#include <algorithm>
#include "network_pass.hpp"

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

// a loop over contiguous staged data, unrolled so that its reads are in flight together
#define WAI_NET_UNROLL _Pragma("GCC unroll 8")

namespace wai {

constexpr int NET_WAVE_LANES = 64;
constexpr int NET_WAVE_LDS_DOUBLES = 20480;   // the 160 KiB of LDS a gfx950 workgroup may take (dynamic)
constexpr int NET_WAVE_STAGE = 6;             // staged doubles per input: n0, n0 n1, n2, n2 n3, n4, n4 n5
constexpr int NET_WAVE_CTL = 8;               // doubles at the head of the staging run that carry a phase's results to the next

// The schedule: offsets into one array of ints (ww), per group the sources below it (depth first, inputs in order), the
// groups below it (ascending: a group's inputs are earlier groups, so inputs precede their group) and its ancestors (from
// its parent upwards) and the positions among its inputs of those that are groups (in input order); per output whether its
// target source has another writer
struct NetWave {
  int n_ww = 0;
  int fan_in = 0;   // the widest fan-in: a group's inputs, a reinjector's outputs
  int stage = 0;    // doubles of the staging run: NET_WAVE_CTL + NET_WAVE_STAGE * max(fan_in, 1)
  int ds_ptr = 0, ds = 0, dg_ptr = 0, dg = 0, an_ptr = 0, an = 0, gc_ptr = 0, gc = 0, out_shared = 0;
};
struct NetWaveView {
  NetWave w;
  const int* ww;
};
struct NetWaveHost {
  NetWave w;
  std::vector<int> ww;
  NetWaveView view() const { return NetWaveView{w, ww.data()}; }
};
// doubles of LDS the wave kernels take:  [ dw | raw 2n | state | staging | iw | ww ]
inline int net_wave_lds_doubles(const NetFlat& h, const NetWave& w) { return net_lds_doubles(h) + w.stage + (w.n_ww + 1) / 2; }

// The schedule of a flat description.  0, or -2 with a text where the wave walk must not run:
//  - a source or group that is taken in more than once (by two groups, or twice by one): two lanes would scale it at once
//    where the serial walk scales it twice.  With every node taken in at most once the groups form a forest, so nothing is
//    reachable along two paths either;
//  - a need above NET_WAVE_LDS_DOUBLES.
// A source that is the target of more than one reinjector output or overflow is NOT refused: its outputs are flagged
// (out_shared) and the one lane that runs the balance chain delivers them, in output order -- the last write wins as in the
// serial text.  Only outputs onto sources nobody else writes are delivered by the lanes.
inline int build_net_wave(const NetFlatHost& F, NetWaveHost& W, std::string& err) {
  const NetFlat& h = F.h;
  const int* iw = F.iw.data();
  const int n = h.n_src, ng = h.n_grp, nr = h.n_rj;
  std::vector<int> taken_src((size_t)n, 0), taken_grp((size_t)ng, 0), parent((size_t)ng, -1);
  for (int g = 0; g < ng; g++)
    for (int p = iw[h.grp_ptr + g]; p < iw[h.grp_ptr + g + 1]; p++) {
      const int kind = iw[h.in_kind + p], idx = iw[h.in_index + p];
      int& taken = kind == NET_SOURCE ? taken_src[idx] : taken_grp[idx];
      if (++taken > 1) {
        err = std::string("network wave walk: ") + (kind == NET_SOURCE ? "source " : "group ") + std::to_string(idx) +
              " is taken in more than once";
        return -2;
      }
      if (kind == NET_GROUP) parent[idx] = g;
    }
  std::vector<std::vector<int>> dsrc((size_t)ng), dgrp((size_t)ng);
  int fan = 0;
  for (int g = 0; g < ng; g++) {
    const int p0 = iw[h.grp_ptr + g], p1 = iw[h.grp_ptr + g + 1];
    fan = std::max(fan, p1 - p0);
    for (int p = p0; p < p1; p++) {
      const int idx = iw[h.in_index + p];
      if (iw[h.in_kind + p] == NET_SOURCE) { dsrc[g].push_back(idx); continue; }
      dsrc[g].insert(dsrc[g].end(), dsrc[idx].begin(), dsrc[idx].end());
      dgrp[g].insert(dgrp[g].end(), dgrp[idx].begin(), dgrp[idx].end());
      dgrp[g].push_back(idx);
    }
    std::sort(dgrp[g].begin(), dgrp[g].end());
  }
  for (int r = 0; r < nr; r++) fan = std::max(fan, iw[h.rj_out_ptr + r + 1] - iw[h.rj_out_ptr + r]);
  std::vector<int> writers((size_t)n, 0);
  for (int p = 0; p < h.n_out; p++) if (iw[h.out_kind + p] == NET_SOURCE) writers[iw[h.out_node + p]]++;
  for (int r = 0; r < nr; r++) if (iw[h.rj_over_kind + r] == NET_SOURCE) writers[iw[h.rj_over + r]]++;
  NetWave& w = W.w;
  w = NetWave();
  w.fan_in = fan;
  w.stage = NET_WAVE_CTL + NET_WAVE_STAGE * std::max(fan, 1);
  std::vector<int>& ww = W.ww;
  ww.clear();
  auto lists = [&](int& ptr_at, int& at, auto&& list_of) {
    ptr_at = (int)ww.size();
    ww.resize(ww.size() + (size_t)ng + 1, 0);
    at = (int)ww.size();
    for (int g = 0; g < ng; g++) {
      const std::vector<int> l = list_of(g);
      ww.insert(ww.end(), l.begin(), l.end());
      ww[(size_t)ptr_at + g + 1] = (int)ww.size() - at;
    }
  };
  lists(w.ds_ptr, w.ds, [&](int g) { return dsrc[g]; });
  lists(w.dg_ptr, w.dg, [&](int g) { return dgrp[g]; });
  lists(w.an_ptr, w.an, [&](int g) { std::vector<int> a; for (int q = parent[g]; q >= 0; q = parent[q]) a.push_back(q); return a; });
  lists(w.gc_ptr, w.gc, [&](int g) {
    std::vector<int> a;
    for (int p = iw[h.grp_ptr + g]; p < iw[h.grp_ptr + g + 1]; p++) if (iw[h.in_kind + p] == NET_GROUP) a.push_back(p - iw[h.grp_ptr + g]);
    return a;
  });
  w.out_shared = (int)ww.size();
  for (int p = 0; p < h.n_out; p++) ww.push_back(iw[h.out_kind + p] == NET_SOURCE && writers[iw[h.out_node + p]] > 1 ? 1 : 0);
  w.n_ww = (int)ww.size();
  const long long bytes = 8LL * net_wave_lds_doubles(h, w);
  if (bytes > 8LL * NET_WAVE_LDS_DOUBLES) {
    err = "network wave walk: needs " + std::to_string(bytes) + " bytes of LDS, a workgroup has " + std::to_string(8 * NET_WAVE_LDS_DOUBLES);
    return -2;
  }
  return 0;
}

// ---- the walk ---------------------------------------------------------------------------------------------------------
// Ex: `width` lanes; lanes(f): every lane runs f(lane); one(f): one lane runs f(); both between two barriers.
// st: the staging run (NetWave::stage doubles): NET_WAVE_CTL words that carry a phase's results to the next, then the staged
// terms.  Every function below is entered by all lanes alike.
namespace netwave {
using namespace netpass;

// group_sum: the lanes gather the six terms of every input; six lanes chain one sum each in input order -- one instruction of
// the wave adds to all six, where one lane would take six; one lane makes the node of the sums
template <class Ex>
WAI_NET_HD inline void group_sum(Ex& ex, const NetFlatView& v, NetState& s, double* st, int g) {
  WAI_NET_FP
  const int p0 = v.iw[v.h.grp_ptr + g], m = v.iw[v.h.grp_ptr + g + 1] - p0;
  double* sd = st + NET_WAVE_CTL;
  ex.lanes([&](int lane) {
    WAI_NET_FP
    const int *ik = v.iw + v.h.in_kind + p0, *ii = v.iw + v.h.in_index + p0;
    for (int i = lane; i < m; i += Ex::width) {
      const double* n = node(s, ik[i], ii[i]);
      double* t = sd + NET_WAVE_STAGE * i;
      t[0] = n[0]; t[1] = n[0] * n[1]; t[2] = n[2]; t[3] = n[2] * n[3]; t[4] = n[4]; t[5] = n[4] * n[5];
    }
  });
  ex.lanes([&](int lane) {
    WAI_NET_FP
    if (lane >= NET_WAVE_STAGE) return;
    double acc = 0.0;
    // (unrolled: the reads of several inputs are in flight while the additions wait for one another)
    WAI_NET_UNROLL
    for (int i = 0; i < m; i++) acc += sd[NET_WAVE_STAGE * i + lane];
    st[lane] = acc;
  });
  ex.one([&]() {
    WAI_NET_FP
    double* G = s.grp + NET_NODE * g;
    const double q = st[0], qh = st[1];
    G[1] = dabs(q) > 1.e-9 ? qh / q : 0.0;
    G[0] = q;
    const double* sep = v.dw + v.h.grp_sep + 8 * g;
    if (q < 0.0 && sep[1] > 0.0) separate(sep, q, G[1], G);
    else if (q < 0.0) {
      const double wq = st[2], wqh = st[3], sq = st[4], sqh = st[5];
      G[2] = wq; G[4] = sq;
      G[3] = dabs(wq) > 1.e-9 ? wqh / wq : 0.0;
      G[5] = dabs(sq) > 1.e-9 ? sqh / sq : 0.0;
    } else G[2] = G[3] = G[4] = G[5] = 0.0;
  });
}

// scale_run: the sources below, lane-strided (each is below exactly once: build_net_wave); then the groups below in schedule
// order and the group itself.  A group's sum is a function of its inputs' states alone, so the order among groups that do not
// contain one another is free; no stack
template <class Ex>
WAI_NET_HD inline void scale_run(Ex& ex, const NetFlatView& v, const NetWaveView& w, NetState& s, double* st, int kind, int index,
                                 double scale) {
  WAI_NET_FP
  if (kind == NET_SOURCE) {
    ex.one([&]() { WAI_NET_FP source_set_rate(v, s, index, s.src[NET_NODE * index] * scale); });
    return;
  }
  const int d0 = w.ww[w.w.ds_ptr + index], d1 = w.ww[w.w.ds_ptr + index + 1];
  ex.lanes([&](int lane) {
    WAI_NET_FP
    const int* ds = w.ww + w.w.ds;
    for (int q = d0 + lane; q < d1; q += Ex::width) source_set_rate(v, s, ds[q], s.src[NET_NODE * ds[q]] * scale);
  });
  const int g0 = w.ww[w.w.dg_ptr + index], g1 = w.ww[w.w.dg_ptr + index + 1];
  for (int q = g0; q < g1; q++) group_sum(ex, v, s, st, w.ww[w.w.dg + q]);
  group_sum(ex, v, s, st, index);
}
// limit_leaf: over and scale from three words of the node, by every lane
template <class Ex>
WAI_NET_HD inline void limit_leaf(Ex& ex, const NetFlatView& v, const NetWaveView& w, NetState& s, double* st, int kind, int index, int nl,
                                  const int* type, const double* limit) {
  WAI_NET_FP
  const double* n = node(s, kind, index);
  bool over = false;
  double scale = 1.0;
  for (int i = 0; i < nl; i++) {
    const double a = dabs(rate_by_type(n, type[i]));
    if (a > limit[i]) { over = true; if (a > 1.e-6) scale = dmin(scale, limit[i] / a); }
  }
  if (over) scale_run(ex, v, w, s, st, kind, index, scale);
}
// limit_inputs_run: the explicit stack and the arena as in the serial text; a frame is written by one lane and read by all.
// The table's |rate|s are gathered by the lanes, the prefix-with-break of each limit runs on a lane of its own, and the lanes
// write the rows.  The inputs that are SOURCES are then limited by the lanes, each against its own row of the table: limit_leaf of a source reads and writes that source alone, and
// the table stands from the group's entry on, so a source's bits do not depend on when among its siblings it is limited (the
// same operations as the serial text, which takes them in input order).  The inputs that are GROUPS follow in input order, as
// there: they share the stack, the arena above the table and the staging run.  A frame's second int counts through the
// schedule's list of those inputs
template <class Ex>
WAI_NET_HD inline void limit_inputs_run(Ex& ex, const NetFlatView& v, const NetWaveView& w, NetState& s, double* st, int atop, int index,
                                        int lim, int nl, const int* type) {
  WAI_NET_FP
  const int* ptr = v.iw + v.h.grp_ptr;
  const int *ik = v.iw + v.h.in_kind, *ii = v.iw + v.h.in_index;
  const int *gcp = w.ww + w.w.gc_ptr, *gc = w.ww + w.w.gc;
  int sp = 1;
  ex.one([&]() { int* f = s.stack; f[0] = index; f[1] = gcp[index]; f[2] = lim; f[3] = -1; });
  while (sp > 0) {
    const int* f = s.stack + NET_FRAME * (sp - 1);
    const int g = f[0], next = f[1], flim = f[2], p0 = ptr[g], m = ptr[g + 1] - p0;
    int tab = f[3];
    if (tab < 0) {   // on entry: the group's node_limit table [m][3] from its inputs' rates as they stand
      tab = atop;
      double* sd = st + NET_WAVE_CTL;
      ex.lanes([&](int lane) {
        WAI_NET_FP
        for (int i = lane; i < m; i += Ex::width) {
          const double* n = node(s, ik[p0 + i], ii[p0 + i]);
          for (int il = 0; il < nl; il++) sd[3 * i + il] = dabs(rate_by_type(n, type[il]));
        }
      });
      // the prefix-with-break of limit il on lane il: where the table breaks and what is left there.  (Without a way out
      // of the loop, so that its reads are in flight together; behind the break nothing is added any more)
      ex.lanes([&](int lane) {
        WAI_NET_FP
        if (lane == 0) s.stack[NET_FRAME * (sp - 1) + 3] = tab;
        if (lane >= nl) return;
        const double limit = s.arena[flim + lane];
        double sum = 0.0, left = 0.0;
        int brk = m;
        WAI_NET_UNROLL
        for (int i = 0; i < m; i++) {
          const double a = sd[3 * i + lane];
          if (brk == m) { if (sum + a > limit) { brk = i; left = limit - sum; } else sum += a; }
        }
        st[2 * lane] = (double)brk; st[2 * lane + 1] = left;
      });
      ex.lanes([&](int lane) {   // every input's row of the table, and limit_leaf of every input that is a source
        WAI_NET_FP
        for (int i = lane; i < m; i += Ex::width) {
          double* row = s.arena + tab + 3 * i;
          for (int il = 0; il < 3; il++) {
            const int brk = il < nl ? (int)st[2 * il] : -1;
            row[il] = i < brk ? sd[3 * i + il] : (i == brk ? st[2 * il + 1] : 0.0);
          }
          if (ik[p0 + i] != NET_SOURCE) continue;
          const int src = ii[p0 + i];
          const double* n = s.src + NET_NODE * src;
          bool over = false;
          double scale = 1.0;
          for (int il = 0; il < nl; il++) {
            const double a = dabs(rate_by_type(n, type[il]));
            if (a > row[il]) { over = true; if (a > 1.e-6) scale = dmin(scale, row[il] / a); }
          }
          if (over) source_set_rate(v, s, src, n[0] * scale);
        }
      });
    }
    atop = tab + 3 * m;   // (what the serial text holds while the frame lives: children pop back to it)
    if (next < gcp[g + 1]) {
      const int i = gc[next], lo = tab + 3 * i, ci = ii[p0 + i];
      if (is_leaf(v, NET_GROUP, ci)) {
        ex.one([&]() { s.stack[NET_FRAME * (sp - 1) + 1] = next + 1; });
        limit_leaf(ex, v, w, s, st, NET_GROUP, ci, nl, type, s.arena + lo);
      } else {
        ex.one([&]() {
          s.stack[NET_FRAME * (sp - 1) + 1] = next + 1;
          int* nf = s.stack + NET_FRAME * sp;
          nf[0] = ci; nf[1] = gcp[ci]; nf[2] = lo; nf[3] = -1;
        });
        sp++;
      }
    } else { group_sum(ex, v, s, st, g); sp--; }
  }
}

// what the injection node of output p can take (its own specified rate, a reinjector's capacity, -1: unrated)
WAI_NET_HD inline double out_node_rate(const NetFlatView& v, const double* raw, const NetState& s, int p) {
  WAI_NET_FP
  const NetFlat& h = v.h;
  const int kind = v.iw[h.out_kind + p], nd = v.iw[h.out_node + p];
  if (kind == NET_SOURCE) return (v.iw[h.src_flags + nd] & 1) ? raw[nd] : -1.0;
  if (kind == NET_REINJ) return s.rj[RJ_STATE * nd + (v.iw[h.out_flow + p] == 1 ? RJ_CAP_W : RJ_CAP_S)];
  return -1.0;
}
// output p of the reinjector with state R carries qq: the separated flows of the serial text
WAI_NET_HD inline void out_flows(const NetFlatView& v, const double* R, int p, double qq, double& qw, double& wh, double& qs, double& sh) {
  WAI_NET_FP
  const int flow = v.iw[v.h.out_flow + p];
  const double oe = v.dw[v.h.out_enth + p];
  qw = flow == 1 ? qq : 0.0;
  qs = flow == 1 ? 0.0 : qq;
  wh = (oe > 0.0 && flow == 1) ? oe : (oe > 0.0 ? 0.0 : R[RJ_IN_WH]);
  sh = (oe > 0.0 && flow == 2) ? oe : (oe > 0.0 ? 0.0 : R[RJ_IN_SH]);
}
WAI_NET_HD inline void deliver_source(const NetFlatView& v, NetState& s, const double* R, int p, double qq) {
  WAI_NET_FP
  double qw, wh, qs, sh, orate_t, oenth_t;
  out_flows(v, R, p, qq, qw, wh, qs, sh);
  total(qw, wh, qs, sh, orate_t, oenth_t);
  const int i = v.iw[v.h.out_node + p];
  s.is_out[i] = 1.0; s.out_rate[i] = orate_t; s.out_enth[i] = oenth_t;
  double* n = s.src + NET_NODE * i;
  n[2] = qw; n[3] = wh; n[4] = qs; n[5] = sh;
}

}  // namespace netwave

// network_pass_serial, wave-wide.  After a limited group only its ANCESTORS are summed again, where the serial text sums every
// later group: a group's sum is a pure function of its inputs' states, and with every node taken in at most once a later
// group that is no ancestor holds nothing that changed, so summing it again would give the bits it has.  This is the only
// place where fewer operations than the serial text run.
template <class Ex>
WAI_NET_HD inline void network_walk_wave(Ex& ex, const NetFlatView& v, const NetWaveView& w, const double* raw, NetState& s, double* st) {
  WAI_NET_FP
  using namespace netwave;
  const NetFlat& h = v.h;
  for (int g = 0; g < h.n_grp; g++) netwave::group_sum(ex, v, s, st, g);
  for (int g = 0; g < h.n_grp; g++) {
    const int nl = v.iw[h.grp_nlimit + g];
    if (!nl) continue;
    const int* type = v.iw + h.grp_ltype + 3 * g;
    const double* limit = v.dw + h.grp_limit + 3 * g;
    if (v.iw[h.grp_scaling + g] == 0) netwave::limit_leaf(ex, v, w, s, st, NET_GROUP, g, nl, type, limit);
    else {
      bool over = false;
      for (int i = 0; i < nl; i++) over = over || dabs(rate_by_type(s.grp + NET_NODE * g, type[i])) > limit[i];
      if (over) {
        ex.one([&]() { for (int i = 0; i < 3; i++) s.arena[i] = limit[i]; });
        netwave::limit_inputs_run(ex, v, w, s, st, 3, g, 0, nl, type);
      }
    }
    for (int q = w.ww[w.w.an_ptr + g]; q < w.ww[w.w.an_ptr + g + 1]; q++) netwave::group_sum(ex, v, s, st, w.ww[w.w.an + q]);
  }
  const int *rik = v.iw + h.rj_in_kind, *rii = v.iw + h.rj_in, *optr = v.iw + h.rj_out_ptr;
  const int *rvk = v.iw + h.rj_over_kind, *rvi = v.iw + h.rj_over, *order = v.iw + h.rj_order;
  const int *oflow = v.iw + h.out_flow, *okind = v.iw + h.out_kind, *onode = v.iw + h.out_node;
  const int* shared = w.ww + w.w.out_shared;
  double* sd = st + NET_WAVE_CTL;
  ex.lanes([&](int lane) { for (int r = lane; r < h.n_rj; r += Ex::width) s.rj[RJ_STATE * r + RJ_FED] = 0.0; });
  for (int q = 0; q < h.n_rj; q++) {   // capacities, downstream first: node rates gathered, the sums chained in output order
    const int r = order[q], p0 = optr[r], m = optr[r + 1] - p0;
    ex.lanes([&](int lane) { WAI_NET_FP for (int i = lane; i < m; i += Ex::width) sd[i] = out_node_rate(v, raw, s, p0 + i); });
    ex.one([&]() {
      WAI_NET_FP
      double cap[3] = {0.0, 0.0, 0.0};
      for (int i = 0; i < m; i++) {
        if (okind[p0 + i] != NET_SOURCE && okind[p0 + i] != NET_REINJ) continue;
        const double node_rate = sd[i];
        double& cc = cap[oflow[p0 + i]];
        if (node_rate > -1.0) { if (cc > -1.0) cc += node_rate; } else cc = -1.0;
      }
      s.rj[RJ_STATE * r + RJ_CAP_W] = cap[1]; s.rj[RJ_STATE * r + RJ_CAP_S] = cap[2];
    });
  }
  for (int q = h.n_rj - 1; q >= 0; q--) {   // distribution, upstream first
    const int r = order[q], p0 = optr[r], m = optr[r + 1] - p0;
    double* R = s.rj + RJ_STATE * r;
    ex.one([&]() {
      WAI_NET_FP
      if (rik[r] == NET_SOURCE || rik[r] == NET_GROUP) {
        const double* in = node(s, rik[r], rii[r]);
        R[RJ_IN_W] = dabs(in[2]); R[RJ_IN_WH] = in[3]; R[RJ_IN_S] = dabs(in[4]); R[RJ_IN_SH] = in[5];
      } else if (R[RJ_FED] == 0.0) { R[RJ_IN_W] = R[RJ_IN_WH] = R[RJ_IN_S] = R[RJ_IN_SH] = 0.0; }
      R[RJ_OUT_W] = R[RJ_OUT_S] = 0.0;
    });
    // what every output asks for before the balance is known (rate, proportion of the input, -1: whatever is left), cut to
    // what its node can take: by the lanes
    ex.lanes([&](int lane) {
      WAI_NET_FP
      const double *orate = v.dw + h.out_rate, *oprop = v.dw + h.out_prop;
      for (int i = lane; i < m; i += Ex::width) {
        const int p = p0 + i;
        double qq;
        if (orate[p] > -1.0) qq = orate[p];
        else if (oprop[p] >= 0.0) qq = oprop[p] * (oflow[p] == 1 ? R[RJ_IN_W] : R[RJ_IN_S]);
        else qq = -1.0;
        if (okind[p]) node_limit_rate(out_node_rate(v, raw, s, p), qq);
        sd[i] = qq;
      }
    });
    // the balance chain in output order; with it, in order, every += into another reinjector, the outputs onto sources with
    // more than one writer, and the overflow
    ex.one([&]() {
      WAI_NET_FP
      double wbal = R[RJ_IN_W], sbal = R[RJ_IN_S], wtot = 0.0, stot = 0.0;   // (the totals start from zero, as R[RJ_OUT_*] do)
      WAI_NET_UNROLL
      for (int i = 0; i < m; i++) {   // (the chain alone: contiguous reads, nothing that depends on a node's address)
        const int p = p0 + i;
        double qq = sd[i];
        double& bal = oflow[p] == 1 ? wbal : sbal;
        double& tot = oflow[p] == 1 ? wtot : stot;
        if (qq < 0.0) qq = bal;
        qq = dmin(qq, bal);
        bal = dmax(bal - qq, 0.0);
        tot += qq;
        sd[i] = qq;
      }
      R[RJ_OUT_W] = wtot; R[RJ_OUT_S] = stot;
      for (int i = 0; i < m; i++) {   // what has to go in output order
        const int p = p0 + i;
        if (okind[p] == NET_REINJ) {
          double qw, wh, qs, sh;
          out_flows(v, R, p, sd[i], qw, wh, qs, sh);
          double* D = s.rj + RJ_STATE * onode[p];
          if (D[RJ_FED] == 0.0) { D[RJ_IN_W] = D[RJ_IN_WH] = D[RJ_IN_S] = D[RJ_IN_SH] = 0.0; D[RJ_FED] = 1.0; }
          if (oflow[p] == 1) { D[RJ_IN_W] += qw; D[RJ_IN_WH] = wh; } else { D[RJ_IN_S] += qs; D[RJ_IN_SH] = sh; }
        } else if (okind[p] == NET_SOURCE && shared[p]) deliver_source(v, s, R, p, sd[i]);
      }
      double* O = R + RJ_OVER;
      O[2] = wbal; O[3] = R[RJ_IN_WH]; O[4] = sbal; O[5] = R[RJ_IN_SH];
      total(wbal, R[RJ_IN_WH], sbal, R[RJ_IN_SH], O[0], O[1]);
      if (rvk[r] == NET_REINJ) {
        double* D = s.rj + RJ_STATE * rvi[r];
        D[RJ_IN_W] = wbal; D[RJ_IN_WH] = R[RJ_IN_WH]; D[RJ_IN_S] = sbal; D[RJ_IN_SH] = R[RJ_IN_SH]; D[RJ_FED] = 1.0;
      } else if (rvk[r] == NET_SOURCE) {   // an overflow source takes what is left, whatever its own rate says
        const int i = rvi[r];
        s.is_out[i] = 1.0; s.out_rate[i] = O[0]; s.out_enth[i] = O[1];
        double* n = s.src + NET_NODE * i;
        n[2] = wbal; n[3] = R[RJ_IN_WH]; n[4] = sbal; n[5] = R[RJ_IN_SH];
      }
    });
    // delivery to the sources that have this output as their one writer: by the lanes
    ex.lanes([&](int lane) {
      WAI_NET_FP
      for (int i = lane; i < m; i += Ex::width)
        if (okind[p0 + i] == NET_SOURCE && !shared[p0 + i]) deliver_source(v, s, R, p0 + i, sd[i]);
    });
  }
}
// network_pass with the wave-wide walk
template <class Ex>
WAI_NET_HD inline void network_pass_wave(Ex& ex, const NetFlatView& v, const NetWaveView& w, const double* raw, NetState& s, double* st) {
  WAI_NET_FP
  ex.lanes([&](int lane) { WAI_NET_FP network_pass_sources(v, raw, s, lane, Ex::width); });
  network_walk_wave(ex, v, w, raw, s, st);
  ex.lanes([&](int lane) { WAI_NET_FP network_pass_final(v, raw, s, lane, Ex::width); });
}

#if defined(__HIPCC__)
// the executor of the kernels: a workgroup of one wave
struct NetWaveDeviceExec {
  static constexpr int width = NET_WAVE_LANES;
  template <class F> __device__ __forceinline__ void lanes(F&& f) { __syncthreads(); f((int)threadIdx.x); __syncthreads(); }
  template <class F> __device__ __forceinline__ void one(F&& f) { __syncthreads(); if (threadIdx.x == 0) f(); __syncthreads(); }
};
// n words from global memory to LDS by the wave, eight loads of a lane in flight before the first is stored
template <class T>
__device__ __forceinline__ void net_wave_copy(T* dst, const T* __restrict__ src, int n, int t) {
  constexpr int U = 8;
  for (int i0 = t; i0 < n; i0 += U * NET_WAVE_LANES) {
    T r[U];
#pragma unroll
    for (int k = 0; k < U; k++) { const int i = i0 + k * NET_WAVE_LANES; r[k] = i < n ? src[i] : T(0); }
#pragma unroll
    for (int k = 0; k < U; k++) { const int i = i0 + k * NET_WAVE_LANES; if (i < n) dst[i] = r[k]; }
  }
}
// The pass of a workgroup of one wave on its dynamic LDS (k_network_pass_wave, k_cb_pass_wave):
//   [ dw | raw 2n | state (net_state_carve) | staging | iw | ww ]      net_wave_lds_doubles(h, w) doubles, decided by the builder
// s: the state's arrays in LDS on return (net, enth: where the factors and the fed sources' enthalpies go, from the caller)
__device__ inline void net_wave_pass_lds(const NetFlat& h, const NetWave& w, const int* __restrict__ iw, const double* __restrict__ dw,
                                         const int* __restrict__ ww, const double* __restrict__ raw, double* net, double* enth, double* lds,
                                         NetState& s) {
  const int t = threadIdx.x, n = h.n_src;
  double* sdw = lds;
  double* sraw = sdw + h.n_dw;
  double* sstate = sraw + 2 * n;
  double* sstage = sstate + net_state_doubles(h);
  int* siw = reinterpret_cast<int*>(sstage + w.stage);
  int* sww = siw + 2 * ((h.n_iw + 1) / 2);
  net_wave_copy(sdw, dw, h.n_dw, t);
  net_wave_copy(sraw, raw, 2 * n, t);
  net_wave_copy(siw, iw, h.n_iw, t);
  net_wave_copy(sww, ww, w.n_ww, t);
  const NetFlatView v{h, siw, sdw};
  const NetWaveView wv{w, sww};
  net_state_carve(h, sstate, s);
  s.net = net; s.enth = enth;
  NetWaveDeviceExec ex;
  network_pass_wave(ex, v, wv, sraw, s, sstage);   // (every executor call starts with a barrier: the copies above are in)
}
#endif

}  // namespace wai

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif

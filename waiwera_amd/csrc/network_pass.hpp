// One pass of the source network (groups, limiters, separators, reinjectors, overflow chains) on a FLAT description: one
// array of ints, one of doubles.  THE pass of the library: the same text runs on the host (network_update and
// wai_network_evaluate, network.hip) and inside a kernel (k_network_pass, kernels_network.hip), and build_net_flat below is
// the one place a description is validated.  Host-only compatible, like mesh_pattern.hpp, ilu_schedule.hpp and
// colour_order.hpp: no HIP header; tests/network_pass_host runs it without a device.
//
// Every sum over a group's inputs runs in input order, and no product and sum are contracted into one rounding: host and
// device then give the same bits -- those recorded in tests/golden/network_pass_bits.json from the recursive pass on a
// network of structs this one replaced.  No recursion and no allocation: an explicit stack of frames walks nested groups,
// and the progressive limiter's node_limit tables live in a scratch arena -- build_net_flat sizes both from the nesting.
#pragma once
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define WAI_NET_HD __host__ __device__
#else
#define WAI_NET_HD
#endif
// no contraction, and only here: the pragma stands at the head of every function body below (at file scope it would reach
// whatever a translation unit includes after this header)
#if defined(__clang__)
#define WAI_NET_FP _Pragma("clang fp contract(off)")
#else
#define WAI_NET_FP
#if defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif
#endif

namespace wai {

// node kinds of a reference (kind, index), as in wai_set_source_network
enum { NET_NONE = 0, NET_SOURCE = 1, NET_GROUP = 2, NET_REINJ = 3 };
// a reinjector's state: capacities (water, steam; -1 unrated), input flows, delivered totals, overflow node, fed flag
enum { RJ_CAP_W = 0, RJ_CAP_S = 1, RJ_IN_W = 2, RJ_IN_WH = 3, RJ_IN_S = 4, RJ_IN_SH = 5, RJ_OUT_W = 6, RJ_OUT_S = 7,
       RJ_OVER = 8, RJ_FED = 14, RJ_STATE = 15 };
constexpr int NET_NODE = 6;    // rate, enthalpy, water rate, water enthalpy, steam rate, steam enthalpy
constexpr int NET_FRAME = 4;   // ints of a stack frame: group, next input, offset of its limits, offset of its table (arena)

// The description: counts, the offsets of its arrays in one array of ints (iw) and one of doubles (dw), and what a pass
// needs beside them.  Plain and trivially copyable; the two word arrays travel with it (NetFlatHost owns them on the
// host, k_network_pass copies them to LDS).
struct NetFlat {
  int n_src = 0, n_grp = 0, n_rj = 0, n_out = 0, n_in = 0;
  int n_iw = 0, n_dw = 0;      // length of iw / dw
  int stack_frames = 0;        // frames of the explicit stack (from the depth of the groups' nesting)
  int arena = 0;               // doubles of the limiters' scratch arena: 3 + the deepest chain of progressive tables
  // iw: per source flags (bit 0 rate specified, bit 1 enthalpy specified); per group the input range [n_grp + 1], the
  // scaling, the number of limits and their types [3]; the inputs' kinds and indices; per reinjector the input, the output
  // range [n_rj + 1], the overflow; the evaluation order (a reinjector after those it delivers or overflows to); per
  // output flow, kind, node
  int src_flags = 0, grp_ptr = 0, grp_scaling = 0, grp_nlimit = 0, grp_ltype = 0, in_kind = 0, in_index = 0;
  int rj_in_kind = 0, rj_in = 0, rj_out_ptr = 0, rj_over_kind = 0, rj_over = 0, rj_order = 0;
  int out_flow = 0, out_kind = 0, out_node = 0;
  // dw: per source the specified enthalpy and the eight separator enthalpies; per group limits [3] and separator [8];
  // per output rate, proportion, enthalpy
  int src_enth0 = 0, src_sep = 0, grp_limit = 0, grp_sep = 0, out_rate = 0, out_prop = 0, out_enth = 0;
};
struct NetFlatView {
  NetFlat h;
  const int* iw;
  const double* dw;
};
// what a pass writes.  src / grp: NET_NODE doubles per node; rj: RJ_STATE per reinjector; out_rate, out_enth, is_out: per
// source, what the reinjectors feed it; arena / stack: scratch (NetFlat::arena doubles, NET_FRAME * stack_frames ints);
// net: the (mode, value) pair per source the residual kernel applies (source_network_rate); enth: the enthalpy of the
// sources a reinjector feeds -- the entries of all other sources are not touched
struct NetState {
  double *src, *grp, *rj, *out_rate, *out_enth, *is_out, *arena;
  int* stack;
  double *net, *enth;
};
// doubles of the state arrays of NetState (without net and enth), the stack's ints counted as half doubles
WAI_NET_HD inline int net_state_doubles(const NetFlat& h) {
  WAI_NET_FP
  return NET_NODE * (h.n_src + h.n_grp) + RJ_STATE * h.n_rj + 3 * h.n_src + h.arena + (NET_FRAME * h.stack_frames + 1) / 2;
}
// the state arrays on one run of doubles, in this order (the kernel's LDS, the host program's buffer)
WAI_NET_HD inline void net_state_carve(const NetFlat& h, double* base, NetState& s) {
  WAI_NET_FP
  s.src = base; base += NET_NODE * h.n_src;
  s.grp = base; base += NET_NODE * h.n_grp;
  s.rj = base; base += RJ_STATE * h.n_rj;
  s.out_rate = base; base += h.n_src;
  s.out_enth = base; base += h.n_src;
  s.is_out = base; base += h.n_src;
  s.arena = base; base += h.arena;
  s.stack = reinterpret_cast<int*>(base);
}

namespace netpass {

WAI_NET_HD inline double dmin(double a, double b) { return b < a ? b : a; }   // std::min
WAI_NET_HD inline double dmax(double a, double b) { return a < b ? b : a; }   // std::max
WAI_NET_HD inline double dabs(double a) { WAI_NET_FP return __builtin_fabs(a); }

// separator.F90:139-166, 212-260: sep = hf, hg of stage 1, then (hf, hg) of stages 2..4
WAI_NET_HD inline void separate(const double* sep, double rate, double enth, double* n) {
  WAI_NET_FP
  double q = rate, h = enth, steam_m = 0.0, steam_e = 0.0;
  for (int st = 0; st < 4; st++) {
    const double hf = sep[2 * st], hg = sep[2 * st + 1];
    if (st > 0 && !(hg > 0.0)) break;
    double f, hw, hs;
    if (h <= hf) { f = 0.0; hw = h; hs = 0.0; }
    else if (h <= hg) { f = (h - hf) / (hg - hf); hw = hf; hs = hg; }
    else { f = 1.0; hw = 0.0; hs = h; }
    const double sr = f * q;
    steam_m += sr; steam_e += sr * hs;
    q = (1.0 - f) * q; h = hw;
  }
  n[2] = q; n[3] = h; n[4] = steam_m;
  n[5] = dabs(steam_m) > 1.e-9 ? steam_e / steam_m : 0.0;
}
WAI_NET_HD inline void source_set_rate(const NetFlatView& v, NetState& s, int i, double rate) {
  WAI_NET_FP
  double* n = s.src + NET_NODE * i;
  n[0] = rate;
  const double* sep = v.dw + v.h.src_sep + 8 * i;
  if (rate < 0.0 && sep[1] > 0.0) separate(sep, rate, n[1], n);
  else n[2] = n[3] = n[4] = n[5] = 0.0;
}
WAI_NET_HD inline double* node(NetState& s, int kind, int index) {
  WAI_NET_FP
  return kind == NET_SOURCE ? s.src + NET_NODE * index : s.grp + NET_NODE * index;
}
WAI_NET_HD inline double rate_by_type(const double* n, int type) { WAI_NET_FP return type == 1 ? n[2] : (type == 2 ? n[4] : n[0]); }

WAI_NET_HD inline void group_sum(const NetFlatView& v, NetState& s, int g) {
  WAI_NET_FP
  const int* ptr = v.iw + v.h.grp_ptr;
  const int *ik = v.iw + v.h.in_kind, *ii = v.iw + v.h.in_index;
  double* G = s.grp + NET_NODE * g;
  double q = 0.0, qh = 0.0;
  for (int p = ptr[g]; p < ptr[g + 1]; p++) { const double* n = node(s, ik[p], ii[p]); q += n[0]; qh += n[0] * n[1]; }
  G[1] = dabs(q) > 1.e-9 ? qh / q : 0.0;
  G[0] = q;
  const double* sep = v.dw + v.h.grp_sep + 8 * g;
  if (q < 0.0 && sep[1] > 0.0) separate(sep, q, G[1], G);
  else if (q < 0.0) {
    double wq = 0, wqh = 0, sq = 0, sqh = 0;
    for (int p = ptr[g]; p < ptr[g + 1]; p++) {
      const double* n = node(s, ik[p], ii[p]);
      wq += n[2]; wqh += n[2] * n[3]; sq += n[4]; sqh += n[4] * n[5];
    }
    G[2] = wq; G[4] = sq;
    G[3] = dabs(wq) > 1.e-9 ? wqh / wq : 0.0;
    G[5] = dabs(sq) > 1.e-9 ? sqh / sq : 0.0;
  } else G[2] = G[3] = G[4] = G[5] = 0.0;
}

// scale_rate: everything below (kind, index) times `scale`, the groups summed again on the way up.  Frames above sp.
WAI_NET_HD inline void scale_run(const NetFlatView& v, NetState& s, int& sp, int kind, int index, double scale) {
  WAI_NET_FP
  if (kind == NET_SOURCE) { source_set_rate(v, s, index, s.src[NET_NODE * index] * scale); return; }
  const int* ptr = v.iw + v.h.grp_ptr;
  const int *ik = v.iw + v.h.in_kind, *ii = v.iw + v.h.in_index;
  const int base = sp;
  int* f = s.stack + NET_FRAME * sp++;
  f[0] = index; f[1] = ptr[index];
  while (sp > base) {
    f = s.stack + NET_FRAME * (sp - 1);
    const int g = f[0];
    if (f[1] < ptr[g + 1]) {
      const int p = f[1]++;
      if (ik[p] == NET_SOURCE) source_set_rate(v, s, ii[p], s.src[NET_NODE * ii[p]] * scale);
      else { int* n = s.stack + NET_FRAME * sp++; n[0] = ii[p]; n[1] = ptr[ii[p]]; }
    } else { group_sum(v, s, g); sp--; }
  }
}
// a source or a uniform group under limits: one factor for everything below
WAI_NET_HD inline void limit_leaf(const NetFlatView& v, NetState& s, int& sp, int kind, int index, int nl, const int* type,
                                  const double* limit) {
  WAI_NET_FP
  const double* n = node(s, kind, index);
  bool over = false;
  double scale = 1.0;
  for (int i = 0; i < nl; i++) {
    const double a = dabs(rate_by_type(n, type[i]));
    if (a > limit[i]) { over = true; if (a > 1.e-6) scale = dmin(scale, limit[i] / a); }
  }
  if (over) scale_run(v, s, sp, kind, index, scale);
}
WAI_NET_HD inline bool is_leaf(const NetFlatView& v, int kind, int index) {
  WAI_NET_FP
  return kind == NET_SOURCE || v.iw[v.h.grp_scaling + index] == 0;
}
// a progressive group's inputs are limited in order until the total is met; the limits of (kind, index)
// are the three doubles at arena[lim]; atop: the arena's first free double
WAI_NET_HD inline void limit_inputs_run(const NetFlatView& v, NetState& s, int& sp, int atop, int kind, int index, int lim, int nl,
                                        const int* type) {
  WAI_NET_FP
  if (is_leaf(v, kind, index)) { limit_leaf(v, s, sp, kind, index, nl, type, s.arena + lim); return; }
  const int* ptr = v.iw + v.h.grp_ptr;
  const int *ik = v.iw + v.h.in_kind, *ii = v.iw + v.h.in_index;
  const int base = sp;
  int* f = s.stack + NET_FRAME * sp++;
  f[0] = index; f[1] = ptr[index]; f[2] = lim; f[3] = -1;
  while (sp > base) {
    f = s.stack + NET_FRAME * (sp - 1);
    const int g = f[0], p0 = ptr[g], m = ptr[g + 1] - p0;
    if (f[3] < 0) {   // on entry: the group's node_limit table [m][3] from its inputs' rates as they stand
      f[3] = atop; atop += 3 * m;
      double* tab = s.arena + f[3];
      const double* limit = s.arena + f[2];
      for (int q = 0; q < 3 * m; q++) tab[q] = 0.0;
      for (int il = 0; il < nl; il++) {
        double sum = 0.0;
        for (int i = 0; i < m; i++) {
          const double a = dabs(rate_by_type(node(s, ik[p0 + i], ii[p0 + i]), type[il]));
          if (sum + a > limit[il]) { tab[i * 3 + il] = limit[il] - sum; break; }
          tab[i * 3 + il] = a;
          sum += a;
        }
      }
    }
    if (f[1] < p0 + m) {
      const int p = f[1]++, lo = f[3] + 3 * (p - p0);
      if (is_leaf(v, ik[p], ii[p])) limit_leaf(v, s, sp, ik[p], ii[p], nl, type, s.arena + lo);
      else { int* n = s.stack + NET_FRAME * sp++; n[0] = ii[p]; n[1] = ptr[ii[p]]; n[2] = lo; n[3] = -1; }
    } else { group_sum(v, s, g); atop = f[3]; sp--; }
  }
}
WAI_NET_HD inline void node_limit_rate(double node_rate, double& rate) {   // reinjector.F90:199-215
  if (node_rate > -1.0) rate = rate > -1.0 ? dmin(rate, node_rate) : node_rate;
}
WAI_NET_HD inline void total(double wr, double wh, double sr, double sh, double& rate, double& enth) {
  WAI_NET_FP
  rate = wr + sr;
  enth = rate > 1.e-6 ? (wr * wh + sr * sh) / rate : 0.0;
}

}  // namespace netpass

// ---- the pass in three parts: sources i0, i0 + stride, .. (independent of one another); the groups and reinjectors (one
// thread); the sources again ------------------------------------------------------------------------------------------
// raw: the sources' own rates [n], then their flowing enthalpies [n]
WAI_NET_HD inline void network_pass_sources(const NetFlatView& v, const double* raw, NetState& s, int i0, int stride) {
  WAI_NET_FP
  const int n = v.h.n_src;
  for (int i = i0; i < n; i += stride) {
    s.src[NET_NODE * i + 1] = raw[n + i];
    netpass::source_set_rate(v, s, i, raw[i]);
    s.out_rate[i] = 0.0; s.out_enth[i] = 0.0; s.is_out[i] = 0.0;
  }
}
WAI_NET_HD inline void network_pass_serial(const NetFlatView& v, const double* raw, NetState& s) {
  WAI_NET_FP
  using namespace netpass;
  const NetFlat& h = v.h;
  int sp = 0;
  for (int g = 0; g < h.n_grp; g++) group_sum(v, s, g);
  for (int g = 0; g < h.n_grp; g++) {
    const int nl = v.iw[h.grp_nlimit + g];
    if (!nl) continue;
    const int* type = v.iw + h.grp_ltype + 3 * g;
    const double* limit = v.dw + h.grp_limit + 3 * g;
    if (v.iw[h.grp_scaling + g] == 0) limit_leaf(v, s, sp, NET_GROUP, g, nl, type, limit);
    else {
      bool over = false;
      for (int i = 0; i < nl; i++) over = over || dabs(rate_by_type(s.grp + NET_NODE * g, type[i])) > limit[i];
      if (over) {
        for (int i = 0; i < 3; i++) s.arena[i] = limit[i];
        limit_inputs_run(v, s, sp, 3, NET_GROUP, g, 0, nl, type);
      }
    }
    for (int gj = g + 1; gj < h.n_grp; gj++) group_sum(v, s, gj);   // sum_out
  }
  const int* flags = v.iw + h.src_flags;
  const int *rik = v.iw + h.rj_in_kind, *rii = v.iw + h.rj_in, *optr = v.iw + h.rj_out_ptr;
  const int *rvk = v.iw + h.rj_over_kind, *rvi = v.iw + h.rj_over, *order = v.iw + h.rj_order;
  const int *oflow = v.iw + h.out_flow, *okind = v.iw + h.out_kind, *onode = v.iw + h.out_node;
  const double *orate = v.dw + h.out_rate, *oprop = v.dw + h.out_prop, *oenth = v.dw + h.out_enth;
  // what the injection sources can take: their own specified rate, -1 if none
  for (int r = 0; r < h.n_rj; r++) s.rj[RJ_STATE * r + RJ_FED] = 0.0;
  for (int q = 0; q < h.n_rj; q++) {   // capacities, downstream first
    const int r = order[q];
    double cap[3] = {0.0, 0.0, 0.0};
    for (int p = optr[r]; p < optr[r + 1]; p++) {
      double node_rate = -1.0;
      if (okind[p] == NET_SOURCE) node_rate = (flags[onode[p]] & 1) ? raw[onode[p]] : -1.0;
      else if (okind[p] == NET_REINJ) node_rate = s.rj[RJ_STATE * onode[p] + (oflow[p] == 1 ? RJ_CAP_W : RJ_CAP_S)];
      else continue;
      double& cc = cap[oflow[p]];
      if (node_rate > -1.0) { if (cc > -1.0) cc += node_rate; } else cc = -1.0;
    }
    s.rj[RJ_STATE * r + RJ_CAP_W] = cap[1]; s.rj[RJ_STATE * r + RJ_CAP_S] = cap[2];
  }
  for (int q = h.n_rj - 1; q >= 0; q--) {   // distribution, upstream first
    const int r = order[q];
    double* R = s.rj + RJ_STATE * r;
    if (rik[r] == NET_SOURCE || rik[r] == NET_GROUP) {
      const double* in = node(s, rik[r], rii[r]);
      R[RJ_IN_W] = dabs(in[2]); R[RJ_IN_WH] = in[3]; R[RJ_IN_S] = dabs(in[4]); R[RJ_IN_SH] = in[5];
    } else if (R[RJ_FED] == 0.0) { R[RJ_IN_W] = R[RJ_IN_WH] = R[RJ_IN_S] = R[RJ_IN_SH] = 0.0; }
    double wbal = R[RJ_IN_W], sbal = R[RJ_IN_S];
    R[RJ_OUT_W] = R[RJ_OUT_S] = 0.0;
    for (int p = optr[r]; p < optr[r + 1]; p++) {
      double qw = 0.0, qs = 0.0;
      double& qq = oflow[p] == 1 ? qw : qs;
      if (orate[p] > -1.0) qq = orate[p];                                               // rate output
      else if (oprop[p] >= 0.0) qq = oprop[p] * (oflow[p] == 1 ? R[RJ_IN_W] : R[RJ_IN_S]);   // proportion output
      else qq = -1.0;                                                                   // whatever is left
      double node_rate = -1.0;
      if (okind[p] == NET_SOURCE) node_rate = (flags[onode[p]] & 1) ? raw[onode[p]] : -1.0;
      else if (okind[p] == NET_REINJ) node_rate = s.rj[RJ_STATE * onode[p] + (oflow[p] == 1 ? RJ_CAP_W : RJ_CAP_S)];
      if (okind[p]) node_limit_rate(node_rate, qq);
      double& bal = oflow[p] == 1 ? wbal : sbal;
      double& tot = oflow[p] == 1 ? R[RJ_OUT_W] : R[RJ_OUT_S];
      if (qq < 0.0) qq = bal;
      qq = dmin(qq, bal);
      bal = dmax(bal - qq, 0.0);
      tot += qq;
      // enthalpies: specified for this flow type, or the input's
      const double wh = (oenth[p] > 0.0 && oflow[p] == 1) ? oenth[p] : (oenth[p] > 0.0 ? 0.0 : R[RJ_IN_WH]);
      const double sh = (oenth[p] > 0.0 && oflow[p] == 2) ? oenth[p] : (oenth[p] > 0.0 ? 0.0 : R[RJ_IN_SH]);
      double orate_t, oenth_t;
      total(qw, wh, qs, sh, orate_t, oenth_t);
      if (okind[p] == NET_SOURCE) {
        const int i = onode[p];
        s.is_out[i] = 1.0; s.out_rate[i] = orate_t; s.out_enth[i] = oenth_t;
        double* n = s.src + NET_NODE * i;
        n[2] = qw; n[3] = wh; n[4] = qs; n[5] = sh;
      } else if (okind[p] == NET_REINJ) {
        double* D = s.rj + RJ_STATE * onode[p];
        if (D[RJ_FED] == 0.0) { D[RJ_IN_W] = D[RJ_IN_WH] = D[RJ_IN_S] = D[RJ_IN_SH] = 0.0; D[RJ_FED] = 1.0; }
        if (oflow[p] == 1) { D[RJ_IN_W] += qw; D[RJ_IN_WH] = wh; } else { D[RJ_IN_S] += qs; D[RJ_IN_SH] = sh; }
      }
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
  }
}
// reinjector_output_update for the fed sources, then what the residual kernel is handed (source_network_rate): mode 2
// with the output rate for fed sources, mode 1 with rate / raw where the rate changed, otherwise 0; the enthalpy of fed
// sources, and of those only
WAI_NET_HD inline void network_pass_final(const NetFlatView& v, const double* raw, NetState& s, int i0, int stride) {
  WAI_NET_FP
  const int n = v.h.n_src;
  for (int i = i0; i < n; i += stride) {
    double* nd = s.src + NET_NODE * i;
    double mode = 0.0, val = 0.0;
    if (s.is_out[i] != 0.0) {
      nd[0] = s.out_rate[i];
      nd[1] = (v.iw[v.h.src_flags + i] & 2) ? v.dw[v.h.src_enth0 + i] : s.out_enth[i];
      mode = 2.0; val = s.out_rate[i];
      if (s.enth) s.enth[i] = nd[1];
    } else if (nd[0] != raw[i]) {
      mode = 1.0; val = raw[i] != 0.0 ? nd[0] / raw[i] : 1.0;
    }
    if (s.net) { s.net[2 * i] = mode; s.net[2 * i + 1] = val; }
  }
}
WAI_NET_HD inline void network_pass(const NetFlatView& v, const double* raw, NetState& s) {
  WAI_NET_FP
  network_pass_sources(v, raw, s, 0, 1);
  network_pass_serial(v, raw, s);
  network_pass_final(v, raw, s, 0, 1);
}
// What is kept of a pass, on the host and on the device alike (Network::h_state, d_state; wai_get_source_network,
// wai_network_evaluate): sources NET_NODE doubles each, groups NET_NODE each, reinjectors 8 each (delivered water and steam,
// then the overflow node).  Entries i0, i0 + stride, ..
WAI_NET_HD inline int net_kept_doubles(const NetFlat& h) { return NET_NODE * (h.n_src + h.n_grp) + 8 * h.n_rj; }
WAI_NET_HD inline void net_state_keep(const NetFlat& h, const NetState& s, double* out, int i0, int stride) {
  const int nn = NET_NODE * (h.n_src + h.n_grp);   // sources and groups are one run of the state
  for (int i = i0; i < nn; i += stride) out[i] = s.src[i];
  for (int i = i0; i < 8 * h.n_rj; i += stride) out[nn + i] = s.rj[RJ_STATE * (i >> 3) + RJ_OUT_W + (i & 7)];
}

// ---- the builder (host) ---------------------------------------------------------------------------------------------
// the order in which reinjectors are evaluated: a reinjector after every reinjector it delivers or overflows to (depth
// first from reinjector 0, outputs in order, then the overflow).  false: the reinjectors form a cycle
inline bool net_reinjector_order(int n_reinj, const int* rj_out_ptr, const int* out_kind, const int* out_node,
                                 const int* rj_overflow_kind, const int* rj_overflow, std::vector<int>& order) {
  order.clear();
  std::vector<int> state((size_t)(n_reinj > 0 ? n_reinj : 0), 0), stack, pos;
  for (int r0 = 0; r0 < n_reinj; r0++) {
    if (state[r0] == 2) continue;
    stack.assign(1, r0); pos.assign(1, rj_out_ptr[r0]);
    state[r0] = 1;
    while (!stack.empty()) {
      const int r = stack.back();
      int next = -1;
      while (pos.back() <= rj_out_ptr[r + 1] && next < 0) {   // position rj_out_ptr[r + 1] stands for the overflow
        const int p = pos.back()++;
        if (p < rj_out_ptr[r + 1]) { if (out_kind[p] == NET_REINJ) next = out_node[p]; }
        else if (rj_overflow_kind[r] == NET_REINJ) next = rj_overflow[r];
      }
      if (next < 0) { state[r] = 2; order.push_back(r); stack.pop_back(); pos.pop_back(); continue; }
      if (state[next] == 1) return false;
      if (state[next] == 0) { state[next] = 1; stack.push_back(next); pos.push_back(rj_out_ptr[next]); }
    }
  }
  return true;
}

struct NetFlatHost {
  NetFlat h;
  std::vector<int> iw;
  std::vector<double> dw;
  NetFlatView view() const { return NetFlatView{h, iw.data(), dw.data()}; }
};

// The flat description from the arrays of wai_set_source_network, validated here and nowhere else (the refusals' texts are
// the library's), the sources' separators (8 doubles each, null: none) and specified enthalpies (null: 0).
// 0, or -2 with a text
inline int build_net_flat(NetFlatHost& F, int n, const int* rate_specified, const int* enthalpy_specified, const double* src_sep,
                          const double* src_enth0, int n_groups, const int* grp_ptr, const int* grp_in_kind, const int* grp_in,
                          const int* grp_scaling, const int* grp_limit_type, const double* grp_limit, const double* grp_sep,
                          int n_reinj, const int* rj_in_kind, const int* rj_in, const int* rj_out_ptr, const int* out_flow,
                          const int* out_kind, const int* out_node, const double* out_rate, const double* out_proportion,
                          const double* out_enthalpy, const int* rj_overflow_kind, const int* rj_overflow, std::string& err) {
  if (n <= 0 || !rate_specified || !enthalpy_specified) { err = "source network without sources"; return -2; }
  if (n_groups < 0) n_groups = 0;
  if (n_reinj < 0) n_reinj = 0;
  auto ok = [&](int kind, int idx) {
    return kind == 0 || (kind == 1 && idx >= 0 && idx < n) || (kind == 2 && idx >= 0 && idx < n_groups) ||
           (kind == 3 && idx >= 0 && idx < n_reinj);
  };
  const int n_in = n_groups ? grp_ptr[n_groups] : 0, n_out = n_reinj ? rj_out_ptr[n_reinj] : 0;
  for (int g = 0; g < n_groups; g++)
    for (int q = grp_ptr[g]; q < grp_ptr[g + 1]; q++)
      if (!ok(grp_in_kind[q], grp_in[q]) || grp_in_kind[q] == 0 || grp_in_kind[q] == 3 || (grp_in_kind[q] == 2 && grp_in[q] >= g)) {
        err = "source network group: inputs are sources or earlier groups"; return -2;
      }
  for (int r = 0; r < n_reinj; r++) {
    if (!ok(rj_in_kind[r], rj_in[r]) || rj_in_kind[r] == 3 || !ok(rj_overflow_kind[r], rj_overflow[r]) || rj_overflow_kind[r] == 2) {
      err = "source network reinjector: bad input / overflow reference"; return -2;
    }
    for (int q = rj_out_ptr[r]; q < rj_out_ptr[r + 1]; q++)
      if (!ok(out_kind[q], out_node[q]) || out_kind[q] == 2 || (out_flow[q] != 1 && out_flow[q] != 2)) {
        err = "source network reinjector: bad output"; return -2;
      }
  }
  std::vector<int> order;
  if (!net_reinjector_order(n_reinj, rj_out_ptr, out_kind, out_node, rj_overflow_kind, rj_overflow, order)) {
    err = "source network reinjectors form a cycle"; return -2;
  }
  NetFlat& h = F.h;
  h = NetFlat();
  h.n_src = n; h.n_grp = n_groups; h.n_rj = n_reinj; h.n_out = n_out; h.n_in = n_in;
  int io = 0, dpos = 0;
  auto ints = [&](int count) { const int at = io; io += count; return at; };
  auto dbls = [&](int count) { const int at = dpos; dpos += count; return at; };
  h.src_flags = ints(n); h.grp_ptr = ints(n_groups + 1); h.grp_scaling = ints(n_groups); h.grp_nlimit = ints(n_groups);
  h.grp_ltype = ints(3 * n_groups); h.in_kind = ints(n_in); h.in_index = ints(n_in);
  h.rj_in_kind = ints(n_reinj); h.rj_in = ints(n_reinj); h.rj_out_ptr = ints(n_reinj + 1); h.rj_over_kind = ints(n_reinj);
  h.rj_over = ints(n_reinj); h.rj_order = ints(n_reinj); h.out_flow = ints(n_out); h.out_kind = ints(n_out); h.out_node = ints(n_out);
  h.src_enth0 = dbls(n); h.src_sep = dbls(8 * n); h.grp_limit = dbls(3 * n_groups); h.grp_sep = dbls(8 * n_groups);
  h.out_rate = dbls(n_out); h.out_prop = dbls(n_out); h.out_enth = dbls(n_out);
  h.n_iw = io; h.n_dw = dpos;
  F.iw.assign((size_t)io, 0);
  F.dw.assign((size_t)dpos, 0.0);
  int* iw = F.iw.data();
  double* dw = F.dw.data();
  for (int i = 0; i < n; i++) {
    iw[h.src_flags + i] = (rate_specified[i] ? 1 : 0) | (enthalpy_specified[i] ? 2 : 0);
    dw[h.src_enth0 + i] = src_enth0 ? src_enth0[i] : 0.0;
    for (int q = 0; q < 8; q++) dw[h.src_sep + 8 * i + q] = src_sep ? src_sep[8 * i + q] : 0.0;
  }
  // nesting: depth[g] groups on the longest chain down from g; table[g] doubles of the progressive tables on such a chain
  std::vector<int> depth((size_t)n_groups, 1), table((size_t)n_groups, 0);
  int max_depth = 0, max_table = 0;
  iw[h.grp_ptr] = 0;
  for (int g = 0; g < n_groups; g++) {
    iw[h.grp_ptr + g + 1] = grp_ptr[g + 1] - grp_ptr[0];
    iw[h.grp_scaling + g] = grp_scaling ? grp_scaling[g] : 0;
    int nl = 0;
    for (int l = 0; l < 3; l++)
      if (grp_limit_type && grp_limit_type[3 * g + l] >= 0) {
        iw[h.grp_ltype + 3 * g + nl] = grp_limit_type[3 * g + l]; dw[h.grp_limit + 3 * g + nl] = grp_limit[3 * g + l]; nl++;
      }
    iw[h.grp_nlimit + g] = nl;
    for (int q = 0; q < 8; q++) dw[h.grp_sep + 8 * g + q] = grp_sep ? grp_sep[8 * g + q] : 0.0;
    int below = 0, tbelow = 0;
    for (int q = grp_ptr[g]; q < grp_ptr[g + 1]; q++) {
      iw[h.in_kind + q - grp_ptr[0]] = grp_in_kind[q]; iw[h.in_index + q - grp_ptr[0]] = grp_in[q];
      if (grp_in_kind[q] == NET_GROUP) {
        below = depth[grp_in[q]] > below ? depth[grp_in[q]] : below;
        tbelow = table[grp_in[q]] > tbelow ? table[grp_in[q]] : tbelow;
      }
    }
    depth[g] = 1 + below;
    table[g] = iw[h.grp_scaling + g] != 0 ? 3 * (grp_ptr[g + 1] - grp_ptr[g]) + tbelow : 0;
    max_depth = depth[g] > max_depth ? depth[g] : max_depth;
    max_table = table[g] > max_table ? table[g] : max_table;
  }
  // a chain of limit_inputs frames and, above it, a chain of scale frames: at most two frames per level of the nesting
  h.stack_frames = 2 * max_depth + 2;
  h.arena = 3 + max_table;
  iw[h.rj_out_ptr] = 0;
  for (int r = 0; r < n_reinj; r++) {
    iw[h.rj_in_kind + r] = rj_in_kind[r]; iw[h.rj_in + r] = rj_in[r];
    iw[h.rj_out_ptr + r + 1] = rj_out_ptr[r + 1] - rj_out_ptr[0];
    iw[h.rj_over_kind + r] = rj_overflow_kind[r]; iw[h.rj_over + r] = rj_overflow[r];
    iw[h.rj_order + r] = order[r];
  }
  for (int q = 0; q < n_out; q++) {
    const int p = rj_out_ptr[0] + q;
    iw[h.out_flow + q] = out_flow[p]; iw[h.out_kind + q] = out_kind[p]; iw[h.out_node + q] = out_node[p];
    dw[h.out_rate + q] = out_rate[p]; dw[h.out_prop + q] = out_proportion[p]; dw[h.out_enth + q] = out_enthalpy[p];
  }
  return 0;
}

// doubles a workgroup needs to hold the description, the raw rates and the state (k_network_pass's LDS), and the limit
constexpr int NET_LDS_DOUBLES = 8192;   // the 64 KB of static LDS a workgroup may declare
inline int net_lds_doubles(const NetFlat& h) { return h.n_dw + (h.n_iw + 1) / 2 + 2 * h.n_src + net_state_doubles(h); }

}  // namespace wai

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif

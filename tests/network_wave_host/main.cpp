// The source network's wave-wide walk (waiwera_amd/csrc/network_wave.hpp) without a device: reads a network and the sources'
// raw rates from a text file of records "name count values..." (the format of tests/network_pass_host), builds the flat
// description and the wave schedule, and runs network_pass_wave over 64 EMULATED lanes three times -- lanes ascending,
// descending and in a seeded shuffle.  Every double each run wrote is printed in hexadecimal; a difference between the three
// is a race between the lanes of one phase.  tests/test_network_wave_host.py builds this with the address and
// undefined-behaviour sanitizers and compares with the recorded bits (tests/golden/network_pass_bits.json).
//   network_wave_host FILE [SEED]  ->  "schedule.NAME ints..." for fan_in stage lds ds_ptr ds dg_ptr dg an_ptr an gc_ptr gc out_shared,
//                                      then per ORDER in ascending, descending, shuffled: "sources.ORDER ..." (6 each),
//                                      "groups.ORDER ..." (6 each), "reinjectors.ORDER ..." (8 each), "net.ORDER ..." (2 each),
//                                      "enth.ORDER ..." (1 each, started from the record enth_in)
//                                      or "error -2 text" (the flat description) / "refused -2 text" (the schedule)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <random>
#include <sstream>
#include <string>
#include <vector>
#include "network_wave.hpp"

using namespace wai;

// 64 emulated lanes: a phase is a loop over them in the order given; between phases nothing runs, so a barrier is nothing
struct HostExec {
  static constexpr int width = NET_WAVE_LANES;
  int order[NET_WAVE_LANES];
  template <class F> void lanes(F&& f) { for (int k = 0; k < width; k++) f(order[k]); }
  template <class F> void one(F&& f) { f(); }
};

static std::map<std::string, std::vector<std::string>> read_records(const char* path) {
  std::map<std::string, std::vector<std::string>> rec;
  std::ifstream in(path);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string name, tok;
    size_t count = 0;
    if (!(ss >> name >> count)) continue;
    std::vector<std::string>& v = rec[name];
    while (ss >> tok) v.push_back(tok);
    if (v.size() != count) { std::fprintf(stderr, "record %s: %zu values, %zu announced\n", name.c_str(), v.size(), count); std::exit(2); }
  }
  return rec;
}
static std::vector<int> ints(const std::map<std::string, std::vector<std::string>>& rec, const char* name) {
  std::vector<int> out;
  auto it = rec.find(name);
  if (it == rec.end()) { std::fprintf(stderr, "record %s is missing\n", name); std::exit(2); }
  for (const std::string& t : it->second) out.push_back((int)std::strtol(t.c_str(), nullptr, 10));
  return out;
}
static std::vector<double> dbls(const std::map<std::string, std::vector<std::string>>& rec, const char* name) {
  std::vector<double> out;
  auto it = rec.find(name);
  if (it == rec.end()) { std::fprintf(stderr, "record %s is missing\n", name); std::exit(2); }
  for (const std::string& t : it->second) out.push_back(std::strtod(t.c_str(), nullptr));   // (hexadecimal: exact)
  return out;
}
static void print(const char* name, const char* order, const double* v, size_t n) {
  std::printf("%s.%s", name, order);
  for (size_t i = 0; i < n; i++) std::printf(" %a", v[i]);
  std::printf("\n");
}
static void print_ints(const char* name, const int* v, size_t n) {
  std::printf("schedule.%s", name);
  for (size_t i = 0; i < n; i++) std::printf(" %d", v[i]);
  std::printf("\n");
}
// arrays that may be empty still hand the builder a valid pointer
template <class T> static const T* data(std::vector<T>& v) { if (v.empty()) v.resize(1); return v.data(); }

int main(int argc, char** argv) {
  if (argc != 2 && argc != 3) { std::fprintf(stderr, "usage: network_wave_host FILE [SEED]\n"); return 2; }
  const auto rec = read_records(argv[1]);
  const unsigned seed = argc == 3 ? (unsigned)std::strtoul(argv[2], nullptr, 10) : 20250u;
  const int n = ints(rec, "n")[0], ng = ints(rec, "n_groups")[0], nr = ints(rec, "n_reinj")[0];
  std::vector<int> rs = ints(rec, "rate_specified"), es = ints(rec, "enthalpy_specified"), gptr = ints(rec, "grp_ptr"),
                   gk = ints(rec, "grp_in_kind"), gi = ints(rec, "grp_in"), gs = ints(rec, "grp_scaling"),
                   glt = ints(rec, "grp_limit_type"), rk = ints(rec, "rj_in_kind"), ri = ints(rec, "rj_in"),
                   rptr = ints(rec, "rj_out_ptr"), of = ints(rec, "out_flow"), ok = ints(rec, "out_kind"),
                   on = ints(rec, "out_node"), vk = ints(rec, "rj_overflow_kind"), vi = ints(rec, "rj_overflow");
  std::vector<double> sep = dbls(rec, "src_sep"), e0 = dbls(rec, "src_enth0"), gl = dbls(rec, "grp_limit"),
                      gsep = dbls(rec, "grp_sep"), orate = dbls(rec, "out_rate"), oprop = dbls(rec, "out_proportion"),
                      oenth = dbls(rec, "out_enthalpy"), raw = dbls(rec, "raw"), enth_in = dbls(rec, "enth_in");
  if ((int)rs.size() != n || (int)es.size() != n || (int)sep.size() != 8 * n || (int)e0.size() != n || (int)raw.size() != 2 * n ||
      (int)enth_in.size() != n || (int)gptr.size() != ng + 1 || (int)rptr.size() != nr + 1) {
    std::fprintf(stderr, "records do not fit n, n_groups, n_reinj\n");
    return 2;
  }
  NetFlatHost F;
  std::string err;
  int e = build_net_flat(F, n, data(rs), data(es), data(sep), data(e0), ng, data(gptr), data(gk), data(gi), data(gs), data(glt),
                         data(gl), data(gsep), nr, data(rk), data(ri), data(rptr), data(of), data(ok), data(on), data(orate),
                         data(oprop), data(oenth), data(vk), data(vi), err);
  if (e) { std::printf("error %d %s\n", e, err.c_str()); return 0; }
  NetWaveHost W;
  e = build_net_wave(F, W, err);
  if (e) { std::printf("refused %d %s\n", e, err.c_str()); return 0; }
  const NetWave& w = W.w;
  // the schedule's arrays on an allocation of exactly their size (W.ww is that already)
  if ((int)W.ww.size() != w.n_ww) { std::fprintf(stderr, "schedule: n_ww\n"); return 2; }
  const int sizes[3] = {w.fan_in, w.stage, net_wave_lds_doubles(F.h, w)};
  print_ints("fan_in", sizes, 1); print_ints("stage", sizes + 1, 1); print_ints("lds", sizes + 2, 1);
  const int* ww = W.ww.data();
  print_ints("ds_ptr", ww + w.ds_ptr, (size_t)ng + 1);
  print_ints("ds", ww + w.ds, (size_t)ww[w.ds_ptr + ng]);
  print_ints("dg_ptr", ww + w.dg_ptr, (size_t)ng + 1);
  print_ints("dg", ww + w.dg, (size_t)ww[w.dg_ptr + ng]);
  print_ints("an_ptr", ww + w.an_ptr, (size_t)ng + 1);
  print_ints("an", ww + w.an, (size_t)ww[w.an_ptr + ng]);
  print_ints("gc_ptr", ww + w.gc_ptr, (size_t)ng + 1);
  print_ints("gc", ww + w.gc, (size_t)ww[w.gc_ptr + ng]);
  print_ints("out_shared", ww + w.out_shared, (size_t)F.h.n_out);
  const char* names[3] = {"ascending", "descending", "shuffled"};
  for (int o = 0; o < 3; o++) {
    HostExec ex;
    for (int k = 0; k < HostExec::width; k++) ex.order[k] = o == 1 ? HostExec::width - 1 - k : k;
    if (o == 2) {
      std::mt19937 gen(seed);
      for (int k = HostExec::width - 1; k > 0; k--) { const int j = (int)(gen() % (unsigned)(k + 1)); std::swap(ex.order[k], ex.order[j]); }
    }
    // the state and the staging run on allocations of exactly the sizes the builders announce: the sanitizer sees a step
    // outside either
    std::vector<double> state((size_t)net_state_doubles(F.h), 0.0), stage((size_t)w.stage, 0.0), net(2 * (size_t)n, -7.0), enth = enth_in;
    NetState s;
    net_state_carve(F.h, state.data(), s);
    s.net = net.data(); s.enth = enth.data();
    network_pass_wave(ex, F.view(), W.view(), raw.data(), s, stage.data());
    print("sources", names[o], s.src, (size_t)NET_NODE * n);
    print("groups", names[o], s.grp, (size_t)NET_NODE * ng);
    std::vector<double> rj8;
    for (int r = 0; r < nr; r++) for (int q = 0; q < 8; q++) rj8.push_back(s.rj[RJ_STATE * r + RJ_OUT_W + q]);
    print("reinjectors", names[o], rj8.data(), rj8.size());
    print("net", names[o], net.data(), net.size());
    print("enth", names[o], enth.data(), enth.size());
  }
  return 0;
}

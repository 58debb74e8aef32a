// Stand-alone host of csrc/ilu_schedule.hpp and csrc/asm_pattern.hpp for tests/test_pc_setup_host.py.  The file named on
// the command line holds "name count values..." records; mode `schedule` reads rowptr, colidx, sub, the scalars N, W, np and
// the members of ScheduleOpts and calls build_host_schedule; mode `asm` reads rowptr, colidx, grp, gci, gslot, sub,
// net_cells and the scalars N, overlap, levels, sublu and calls build_asm_pattern.  Prints "error <code> <text>" or every
// fact and table, one "name values..." line each.  No HIP, no device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include "asm_pattern.hpp"
#include "ilu_schedule.hpp"

using Input = std::map<std::string, std::vector<int>>;

template <class T>
static void print(const char* name, const std::vector<T>& v) {
  std::printf("%s", name);
  for (T x : v) std::printf(" %lld", (long long)x);
  std::printf("\n");
}
static void print(const char* name, long long x) { std::printf("%s %lld\n", name, x); }

static int scalar(const Input& in, const char* name) {
  const auto it = in.find(name);
  if (it == in.end() || it->second.size() != 1) { std::fprintf(stderr, "no scalar %s\n", name); std::exit(2); }
  return it->second[0];
}
static const std::vector<int>& list(const Input& in, const char* name) {
  static const std::vector<int> none;
  const auto it = in.find(name);
  return it == in.end() ? none : it->second;
}

static int schedule(const Input& in) {
  wai::ScheduleOpts o;
  o.ghosts = scalar(in, "ghosts"); o.allow_wide = scalar(in, "allow_wide"); o.sublu = scalar(in, "sublu"); o.fill = scalar(in, "fill");
  o.mesh_W = scalar(in, "mesh_W"); o.box_faces = scalar(in, "box_faces"); o.max_seg = scalar(in, "max_seg");
  o.ilu_general = scalar(in, "ilu_general"); o.pc_rows = scalar(in, "pc_rows"); o.pc_wave = scalar(in, "pc_wave");
  wai::HostSchedule h;
  std::string err;
  const int rc = wai::build_host_schedule(list(in, "rowptr"), list(in, "colidx"), list(in, "sub"), scalar(in, "N"), scalar(in, "W"),
                                          scalar(in, "np"), o, h, err);
  if (rc) { std::printf("error %d %s\n", rc, err.c_str()); return 0; }
  print("nsub", h.nsub); print("max_rows", h.max_rows); print("max_lev", h.max_lev); print("max_nl", h.max_nl);
  print("max_nlu", h.max_nlu); print("max_ublocks", h.max_ublocks); print("max_ublocks_w", h.max_ublocks_w);
  print("n_int", h.n_int); print("n_bnd", h.n_bnd); print("nlev_f", h.nlev_f); print("nlev_b", h.nlev_b);
  print("n_templates", h.n_templates); print("template_rows", h.template_rows);
  print("wide", h.wide); print("big", h.big); print("sublu", h.sublu); print("diag_only", h.diag_only); print("scaled", h.scaled);
  print("park", h.park); print("fast3", h.fast3); print("rows_kernel", h.rows_kernel); print("wave_kernel", h.wave_kernel);
  print("park_serves", wai::park_serves(h, scalar(in, "np")));
  print("lev_f_ptr", h.lev_f_ptr); print("lev_b_ptr", h.lev_b_ptr); print("sub", h.sub);
  print("nlev", h.nlev); print("info", h.info); print("infow", h.infow); print("uoff", h.uoff); print("uoffw", h.uoffw);
  print("tslot", h.tslot); print("split", h.split); print("order", h.order); print("sub_int", h.sub_int); print("sub_bnd", h.sub_bnd);
  print("ord_f", h.ord_f); print("ord_b", h.ord_b); print("c16", h.c16); print("seg", h.seg); print("t_info", h.t_info);
  print("t_uoff", h.t_uoff); print("t_c16", h.t_c16); print("desc", h.desc);
  return 0;
}

static int extended(const Input& in) {
  wai::AsmPattern p;
  std::string err;
  const int rc = wai::build_asm_pattern(list(in, "rowptr"), list(in, "colidx"), scalar(in, "N"), list(in, "grp"), list(in, "gci"),
                                        list(in, "gslot"), list(in, "sub"), scalar(in, "overlap"), scalar(in, "levels"),
                                        scalar(in, "sublu") != 0, list(in, "net_cells"), p, err);
  if (rc) { std::printf("error %d %s\n", rc, err.c_str()); return 0; }
  print("W", p.W);
  print("ext_ptr", p.ext_ptr); print("ext_rows", p.ext_rows); print("erp", p.erp); print("ecol", p.ecol); print("esrc", p.esrc);
  print("ell_col", p.ell_col); print("gmap", p.gmap); print("ext_row", p.ext_row);
  print("net_pos", p.net_pos); print("net_pair", p.net_pair);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3 || (std::strcmp(argv[1], "schedule") && std::strcmp(argv[1], "asm"))) {
    std::fprintf(stderr, "usage: %s schedule|asm input-file\n", argv[0]);
    return 2;
  }
  std::ifstream f(argv[2]);
  Input in;
  std::string name;
  size_t count;
  while (f >> name >> count) {
    std::vector<int>& v = in[name];
    v.resize(count);
    for (int& x : v)
      if (!(f >> x)) { std::fprintf(stderr, "short record %s in %s\n", name.c_str(), argv[2]); return 2; }
  }
  return std::strcmp(argv[1], "asm") ? schedule(in) : extended(in);
}

// Stand-alone host of csrc/tile_schedule.hpp for tests/test_tile_schedule_host.py.  The file named on the command line holds
// "name count values..." records.  Mode `tiles` reads rowptr, colidx, sub, tile_ptr and the scalars N, W, np: check_tiles, then
// the big schedule of build_host_schedule, then build_tile_schedule with every row's own tile.  Mode `asm` reads overlap and
// levels too: the extended pattern of build_asm_pattern (one rank, no network), its schedule, and build_tile_schedule with the
// tile every row of E inherits from the row it stands for.  Prints "error <code> <text>" or every fact and table, one
// "name values..." line each.  No HIP, no device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include "asm_pattern.hpp"
#include "ilu_schedule.hpp"
#include "tile_schedule.hpp"

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

// the schedule of (rowptr, colidx, sub) as build_schedule asks for it, then its tiles
static int tiles_of(const std::vector<int>& rowptr, const std::vector<int>& colidx, const std::vector<int>& sub, int N, int W, int np,
                    int mesh_W, bool allow_wide, const std::vector<int>& row_tile) {
  wai::ScheduleOpts o;
  o.mesh_W = mesh_W; o.allow_wide = allow_wide;
  wai::HostSchedule h;
  std::string err;
  if (const int rc = wai::build_host_schedule(rowptr, colidx, sub, N, W, np, o, h, err)) { std::printf("error %d %s\n", rc, err.c_str()); return 0; }
  print("big", h.big); print("nlev_f", h.nlev_f); print("nlev_b", h.nlev_b); print("info", h.info);
  if (!h.big || h.sublu) return 0;
  wai::HostTiles t;
  if (const int rc = wai::build_tile_schedule(rowptr, colidx, sub, h.info, row_tile, N, h.nlev_f, h.nlev_b, t, err)) {
    std::printf("error %d %s\n", rc, err.c_str());
    return 0;
  }
  print("n_tiles", t.n_tiles); print("ntl_f", t.ntl_f); print("ntl_b", t.ntl_b); print("max_tile_rows", t.max_tile_rows);
  print("max_in_levels", t.max_in_levels); print("serve", t.serve);
  print("tl_f_ptr", t.tl_f_ptr); print("tl_b_ptr", t.tl_b_ptr); print("tile_ptr", t.tile_ptr); print("tile_lev", t.tile_lev);
  print("tile_nin", t.tile_nin); print("ord_f", t.ord_f); print("ord_b", t.ord_b); print("row_lev", t.row_lev);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3 || (std::strcmp(argv[1], "tiles") && std::strcmp(argv[1], "asm"))) {
    std::fprintf(stderr, "usage: %s tiles|asm input-file\n", argv[0]);
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
  const int N = scalar(in, "N"), W = scalar(in, "W"), np = scalar(in, "np");
  const std::vector<int>&rowptr = list(in, "rowptr"), &colidx = list(in, "colidx"), &sub = list(in, "sub"), &tile_ptr = list(in, "tile_ptr");
  std::string err;
  if (const int rc = wai::check_tiles(tile_ptr, sub, N, err)) { std::printf("error %d %s\n", rc, err.c_str()); return 0; }
  const std::vector<int> id = wai::tile_of_rows(tile_ptr, N);
  if (!std::strcmp(argv[1], "tiles")) return tiles_of(rowptr, colidx, sub, N, W, np, W, true, id);
  wai::AsmPattern p;
  const std::vector<int> none;
  if (const int rc = wai::build_asm_pattern(rowptr, colidx, N, none, none, none, sub, scalar(in, "overlap"), scalar(in, "levels"), false, none, p, err)) {
    std::printf("error %d %s\n", rc, err.c_str());
    return 0;
  }
  const int n_ext = (int)p.ext_rows.size();
  std::vector<int> etile(n_ext);
  for (int q = 0; q < n_ext; q++) etile[q] = id[p.ext_rows[q]];
  print("ext_ptr", p.ext_ptr); print("ext_rows", p.ext_rows); print("erp", p.erp); print("ecol", p.ecol); print("etile", etile);
  return tiles_of(p.erp, p.ecol, p.ext_ptr, n_ext, p.W, np, W, scalar(in, "levels") == 0, etile);   // (allow_wide as build_asm asks, unfused)
}

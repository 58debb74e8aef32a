// Stand-alone host of csrc/coarse_space.hpp for tests/test_coarse_space_host.py.  The file named on the command line holds
// "name count values..." records: rowptr, colidx, agg and the scalars N, nc, bs.  Calls build_coarse_space and prints
// "error <code> <text>" or every fact and table, one "name values..." line each.  No HIP, no device.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include "coarse_space.hpp"

using Input = std::map<std::string, std::vector<int>>;

static void print(const char* name, const std::vector<int>& v) {
  std::printf("%s", name);
  for (int x : v) std::printf(" %d", x);
  std::printf("\n");
}
static void print(const char* name, long long x) { std::printf("%s %lld\n", name, x); }

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s input-file\n", argv[0]);
    return 2;
  }
  std::ifstream f(argv[1]);
  Input in;
  std::string name;
  size_t count;
  while (f >> name >> count) {
    std::vector<int>& v = in[name];
    v.resize(count);
    for (int& x : v)
      if (!(f >> x)) { std::fprintf(stderr, "short record %s in %s\n", name.c_str(), argv[1]); return 2; }
  }
  for (const char* s : {"N", "nc", "bs"})
    if (in[s].size() != 1) { std::fprintf(stderr, "no scalar %s\n", s); return 2; }
  wai::CoarseSpace h;
  std::string err;
  const int rc = wai::build_coarse_space(in["rowptr"], in["colidx"], in["N"][0], in["agg"], in["nc"][0], in["bs"][0], h, err);
  if (rc) { std::printf("error %d %s\n", rc, err.c_str()); return 0; }
  print("n", h.n); print("nc", h.nc); print("bs", h.bs); print("max_rows", h.max_rows);
  print("agg_ptr", h.agg_ptr); print("agg_rows", h.agg_rows); print("c_rowptr", h.c_rowptr); print("c_colidx", h.c_colidx);
  print("ent_ptr", h.ent_ptr); print("ent_row", h.ent_row); print("ent_slot", h.ent_slot);
  return 0;
}

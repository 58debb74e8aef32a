// Stand-alone host of csrc/colour_order.hpp for tests/test_colour_order_host.py.  The file named on the command line holds
// "name count values..." records: rowptr, colidx, sub and the scalar N.  Calls build_colour_order and prints
// "error <code> <text>" or every fact and table, one "name values..." line each.  No HIP, no device.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include "colour_order.hpp"

using Input = std::map<std::string, std::vector<int>>;

template <class T>
static void print(const char* name, const std::vector<T>& v) {
  std::printf("%s", name);
  for (T x : v) std::printf(" %llu", (unsigned long long)x);
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
  if (in["N"].size() != 1) { std::fprintf(stderr, "no scalar N\n"); return 2; }
  wai::HostColourOrder h;
  std::string err;
  const int rc = wai::build_colour_order(in["rowptr"], in["colidx"], in["sub"], in["N"][0], h, err);
  if (rc) { std::printf("error %d %s\n", rc, err.c_str()); return 0; }
  print("nsub", h.nsub); print("max_rows", h.max_rows); print("max_colours", h.max_colours); print("diag_only", h.diag_only);
  print("max_blocks", h.max_blocks);
  print("sub", h.sub); print("col_ptr", h.col_ptr); print("colour", h.colour); print("ncolours", h.ncolours); print("rows", h.rows);
  print("slots", h.slots); print("counts", h.counts);
  return 0;
}

// Stand-alone host of csrc/cell_order.hpp for tests/test_cell_order_host.py.  The file named on the command line holds
// "name count values..." records: faces (2 ints per face), cen (3 doubles per cell, written with 17 digits) and the scalars
// n and S.  Calls build_cell_order and prints "error <code> <text>" or n_sub, perm, sub_ptr and h, one "name values..."
// line each.  No HIP, no device.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include "cell_order.hpp"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s input-file\n", argv[0]);
    return 2;
  }
  std::ifstream f(argv[1]);
  std::map<std::string, std::vector<double>> in;
  std::string name;
  size_t count;
  while (f >> name >> count) {
    std::vector<double>& v = in[name];
    v.resize(count);
    for (double& x : v) {
      std::string tok;   // (strtod: "nan" and "inf" are values here)
      if (!(f >> tok)) { std::fprintf(stderr, "short record %s in %s\n", name.c_str(), argv[1]); return 2; }
      x = std::strtod(tok.c_str(), nullptr);
    }
  }
  if (in["n"].size() != 1 || in["S"].size() != 1) { std::fprintf(stderr, "no scalars n, S\n"); return 2; }
  const int n = (int)in["n"][0], S = (int)in["S"][0];
  std::vector<int> faces(in["faces"].begin(), in["faces"].end());
  const std::vector<double>& cen = in["cen"];
  if (cen.size() != (size_t)3 * n || faces.size() % 2) { std::fprintf(stderr, "cen has not 3 n values, or an odd face record\n"); return 2; }
  wai::CellOrder o;
  std::string err;
  const int rc = wai::build_cell_order(n, (int)faces.size() / 2, faces.data(), cen.data(), 3, S, o, err);
  if (rc) { std::printf("error %d %s\n", rc, err.c_str()); return 0; }
  std::printf("n_sub %d\n", o.n_sub);
  std::printf("perm");
  for (int x : o.perm) std::printf(" %d", x);
  std::printf("\nsub_ptr");
  for (int x : o.sub_ptr) std::printf(" %d", x);
  std::printf("\nh %.17g %.17g %.17g\n", o.h[0], o.h[1], o.h[2]);
  return 0;
}

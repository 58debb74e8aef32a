// Stand-alone host of csrc/ilu_schedule.hpp's packing phase for tests/test_park_groups_host.py.  The file named on the command
// line holds "name count values..." records: rowptr, colidx, sub, the scalars N, W, np, ghosts and box_faces.  Calls
// build_host_schedule and prints what the packing phase read and made, one "name values..." line each.  No HIP, no device.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include "ilu_schedule.hpp"

using Input = std::map<std::string, std::vector<int>>;

static void print(const char* name, const std::vector<int>& v) {
  std::printf("%s", name);
  for (int x : v) std::printf(" %d", x);
  std::printf("\n");
}
static int scalar(const Input& in, const char* name) {
  const auto it = in.find(name);
  if (it == in.end() || it->second.size() != 1) { std::fprintf(stderr, "no scalar %s\n", name); std::exit(2); }
  return it->second[0];
}
static const std::vector<int>& list(const Input& in, const char* name) {
  const auto it = in.find(name);
  if (it == in.end()) { std::fprintf(stderr, "no list %s\n", name); std::exit(2); }
  return it->second;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s input-file\n", argv[0]); return 2; }
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
  wai::ScheduleOpts o;
  o.ghosts = scalar(in, "ghosts"); o.box_faces = scalar(in, "box_faces"); o.mesh_W = scalar(in, "W");
  wai::HostSchedule h;
  std::string err;
  const int rc = wai::build_host_schedule(list(in, "rowptr"), list(in, "colidx"), list(in, "sub"), scalar(in, "N"), scalar(in, "W"),
                                          scalar(in, "np"), o, h, err);
  if (rc) { std::fprintf(stderr, "error %d %s\n", rc, err.c_str()); return 1; }
  print("facts", {h.nsub, h.max_rows, h.max_ublocks, (int)wai::park_serves(h, scalar(in, "np"))});
  print("n_groups", {h.n_groups[0], h.n_groups[1], h.n_groups[2]});
  print("n_shared", {h.n_shared[0], h.n_shared[1], h.n_shared[2]});
  print("sub", h.sub); print("nlev", h.nlev); print("ucount", h.ucount); print("uoff", h.uoff); print("info", h.info);
  print("order", h.order); print("sub_int", h.sub_int); print("sub_bnd", h.sub_bnd);
  print("groups0", h.groups[0]); print("groups1", h.groups[1]); print("groups2", h.groups[2]);
  return 0;
}

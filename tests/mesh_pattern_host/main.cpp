// Stand-alone host of csrc/mesh_pattern.hpp for tests/test_mesh_pattern_host.py: reads "n_owned n_halo n_bc n_faces" and
// the face list (two cell indices per face) from the file named on the command line, calls build_mesh_pattern and prints
// either "error <text>" or every member of MeshPattern, one "name values..." line each.  No HIP, no device.
#include <cstdio>
#include <fstream>
#include "mesh_pattern.hpp"

static void print(const char* name, const std::vector<int>& v) {
  std::printf("%s", name);
  for (int x : v) std::printf(" %d", x);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s mesh-file\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  int n_owned = 0, n_halo = 0, n_bc = 0, n_faces = 0;
  if (!(in >> n_owned >> n_halo >> n_bc >> n_faces) || n_owned <= 0 || n_halo < 0 || n_bc < 0 || n_faces < 0) {
    std::fprintf(stderr, "bad header in %s\n", argv[1]);
    return 2;
  }
  std::vector<int> face_cells((size_t)2 * n_faces);
  for (int& v : face_cells)
    if (!(in >> v)) { std::fprintf(stderr, "short face list in %s\n", argv[1]); return 2; }
  wai::MeshPattern p;
  std::string err;
  const int rc = wai::build_mesh_pattern(n_owned, n_owned + n_halo, n_owned + n_halo + n_bc, n_faces, face_cells.data(), p, err);
  if (rc) {
    std::printf("error %d %s\n", rc, err.c_str());
    return 0;
  }
  std::printf("max_deg %d\nW %d\nnnzb %d\n", p.max_deg, p.W, p.nnzb);
  print("adj_face", p.adj_face); print("adj_other", p.adj_other); print("adj_blk", p.adj_blk); print("adj_tblk", p.adj_tblk);
  print("diag", p.diag); print("rowptr", p.rowptr); print("colidx", p.colidx); print("ell_col", p.ell_col);
  return 0;
}

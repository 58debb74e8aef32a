// The mesh's connectivity as the library keeps it: the cell -> face adjacency of the owned cells and the BCSR / block-ELL
// pattern of the Jacobian on it.  Pure host code -- no HIP header, no device -- so that a plain C++ program can call it
// (tests/mesh_pattern_host); wai_ctx_create (context.hip) uploads what it builds.  Not part of the ABI.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

namespace wai {

// most faces of an owned cell (boundary faces included) and most blocks of a matrix row -- the cell itself and at most 15
// neighbouring cells (include/waiwera_hip.h)
constexpr int MAX_CELL_FACES = 16;

struct MeshPattern {
  int max_deg = 0, W = 0, nnzb = 0;
  // ELL cell->face adjacency of owned cells, slot-major: [slot * n_owned + cell] (DeviceMesh, context.hpp)
  std::vector<int> adj_face, adj_other, adj_blk, adj_tblk;
  std::vector<int> diag, rowptr, colidx;   // matrix slot of (cell, cell); BCSR rows of the owned cells, columns ascending
  std::vector<int> ell_col;                // block-ELL column planes [W][n_owned], padding = the row's own index
};

// Cells 0 .. n_owned - 1 are owned (the matrix rows), .. n_prim - 1 ghosts (columns only), .. n_local - 1 boundary cells
// (no column); face f joins face_cells[2 f] and face_cells[2 f + 1].  n_owned > 0.  Returns 0, or -2 with `err` set.
inline int build_mesh_pattern(int n_owned, int n_prim, int n_local, int n_faces, const int* face_cells,
                              MeshPattern& out, std::string& err) {
  const int N = n_owned, NL = n_local, NF = n_faces;
  // cell -> face adjacency (ascending face index per cell) and BCSR pattern
  std::vector<int> deg(N, 0);
  for (int f = 0; f < NF; f++)
    for (int s = 0; s < 2; s++) {
      const int cc = face_cells[2 * f + s];
      if (cc < 0 || cc >= NL) { err = "face cell index out of range"; return -2; }
      if (cc < N) deg[cc]++;
    }
  out.max_deg = *std::max_element(deg.begin(), deg.end());
  if (out.max_deg > MAX_CELL_FACES) {   // (documented beside wai_mesh_desc, include/waiwera_hip.h)
    const int cell = (int)(std::max_element(deg.begin(), deg.end()) - deg.begin());
    err = "cell " + std::to_string(cell) + " has " + std::to_string(out.max_deg) + " faces: at most " +
          std::to_string(MAX_CELL_FACES) + " supported";
    return -2;
  }
  std::vector<int> &adj_face = out.adj_face, &adj_other = out.adj_other, &adj_blk = out.adj_blk;
  adj_face.assign((size_t)out.max_deg * N, -1);
  adj_other.assign((size_t)out.max_deg * N, 0);
  adj_blk.assign((size_t)out.max_deg * N, -1);
  std::vector<int> fill(N, 0);
  for (int f = 0; f < NF; f++)
    for (int s = 0; s < 2; s++) {
      const int cc = face_cells[2 * f + s];
      if (cc >= N) continue;
      const int slot = fill[cc]++;
      adj_face[(size_t)slot * N + cc] = f * 2 + s;
      adj_other[(size_t)slot * N + cc] = face_cells[2 * f + 1 - s];
    }
  out.W = 0;
  out.rowptr.assign(N + 1, 0);
  for (int i = 0; i < N; i++) {
    int cnt = 1;
    for (int s = 0; s < deg[i]; s++)
      if (adj_other[(size_t)s * N + i] < n_prim) cnt++;
    out.rowptr[i + 1] = out.rowptr[i] + cnt;
    if (cnt > MAX_CELL_FACES) {   // 16 faces and none of them a boundary face: 15 neighbouring cells at most
      err = "cell " + std::to_string(i) + " has " + std::to_string(cnt - 1) + " neighbouring cells (a matrix row of " +
            std::to_string(cnt) + " blocks): at most 15 supported";
      return -2;
    }
    out.W = std::max(out.W, cnt);
  }
  out.nnzb = out.rowptr[N];
  out.colidx.resize(out.nnzb);
  out.diag.resize(N);
  out.ell_col.resize((size_t)out.W * N);
  for (int i = 0; i < N; i++) {
    int* row = out.colidx.data() + out.rowptr[i];
    int cnt = 0;
    row[cnt++] = i;
    for (int s = 0; s < deg[i]; s++) {
      const int o = adj_other[(size_t)s * N + i];
      if (o < n_prim) row[cnt++] = o;
    }
    std::sort(row, row + cnt);
    for (int q = 0; q < cnt; q++) {
      if (row[q] == i) out.diag[i] = q;
      if (q > 0 && row[q] == row[q - 1]) { err = "duplicate connection between two cells"; return -2; }
      out.ell_col[(size_t)q * N + i] = row[q];
    }
    for (int q = cnt; q < out.W; q++) out.ell_col[(size_t)q * N + i] = i;  // padding: zero block on the diagonal column
    for (int s = 0; s < deg[i]; s++) {
      const int o = adj_other[(size_t)s * N + i];
      if (o >= n_prim) continue;
      const int* p = std::lower_bound(row, row + cnt, o);
      adj_blk[(size_t)s * N + i] = (int)(p - row);
    }
  }
  // the transposed slot: where column i sits in the block row of its neighbour o (an owned row), for the column-wise
  // Jacobian sweep (k_jacobian_sym)
  out.adj_tblk.assign((size_t)out.max_deg * N, -1);
  for (int i = 0; i < N; i++)
    for (int s = 0; s < deg[i]; s++) {
      const int o = adj_other[(size_t)s * N + i];
      if (o >= N) continue;
      const int* row = out.colidx.data() + out.rowptr[o];
      const int cnt = out.rowptr[o + 1] - out.rowptr[o];
      const int* p = std::lower_bound(row, row + cnt, i);
      if (p < row + cnt && *p == i) out.adj_tblk[(size_t)s * N + i] = (int)(p - row);
    }
  return 0;
}

}  // namespace wai

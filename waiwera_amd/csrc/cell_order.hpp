// The compact cell order (wai_cell_order): cuts a mesh given by its cell centroids and interior faces into compact
// subdomains of at most S cells by recursive coordinate bisection and numbers the cells inside each like a brick, x fastest.
// The preconditioner's fast paths assume such subdomains; chunks of consecutive cells of a mesh file are slabs of one layer
// (or, for a numbering without locality, scattered cells), which cut the strong vertical couplings of thin layers.  Pure
// host code -- no device header, no context, no environment -- so that a plain C++ program can call it
// (tests/cell_order_host); capi.hip hands it to the ABI.
//
// Axis spacings: a face's axis a is the one with the largest |c[i][a] - c[j][a]| (ties: the lowest a); h[a] is the mean of
// that difference over the faces of axis a, summed in face order.  An axis without a face of its own counts as extent 0;
// with no faces at all h = 1 on every axis.
// Bisection of a set of k cells, from all cells: L = ceil(k / S); L <= 1 is a leaf.  Otherwise the axis a with the largest
// (max c[.][a] - min c[.][a]) / h[a] (ties: the lowest a); the set sorted by c[.][a], then by the remaining axes in the
// order z, y, x, then by input index; the first floor(k * (L / 2) / L) cells (integer L / 2) go left, the rest right.  So no
// leaf exceeds S and there are at most ceil(n / S) leaves.
// Numbering: the leaves depth-first, left before right; inside a leaf the cells by (z, y, x, input index) ascending.
// Doubles are compared as given.  Every sort key ends in the input index, so every order is total: the three global orders
// (one per axis) are made once, and a set is sorted by its cells' ranks in one of them -- O(n log n) per level of the tree,
// no recursion (the sets are ranges of one array, taken from a stack).
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <utility>
#include <vector>

namespace wai {

struct CellOrder {
  int n_sub = 0;
  std::vector<int> perm;      // perm[new] = old
  std::vector<int> sub_ptr;   // [n_sub + 1] the leaves as ranges of the new numbering
  double h[3] = {1.0, 1.0, 1.0};   // the axis spacings
  bool has_faces[3] = {false, false, false};
};

// centroids: cen[i * stride + a], a = 0..2, stride >= 3.  face_cells: m pairs.  Returns 0, or -2 with `err` set; `out` is
// built from nothing either way.
inline int build_cell_order(int n, int m, const int* face_cells, const double* cen, int stride, int S, CellOrder& out,
                            std::string& err) {
  out = CellOrder();
  if (S < 1) { err = "cell order: the subdomain cap must be at least 1"; return -2; }
  if (n < 0 || m < 0 || stride < 3) { err = "cell order: negative cell or face count, or a centroid stride below 3"; return -2; }
  if ((n && !cen) || (m && !face_cells)) { err = "cell order: null centroids or faces"; return -2; }
  auto c = [&](int i, int a) { return cen[(size_t)i * stride + a]; };
  for (int i = 0; i < n; i++)
    for (int a = 0; a < 3; a++)
      if (!std::isfinite(c(i, a))) { err = "cell order: a centroid is not finite"; return -2; }
  // axis spacings
  double sum[3] = {0.0, 0.0, 0.0};
  long long cnt[3] = {0, 0, 0};
  for (int f = 0; f < m; f++) {
    const int i = face_cells[2 * f], j = face_cells[2 * f + 1];
    if (i < 0 || i >= n || j < 0 || j >= n) { err = "cell order: a face names a cell outside [0, n)"; return -2; }
    int a = 0;
    double d = std::fabs(c(i, 0) - c(j, 0));
    for (int b = 1; b < 3; b++) {
      const double e = std::fabs(c(i, b) - c(j, b));
      if (e > d) { d = e; a = b; }
    }
    sum[a] += d;
    cnt[a]++;
  }
  for (int a = 0; a < 3; a++) {
    out.has_faces[a] = cnt[a] > 0;
    if (m) out.h[a] = cnt[a] ? sum[a] / (double)cnt[a] : 1.0;
  }
  const bool no_faces = m == 0;
  // the three global orders: by c[.][a], then the remaining axes in the order z, y, x, then the input index
  std::vector<int> order[3], rank[3];
  for (int a = 0; a < 3; a++) {
    int rest[2], r = 0;
    for (int b = 2; b >= 0; b--)
      if (b != a) rest[r++] = b;
    struct Key { double k0, k1, k2; int id; };   // sorted by value: the keys lie side by side, whatever the numbering
    std::vector<Key> keys(n);
    for (int i = 0; i < n; i++) keys[i] = {c(i, a), c(i, rest[0]), c(i, rest[1]), i};
    std::sort(keys.begin(), keys.end(), [](const Key& p, const Key& q) {
      if (p.k0 != q.k0) return p.k0 < q.k0;
      if (p.k1 != q.k1) return p.k1 < q.k1;
      if (p.k2 != q.k2) return p.k2 < q.k2;
      return p.id < q.id;
    });
    std::vector<int>& o = order[a];
    o.resize(n);
    rank[a].resize(n);
    for (int k = 0; k < n; k++) { o[k] = keys[k].id; rank[a][o[k]] = k; }
  }
  std::vector<int>& set = out.perm;
  set.resize(n);
  for (int i = 0; i < n; i++) set[i] = i;
  std::vector<int> key;
  auto sort_range = [&](int lo, int hi, int a) {   // set[lo, hi) by the cells' ranks in order a
    key.resize(hi - lo);
    for (int k = lo; k < hi; k++) key[k - lo] = rank[a][set[k]];
    std::sort(key.begin(), key.end());
    for (int k = lo; k < hi; k++) set[k] = order[a][key[k - lo]];
  };
  out.sub_ptr.push_back(0);
  std::vector<std::pair<int, int>> stack;
  if (n) stack.push_back({0, n});
  while (!stack.empty()) {
    const int lo = stack.back().first, hi = stack.back().second;
    stack.pop_back();
    const long long k = hi - lo, L = (k + S - 1) / S;
    if (L <= 1) {   // a leaf: ranges come off the stack left before right, so the leaves are made in their final order
      sort_range(lo, hi, 2);
      out.sub_ptr.push_back(hi);
      continue;
    }
    double mn[3], mx[3];
    for (int a = 0; a < 3; a++) mn[a] = mx[a] = c(set[lo], a);
    for (int q = lo + 1; q < hi; q++)
      for (int a = 0; a < 3; a++) {
        const double v = c(set[q], a);
        if (v < mn[a]) mn[a] = v;
        if (v > mx[a]) mx[a] = v;
      }
    int best = 0;
    double ebest = 0.0;
    for (int a = 0; a < 3; a++) {
      const double e = no_faces || out.has_faces[a] ? (mx[a] - mn[a]) / out.h[a] : 0.0;
      if (a == 0 || e > ebest) { ebest = e; best = a; }
    }
    sort_range(lo, hi, best);
    const int left = (int)(k * (L / 2) / L);
    stack.push_back({lo + left, hi});
    stack.push_back({lo, lo + left});
  }
  out.n_sub = (int)out.sub_ptr.size() - 1;
  return 0;
}

}  // namespace wai

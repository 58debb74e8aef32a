// The symbolic phase of the two-level preconditioner's coarse space (wai_set_pc_coarse) on a block matrix given as host CSR
// (ascending columns): one coarse level, piecewise constant over aggregates of cells.  agg[i] in [0, nc) names the aggregate of
// block row i; the prolongation P has P[(i,k),(I,k)] = 1 where agg[i] = I, so the Galerkin matrix Ac = P^T A P has block
// (I, J) = the sum of the blocks A_ij over i in I, j in J, and the restriction sums a residual's blocks over each aggregate.
// What the device needs of that is made here: every aggregate's rows in ascending order, the coarse pattern, and for every
// coarse block the ordered list of the fine (row, slot) blocks that go into it -- the order in which k_coarse_galerkin takes
// them.  Pure host code -- no device header, no context, no environment -- so that a plain C++ program can call it
// (tests/coarse_space_host); pc_setup.hip uploads what build_coarse_space makes.  Not part of the ABI.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

namespace wai {

constexpr int COARSE_MAX_UNKNOWNS = 1024;   // most coarse unknowns nc * bs: the coarse matrix is inverted densely (<= 8 MB)

struct CoarseSpace {
  int n = 0, nc = 0, bs = 0;
  int max_rows = 0;                 // rows of the largest aggregate
  std::vector<int> agg;             // [n] as given
  std::vector<int> agg_ptr;         // [nc + 1] ranges of agg_rows
  std::vector<int> agg_rows;        // every aggregate's rows, ascending
  std::vector<int> c_rowptr;        // [nc + 1] the coarse pattern: CSR over the aggregates, ...
  std::vector<int> c_colidx;        // ... ascending columns
  std::vector<int> ent_ptr;         // [coarse blocks + 1] ranges of the contribution lists
  std::vector<int> ent_row;         // fine block row of a contribution, ...
  std::vector<int> ent_slot;        // ... and its slot in that row (BCSR block rowptr[row] + slot)
};

// The coarse space of the N x N block matrix (rowptr, colidx) under agg[0 .. N).  Columns >= N (partition ghosts) belong to
// no aggregate and contribute nothing.  A coarse block's contributions are ordered by (fine row, slot), both ascending.
// Returns 0, or -2 with `err` set; `out` is built from nothing either way.
inline int build_coarse_space(const std::vector<int>& rowptr, const std::vector<int>& colidx, int N, const std::vector<int>& agg,
                              int nc, int bs, CoarseSpace& out, std::string& err) {
  out = CoarseSpace();
  if (N < 1 || (int)rowptr.size() != N + 1) { err = "coarse space: the pattern has not n_owned rows"; return -2; }
  if ((int)agg.size() != N) { err = "coarse space: agg must name an aggregate for each of the n_owned cells"; return -2; }
  if (nc < 1) { err = "coarse space: nc < 1"; return -2; }
  if (bs < 1) { err = "coarse space: block size < 1"; return -2; }
  if ((long long)nc * bs > COARSE_MAX_UNKNOWNS) {
    err = "coarse space: nc * bs = " + std::to_string((long long)nc * bs) + " coarse unknowns, more than " +
          std::to_string(COARSE_MAX_UNKNOWNS);
    return -2;
  }
  std::vector<int> count(nc, 0);
  for (int i = 0; i < N; i++) {
    if (agg[i] < 0 || agg[i] >= nc) {
      err = "coarse space: agg[" + std::to_string(i) + "] = " + std::to_string(agg[i]) + " is outside [0, nc = " + std::to_string(nc) + ")";
      return -2;
    }
    count[agg[i]]++;
  }
  for (int I = 0; I < nc; I++)
    if (count[I] == 0) { err = "coarse space: aggregate " + std::to_string(I) + " is empty"; return -2; }
  out.n = N; out.nc = nc; out.bs = bs;
  out.agg = agg;
  out.agg_ptr.assign(nc + 1, 0);
  for (int I = 0; I < nc; I++) {
    out.agg_ptr[I + 1] = out.agg_ptr[I] + count[I];
    out.max_rows = std::max(out.max_rows, count[I]);
  }
  out.agg_rows.resize(N);
  {
    std::vector<int> fill(out.agg_ptr.begin(), out.agg_ptr.end() - 1);
    for (int i = 0; i < N; i++) out.agg_rows[fill[agg[i]]++] = i;   // ascending i: every aggregate's rows ascend
  }
  // the coarse pattern and the lists, one coarse row at a time: the row's fine blocks bucketed by the column's aggregate
  out.c_rowptr.assign(1, 0);
  out.ent_ptr.assign(1, 0);
  std::vector<int> n_in(nc, 0), first(nc, 0), cols;
  for (int I = 0; I < nc; I++) {
    cols.clear();
    for (int p = out.agg_ptr[I]; p < out.agg_ptr[I + 1]; p++) {
      const int i = out.agg_rows[p];
      for (int q = rowptr[i]; q < rowptr[i + 1]; q++) {
        const int j = colidx[q];
        if (j < 0 || j >= N) continue;
        if (n_in[agg[j]]++ == 0) cols.push_back(agg[j]);
      }
    }
    std::sort(cols.begin(), cols.end());
    int at = out.ent_ptr.back();
    for (int J : cols) {
      first[J] = at;
      at += n_in[J];
      out.c_colidx.push_back(J);
      out.ent_ptr.push_back(at);
    }
    out.c_rowptr.push_back((int)out.c_colidx.size());
    out.ent_row.resize(at);
    out.ent_slot.resize(at);
    for (int p = out.agg_ptr[I]; p < out.agg_ptr[I + 1]; p++) {
      const int i = out.agg_rows[p];
      for (int q = rowptr[i]; q < rowptr[i + 1]; q++) {
        const int j = colidx[q];
        if (j < 0 || j >= N) continue;
        const int at_j = first[agg[j]]++;
        out.ent_row[at_j] = i;
        out.ent_slot[at_j] = q - rowptr[i];
      }
    }
    for (int J : cols) n_in[J] = 0;
  }
  return 0;
}

}  // namespace wai

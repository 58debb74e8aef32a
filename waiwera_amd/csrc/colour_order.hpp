// The symbolic phase of block-Jacobi ILU(0) in MULTICOLOUR order (wai_set_pc_ordering) on a block matrix given as host CSR
// (ascending columns, structurally symmetric): every subdomain's rows are eliminated sorted by (colour, row index), where
// rows of one colour are not coupled to each other inside the subdomain -- so both substitutions have as many levels as
// the subdomain has colours (2 on hexahedral and MINC meshes) instead of a dependency chain as long as the subdomain.
// Nothing is renumbered: the factor lives on the matrix' own column planes, and a row's descriptor names its in-subdomain
// slots in elimination order.  Pure host code -- no device header, no context, no environment -- so that a plain C++ program
// can call it (tests/colour_order_host); pc_setup.hip uploads what build_colour_order makes.  Not part of the ABI.
//
// Colouring (greedy, per subdomain): rows in ascending index; a row gets the smallest colour >= 0 none of its already
// coloured in-subdomain neighbours has.  Neighbours: the off-diagonal columns of the row that lie in its subdomain.  A row
// of at most 16 blocks has at most 15 such neighbours, hence at most 16 colours.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

namespace wai {

constexpr int COLOUR_MAX_BLOCKS = 16;   // most blocks of a row: slot numbers are 4 bits

// What a colour order says besides its tables: ColourSchedule (context.hpp) is these facts plus the tables on the device.
struct ColourFacts {
  int nsub = 0, max_rows = 0;
  int max_colours = 0;        // most colours of any subdomain: the launches of a sweep
  bool diag_only = false;     // ILU(0) in this order never updates an off-diagonal block: the cell graph has no triangle inside a subdomain
  int max_blocks = 0;         // most blocks of any row
  std::vector<int> sub;       // host copy of sub_ptr
  std::vector<int> col_ptr;   // [max_colours + 1] row ranges of each colour in `rows`
};

// The facts and every table as the device gets it.
struct HostColourOrder : ColourFacts {
  std::vector<int> colour;    // per row
  std::vector<int> ncolours;  // per subdomain
  std::vector<int> rows;      // the launch lists: all rows sorted by (colour, row index)
  // per row: its in-subdomain off-diagonal slots in elimination order, 4 bits each from bit 0 -- first the lower ones (rows
  // eliminated before this one: smaller colour), then the upper ones, each group by ascending (colour, row index) of the column
  std::vector<unsigned long long> slots;
  std::vector<int> counts;    // per row: lower | upper << 8 | diagonal slot << 16 | colour << 24
};

// (constexpr: the kernels decode a descriptor with the same functions)
constexpr int colour_nlower(int counts) { return counts & 0xff; }
constexpr int colour_nupper(int counts) { return (counts >> 8) & 0xff; }
constexpr int colour_dslot(int counts) { return (counts >> 16) & 0xff; }
constexpr int colour_of(int counts) { return (counts >> 24) & 0xff; }
constexpr int colour_slot(unsigned long long slots, int p) { return (int)((slots >> (4 * p)) & 15); }

// The colour order of the N x N block matrix (rowptr, colidx) under the subdomains sub[0] = 0 <= .. <= sub[nsub] = N.
// Columns >= N (partition ghosts) and columns of other subdomains are not part of a subdomain's block.  Returns 0, or -2 with
// `err` set; `out` is built from nothing either way.
inline int build_colour_order(const std::vector<int>& rowptr, const std::vector<int>& colidx, const std::vector<int>& sub, int N,
                              HostColourOrder& out, std::string& err) {
  out = HostColourOrder();
  if (sub.empty() || sub.front() != 0 || sub.back() != N) { err = "multicolour ordering: sub_ptr must cover [0, n_owned]"; return -2; }
  if (!std::is_sorted(sub.begin(), sub.end())) { err = "multicolour ordering: sub_ptr not monotone"; return -2; }
  if ((int)rowptr.size() != N + 1) { err = "multicolour ordering: the pattern has not n_owned rows"; return -2; }
  out.sub = sub;
  out.nsub = (int)sub.size() - 1;
  out.colour.assign(N, -1);
  out.ncolours.assign(out.nsub, 0);
  out.slots.assign(N, 0);
  out.counts.assign(N, 0);
  out.diag_only = true;
  std::vector<int> diag(N, -1);
  for (int sd = 0; sd < out.nsub; sd++) {
    const int lo = sub[sd], hi = sub[sd + 1];
    out.max_rows = std::max(out.max_rows, hi - lo);
    // colours
    for (int i = lo; i < hi; i++) {
      const int cnt = rowptr[i + 1] - rowptr[i];
      if (cnt > COLOUR_MAX_BLOCKS) { err = "multicolour ordering: a row has more than 16 blocks"; return -2; }
      out.max_blocks = std::max(out.max_blocks, cnt);
      unsigned used = 0;
      for (int q = rowptr[i]; q < rowptr[i + 1]; q++) {
        const int j = colidx[q];
        if (j == i) diag[i] = q - rowptr[i];
        else if (j >= lo && j < i) used |= 1u << out.colour[j];
      }
      if (diag[i] < 0) { err = "multicolour ordering: a row has no diagonal block"; return -2; }
      int c = 0;
      while (used & (1u << c)) c++;
      out.colour[i] = c;
      out.ncolours[sd] = std::max(out.ncolours[sd], c + 1);
    }
    out.max_colours = std::max(out.max_colours, out.ncolours[sd]);
    // descriptors: the in-subdomain slots by (colour, row index) of their columns
    for (int i = lo; i < hi; i++) {
      const int* row = colidx.data() + rowptr[i];
      const int cnt = rowptr[i + 1] - rowptr[i];
      int order[COLOUR_MAX_BLOCKS], m = 0;
      for (int q = 0; q < cnt; q++)
        if (row[q] != i && row[q] >= lo && row[q] < hi) order[m++] = q;
      auto key = [&](int q) { return (long long)out.colour[row[q]] * N + row[q]; };
      std::sort(order, order + m, [&](int a, int b) { return key(a) < key(b); });
      const long long own = (long long)out.colour[i] * N + i;
      int nl = 0;
      unsigned long long pack = 0;
      for (int p = 0; p < m; p++) {
        if (out.colour[row[order[p]]] == out.colour[i]) { err = "multicolour ordering: the pattern is not structurally symmetric"; return -2; }
        if (key(order[p]) < own) nl++;
        pack |= (unsigned long long)order[p] << (4 * p);
      }
      out.slots[i] = pack;
      out.counts[i] = nl | ((m - nl) << 8) | (diag[i] << 16) | (out.colour[i] << 24);
    }
    // a triangle inside the subdomain: rows a, b, c eliminated in this order and coupled pairwise -- eliminating a from c
    // updates A_cb, an off-diagonal block
    for (int i = lo; i < hi && out.diag_only; i++) {
      const int* row = colidx.data() + rowptr[i];
      const int cnt = rowptr[i + 1] - rowptr[i];
      for (int q = 0; q < cnt && out.diag_only; q++) {
        const int k = row[q];
        if (k <= i || k >= hi) continue;
        const int* rk = colidx.data() + rowptr[k];
        for (int r = 0; r < rowptr[k + 1] - rowptr[k]; r++) {
          const int j = rk[r];
          if (j > k && j < hi && std::binary_search(row, row + cnt, j)) { out.diag_only = false; break; }
        }
      }
    }
  }
  // the launch lists: rows of each colour over all subdomains
  out.col_ptr.assign(out.max_colours + 1, 0);
  for (int i = 0; i < N; i++) out.col_ptr[out.colour[i] + 1]++;
  for (int c = 0; c < out.max_colours; c++) out.col_ptr[c + 1] += out.col_ptr[c];
  out.rows.resize(N);
  std::vector<int> at(out.col_ptr.begin(), out.col_ptr.end() - 1);
  for (int i = 0; i < N; i++) out.rows[at[out.colour[i]]++] = i;
  return 0;
}

}  // namespace wai

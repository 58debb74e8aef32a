// The pattern of the extended system of PCASM, block-Jacobi ILU(k) and sub-preconditioner lu: the overlapped row set of
// every subdomain, each set's rows restricted to the set as a block of one matrix E, the source network's pairs, the
// level-of-fill (or complete) fill inside every block, and the block-ELL planes and gather map the device gets.  Pure host
// code -- no device header, no context -- so that a plain C++ program can call it (tests/pc_setup_host); build_asm
// (pc_setup.hip) fetches the ghost rows, uploads what build_asm_pattern makes and builds E's schedule.  Not part of the ABI.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

namespace wai {

// ILU(k) symbolic phase on the blocks of a block matrix (host CSR, ascending columns, all columns inside the
// row's block): level-of-fill rule of PETSc's MatILUFactorSymbolic -- an entry created while row k is
// eliminated from row i gets lev(i,k) + lev(k,j) + 1, an entry reached twice keeps the smaller level, kept when
// <= levels ("sub_preconditioner": {"factor": {"levels": k}}, src/timestepper.F90:1716-1718, 1827).  ILU(k)'s
// numeric phase is ILU(0) on the filled pattern with explicit zeros, which is how it runs here.
// src: per entry the index it is filled from (kept for original entries, -1 for fill).
// levels = ILU_COMPLETE_FILL keeps every level: the pattern of the blocks' exact LU factors (sub-preconditioner lu).
// Returns 0, or the width of the first row found with more than max_width entries (the patterns are left as they were).
constexpr int ILU_COMPLETE_FILL = 1 << 28;
inline int iluk_fill(const std::vector<int>& ptr, int levels, int max_width, std::vector<int>& rp, std::vector<int>& col, std::vector<int>& src) {
  const int n = (int)rp.size() - 1;
  std::vector<int> orp(n + 1, 0), ocol, osrc, olev, odiag(n, 0);
  ocol.reserve(col.size() * (size_t)(1 + 2 * std::min(levels, 8))); osrc.reserve(ocol.capacity()); olev.reserve(ocol.capacity());
  std::vector<int> wc, wl, ws;
  for (size_t b = 0; b + 1 < ptr.size(); b++)
    for (int i = ptr[b]; i < ptr[b + 1]; i++) {
      wc.assign(col.begin() + rp[i], col.begin() + rp[i + 1]);
      ws.assign(src.begin() + rp[i], src.begin() + rp[i + 1]);
      wl.assign(wc.size(), 0);
      for (size_t a = 0; a < wc.size() && wc[a] < i; a++) {   // eliminate with row k = wc[a], ascending (fill included)
        const int k = wc[a], lik = wl[a];
        for (int r = odiag[k] + 1; r < orp[k + 1]; r++) {
          const int j = ocol[r], lv = lik + olev[r] + 1;
          if (lv > levels) continue;
          const size_t pos = (size_t)(std::lower_bound(wc.begin() + a + 1, wc.end(), j) - wc.begin());
          if (pos < wc.size() && wc[pos] == j) { wl[pos] = std::min(wl[pos], lv); continue; }
          wc.insert(wc.begin() + pos, j); wl.insert(wl.begin() + pos, lv); ws.insert(ws.begin() + pos, -1);
        }
        if ((int)wc.size() > max_width) return (int)wc.size();
      }
      orp[i] = (int)ocol.size();
      odiag[i] = -1;
      for (size_t a = 0; a < wc.size(); a++) {
        if (wc[a] == i) odiag[i] = (int)ocol.size();
        ocol.push_back(wc[a]); osrc.push_back(ws[a]); olev.push_back(wl[a]);
      }
      orp[i + 1] = (int)ocol.size();
      if (odiag[i] < 0) odiag[i] = orp[i + 1] - 1;
    }
  rp.swap(orp); col.swap(ocol); src.swap(osrc);
  return 0;
}

constexpr int MAX_FACTOR_ROW = 255;   // slots of a factor row (8-bit row descriptors)

// The local matrix the row sets grow on: rows 0 .. N - 1 are the Jacobian's own, rows N .. N + H - 1 the partition-ghost
// cells' as received from their owners (grp / gci / gslot: CSR with the sender's slot of every entry; empty on one rank)
struct AsmRows {
  const std::vector<int>&rowptr, &colidx, &grp, &gci, &gslot;
  int N, H;
  int begin(int i) const { return i < N ? rowptr[i] : grp[i - N]; }
  int end(int i) const { return i < N ? rowptr[i + 1] : grp[i - N + 1]; }
  int col(int i, int e) const { return i < N ? colidx[e] : gci[e]; }
  // slot * n + row in J's block-ELL planes, or the ghost rows' (<= -2)
  int src(int i, int e) const { return i < N ? (e - rowptr[i]) * N + i : -(2 + gslot[e] * H + (i - N)); }
};

struct AsmPattern {
  std::vector<int> ext_ptr, ext_rows;   // block b's rows, ascending: ext_rows[ext_ptr[b] .. ext_ptr[b + 1])
  // E as CSR over the extended numbering (columns are positions in ext_rows), fill and network pairs included; src: where
  // an entry's block comes from (AsmRows::src), -1 for none
  std::vector<int> erp, ecol, esrc;
  int W = 1;                            // most blocks of a row of E
  // what the device gets: E's block-ELL column planes and gather map [W][n_ext] (padding: the row itself, -1), and the row
  // of the local matrix behind every row of E, bit 31 set where the block owns it
  std::vector<int> ell_col, gmap, ext_row;
  std::vector<int> net_pos, net_pair;   // where the blocks of the network's E land in the extended planes
};

// the overlapped row set of every subdomain (MatIncreaseOverlap over the matrix graph), in ascending row order (PETSc
// sorts the subdomain index sets)
inline void asm_row_sets(const AsmRows& A, const std::vector<int>& sub, int overlap, AsmPattern& out) {
  const int nsub = (int)sub.size() - 1, NX = A.N + A.H;
  std::vector<int>& ext_rows = out.ext_rows;
  std::vector<int> mark(NX, -1);
  out.ext_ptr.assign(nsub + 1, 0);
  ext_rows.reserve((size_t)A.N * 2);
  for (int sd = 0; sd < nsub; sd++) {
    const size_t start = ext_rows.size();
    for (int i = sub[sd]; i < sub[sd + 1]; i++) { ext_rows.push_back(i); mark[i] = sd; }
    size_t lo = start;
    for (int l = 0; l < overlap; l++) {
      const size_t hi = ext_rows.size();
      for (size_t q = lo; q < hi; q++) {
        const int i = ext_rows[q];
        for (int e = A.begin(i); e < A.end(i); e++) {
          const int j = A.col(i, e);
          if (j >= NX || mark[j] == sd) continue;
          ext_rows.push_back(j); mark[j] = sd;
        }
      }
      lo = hi;
    }
    std::sort(ext_rows.begin() + start, ext_rows.end());
    out.ext_ptr[sd + 1] = (int)ext_rows.size();
  }
}

// every set's rows restricted to the set
// (columns are positions in the extended numbering: block b's rows are ext_ptr[b] .. ext_ptr[b + 1])
inline void asm_restrict_rows(const AsmRows& A, AsmPattern& out) {
  const int nsub = (int)out.ext_ptr.size() - 1, NX = A.N + A.H, n_ext = (int)out.ext_rows.size();
  std::vector<int> mark(NX, -1), loc(NX, 0);
  out.erp.assign(n_ext + 1, 0);
  out.ecol.reserve((size_t)n_ext * 7); out.esrc.reserve((size_t)n_ext * 7);
  for (int sd = 0; sd < nsub; sd++) {
    const int a0 = out.ext_ptr[sd], b0 = out.ext_ptr[sd + 1];
    for (int q = a0; q < b0; q++) { mark[out.ext_rows[q]] = sd; loc[out.ext_rows[q]] = q; }
    for (int q = a0; q < b0; q++) {
      const int i = out.ext_rows[q];
      for (int e = A.begin(i); e < A.end(i); e++) {
        const int j = A.col(i, e);
        if (j >= NX || mark[j] != sd) continue;
        out.ecol.push_back(loc[j]);
        out.esrc.push_back(A.src(i, e));
      }
      out.erp[q + 1] = (int)out.ecol.size();
    }
  }
}

// The source network's blocks (flow_simulation_modify_jacobian, src/flow_simulation.F90:3023-3084: the reference widens
// the BAIJ pattern by the network's dependencies and PETSc factors what it finds there): every pair of network cells
// that share a subdomain's row set gets an entry (a structural zero of A where the cells are not neighbours; the
// values are added after the gather, k_asm_add_couplings), before the fill levels are counted.
// netidx: per row of the local matrix its place among the network's cells, or -1
inline void asm_add_network_pairs(const std::vector<int>& netidx, int N, size_t mnet, AsmPattern& out) {
  const int nsub = (int)out.ext_ptr.size() - 1, n_ext = (int)out.ext_rows.size();
  const std::vector<int>&ext_ptr = out.ext_ptr, &ext_rows = out.ext_rows, &erp = out.erp, &ecol = out.ecol, &esrc = out.esrc;
  std::vector<int> nrp(n_ext + 1, 0), ncol, nsrc;
  ncol.reserve(ecol.size() + mnet * mnet); nsrc.reserve(ncol.capacity());
  for (int sd = 0; sd < nsub; sd++) {
    std::vector<int> cells;   // ext positions of the network cells in this subdomain's row set
    for (int q = ext_ptr[sd]; q < ext_ptr[sd + 1]; q++) if (ext_rows[q] < N && netidx[ext_rows[q]] >= 0) cells.push_back(q);
    for (int q = ext_ptr[sd]; q < ext_ptr[sd + 1]; q++) {
      const bool isnet = ext_rows[q] < N && netidx[ext_rows[q]] >= 0 && cells.size() > 1;
      if (!isnet) {
        for (int e = erp[q]; e < erp[q + 1]; e++) { ncol.push_back(ecol[e]); nsrc.push_back(esrc[e]); }
      } else {   // merge the row's columns with the network cells' positions (both ascending)
        size_t a2 = 0;
        int e = erp[q];
        while (e < erp[q + 1] || a2 < cells.size()) {
          const int ca = e < erp[q + 1] ? ecol[e] : 0x7fffffff, cb = a2 < cells.size() ? cells[a2] : 0x7fffffff;
          if (ca <= cb) { ncol.push_back(ca); nsrc.push_back(esrc[e]); e++; if (cb == ca) a2++; }
          else { ncol.push_back(cb); nsrc.push_back(-1); a2++; }
        }
      }
      nrp[q + 1] = (int)ncol.size();
    }
  }
  out.erp.swap(nrp); out.ecol.swap(ncol); out.esrc.swap(nsrc);
}

// E's block-ELL planes, the gather map and the rows behind E's rows with their ownership bit
inline void asm_device_arrays(const std::vector<int>& sub, AsmPattern& out) {
  const int nsub = (int)sub.size() - 1, n_ext = (int)out.ext_rows.size(), W = out.W;
  out.ell_col.assign((size_t)W * n_ext, 0); out.gmap.assign((size_t)W * n_ext, -1); out.ext_row.assign(n_ext, 0);
  for (int sd = 0; sd < nsub; sd++)
    for (int q = out.ext_ptr[sd]; q < out.ext_ptr[sd + 1]; q++) {
      const int i = out.ext_rows[q];
      const bool own = i >= sub[sd] && i < sub[sd + 1];
      out.ext_row[q] = own ? (int)((unsigned)i | 0x80000000u) : i;
      const int cnt = out.erp[q + 1] - out.erp[q];
      for (int t = 0; t < W; t++) {
        out.ell_col[(size_t)t * n_ext + q] = t < cnt ? out.ecol[out.erp[q] + t] : q;
        out.gmap[(size_t)t * n_ext + q] = t < cnt ? out.esrc[out.erp[q] + t] : -1;
      }
    }
}

// where the blocks of the network's E land in the extended planes: plane position t * n_ext + q, pair = row * m + column
inline void asm_network_positions(const std::vector<int>& netidx, int N, int mnet, AsmPattern& out) {
  const int n_ext = (int)out.ext_rows.size();
  for (int q = 0; q < n_ext; q++) {
    const int i = out.ext_rows[q];
    if (i >= N || netidx[i] < 0) continue;
    for (int t = 0; t < out.erp[q + 1] - out.erp[q]; t++) {
      const int j = out.ext_rows[out.ecol[out.erp[q] + t]];
      if (j < N && netidx[j] >= 0) { out.net_pos.push_back(t * n_ext + q); out.net_pair.push_back(netidx[i] * mnet + netidx[j]); }
    }
  }
}

// PCASM: the overlapped row set of every subdomain (owned rows, and across a rank boundary the ghost rows), the extended
// matrix that holds each set as its own block, and the map that fills it from the Jacobian.
// levels > 0: ILU(k) fill inside every block; overlap 0 with levels > 0 is block Jacobi + ILU(k) on the same path.
// sublu: complete fill instead (sub-preconditioner lu; levels is 0 then).  net_cells: the distinct cells of the network's
// sources whose blocks go into the pattern (empty: none).  Returns 0, or -2 with `err` set.
inline int build_asm_pattern(const std::vector<int>& rowptr, const std::vector<int>& colidx, int N, const std::vector<int>& grp,
                             const std::vector<int>& gci, const std::vector<int>& gslot, const std::vector<int>& sub, int overlap,
                             int levels, bool sublu, const std::vector<int>& net_cells, AsmPattern& out, std::string& err) {
  out = AsmPattern();
  const AsmRows A{rowptr, colidx, grp, gci, gslot, N, grp.empty() ? 0 : (int)grp.size() - 1};
  asm_row_sets(A, sub, overlap, out);
  asm_restrict_rows(A, out);
  const int mnet = (int)net_cells.size(), n_ext = (int)out.ext_rows.size();
  std::vector<int> netidx(mnet > 0 ? A.N + A.H : 0, -1);
  for (int r = 0; r < mnet; r++) netidx[net_cells[r]] = r;
  if (mnet > 0) asm_add_network_pairs(netidx, N, (size_t)mnet, out);
  if (sublu) {
    // the exact LU of a block is ILU with every level kept.  A block whose complete fill does not fit a factor row is
    // refused -- it never falls back to an incomplete factor
    if (const int w = iluk_fill(out.ext_ptr, ILU_COMPLETE_FILL, MAX_FACTOR_ROW, out.erp, out.ecol, out.esrc)) {
      err = "sub-preconditioner lu: the complete fill of a block gives a factor row of " + std::to_string(w) +
            " blocks or more, the cap is " + std::to_string(MAX_FACTOR_ROW) + " (smaller subdomains, or sub-preconditioner ilu)";
      return -2;
    }
  } else if (levels > 0) iluk_fill(out.ext_ptr, levels, 1 << 30, out.erp, out.ecol, out.esrc);
  for (int q = 0; q < n_ext; q++) out.W = std::max(out.W, out.erp[q + 1] - out.erp[q]);
  if (out.W > MAX_FACTOR_ROW) { err = "ILU(k): more than 255 blocks in a factor row"; return -2; }
  asm_device_arrays(sub, out);
  if (mnet > 0) asm_network_positions(netidx, N, mnet, out);
  return 0;
}

}  // namespace wai

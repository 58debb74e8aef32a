// The scratch plan of the batched coupling build (kernels_coupling.hip; wai_set_coupling_build): every column (j, k) of the
// source network's Jacobian blocks E -- network cell j, primary k -- is evaluated on PRIVATE copies of what the column loop
// borrows from the global state, and this header says where those copies live and how many columns run at once.
// Pure host code -- no device header, no context, no environment -- so that a plain C++ program can call it
// (tests/coupling_batch_host); network_couplings (network.hip) fills in the sizes and the byte cap.  Not part of the ABI.
//
// One column's scratch, in doubles, contiguous:
//   [ h | record df | raw 2n | net 2n | enth n | g0 ml*bs ]
//     h       the column's finite-difference step
//     record  the fluid record of cell j on y_jk + h (the fields of store_state; the others copied from the global record)
//     raw     the sources' own rates [n] and flowing enthalpies [n] on that record
//     net     the (mode, value) pairs the column's network pass hands the residual
//     enth    the sources' enthalpies: the global array, the fed sources' entries rewritten by the column's pass
//     g0      the residual of the network's ml rows with the global factors held
// Column q of a chunk starts at q * per_col.  A chunk is as many columns as fit the byte cap, all of them if they do.
#pragma once
#include <string>

namespace wai {

struct CouplingBatch {
  int ncol = 0;                 // m * bs columns
  int off_h = 0, off_rec = 0, off_raw = 0, off_net = 0, off_enth = 0, off_g0 = 0;
  long long per_col = 0;        // doubles of one column
  int chunk = 0;                // columns per chunk (the last may be shorter)
  int n_chunks = 0, last = 0;   // chunks, and the columns of the last one
  long long doubles = 0;        // chunk * per_col: the scratch to allocate
};

// m network cells (columns' cells), ml of them rows on this rank, bs primaries, df doubles of a fluid record, n sources;
// cap_bytes: the most scratch one chunk may take.  0, or -2 with a text where not even one column fits
inline int coupling_batch_plan(int m, int ml, int bs, int df, int n, long long cap_bytes, CouplingBatch& b, std::string& err) {
  b = CouplingBatch();
  if (m <= 0 || ml < 0 || bs <= 0 || df <= 0 || n <= 0) { err = "coupling batch: no columns, no sources or no record"; return -2; }
  b.ncol = m * bs;
  b.off_h = 0;
  b.off_rec = 1;
  b.off_raw = b.off_rec + df;
  b.off_net = b.off_raw + 2 * n;
  b.off_enth = b.off_net + 2 * n;
  b.off_g0 = b.off_enth + n;
  b.per_col = (long long)b.off_g0 + (long long)ml * bs;
  const long long bytes = 8 * b.per_col, fit = cap_bytes / bytes;
  if (fit < 1) {
    err = "coupling batch: one column's scratch (" + std::to_string(bytes) + " bytes) exceeds the cap (" +
          std::to_string(cap_bytes) + " bytes)";
    return -2;
  }
  b.chunk = fit < b.ncol ? (int)fit : b.ncol;
  b.n_chunks = (b.ncol + b.chunk - 1) / b.chunk;
  b.last = b.ncol - (b.n_chunks - 1) * b.chunk;
  b.doubles = (long long)b.chunk * b.per_col;
  return 0;
}

}  // namespace wai

// The scratch plan of the batched coupling build (waiwera_amd/csrc/coupling_batch.hpp) without a device:
// tests/test_coupling_batch_host.py builds this with the address and undefined-behaviour sanitizers.
//   coupling_batch_host M ML BS DF N CAP [M ML BS DF N CAP ...]
// prints one line per case: "plan ncol off_h off_rec off_raw off_net off_enth off_g0 per_col chunk n_chunks last doubles",
// then "chunks" and the (first column, columns) pair of every chunk as network_couplings walks them -- or "error TEXT".
#include <cstdio>
#include <cstdlib>
#include <string>

#include "coupling_batch.hpp"

int main(int argc, char** argv) {
  if (argc < 7 || (argc - 1) % 6) { std::fprintf(stderr, "usage: coupling_batch_host M ML BS DF N CAP ...\n"); return 2; }
  for (int a = 1; a + 5 < argc; a += 6) {
    const int m = std::atoi(argv[a]), ml = std::atoi(argv[a + 1]), bs = std::atoi(argv[a + 2]), df = std::atoi(argv[a + 3]),
              n = std::atoi(argv[a + 4]);
    const long long cap = std::atoll(argv[a + 5]);
    wai::CouplingBatch b;
    std::string err;
    if (wai::coupling_batch_plan(m, ml, bs, df, n, cap, b, err)) { std::printf("error %s\n", err.c_str()); continue; }
    std::printf("plan %d %d %d %d %d %d %d %lld %d %d %d %lld chunks", b.ncol, b.off_h, b.off_rec, b.off_raw, b.off_net, b.off_enth,
                b.off_g0, b.per_col, b.chunk, b.n_chunks, b.last, b.doubles);
    for (int ch = 0; ch < b.n_chunks; ch++) std::printf(" %d %d", ch * b.chunk, ch + 1 < b.n_chunks ? b.chunk : b.last);
    std::printf("\n");
  }
  return 0;
}

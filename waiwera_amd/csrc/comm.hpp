// RCCL communicator wrapper (see comm.cpp).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <functional>
#include <string>

namespace wai {

struct NcclId { char internal[128]; };  // ncclUniqueId

struct Comm {
  void* handle = nullptr;  // ncclComm_t
  int rank = 0, nranks = 1;
  long long n_allreduce = 0, n_exchange = 0;   // collectives enqueued so far (tests, reports)
  long long n_gather = 0;                      // ... and gathers to a root (comm_gatherv; its counts' all-reduce is in n_allreduce)
  bool mute = false;                           // timing probe (wai_bench_mute_comm): collectives return without calling RCCL
};

int comm_unique_id(char id[128], std::string& err);
Comm* comm_create(int rank, int nranks, const char id[128], std::string& err);
void comm_destroy(Comm* c);
int comm_count(Comm* c);
// op: 0 sum, 1 max, 2 min; in place on a device buffer, enqueued on stream
int comm_allreduce(Comm* c, double* buf, size_t count, int op, hipStream_t stream, std::string& err);
// neighbour exchange of packed slabs (doubles), enqueued on stream
int comm_exchange(Comm* c, int n_nbr, const int* nbr_rank, const int* send_ptr, const int* recv_ptr,
                  int dof, const double* sendbuf, double* recvbuf, hipStream_t stream, std::string& err);
// Gather of row slabs to `root`, enqueued on stream: every rank hands `rows` rows of `width` doubles (device, contiguous;
// rows may be 0).  counts (device, nranks doubles, scratch) is all-reduced and read back: on return h_counts[r] is rank
// r's row count on EVERY rank.  recvbuf(total_rows) is asked for once the counts are known and returns the root's device
// buffer for all slabs in rank order (nullptr: failure, err set); it is called on the root only, and the root's own
// slab is copied into its place.  One rank, or no communicator: h_counts[0] = rows and nothing else happens --
// the caller reads sendbuf.
int comm_gatherv(Comm* c, int root, const double* sendbuf, size_t rows, int width, double* counts, long long* h_counts,
                 const std::function<double*(size_t)>& recvbuf, hipStream_t stream, std::string& err);

}  // namespace wai

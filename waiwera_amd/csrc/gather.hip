// wai_gather_rows / wai_gather_fluid (include/waiwera_hip.h): rows of doubles that live on the ranks' devices, each with
// its place in a whole-mesh array, brought together on one rank -- what the reference gets from VecView of a global Vec
// into its HDF5 viewer (src/flow_simulation.F90:2695-2800; PETSc gathers to the writing ranks).  The library's communicator
// is the only one every host has (a Fortran host has no other), so the gather lives here.
//
// Sending side: one kernel packs the rows as [row][ncomp + 1], the last column the row's place as a double -- places are
// int32, so exact -- and the slab goes to the root in one piece (comm_gatherv).  wai_gather_fluid packs chosen columns of
// the device-resident SoA fluid record instead: nothing passes through the sending rank's host.
// Root: one kernel puts every received row at out[place][:] and claims the place in an int array with atomicCAS; the
// first place found out of range or claimed twice is written to a four-word flag, read once.  A host `out` is staged.
// Everything is enqueued on the compute stream, behind whatever produced `local`.
#include "host.hpp"

using namespace wai;

namespace {

constexpr int GT = 256;
constexpr int MAX_GATHER_FIELDS = 32;
struct FieldList { int n; int f[MAX_GATHER_FIELDS]; };   // by value to the kernel

inline int blocks_for(size_t n) { return (int)((n + GT - 1) / GT); }

// send[i][0 .. ncomp) = local[i][:], send[i][ncomp] = index[i]; one thread per element of send: reads and writes coalesced
__global__ void __launch_bounds__(GT) k_gather_pack(const double* __restrict__ local, const int* __restrict__ index, size_t n, int ncomp,
                                                    double* __restrict__ send) {
  const size_t t = (size_t)blockIdx.x * GT + threadIdx.x;
  const size_t w = (size_t)ncomp + 1;
  if (t >= n * w) return;
  const size_t i = t / w;
  const int k = (int)(t - i * w);
  send[t] = k < ncomp ? local[i * ncomp + k] : (double)index[i];
}

// send[i][k] = flu[fields[k] * n_local + i] for the owned cells i, send[i][nf] = index[i].  One thread per cell: for each
// column a wave reads 64 consecutive doubles of that column's plane, so every column is one coalesced stream through the
// record; a wave's stores of one column land (nf + 1) doubles apart and meet in L2 before they reach memory
__global__ void __launch_bounds__(GT) k_gather_pack_fluid(const double* __restrict__ flu, size_t n_local, int n_owned, FieldList fl,
                                                          const int* __restrict__ index, double* __restrict__ send) {
  const int i = blockIdx.x * GT + threadIdx.x;
  if (i >= n_owned) return;
  double* row = send + (size_t)i * (fl.n + 1);
  for (int k = 0; k < fl.n; k++) row[k] = flu[(size_t)fl.f[k] * n_local + i];
  row[fl.n] = (double)index[i];
}

// out[place][:] = slab[i][0 .. ncomp) for every received row i; one thread per element of the slab, the thread of a row's
// last column claims the place.  flag: [0] 0 none | 1 out of range | 2 claimed twice (the first found wins the word),
// [1] the place, [2] [3] the received rows (out of range: [3] = -1).  A row whose place is out of range is not stored;
// of two rows that claim one place either may be -- the call fails and says so
__global__ void __launch_bounds__(GT) k_gather_place(const double* __restrict__ slab, size_t total, int ncomp, int n_global,
                                                     double* __restrict__ out, int* __restrict__ claim, int* __restrict__ flag) {
  const size_t t = (size_t)blockIdx.x * GT + threadIdx.x;
  const size_t w = (size_t)ncomp + 1;
  if (t >= total * w) return;
  const size_t i = t / w;
  const int k = (int)(t - i * w);
  const double pd = slab[i * w + ncomp];
  const bool inside = pd >= 0.0 && pd < (double)n_global;
  const int p = inside ? (int)pd : -1;
  if (k < ncomp) {
    if (inside) out[(size_t)p * ncomp + k] = slab[t];
    return;
  }
  if (!inside) {
    if (atomicCAS(&flag[0], 0, 1) == 0) { flag[1] = (int)fmax(fmin(pd, 2147483647.0), -2147483648.0); flag[2] = (int)i; flag[3] = -1; }
    return;
  }
  const int old = atomicCAS(&claim[p], -1, (int)i);
  if (old != -1 && atomicCAS(&flag[0], 0, 2) == 0) { flag[1] = p; flag[2] = old; flag[3] = (int)i; }
}

int launched_ok(wai_ctx* c, const char* kernel) {
  if (hipError_t e = hipGetLastError(); e != hipSuccess) { c->err = std::string(kernel) + ": " + hipGetErrorString(e); return -1; }
  return 0;
}

// at least `need` elements in b (cap: what it holds); kept from call to call
template <class T>
int grow(wai_ctx* c, DevBuf<T>& b, size_t& cap, size_t need) {
  if (b && need <= cap) return 0;
  cap = 0;
  if (b.alloc(c, need)) return -1;
  cap = std::max<size_t>(need, 1);
  return 0;
}

// a host array staged into b, a device array used in place
template <class T>
int on_device(wai_ctx* c, const T* p, size_t n, DevBuf<T>& b, size_t& cap, const T** dev) {
  *dev = p;
  if (!n || is_device_ptr(p)) return 0;
  if (grow(c, b, cap, n)) return -1;
  HIPCHK(c, hipMemcpyAsync(b, p, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
  *dev = b;
  return 0;
}

int check_args(wai_ctx* c, const char* who, int root, int n_global, const void* out) {
  const int nr = c->comm ? c->comm->nranks : 1, me = c->comm ? c->comm->rank : 0;
  if (root < 0 || root >= nr) { c->err = std::string(who) + ": root " + std::to_string(root) + " of " + std::to_string(nr) + " ranks"; return -2; }
  if (n_global < 0 || (me == root && n_global > 0 && !out)) { c->err = std::string(who) + ": the root needs out[n_global][ncomp]"; return -2; }
  return 0;
}

// c->gat.send holds this rank's `rows` packed rows: to the root, and there into out
int gather_packed(wai_ctx* c, const char* who, int root, int ncomp, size_t rows, int n_global, double* out) {
  Gather& g = c->gat;
  const int nr = c->comm ? c->comm->nranks : 1, me = c->comm ? c->comm->rank : 0;
  const size_t w = (size_t)ncomp + 1;
  if (grow(c, g.counts, g.n_counts, (size_t)nr)) return -1;
  std::vector<long long> cnt(nr, 0);
  auto recvbuf = [&](size_t total) -> double* { return grow(c, g.recv, g.n_recv, total * w) ? nullptr : g.recv.get(); };
  if (comm_gatherv(c->comm, root, g.send, rows, (int)w, g.counts, cnt.data(), recvbuf, c->stream, c->err)) return -1;
  if (me != root || (c->comm && c->comm->mute)) return 0;
  const double* slab = nr > 1 ? g.recv.get() : g.send.get();
  size_t total = 0;
  for (long long n : cnt) total += (size_t)n;
  if (total > (size_t)0x7fffffff) { c->err = std::string(who) + ": more than 2^31 - 1 rows"; return -2; }
  const bool dev_out = n_global > 0 && is_device_ptr(out);
  const size_t n_out = (size_t)n_global * ncomp;
  double* dout = out;
  if (!dev_out) {
    if (grow(c, g.out, g.n_out, n_out)) return -1;
    dout = g.out;
    // places nobody sends keep what out held.  With n_global rows on their way every place is either filled exactly once or
    // the call fails (a place out of range or claimed twice): nothing of out survives, and nothing of it is sent up
    if (n_out && total < (size_t)n_global) HIPCHK(c, hipMemcpyAsync(dout, out, n_out * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  if (grow(c, g.claim, g.n_claim, (size_t)n_global) || (!g.flag && g.flag.alloc(c, 4))) return -1;
  if (n_global) HIPCHK(c, hipMemsetAsync(g.claim, 0xff, (size_t)n_global * sizeof(int), c->stream));
  HIPCHK(c, hipMemsetAsync(g.flag, 0, 4 * sizeof(int), c->stream));
  if (total) {
    hipLaunchKernelGGL(k_gather_place, blocks_for(total * w), GT, 0, c->stream, slab, total, ncomp, n_global, dout, g.claim.get(), g.flag.get());
    if (launched_ok(c, "k_gather_place")) return -1;
  }
  int hf[4] = {0, 0, 0, 0};
  HIPCHK(c, hipMemcpyAsync(hf, g.flag, sizeof hf, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (hf[0]) {
    auto whose = [&](int row) {      // "rank r (its row k)" of a received row
      long long first = 0;
      int r = 0;
      while (r < nr - 1 && row >= first + cnt[r]) first += cnt[r++];
      return "rank " + std::to_string(r) + " (its row " + std::to_string(row - first) + ")";
    };
    if (hf[0] == 1)
      c->err = std::string(who) + ": place " + std::to_string(hf[1]) + " sent by " + whose(hf[2]) + " is outside [0, " + std::to_string(n_global) + ")";
    else
      c->err = std::string(who) + ": place " + std::to_string(hf[1]) + " is claimed twice, by " + whose(hf[2]) + " and by " + whose(hf[3]);
    return -2;
  }
  if (!dev_out && n_out) {
    HIPCHK(c, hipMemcpyAsync(out, dout, n_out * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return 0;
}

}  // namespace

extern "C" {

int wai_gather_rows(wai_ctx* c, int root, int ncomp, const double* local, int n_local, const int* index, int n_global, double* out) {
  if (!c) return -2;
  if (ncomp < 1 || n_local < 0 || (n_local > 0 && (!local || !index))) { c->err = "wai_gather_rows: ncomp >= 1, n_local >= 0, local and index for the rows"; return -2; }
  if (int e = check_args(c, "wai_gather_rows", root, n_global, out)) return e;
  Gather& g = c->gat;
  const size_t rows = (size_t)n_local;
  const double* dl = nullptr;
  const int* di = nullptr;
  if (on_device(c, local, rows * ncomp, g.in, g.n_in, &dl) || on_device(c, index, rows, g.idx, g.n_idx, &di)) return -1;
  if (grow(c, g.send, g.n_send, rows * (ncomp + 1))) return -1;
  if (rows) {
    hipLaunchKernelGGL(k_gather_pack, blocks_for(rows * (ncomp + 1)), GT, 0, c->stream, dl, di, rows, ncomp, g.send.get());
    if (launched_ok(c, "k_gather_pack")) return -1;
  }
  return gather_packed(c, "wai_gather_rows", root, ncomp, rows, n_global, out);
}

int wai_gather_fluid(wai_ctx* c, int root, int which, int nf, const int* fields, const int* index, int n_global, double* out) {
  if (!c) return -2;
  if (which < 0 || which > 2 || nf < 1 || nf > MAX_GATHER_FIELDS || !fields || !index) {
    c->err = "wai_gather_fluid: which 0 .. 2, 1 .. " + std::to_string(MAX_GATHER_FIELDS) + " fields, an index per owned cell";
    return -2;
  }
  if (which == 1 && c->last_iter_partial) {   // as wai_get_fluid
    c->err = "wai_gather_fluid(1): the last-iteration record is partial after wai_newton_step (temperature, region, old region); "
             "call wai_pre_iteration for the whole record";
    return -2;
  }
  FieldList fl;
  fl.n = nf;
  for (int k = 0; k < nf; k++) {
    if (fields[k] < 0 || fields[k] >= c->df) { c->err = "wai_gather_fluid: field " + std::to_string(fields[k]) + " of a record of " + std::to_string(c->df); return -2; }
    fl.f[k] = fields[k];
  }
  if (int e = check_args(c, "wai_gather_fluid", root, n_global, out)) return e;
  Gather& g = c->gat;
  const int n = c->mesh.n_owned;
  const int* di = nullptr;
  if (on_device(c, index, (size_t)n, g.idx, g.n_idx, &di)) return -1;
  if (grow(c, g.send, g.n_send, (size_t)n * (nf + 1))) return -1;
  const double* flu = which == 0 ? c->flu : (which == 1 ? c->flu_last_iter : c->flu_last_step);
  hipLaunchKernelGGL(k_gather_pack_fluid, blocks_for((size_t)n), GT, 0, c->stream, flu, (size_t)c->mesh.n_local, n, fl, di, g.send.get());
  if (launched_ok(c, "k_gather_pack_fluid")) return -1;
  return gather_packed(c, "wai_gather_fluid", root, nf, (size_t)n, n_global, out);
}

int wai_gather_stats(wai_ctx* c, long long* gathers) {
  if (!c || !gathers) return -2;
  *gathers = c->comm ? c->comm->n_gather : 0;
  return 0;
}

}  // extern "C"

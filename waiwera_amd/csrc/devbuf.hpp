// The one owner of device memory (and of the three pinned host buffers) in libwaiwera_hip.so.  A DevBuf field OWNS what
// it points to: move-only, freed by its destructor, so a struct's lifetime is its buffers' lifetime and no free list
// is kept anywhere.  Everything handed to a kernel -- plain pointers, Bcsr, MeshView, Fin, Tracers -- is a VIEW and owns
// nothing; the implicit conversion to T* makes an owner read like the raw pointer it replaces at every launch site.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <string>
#include <utility>
#include <vector>

#define HIPCHK(c, call)                                                                 \
  do {                                                                                  \
    hipError_t e_ = (call);                                                             \
    if (e_ != hipSuccess) {                                                             \
      (c)->err = std::string(#call) + ": " + hipGetErrorString(e_);                     \
      return -1;                                                                        \
    }                                                                                   \
  } while (0)

namespace wai {

// live device allocations of the process and their bytes (wai_test_device_memory)
inline std::atomic<long long> dev_live_allocs{0}, dev_live_bytes{0};

// PINNED: host memory of hipHostMalloc instead (not counted).  Ctx is wai_ctx, which holds DevBufs and is incomplete here
template <class T, bool PINNED = false>
class DevBuf {
  T* p_ = nullptr;
  size_t bytes_ = 0;

 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p_, o.p_); std::swap(bytes_, o.bytes_); return *this; }   // o's destructor frees what this held
  ~DevBuf() { reset(); }
  // hipFree synchronises the device: a kernel still reading the buffer is waited for
  void reset() {
    if (!p_) return;
    if constexpr (PINNED) (void)hipHostFree(p_);
    else { (void)hipFree(p_); dev_live_allocs -= 1; dev_live_bytes -= (long long)bytes_; }
    p_ = nullptr; bytes_ = 0;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  // frees what it held, then n elements (at least one), uninitialised; on failure c->err is set and the buffer is empty
  template <class Ctx>
  int alloc(Ctx* c, size_t n, unsigned host_flags = hipHostMallocDefault) {
    reset();
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    void* p = nullptr;
    if constexpr (PINNED) HIPCHK(c, hipHostMalloc(&p, bytes, host_flags));
    else { HIPCHK(c, hipMalloc(&p, bytes)); dev_live_allocs += 1; dev_live_bytes += (long long)bytes; }
    p_ = static_cast<T*>(p); bytes_ = bytes;
    return 0;
  }
  template <class Ctx>
  int alloc_zeroed(Ctx* c, size_t n) {
    if (alloc(c, n)) return -1;
    HIPCHK(c, hipMemset(p_, 0, bytes_));
    return 0;
  }
  template <class Ctx>
  int upload(Ctx* c, const std::vector<T>& v) {
    if (alloc(c, v.size())) return -1;
    if (!v.empty()) HIPCHK(c, hipMemcpy(p_, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
  }
};
template <class T> using PinnedBuf = DevBuf<T, true>;

}  // namespace wai

// device_buffer.hpp -- the two owners of device and pinned memory (host code only).  Nothing else in csrc/ allocates or frees
// either kind, apart from HipBackend::end_of_call(), which frees what a call handed over with release().
#pragma once
#include <hip/hip_runtime_api.h>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>

namespace sabc {

// bytes these types own right now: [0] device, [1] pinned (sabc_debug_live_bytes)
inline std::atomic<int64_t> g_live_bytes[2];

// `count` elements of device memory.  Move-only; the destructor frees, so the owner's device has to be current then.
template <class T>
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  DeviceBuffer(DeviceBuffer &&o) noexcept { *this = std::move(o); }
  DeviceBuffer &operator=(DeviceBuffer &&o) noexcept { std::swap(p_, o.p_); std::swap(n_, o.n_); return *this; }   // (o frees what this held)
  ~DeviceBuffer() { reset(); }
  // ext_flags == 0: hipMalloc; otherwise hipExtMallocWithFlags (hipDeviceMallocFinegrained, hipDeviceMallocUncached).
  // Whatever the buffer held before is freed first; on failure it is left empty.
  hipError_t alloc(size_t count, unsigned ext_flags = 0) {
    reset();
    const hipError_t e = ext_flags ? hipExtMallocWithFlags((void **)&p_, count * sizeof(T), ext_flags) : hipMalloc((void **)&p_, count * sizeof(T));
    if (e != hipSuccess) { p_ = nullptr; return e; }
    n_ = count;
    g_live_bytes[0] += (int64_t)(n_ * sizeof(T));
    return hipSuccess;
  }
  T *get() const { return p_; }                      // the allocation's base
  size_t count() const { return n_; }
  void reset() { if (p_) (void)hipFree(release()); }  // hipFree NOW (it waits for every stream of the process)
  T *release() {                                     // gives the allocation up: to the deferred list of a call, or to be parked
    g_live_bytes[0] -= (int64_t)(n_ * sizeof(T));
    n_ = 0;
    return std::exchange(p_, nullptr);
  }

 private:
  T *p_ = nullptr;
  size_t n_ = 0;
};

// `count` elements of pinned host memory mapped into the device: one allocation, two addresses.
template <class T>
class MappedHostBuffer {
 public:
  MappedHostBuffer() = default;
  MappedHostBuffer(MappedHostBuffer &&o) noexcept { *this = std::move(o); }
  MappedHostBuffer &operator=(MappedHostBuffer &&o) noexcept { std::swap(h_, o.h_); std::swap(d_, o.d_); std::swap(n_, o.n_); return *this; }
  ~MappedHostBuffer() { reset(); }
  hipError_t alloc(size_t count) {
    reset();
    hipError_t e = hipHostMalloc((void **)&h_, count * sizeof(T), hipHostMallocMapped);
    if (e != hipSuccess) { h_ = nullptr; return e; }
    n_ = count;
    g_live_bytes[1] += (int64_t)(n_ * sizeof(T));
    e = hipHostGetDevicePointer((void **)&d_, h_, 0);
    if (e != hipSuccess) reset();
    return e;
  }
  T *host() const { return h_; }
  T *dev() const { return d_; }
  size_t count() const { return n_; }
  void reset() {
    if (!h_) return;
    (void)hipHostFree(h_);
    g_live_bytes[1] -= (int64_t)(n_ * sizeof(T));
    h_ = d_ = nullptr; n_ = 0;
  }

 private:
  T *h_ = nullptr, *d_ = nullptr;
  size_t n_ = 0;
};

}  // namespace sabc

// What the host drivers of the device units share (pairing.hip, pairing_bls.hip): device memory and a stream that free themselves,
// the error macro, and the arithmetic of launches and chunk loops.  Host code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "../../include/zkhip.h"

namespace zkhip {

// `capacity()` elements of T on the device.  The memory is freed once, on every path: by the destructor, or by a reserve() that has to
// grow.  reserve() frees BEFORE it allocates, so a group of buffers that grows together never holds more than its new sizes.
template <class T>
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  ~DeviceBuffer() { release(); }
  // room for n elements; what the buffer held is lost when it grows.  A failed allocation leaves it empty.
  hipError_t reserve(size_t n) {
    if (n <= cap_) return hipSuccess;
    release();
    const hipError_t e = hipMalloc(&p_, n * sizeof(T));
    if (e != hipSuccess) p_ = nullptr;
    else cap_ = n;
    return e;
  }
  void release() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    cap_ = 0;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t capacity() const { return cap_; }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

// A non-blocking stream.  Declared in front of a context's buffers it is destroyed behind them.
struct DeviceStream {
  hipStream_t s = nullptr;
  DeviceStream() = default;
  DeviceStream(const DeviceStream&) = delete;
  DeviceStream& operator=(const DeviceStream&) = delete;
  ~DeviceStream() { if (s) (void)hipStreamDestroy(s); }
  hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
  operator hipStream_t() const { return s; }
};

// a HIP call inside a function that has errbuf / errlen and returns a ZKHIP_* code
#define ZK_HIP_TRY(prefix, x)                                                                         \
  do {                                                                                                \
    hipError_t e_ = (x);                                                                              \
    if (e_ != hipSuccess) {                                                                           \
      if (errbuf) snprintf(errbuf, errlen, prefix ": %s: %s", #x, hipGetErrorString(e_));             \
      return ZKHIP_ERR_HIP;                                                                           \
    }                                                                                                 \
  } while (0)

inline unsigned blocks_for(size_t n, size_t per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// body(lo, m) for the chunks [lo, lo + m) of `count` items, `chunk` at a time; stops at the first code that is not ZKHIP_OK
template <class Body>
int for_each_chunk(size_t count, size_t chunk, Body body) {
  for (size_t lo = 0; lo < count; lo += chunk) {
    const int rc = body(lo, count - lo < chunk ? count - lo : chunk);
    if (rc != ZKHIP_OK) return rc;
  }
  return ZKHIP_OK;
}

// The selftest kernels' driver: out[i] = kernel(op, a[i], b[i]) on n sets of 72 ABI limbs, on the null stream.
template <class Kernel>
hipError_t selftest_launch(Kernel kernel, unsigned per_block, unsigned block, int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out) {
  DeviceBuffer<uint64_t> da, db, dr;
  hipError_t e = da.reserve(n * 72);
  if (e == hipSuccess) e = db.reserve(n * 72);
  if (e == hipSuccess) e = dr.reserve(n * 72);
  if (e == hipSuccess) e = hipMemcpy(da, a, n * 576, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(db, b, n * 576, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(kernel, dim3(blocks_for(n, per_block)), dim3(block), 0, 0, op, da.get(), db.get(), n, dr.get());
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, dr, n * 576, hipMemcpyDeviceToHost);
  return e;
}

}  // namespace zkhip

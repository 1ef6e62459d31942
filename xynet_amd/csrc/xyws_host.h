// xyws_host.h — internal: the host-side helpers the context's entry points
// (xyws_ctx.h) and the stream decoder's host path (xyws_stream.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "xyws.h"

namespace xyws_internal {

struct device_guard {
  int prev = -1;
  bool ok = false;
  explicit device_guard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = hipSetDevice(dev) == hipSuccess;
  }
  ~device_guard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

inline int hip_err(hipError_t e) { return e == hipSuccess ? XYWS_OK : XYWS_ERR_HIP; }

// Zero device memory and wait until it is zero: hipMemset on device memory may
// return before the memset ran (it goes to the null stream, which does not
// order the caller's non-blocking streams); a kernel on such a stream would
// otherwise read the allocation's old contents (scratch tickets, epochs).
inline hipError_t zero_now(void* p, size_t n) {
  hipError_t e = hipMemset(p, 0, n);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  return e;
}

inline bool capturing(hipStream_t s) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(s, &cs);
  return cs != hipStreamCaptureStatusNone;
}

// A device range as the kernels address it: bytes [lo, hi) from the
// 16-byte-aligned address at or below its start.
struct range16 {
  uint8_t* base;
  uint64_t lo, hi;
};
inline range16 span16(const void* p, uint64_t len) {
  const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
  return range16{reinterpret_cast<uint8_t*>(addr & ~(uintptr_t)15), addr & 15, (addr & 15) + len};
}

inline int grid_for(uint64_t items, uint32_t per_block, uint32_t cap) {
  uint64_t g = (items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}

// The grid of a fan-out launch (k_room_fanout, k_backlog_deliver): x strides
// over the n connections, y over the copy steps of one connection's range, so
// that about `aim` workgroups are in flight and at most slices_max share one
// connection. !copies: the launch writes result rows only.
inline dim3 fanout_grid(uint64_t n, bool copies, uint32_t cap, uint32_t aim, uint32_t slices_max) {
  const uint32_t gx = (uint32_t)grid_for(n, 1, cap);
  uint32_t gy = (aim + gx - 1u) / gx;
  if (gy > slices_max) gy = slices_max;
  return dim3(gx, copies ? gy : 1u);
}

// One device scratch area: every buffer a context owns is one of these, and
// this is the only place one is allocated or freed. `units` is what the area
// covers in its owner's unit (runs, segments, table entries, bytes); the owner
// states its floor where it calls grow().
struct dev_area {
  void* mem = nullptr;
  uint64_t units = 0;

  // Grown to cover `want` units in `bytes` bytes, the first `zero` of them
  // zeroed before any kernel can read them. Never under graph capture
  // (XYWS_ERR_CAPACITY: xyws_ctx_reserve beforehand). The new allocation comes
  // first, so a failure keeps the old one; the old one is freed once the
  // device is idle: a call in flight may still use it.
  int grow(uint64_t want, uint64_t bytes, uint64_t zero, bool capturing) {
    if (mem && want <= units) return XYWS_OK;
    if (capturing) return XYWS_ERR_CAPACITY;
    void* m = nullptr;
    if (hipMalloc(&m, bytes) != hipSuccess) return XYWS_ERR_NOMEM;
    if (mem) {
      (void)hipDeviceSynchronize();
      (void)hipFree(mem);
    }
    mem = m;
    units = want;
    return !zero || zero_now(m, zero) == hipSuccess ? XYWS_OK : XYWS_ERR_HIP;
  }
  // (the owner has made the device idle)
  void release() {
    if (mem) (void)hipFree(mem);
    mem = nullptr;
    units = 0;
  }
};

}  // namespace xyws_internal

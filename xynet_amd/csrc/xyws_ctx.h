// xyws_ctx.h — internal: the C-ABI context (per-stream device scratch slots)
// shared by the entry points in xyws.hip and xyws_frames.hip. Each host-side
// rule is stated once here: how a buffer grows (dev_area, xyws_host.h), which
// slot a stream has (find_slot, acquire_slot), what a reserve gives a slot
// (reserve_slot) and which slots get it (reserve_bound_and_spare), and how an
// entry point begins (call_scope).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>

#include "xyws.h"
#include "xyws_host.h"
#include "xyws_stream.h"

// ---------------------------------------------------------------------------
// Frame table (device scratch, SoA) consumed by k_unmask_tiles. Entries are
// sorted by position and non-overlapping; [ps, pe) is the payload range to
// unmask (already clipped), kw the key word for 4-byte-aligned positions.
struct frame_table {
  uint64_t* start;
  uint64_t* ps;
  uint64_t* pe;
  uint32_t* kw;
  uint64_t* count;  // number of valid entries (device)
};

// Device scratch is kept per (context, stream): a decode's run records, flags
// and frame table belong to the stream it was enqueued on, so calls on one
// context from several streams (an io_uring service overlapping batches) run
// concurrently without sharing scratch. XYWS_SLOTS streams get a slot each;
// when a further stream arrives while every slot is bound, the device is
// synchronized (every slot idle) and the bindings start over.
#define XYWS_SLOTS 16

// Every buffer is a dev_area and grows by its one rule; these floors are the
// smallest allocation of each.
constexpr uint64_t TAB_MIN_ENTRIES = 1024, IOV_MIN_BYTES = 1u << 20, AUX_MIN_BYTES = 65536, STAGE_MIN_BYTES = 4096;

struct scratch_slot {
  bool bound = false;
  hipStream_t stream = nullptr;
  xyws_internal::dev_area tab;  // frame table scratch (indexed + serial modes; units: entries)
  stream_scratch ss;            // fused stream decoder scratch (xyws_stream.hip)
  xyws_internal::dev_area aux;  // frame-list kernels' scratch (xyws_frames.hip): block sums, message tables
  xyws_internal::dev_area iov;  // xyws_decode_stream_iov: the pieces of one buffer sequence, gathered
};

#define XYWS_ARENA_STREAMS 8
struct xyws_ctx {
  int device = 0;
  std::mutex mu;
  uint32_t* err = nullptr;  // device error word (serial / indexed modes)
  // xyws_ctx_reserve, xyws_ctx_reserve_iov: the largest asked for so far.
  // reserve_slot applies all three to a slot
  uint64_t reserve_bytes = 0, reserve_frames = 0, reserve_iov = 0;
  xyws_internal::dev_area stage;  // xyws_mask_bytes: device copy of host bytes (under mu)
  scratch_slot slot[XYWS_SLOTS];
  // recv arenas share a few streams of the context (arena k: stream k mod
  // XYWS_ARENA_STREAMS), so that any number of connections bind at most that
  // many scratch slots (created on first use, destroyed with the context)
  hipStream_t arena_stream[XYWS_ARENA_STREAMS] = {};
  uint32_t arena_rr = 0;
};

namespace xyws_internal {

inline int ensure_table(scratch_slot* sl, uint64_t n, bool capture) {
  const uint64_t cap = n < TAB_MIN_ENTRIES ? TAB_MIN_ENTRIES : n;
  return sl->tab.grow(cap, cap * (8 + 8 + 8 + 4) + 64, 0, capture);
}

inline frame_table table_of(scratch_slot* sl) {
  frame_table t;
  char* m = static_cast<char*>(sl->tab.mem);
  t.start = reinterpret_cast<uint64_t*>(m);
  t.ps = t.start + sl->tab.units;
  t.pe = t.ps + sl->tab.units;
  t.count = t.pe + sl->tab.units;
  t.kw = reinterpret_cast<uint32_t*>(t.count + 8);
  return t;
}

// An area counted in bytes, of at least `bytes` and its floor (ctx->mu held).
inline int ensure_bytes(dev_area* a, uint64_t bytes, uint64_t floor, bool capture) {
  const uint64_t cap = bytes < floor ? floor : bytes;
  return a->grow(cap, cap, 0, capture);
}
inline int ensure_iov(scratch_slot* sl, uint64_t bytes, bool capture) {
  return ensure_bytes(&sl->iov, bytes, IOV_MIN_BYTES, capture);
}
inline int ensure_aux(scratch_slot* sl, uint64_t bytes, bool capture) {
  return ensure_bytes(&sl->aux, bytes, AUX_MIN_BYTES, capture);
}

// The slot bound to `stream`, or null (ctx->mu held).
inline scratch_slot* find_slot(xyws_ctx* ctx, hipStream_t stream) {
  for (auto& sl : ctx->slot)
    if (sl.bound && sl.stream == stream) return &sl;
  return nullptr;
}

// Everything the context has recorded (xyws_ctx_reserve, xyws_ctx_reserve_iov)
// applied to one slot: whatever call brings a slot its reserve, it brings all.
inline int reserve_slot(xyws_ctx* ctx, scratch_slot* sl) {
  if (ctx->reserve_iov)
    if (const int rc = ensure_iov(sl, ctx->reserve_iov, false)) return rc;
  if (ctx->reserve_frames)
    if (const int rc = ensure_table(sl, ctx->reserve_frames, false)) return rc;
  if (!ctx->reserve_bytes && !ctx->reserve_frames) return XYWS_OK;
  return stream_scratch_reserve(&sl->ss, ctx->reserve_bytes, ctx->reserve_frames);
}

// reserve_slot for the slots bound to a stream now and one spare, the first
// unbound one: the one the next new stream binds, so that a stream first used
// inside graph capture finds its reserve. Not all XYWS_SLOTS up front: the
// per-frame tables are tens of GB for 2^26 frames; the others get theirs when
// a stream binds them (acquire_slot).
inline int reserve_bound_and_spare(xyws_ctx* ctx) {
  bool spare = true;
  for (auto& sl : ctx->slot) {
    if (sl.bound || spare)
      if (const int rc = reserve_slot(ctx, &sl)) return rc;
    if (!sl.bound) spare = false;
  }
  return XYWS_OK;
}

// The slot of `stream` (ctx->mu held).
inline int acquire_slot(xyws_ctx* ctx, hipStream_t stream, bool capture, scratch_slot** out) {
  scratch_slot* pick = find_slot(ctx, stream);
  if (!pick) {
    bool any_free = false;
    for (auto& sl : ctx->slot) any_free = any_free || !sl.bound;
    if (!any_free) {
      // every slot bound to another stream: wait until all of them are idle
      if (capture) return XYWS_ERR_CAPACITY;
      if (hipDeviceSynchronize() != hipSuccess) return XYWS_ERR_HIP;
      for (auto& sl : ctx->slot) sl.bound = false;
    }
    for (auto& sl : ctx->slot)
      if (!sl.bound) { pick = &sl; break; }
    if (!capture)
      if (const int rc = reserve_slot(ctx, pick)) return rc;
  }
  pick->bound = true;
  pick->stream = stream;
  *out = pick;
  return XYWS_OK;
}

// The prologue of an entry point that queues work on a stream with a scratch
// slot: ctx->mu held and the context's device current for the scope's life,
// the stream, whether it is capturing, its slot. rc != XYWS_OK: return it.
struct call_scope {
  std::lock_guard<std::mutex> lk;
  device_guard g;
  hipStream_t s;
  bool capt = false;
  scratch_slot* sl = nullptr;
  int rc;
  call_scope(xyws_ctx* ctx, void* stream)
      : lk(ctx->mu), g(ctx->device), s((hipStream_t)stream), rc(g.ok ? XYWS_OK : XYWS_ERR_HIP) {
    if (rc) return;
    capt = capturing(s);
    rc = acquire_slot(ctx, s, capt, &sl);
  }
};

}  // namespace xyws_internal

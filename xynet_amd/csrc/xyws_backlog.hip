// xyws_backlog.hip — xyws_backlog_streams: each room's newest frames kept in a
// log on the device and copied behind the send bytes of every connection that
// joins (the reference's chat_room::m_recent_messages, deliver_recent_messages
// and join, example/websocket/websocket_chat.cpp:34-47, 89-95). The semantics
// are stated in include/xyws.h; this is how they are computed.
//
// Two launches, the rooms' carries the hand-over between them. No workgroup
// waits for another inside a launch, nothing spins, there are no atomics.
//
// k_backlog_fold: one workgroup per room, rooms grid-strided, shaped like the
// broadcast's wire build. The members are taken in tiles of BL_TILE, one
// member per thread:
//   1. the thread loads its member and its gate as the wire build does
//      (bounds-checked index; load_member, xyws_room.h), walks the stored
//      records, tests each (frame_of) and counts and sizes the frames;
//   2. two workgroup scans give each member the index of its first message
//      and its byte offset in the wire; the fold uses the index (step 3) and
//      of the second scan only the total (the copy takes the wire's suffix as
//      a whole); the running sums are carried between tiles in registers;
//   3. a thread whose member holds one of the last min(keep, N) messages
//      walks its records again and writes those frame sizes into at most
//      XYWS_BACKLOG_MAX LDS slots.
// After the last tile every thread computes the same selection from the slots
// and the carry, and the workgroup copies the surviving old bytes and the
// surviving wire suffix into the other half of the log in 16-byte lines
// (xyws_lines.h): the line on the seam is composed from both sources in
// registers.
//
// k_backlog_deliver: the fan-out's geometry and copy (xyws_room.h, copy_span):
// blockIdx.x strides over the connections, blockIdx.y over BC_STEP-byte chunks
// of the destination range. The source is log + start, its length the
// carry's. The y == 0 workgroup writes the connection's result row.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>

#include "xyws.h"
#include "xyws_device.h"
#include "xyws_ctx.h"
#include "xyws_frameops.h"
#include "xyws_lines.h"
#include "xyws_room.h"

#define BL_THREADS BC_WIRE_THREADS  // the fold: the one workgroup a room gets (block_scan's size)
#define BL_TILE BL_THREADS          // members per tile of the fold: one per thread
#define BL_CARRY_WORDS 24u          // sizeof(xyws_backlog_carry) / 8

using namespace xyws_internal;

namespace {

// The half size of a log (0: no log).
XYWS_DEV uint64_t half_of(uint64_t log, uint64_t log_cap) { return log ? (log_cap >> 1) & ~15ull : 0; }

__global__ void __launch_bounds__(BL_THREADS)
    k_backlog_fold(const xyws_reasm_conn* __restrict__ reasm, const xyws_reasm_result* __restrict__ rres,
                   const xyws_bcast_conn* __restrict__ bconns, uint64_t n, const xyws_room* __restrict__ rooms,
                   const xyws_room_result* __restrict__ room_results, const xyws_backlog_room* __restrict__ brooms,
                   xyws_backlog_room_result* __restrict__ broom_results, uint64_t n_rooms) {
  static_assert(sizeof(xyws_backlog_carry) == 8 * BL_CARRY_WORDS && sizeof(xyws_backlog_room) == 32 &&
                    sizeof(xyws_backlog_room_result) == 32 && sizeof(xyws_backlog_conn) == 64 &&
                    sizeof(xyws_backlog_result) == 32 && offsetof(xyws_backlog_carry, flen) == 32 &&
                    offsetof(xyws_backlog_conn, room) == 32 && offsetof(xyws_backlog_room, keep) == 24 &&
                    offsetof(xyws_bcast_result, status) == 16,
                "layouts");
  __shared__ uint64_t s_c[BL_CARRY_WORDS];      // the carry as read
  __shared__ uint64_t s_sz[XYWS_BACKLOG_MAX];   // sizes of the last min(keep, N) new frames, in wire order
  __shared__ uint64_t s_w[BL_THREADS / BC_WAVE];
  const uint32_t tid = threadIdx.x;
  for (uint64_t ri = blockIdx.x; ri < n_rooms; ri += gridDim.x) {
    const g_u64* const rq = (const g_u64*)(rooms + ri);
    const g_u64* const rr = (const g_u64*)(room_results + ri);
    const g_u64* const lq = (const g_u64*)(brooms + ri);
    g_u64* const res = broom_results ? (g_u64*)(broom_results + ri) : nullptr;
    const uint64_t log = uniform64(lq[0]);
    const uint64_t H = half_of(log, uniform64(lq[1]));
    const uint64_t bc = uniform64(lq[2]);
    uint32_t keep = uniform32((uint32_t)lq[3]);
    if (!log || !bc || !keep || !H) {  // pass-through: neither the log nor the carry is touched
      if (res && tid == 0) {
        res[0] = 0;
        res[1] = 0;
        res[2] = (uint64_t)XYWS_BL_PASSTHROUGH << 32;
        res[3] = 0;
      }
      continue;
    }
    if (keep > XYWS_BACKLOG_MAX) keep = XYWS_BACKLOG_MAX;
    if (tid < BL_CARRY_WORDS) s_c[tid] = ((const g_u64*)bc)[tid];
    if (tid < XYWS_BACKLOG_MAX) s_sz[tid] = 0;
    __syncthreads();
    const uint64_t wire_len = uniform64(rr[0]);
    const uint64_t N = uniform64(rr[1]) & 0xFFFFFFFFull;
    const uint32_t rst = (uint32_t)(uniform64(rr[2]) >> 32);
    uint64_t o_start = s_c[0], o_len = s_c[1];
    uint32_t o_count = (uint32_t)s_c[2];
    const uint32_t gaps = (uint32_t)(s_c[2] >> 32);
    const uint64_t total = s_c[3];
    if (N == 0) {  // 1. no new message: the carry and the log stay, the row reports them
      if (res && tid == 0) {
        res[0] = o_len;
        res[1] = o_count;
        res[2] = 0;
        res[3] = 0;
      }
      __syncthreads();  // (s_c is rewritten by the next room)
      continue;
    }
    uint32_t st = 0;
    {  // 2. the carry
      bool valid = (o_start == 0 || o_start == H) && o_len <= H && o_count <= XYWS_BACKLOG_MAX;
      uint64_t sum = 0;
      for (uint32_t j = 0; valid && j < o_count; j++) sum = sat_add(sum, s_c[4 + j]);
      if (!valid || sum != o_len) {
        st |= XYWS_BL_BAD_CARRY;
        o_start = o_len = 0;
        o_count = 0;
      }
    }
    const uint64_t members = uniform64(rq[0]);
    const uint64_t nm = members ? uniform64(rq[1]) : 0;
    const uint64_t wire = uniform64(rq[2]);
    const uint64_t wire_cap = wire ? uniform64(rq[3]) : 0;
    const uint64_t K = N < keep ? N : keep;  // slots in use

    // 3. the new frames, counted and sized from the tables
    uint64_t cnt_run = 0, size_run = 0;  // (uniform)
    for (uint64_t base = 0; base < nm; base += BL_TILE) {
      member m = {0, 0, 0, 0, 0, 0, 0};
      uint64_t size = 0, cnt = 0;
      if (base + tid < nm) {
        const uint64_t ci = ((const XYWS_GLOBAL uint32_t*)members)[base + tid];
        if (ci < n) {  // (an entry >= n is ignored, never dereferenced)
          bool receiver, over_cap;  // (the wire build's: not used here)
          load_member(reasm, rres, bconns, ci, m, receiver, over_cap);
#pragma unroll 1
          for (uint32_t r = 0; r < m.stored; r++) {
            frame_info f;
            if (frame_of((const g_u64*)(m.msgs + 40ull * r), m, 0, 0, f)) {
              size += f.h + m.head_len + f.len;
              cnt++;
            }
          }
        }
      }
      uint64_t tc, ts;
      const uint64_t first = cnt_run + (block_scan(cnt, tid, s_w, tc) - cnt);
      block_scan(size, tid, s_w, ts);  // (only the total: the copy takes the wire's suffix as a whole)
      if (cnt && first + cnt > N - K) {  // one of the last K messages is this member's
        uint64_t idx = first;
#pragma unroll 1
        for (uint32_t r = 0; r < m.stored; r++) {
          frame_info f;
          if (!frame_of((const g_u64*)(m.msgs + 40ull * r), m, 0, 0, f)) continue;
          if (idx >= N - K && idx < N) s_sz[idx - (N - K)] = f.h + m.head_len + f.len;
          idx++;
        }
      }
      cnt_run += tc;
      size_run += ts;
    }
    __syncthreads();  // (the slots are read below)

    uint32_t n_old = 0, n_new = 0;
    uint64_t b_old = 0, b_new = 0;
    uint32_t dropped = o_count;
    bool gap = false;
    if (cnt_run != N || size_run != wire_len) {  // 3. the caller passed other tables
      st |= XYWS_BL_MISMATCH | XYWS_BL_GAP;
      gap = true;
    } else if ((rst & XYWS_ROOM_TRUNCATED) || wire_len > wire_cap) {  // 4. the newest frames cannot be read
      st |= XYWS_BL_GAP;
      gap = true;
    } else {  // 5. the selection, from the newest frame backwards
      uint64_t bytes = 0;
      uint32_t taken = 0;
      bool stop = false;
      for (uint32_t j = (uint32_t)K; j-- > 0 && !stop;) {
        const uint64_t sz = s_sz[j];
        if (taken >= keep) {
          stop = true;
        } else if (sz > H - bytes) {
          stop = true;
          st |= XYWS_BL_EVICTED | (taken ? 0u : XYWS_BL_TOO_LONG);
        } else {
          bytes += sz;
          b_new += sz;
          taken++;
          n_new++;
        }
      }
      if (K < N) stop = true;  // (K == keep frames are taken, or the walk ended above)
      for (uint32_t j = o_count; j-- > 0 && !stop;) {
        const uint64_t sz = s_c[4 + j];
        if (taken >= keep) {
          stop = true;
        } else if (sz > H - bytes) {
          stop = true;
          st |= XYWS_BL_EVICTED;
        } else {
          bytes += sz;
          b_old += sz;
          taken++;
          n_old++;
        }
      }
      dropped = o_count - n_old;
    }
    const uint32_t count = n_old + n_new;
    const uint64_t T = b_old + b_new;
    const uint64_t target = (count && o_count && o_start == 0) ? H : 0;  // 6. (an empty backlog starts at 0)

    if (T) {  // 6. both suffixes to log[target ..), old first
      const uint64_t src_old = log + o_start + (o_len - b_old), src_new = wire + (wire_len - b_new);
      const uint64_t dst = log + target;
      g_u8* const dbase = (g_u8*)(dst & ~15ull);
      const uint64_t P0 = dst & 15u, P1 = P0 + T;
      for (uint64_t A = (uint64_t)BC_LINE * tid; A < P1; A += (uint64_t)BC_LINE * BL_THREADS) {
        const uint64_t s = A > P0 ? A : P0, e = A + 16 < P1 ? A + 16 : P1;
        uint64_t q = s - P0;
        uint32_t a = (uint32_t)(s - A);
        const uint32_t ae = (uint32_t)(e - A);
        bytes16 acc = {0, 0};
        if (q < b_old) {  // old bytes q.. at line offset a
          const uint64_t left = b_old - q;
          const uint32_t nb = left < ae - a ? (uint32_t)left : ae - a;
          add_bytes(acc, a, q, load_bytes(src_old + q, nb), nb);
        }
        if (a < ae) add_bytes(acc, a, q, load_bytes(src_new + (q - b_old), ae - a), ae - a);  // new bytes
        put_line(dbase, A, s, e, P0, P1, acc);
      }
    }

    // 7. the carry after the fold
    if (tid < BL_CARRY_WORDS) {
      uint64_t w = 0;
      if (tid == 0) w = target;
      else if (tid == 1) w = T;
      else if (tid == 2) w = (uint64_t)count | ((uint64_t)(gaps + (gap ? 1u : 0u)) << 32);
      else if (tid == 3) w = total + n_new;
      else if (tid < 4 + XYWS_BACKLOG_MAX) {
        const uint32_t i = tid - 4;
        if (i < n_old) w = s_c[4 + (o_count - n_old) + i];
        else if (i < count) w = s_sz[(uint32_t)K - n_new + (i - n_old)];
      }
      ((g_u64*)bc)[tid] = w;
    }
    if (res && tid == 0) {
      res[0] = T;
      res[1] = (uint64_t)count | ((uint64_t)n_new << 32);
      res[2] = (uint64_t)dropped | ((uint64_t)st << 32);
      res[3] = 0;
    }
    __syncthreads();  // (s_c and s_sz are rewritten by the next room)
  }
}

__global__ void __launch_bounds__(BC_THREADS)
    k_backlog_deliver(const xyws_backlog_conn* __restrict__ jconns, uint64_t n,
                      const xyws_backlog_room* __restrict__ brooms, uint64_t n_rooms,
                      xyws_backlog_result* __restrict__ results) {
  const uint32_t tid = threadIdx.x;
  for (uint64_t ci = blockIdx.x; ci < n; ci += gridDim.x) {
    const g_u64* const jq = (const g_u64*)(jconns + ci);
    const uint64_t out = uniform64(jq[0]);
    const uint64_t out_cap = out ? uniform64(jq[1]) : 0;
    const g_u64* const bp = (const g_u64*)uniform64(jq[2]);
    const g_u64* const rp = (const g_u64*)uniform64(jq[3]);
    const uint64_t rf = uniform64(jq[4]);
    const uint64_t room = rf & 0xFFFFFFFFull;
    const uint32_t fl = (uint32_t)(rf >> 32);
    uint64_t base = 0;
    bool receiver = true;
    if (rp) {
      base = uniform64(rp[0]);
      if ((uint32_t)(uniform64(rp[2]) >> 48) & (XYWS_RPL_CLOSED | XYWS_RPL_OVERFLOW)) receiver = false;
    }
    if (bp) {
      base = uniform64(bp[0]);
      if ((uint32_t)uniform64(bp[2]) & XYWS_BC_NOT_RECEIVER) receiver = false;
    }
    uint32_t st = 0;
    uint64_t w = 0, src = 0;
    if (fl & XYWS_BL_JOIN) {
      uint64_t log = 0, H = 0, bc = 0;
      uint32_t keep = 0;
      if (room < n_rooms) {
        const g_u64* const lq = (const g_u64*)(brooms + room);
        log = uniform64(lq[0]);
        H = half_of(log, uniform64(lq[1]));
        bc = uniform64(lq[2]);
        keep = uniform32((uint32_t)lq[3]);
      }
      if (!log || !bc || !keep || !H) {  // no such room, or a pass-through room
        st = XYWS_BLC_NO_ROOM;
      } else if (!receiver) {
        st = XYWS_BLC_NOT_RECEIVER;
      } else {
        const g_u64* const cq = (const g_u64*)bc;
        const uint64_t start = uniform64(cq[0]), len = uniform64(cq[1]);
        if ((start == 0 || start == H) && len <= H) w = len;  // (another carry names nothing readable)
        src = log + start;
        st = XYWS_BLC_JOINED;
      }
    }
    const uint64_t send_len = sat_add(base, w);
    if ((st & XYWS_BLC_JOINED) && send_len > out_cap) st |= XYWS_BLC_TRUNCATED;
    if (results && blockIdx.y == 0 && tid == 0) {
      g_u64* const res = (g_u64*)(results + ci);
      res[0] = send_len;
      res[1] = w;
      res[2] = st;
      res[3] = 0;
    }
    if (!w || base >= out_cap) continue;

    // destination positions count from obase (16-byte aligned): out[k] is at olo + k
    g_u8* const obase = (g_u8*)(out & ~15ull);
    const uint64_t olo = out & 15u;
    const uint64_t wlim = sat_add(olo, out_cap);
    const uint64_t P0 = olo + base, P1 = sat_add(P0, w);
    const uint64_t wl = P1 < wlim ? P1 : wlim;
    copy_span(obase, P0, wl, src, (uint64_t)blockIdx.y * BC_STEP, (uint64_t)gridDim.y * BC_STEP, tid);
  }
}

}  // namespace

extern "C" {

int xyws_backlog_streams(xyws_ctx* ctx, const xyws_reasm_conn* dev_reasm, const xyws_reasm_result* dev_reasm_results,
                         const xyws_bcast_conn* dev_bconns, uint64_t n, const xyws_room* dev_rooms,
                         const xyws_room_result* dev_room_results, const xyws_backlog_room* dev_brooms,
                         xyws_backlog_room_result* dev_broom_results, uint64_t n_rooms,
                         const xyws_backlog_conn* dev_jconns, xyws_backlog_result* dev_results, void* stream) {
  if (!ctx) return XYWS_ERR_INVALID;
  if (n && n_rooms && (!dev_reasm || !dev_reasm_results || !dev_bconns)) return XYWS_ERR_INVALID;
  if (n_rooms && (!dev_rooms || !dev_room_results || !dev_brooms)) return XYWS_ERR_INVALID;
  if (n >= UINT32_MAX) return XYWS_ERR_INVALID;  // (a member index is 32 bits, UINT32_MAX is no index)
  if (!n && !n_rooms) return XYWS_OK;
  if (!n_rooms && !(n && dev_jconns)) return XYWS_OK;  // (nothing to fold, nobody to deliver to)
  std::lock_guard<std::mutex> lk(ctx->mu);
  device_guard g(ctx->device);
  if (!g.ok) return XYWS_ERR_HIP;
  if (n_rooms) {
    const uint32_t grid = grid_for(n_rooms, 1, BC_GRID_CAP);
    hipLaunchKernelGGL(k_backlog_fold, dim3(grid), dim3(BL_THREADS), 0, (hipStream_t)stream, dev_reasm,
                       dev_reasm_results, dev_bconns, n, dev_rooms, dev_room_results, dev_brooms, dev_broom_results,
                       n_rooms);
    const int rc = hip_err(hipGetLastError());
    if (rc != XYWS_OK) return rc;
  }
  if (!n || !dev_jconns) return XYWS_OK;
  const dim3 grid = fanout_grid(n, n_rooms != 0, BC_GRID_CAP, BC_BLOCKS_AIM, BC_SLICES_MAX);
  hipLaunchKernelGGL(k_backlog_deliver, grid, dim3(BC_THREADS), 0, (hipStream_t)stream, dev_jconns, n,
                     dev_brooms, n_rooms, dev_results);
  return hip_err(hipGetLastError());
}

// Internal (tests and measurements, no HIP call): the geometry of
// k_backlog_fold and k_backlog_deliver. out: {members per tile of the fold,
// bytes per delivery step, grid cap, wave size}.
int xyws_debug_backlog_geometry(uint64_t out[4]) {
  if (!out) return XYWS_ERR_INVALID;
  out[0] = BL_TILE;
  out[1] = BC_STEP;
  out[2] = BC_GRID_CAP;
  out[3] = BC_WAVE;
  return XYWS_OK;
}

}  // extern "C"

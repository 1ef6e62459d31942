// xyws_backlog.hip — xyws_backlog_streams: each room's newest frames kept in a
// log on the device and copied behind the send bytes of every connection that
// joins (the reference's chat_room::m_recent_messages, deliver_recent_messages
// and join, example/websocket/websocket_chat.cpp:34-47, 89-95). The semantics
// are stated in include/xyws.h; this is how they are computed. Every table row
// is read and written through xyws_rows.h, which names its words.
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
#include "xyws_rows.h"

#define BL_THREADS BC_WIRE_THREADS  // the fold: the one workgroup a room gets (block_scan's size)
#define BL_TILE BL_THREADS          // members per tile of the fold: one per thread

using namespace xyws_internal;
namespace rows = xyws_rows;

namespace {

// The half size of a log (0: no log).
XYWS_DEV uint64_t half_of(uint64_t log, uint64_t log_cap) { return log ? (log_cap >> 1) & ~15ull : 0; }

__global__ void __launch_bounds__(BL_THREADS)
    k_backlog_fold(const xyws_reasm_conn* __restrict__ reasm, const xyws_reasm_result* __restrict__ rres,
                   const xyws_bcast_conn* __restrict__ bconns, uint64_t n, const xyws_room* __restrict__ rooms,
                   const xyws_room_result* __restrict__ room_results, const xyws_backlog_room* __restrict__ brooms,
                   xyws_backlog_room_result* __restrict__ broom_results, uint64_t n_rooms) {
  __shared__ uint64_t s_c[rows::BLC_WORDS];     // the carry as read
  __shared__ uint64_t s_sz[XYWS_BACKLOG_MAX];   // sizes of the last min(keep, N) new frames, in wire order
  __shared__ uint64_t s_w[BL_THREADS / BC_WAVE];
  const uint32_t tid = threadIdx.x;
  for (uint64_t ri = blockIdx.x; ri < n_rooms; ri += gridDim.x) {
    xyws_backlog_room_result* const res = broom_results ? broom_results + ri : nullptr;
    const rows::backlog_room_row lq = rows::load_backlog_room(brooms + ri);
    const uint64_t log = lq.log, H = half_of(log, lq.log_cap), bc = lq.bc;
    uint32_t keep = lq.keep;
    if (!log || !bc || !keep || !H) {  // pass-through: neither the log nor the carry is touched
      if (res && tid == 0) rows::store_backlog_room_result(res, 0, {0, 0}, {0, XYWS_BL_PASSTHROUGH});
      continue;
    }
    if (keep > XYWS_BACKLOG_MAX) keep = XYWS_BACKLOG_MAX;
    if (tid < rows::BLC_WORDS) s_c[tid] = ((const g_u64*)bc)[tid];
    if (tid < XYWS_BACKLOG_MAX) s_sz[tid] = 0;
    __syncthreads();
    const rows::room_result_row rr = rows::load_room_result(room_results + ri);
    const uint64_t wire_len = rr.wire_len, N = rr.nmsgs;
    const uint32_t rst = rr.status;
    const rows::backlog_counts oc = rows::unpack_backlog_counts(s_c[rows::BLC_COUNTS]);
    uint64_t o_start = s_c[rows::BLC_START], o_len = s_c[rows::BLC_LEN];
    uint32_t o_count = oc.count;
    const uint32_t gaps = oc.gaps;
    const uint64_t total = s_c[rows::BLC_TOTAL];
    if (N == 0) {  // 1. no new message: the carry and the log stay, the row reports them
      if (res && tid == 0) rows::store_backlog_room_result(res, o_len, {o_count, 0}, {0, 0});
      __syncthreads();  // (s_c is rewritten by the next room)
      continue;
    }
    uint32_t st = 0;
    {  // 2. the carry
      bool valid = (o_start == 0 || o_start == H) && o_len <= H && o_count <= XYWS_BACKLOG_MAX;
      uint64_t sum = 0;
      for (uint32_t j = 0; valid && j < o_count; j++) sum = sat_add(sum, s_c[rows::BLC_FLEN + j]);
      if (!valid || sum != o_len) {
        st |= XYWS_BL_BAD_CARRY;
        o_start = o_len = 0;
        o_count = 0;
      }
    }
    const rows::room_row rq = rows::load_room(rooms + ri);
    const uint64_t members = rq.members, nm = rq.n_members, wire = rq.wire, wire_cap = rq.wire_cap;
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
            if (frame_of(rows::row_at<const xyws_message>(m.msgs, r), m, 0, 0, f)) {
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
          if (!frame_of(rows::row_at<const xyws_message>(m.msgs, r), m, 0, 0, f)) continue;
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
        const uint64_t sz = s_c[rows::BLC_FLEN + j];
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
    if (tid < rows::BLC_WORDS) {  // (one word per thread, the reserved ones zero)
      uint64_t w = 0;
      if (tid == rows::BLC_START) w = target;
      else if (tid == rows::BLC_LEN) w = T;
      else if (tid == rows::BLC_COUNTS) w = rows::pack_backlog_counts({count, gaps + (gap ? 1u : 0u)});
      else if (tid == rows::BLC_TOTAL) w = total + n_new;
      else if (tid >= rows::BLC_FLEN && tid < rows::BLC_FLEN + XYWS_BACKLOG_MAX) {
        const uint32_t i = tid - rows::BLC_FLEN;
        if (i < n_old) w = s_c[rows::BLC_FLEN + (o_count - n_old) + i];
        else if (i < count) w = s_sz[(uint32_t)K - n_new + (i - n_old)];
      }
      ((g_u64*)bc)[tid] = w;
    }
    if (res && tid == 0) rows::store_backlog_room_result(res, T, {count, n_new}, {dropped, st});
    __syncthreads();  // (s_c and s_sz are rewritten by the next room)
  }
}

__global__ void __launch_bounds__(BC_THREADS)
    k_backlog_deliver(const xyws_backlog_conn* __restrict__ jconns, uint64_t n,
                      const xyws_backlog_room* __restrict__ brooms, uint64_t n_rooms,
                      xyws_backlog_result* __restrict__ results) {
  const uint32_t tid = threadIdx.x;
  for (uint64_t ci = blockIdx.x; ci < n; ci += gridDim.x) {
    const rows::backlog_conn_row jq = rows::load_backlog_conn(jconns + ci);
    const uint64_t out = jq.out, out_cap = jq.out_cap, room = jq.join.room;
    const uint32_t fl = jq.join.flags;
    uint64_t base = 0;
    bool receiver = true;
    if (jq.reply) {
      const rows::reply_result_row rp = rows::load_reply_result<true>((const xyws_reply_result*)jq.reply);
      base = rp.reply_len;
      if (rp.status & (XYWS_RPL_CLOSED | XYWS_RPL_OVERFLOW)) receiver = false;
    }
    if (jq.bcast) {
      const rows::bcast_result_row bp = rows::load_bcast_result((const xyws_bcast_result*)jq.bcast);
      base = bp.send_len;
      if (bp.status & XYWS_BC_NOT_RECEIVER) receiver = false;
    }
    uint32_t st = 0;
    uint64_t w = 0, src = 0;
    if (fl & XYWS_BL_JOIN) {
      uint64_t log = 0, H = 0, bc = 0;
      uint32_t keep = 0;
      if (room < n_rooms) {
        const rows::backlog_room_row lq = rows::load_backlog_room(brooms + room);
        log = lq.log;
        H = half_of(log, lq.log_cap);
        bc = lq.bc;
        keep = lq.keep;
      }
      if (!log || !bc || !keep || !H) {  // no such room, or a pass-through room
        st = XYWS_BLC_NO_ROOM;
      } else if (!receiver) {
        st = XYWS_BLC_NOT_RECEIVER;
      } else {
        const rows::backlog_span cq = rows::load_backlog_span((const xyws_backlog_carry*)bc);
        const uint64_t start = cq.start, len = cq.len;
        if ((start == 0 || start == H) && len <= H) w = len;  // (another carry names nothing readable)
        src = log + start;
        st = XYWS_BLC_JOINED;
      }
    }
    const uint64_t send_len = sat_add(base, w);
    if ((st & XYWS_BLC_JOINED) && send_len > out_cap) st |= XYWS_BLC_TRUNCATED;
    if (results && blockIdx.y == 0 && tid == 0) {
      rows::store_backlog_result(results + ci, send_len, w, st);
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

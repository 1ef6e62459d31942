// xyws_hold.hip — xyws_hold_streams: the message a recv boundary cut, kept on
// the device between sweeps and handed to xyws_broadcast_streams whole in the
// sweep that completes it (the reference's chat session reads a message to
// its end before chat_room::deliver, example/websocket/websocket_chat.cpp:
// 177-200). The semantics are stated in include/xyws.h; this is how they are
// computed.
//
// As in k_reply_streams and k_reasm_streams one wave (a 64-thread workgroup)
// takes one connection, connections are grid-strided, no workgroup talks to
// another, nothing spins, there are no atomics. Per connection:
//   1. the state walk is wave-uniform, in scalar registers: it reads the table
//      entries, the reassembly row, the hold carry, record 0 and record
//      nmsgs - 1, and leaves the new carry, the result bits, the delivered
//      record (if any) and at most two byte ranges to copy: the part appended
//      to the held message, and the message open at the end that begins a hold;
//   2. the copies, by the whole wave in 16-byte lines (copy_span,
//      xyws_lines.h; neighbouring areas may share a range's first and last
//      line);
//   3. the record row goes to the view one record per lane, strided, out_off
//      moved by hold_cap; record 0 is the delivered message when there is one;
//   4. lane 0 writes the carry, the view entry, the view row and the result.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>

#include "xyws.h"
#include "xyws_device.h"
#include "xyws_ctx.h"
#include "xyws_frameops.h"
#include "xyws_lines.h"

#define HOLD_LANES 64u      // lanes per connection: one wave
#define HOLD_LINE 16u       // bytes a lane writes per copy step
#define HOLD_STEP (HOLD_LINE * HOLD_LANES)  // bytes a connection's wave writes per step
#define HOLD_GRID_CAP 8192u // 256 CUs x 32 one-wave workgroups; further connections are grid-strided

using namespace xyws_internal;

namespace {

// L bytes from address S to address D, by the whole wave. The caller has
// checked both ranges; they do not overlap (message bytes and hold).
XYWS_DEV void copy_range(uint64_t D, uint64_t S, uint64_t L, uint32_t lane) {
  if (L) copy_span((g_u8*)(D & ~15ull), D & 15u, (D & 15u) + L, S, 0, HOLD_STEP, lane);
}

__global__ void __launch_bounds__(HOLD_LANES)
    k_hold_streams(const xyws_reasm_conn* __restrict__ reasm, const xyws_reasm_result* __restrict__ rres,
                   const xyws_hold_conn* __restrict__ hold, uint64_t n, xyws_reasm_conn* __restrict__ view,
                   xyws_reasm_result* __restrict__ vres, xyws_hold_result* __restrict__ results) {
  static_assert(sizeof(xyws_hold_conn) == 32 && sizeof(xyws_hold_carry) == 32 && sizeof(xyws_hold_result) == 32 &&
                    offsetof(xyws_hold_conn, hc) == 8 && offsetof(xyws_hold_conn, vmsgs) == 16 &&
                    offsetof(xyws_hold_conn, vmsg_cap) == 24 && offsetof(xyws_hold_carry, held) == 8 &&
                    offsetof(xyws_hold_carry, nframes) == 16 && offsetof(xyws_hold_carry, status) == 24 &&
                    offsetof(xyws_hold_carry, opcode) == 28 && offsetof(xyws_hold_result, delivered_len) == 8 &&
                    offsetof(xyws_hold_result, status) == 16 && sizeof(xyws_message) == 40 &&
                    offsetof(xyws_message, status) == 32 && offsetof(xyws_message, opcode) == 36 &&
                    sizeof(xyws_reasm_conn) == 64 && sizeof(xyws_reasm_result) == 32 &&
                    offsetof(xyws_reasm_result, status) == 20,
                "layouts");
  const uint32_t lane = threadIdx.x;
  for (uint64_t ci = blockIdx.x; ci < n; ci += gridDim.x) {
    const g_u64* const rq = (const g_u64*)(reasm + ci);
    const g_u64* const ar = (const g_u64*)(rres + ci);
    const g_u64* const hq = (const g_u64*)(hold + ci);
    g_u64* const vq = (g_u64*)(view + ci);
    g_u64* const vr = (g_u64*)(vres + ci);
    g_u64* const res = results ? (g_u64*)(results + ci) : nullptr;
    const uint64_t out = uniform64(rq[0]);
    const uint64_t hold_cap = uniform64(hq[0]);
    g_u64* const hc = (g_u64*)uniform64(hq[1]);
    const uint64_t H = (hold_cap / 2) & ~15ull;

    // 0. pass-through: the inputs verbatim
    if (!out || !hc || !H) {
      if (lane < 8) vq[lane] = rq[lane];
      if (lane < 4) vr[lane] = ar[lane];
      if (res && lane < 4) res[lane] = lane == 2 ? (uint64_t)XYWS_HOLD_PASSTHROUGH : 0;
      continue;
    }

    const uint64_t out_cap = uniform64(rq[1]);
    const uint64_t mcp = uniform64(rq[2]);
    const uint64_t msgs = uniform64(rq[3]);
    const uint64_t msg_cap = msgs ? uniform64(rq[4]) : 0;
    const uint64_t a0 = uniform64(ar[0]), nmsgs = uniform64(ar[1]), a2 = uniform64(ar[2]), a3 = uniform64(ar[3]);
    const uint32_t rst = (uint32_t)(a2 >> 32);
    const uint64_t vmsgs = uniform64(hq[2]);
    const uint64_t vmsg_cap = vmsgs ? uniform64(hq[3]) : 0;
    const uint64_t s = nmsgs < msg_cap ? nmsgs : msg_cap;
    const uint64_t vs = s < vmsg_cap ? s : vmsg_cap;
    const uint64_t hbase = out - hold_cap;

    // the carry, canonical: without ACTIVE only the LOST bit counts
    uint64_t c_start = uniform64(hc[0]), c_held = uniform64(hc[1]), c_nfr = uniform64(hc[2]);
    const uint64_t c3 = uniform64(hc[3]);
    uint32_t c_st = (uint32_t)c3, c_op = (uint32_t)(c3 >> 32) & 0xFFu;
    if (c_st & XYWS_HOLD_ACTIVE) {
      c_st = XYWS_HOLD_ACTIVE;
    } else {
      c_st &= XYWS_HOLD_LOST;
      c_start = c_held = c_nfr = 0;
      c_op = 0;
    }
    auto lose = [&]() {
      c_st = XYWS_HOLD_LOST;
      c_start = c_held = c_nfr = 0;
      c_op = 0;
    };
    auto clear = [&]() {
      c_st = 0;
      c_start = c_held = c_nfr = 0;
      c_op = 0;
    };

    // 1. the walk (wave-uniform)
    uint32_t st = 0;
    uint64_t cpA_D = 0, cpA_S = 0, cpA_L = 0;  // the part appended to the held message
    uint64_t cpB_D = 0, cpB_S = 0, cpB_L = 0;  // the message open at the end
    bool delivered = false;
    uint64_t d_start = 0, d_len = 0, d_nfr = 0, d_w4 = 0;
    if (rst & XYWS_RSM_OVERFLOW) {  // 2.
      if (c_st & XYWS_HOLD_ACTIVE) st |= XYWS_HOLD_DROPPED;
      lose();
    } else {
      uint64_t r0n = 0, r0o = 0, r0l = 0, r0w = 0;  // record 0: nframes, out_off, length, status | opcode << 32
      if (s) {
        const g_u64* const rec = (const g_u64*)msgs;
        r0n = uniform64(rec[1]);
        r0o = uniform64(rec[2]);
        r0l = uniform64(rec[3]);
        r0w = uniform64(rec[4]);
      }
      const uint32_t r0s = (uint32_t)r0w;
      const bool has0 = s && (r0s & XYWS_MSG_CONTINUED);
      if ((c_st & XYWS_HOLD_ACTIVE) && !has0) {  // 5.: its record was not stored
        st |= XYWS_HOLD_DROPPED;
        lose();
      }
      if (has0) {  // 3.
        if (c_st & XYWS_HOLD_ACTIVE) {
          if ((c_start != 0 && c_start != H) || c_held > H || (r0s & XYWS_MSG_TRUNCATED) ||
              !in_range(r0o, r0l, out_cap)) {
            st |= XYWS_HOLD_DROPPED;
            lose();
          } else if (r0l > H - c_held) {
            st |= XYWS_HOLD_DROPPED | XYWS_HOLD_TOO_LONG;
            lose();
          } else {
            cpA_D = hbase + c_start + c_held;
            cpA_S = out + r0o;
            cpA_L = r0l;
            c_held += r0l;
            c_nfr += r0n;
          }
        } else if (!(c_st & XYWS_HOLD_LOST)) {  // attached mid-message
          st |= XYWS_HOLD_DROPPED;
          lose();
        }
        if (r0s & XYWS_MSG_COMPLETE) {
          if (c_st & XYWS_HOLD_ACTIVE) {
            delivered = true;
            d_start = c_start;
            d_len = c_held;
            d_nfr = c_nfr;
            d_w4 = (uint64_t)(r0s & ~XYWS_MSG_CONTINUED) | ((uint64_t)c_op << 32);
            st |= XYWS_HOLD_DELIVERED;
          }
          clear();
        } else if (r0s & XYWS_MSG_INTERRUPTED) {
          clear();
        }
      }
      // 4. the message open at the end
      if ((rst & XYWS_RSM_OPEN) && nmsgs && nmsgs - 1 < s) {
        uint64_t ln = r0n, lo = r0o, ll = r0l, lw = r0w;
        if (nmsgs > 1) {
          const g_u64* const rec = (const g_u64*)(msgs + 40ull * (nmsgs - 1));
          ln = uniform64(rec[1]);
          lo = uniform64(rec[2]);
          ll = uniform64(rec[3]);
          lw = uniform64(rec[4]);
        }
        const uint32_t ls = (uint32_t)lw;
        if (!(ls & (XYWS_MSG_CONTINUED | XYWS_MSG_COMPLETE | XYWS_MSG_INTERRUPTED))) {
          if ((ls & XYWS_MSG_TRUNCATED) || !in_range(lo, ll, out_cap)) {
            st |= XYWS_HOLD_DROPPED;
            lose();
          } else if (ll > H) {
            st |= XYWS_HOLD_DROPPED | XYWS_HOLD_TOO_LONG;
            lose();
          } else {
            const uint64_t target = delivered && d_start == 0 ? H : 0;
            cpB_D = hbase + target;
            cpB_S = out + lo;
            cpB_L = ll;
            c_st = XYWS_HOLD_ACTIVE;
            c_start = target;
            c_held = ll;
            c_nfr = ln;
            c_op = (uint32_t)(lw >> 32) & 0xFFu;
          }
        }
      }
      // 5. after the walk
      if (rst & XYWS_RSM_OPEN) {
        if (!(c_st & (XYWS_HOLD_ACTIVE | XYWS_HOLD_LOST))) {
          st |= XYWS_HOLD_DROPPED;
          lose();
        }
      } else {
        clear();
      }
    }

    // 2. the copies
    copy_range(cpA_D, cpA_S, cpA_L, lane);
    copy_range(cpB_D, cpB_S, cpB_L, lane);

    // 3. the record row
    for (uint64_t j = lane; j < vs; j += HOLD_LANES) {
      const g_u64* const rec = (const g_u64*)(msgs + 40ull * j);
      g_u64* const vrec = (g_u64*)(vmsgs + 40ull * j);
      uint64_t w0 = rec[0], w1 = rec[1], w2 = rec[2] + hold_cap, w3 = rec[3], w4 = rec[4];
      if (j == 0 && delivered) {
        w0 = 0;
        w1 = d_nfr;
        w2 = d_start;
        w3 = d_len;
        w4 = d_w4;
      }
      vrec[0] = w0;
      vrec[1] = w1;
      vrec[2] = w2;
      vrec[3] = w3;
      vrec[4] = w4;
    }

    // 4. the carry, the view entry, the view row, the result
    if (lane == 0) {
      hc[0] = c_start;
      hc[1] = c_held;
      hc[2] = c_nfr;
      hc[3] = (uint64_t)c_st | ((uint64_t)c_op << 32);
      vq[0] = hbase;
      vq[1] = hold_cap + out_cap;
      vq[2] = mcp;
      vq[3] = vmsgs;
      vq[4] = msg_cap < vmsg_cap ? msg_cap : vmsg_cap;
      vq[5] = vq[6] = vq[7] = 0;
      vr[0] = a0;
      vr[1] = nmsgs;
      vr[2] = a2 | (s > vmsg_cap ? (uint64_t)XYWS_RSM_MSG_CAP << 32 : 0);
      vr[3] = a3;
      if (res) {
        res[0] = c_held;
        res[1] = delivered ? d_len : 0;
        res[2] = st | (c_st & (XYWS_HOLD_ACTIVE | XYWS_HOLD_LOST));
        res[3] = 0;
      }
    }
  }
}

}  // namespace

extern "C" {

int xyws_hold_streams(xyws_ctx* ctx, const xyws_reasm_conn* dev_reasm, const xyws_reasm_result* dev_reasm_results,
                      const xyws_hold_conn* dev_hold, uint64_t n, xyws_reasm_conn* dev_view,
                      xyws_reasm_result* dev_view_results, xyws_hold_result* dev_results, void* stream) {
  if (!ctx || (n && (!dev_reasm || !dev_reasm_results || !dev_hold || !dev_view || !dev_view_results)))
    return XYWS_ERR_INVALID;
  if (!n) return XYWS_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  device_guard g(ctx->device);
  if (!g.ok) return XYWS_ERR_HIP;
  const uint32_t grid = grid_for(n, 1, HOLD_GRID_CAP);
  hipLaunchKernelGGL(k_hold_streams, dim3(grid), dim3(HOLD_LANES), 0, (hipStream_t)stream, dev_reasm,
                     dev_reasm_results, dev_hold, n, dev_view, dev_view_results, dev_results);
  return hip_err(hipGetLastError());
}

// Internal (tests and measurements, no HIP call): the geometry of
// k_hold_streams. out: {lanes per connection, bytes per line, bytes per copy
// step, grid cap}.
int xyws_debug_hold_geometry(uint64_t out[4]) {
  if (!out) return XYWS_ERR_INVALID;
  out[0] = HOLD_LANES;
  out[1] = HOLD_LINE;
  out[2] = HOLD_STEP;
  out[3] = HOLD_GRID_CAP;
  return XYWS_OK;
}

}  // extern "C"

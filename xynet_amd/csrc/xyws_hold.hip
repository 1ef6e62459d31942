// xyws_hold.hip — xyws_hold_streams: the message a recv boundary cut, kept on
// the device between sweeps and handed to xyws_broadcast_streams whole in the
// sweep that completes it (the reference's chat session reads a message to
// its end before chat_room::deliver, example/websocket/websocket_chat.cpp:
// 177-200). The semantics are stated in include/xyws.h; this is how they are
// computed. Every table row is read and written through xyws_rows.h, which
// names its words.
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
#include "xyws_rows.h"

#define HOLD_LANES 64u      // lanes per connection: one wave
#define HOLD_LINE 16u       // bytes a lane writes per copy step
#define HOLD_STEP (HOLD_LINE * HOLD_LANES)  // bytes a connection's wave writes per step
#define HOLD_GRID_CAP 8192u // 256 CUs x 32 one-wave workgroups; further connections are grid-strided

using namespace xyws_internal;
namespace rows = xyws_rows;

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
  const uint32_t lane = threadIdx.x;
  for (uint64_t ci = blockIdx.x; ci < n; ci += gridDim.x) {
    // (each row named once: with `view + ci` spelled at both of its uses the per-lane addresses of the
    // pass-through are hoisted out of this loop, and the kernel takes 75 VGPRs for 71: 6 waves for 7)
    const xyws_reasm_conn* const rp = reasm + ci;
    const xyws_reasm_result* const ap = rres + ci;
    const xyws_hold_conn* const hp = hold + ci;
    xyws_reasm_conn* const vq = view + ci;
    xyws_reasm_result* const vr = vres + ci;
    xyws_hold_result* const res = results ? results + ci : nullptr;
    const rows::reasm_conn_row rq = rows::load_reasm_conn<true>(rp);
    const rows::hold_conn_row hq = rows::load_hold_conn(hp);
    const uint64_t out = rq.out, hold_cap = hq.hold_cap;
    xyws_hold_carry* const hc = (xyws_hold_carry*)hq.hc;
    const uint64_t H = (hold_cap / 2) & ~15ull;

    // 0. pass-through: the inputs verbatim
    if (!out || !hc || !H) {
      rows::copy_row(vq, rp, lane);
      rows::copy_row(vr, ap, lane);
      if (res) rows::store_hold_status(res, XYWS_HOLD_PASSTHROUGH, lane);
      continue;
    }

    const uint64_t out_cap = rq.out_cap, msgs = rq.msgs, msg_cap = rq.msg_cap;
    const rows::reasm_result_row ar = rows::load_reasm_result<true>(ap);
    const uint64_t nmsgs = ar.nmsgs;
    const uint32_t rst = ar.counts.status;
    const uint64_t vmsgs = hq.vmsgs, vmsg_cap = hq.vmsg_cap;
    const uint64_t s = nmsgs < msg_cap ? nmsgs : msg_cap;
    const uint64_t vs = s < vmsg_cap ? s : vmsg_cap;
    const uint64_t hbase = out - hold_cap;

    // the carry, canonical: without ACTIVE only the LOST bit counts
    const rows::hold_carry_row c = rows::load_hold_carry(hc);
    uint64_t c_start = c.start, c_held = c.held, c_nfr = c.nframes;
    uint32_t c_st = c.state.status, c_op = c.state.opcode;
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
      rows::message_row r0 = {0, 0, 0, 0, 0};  // record 0
      if (s) r0 = rows::load_message<true>(rows::row_at<const xyws_message>(msgs, 0));
      const uint64_t r0n = r0.nframes, r0o = r0.out_off, r0l = r0.length;
      const uint32_t r0s = rows::unpack_message_meta(r0.meta).status;
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
            d_w4 = rows::pack_message_meta({r0s & ~XYWS_MSG_CONTINUED, c_op});
            st |= XYWS_HOLD_DELIVERED;
          }
          clear();
        } else if (r0s & XYWS_MSG_INTERRUPTED) {
          clear();
        }
      }
      // 4. the message open at the end
      if ((rst & XYWS_RSM_OPEN) && nmsgs && nmsgs - 1 < s) {
        rows::message_row rl = r0;  // the last record
        if (nmsgs > 1) rl = rows::load_message<true>(rows::row_at<const xyws_message>(msgs, nmsgs - 1));
        const uint64_t ln = rl.nframes, lo = rl.out_off, ll = rl.length;
        const rows::message_meta lm = rows::unpack_message_meta(rl.meta);
        const uint32_t ls = lm.status;
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
            c_op = lm.opcode;
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
      rows::message_row rec = rows::load_message<false>(rows::row_at<const xyws_message>(msgs, j));
      rec.out_off += hold_cap;
      if (j == 0 && delivered) rec = {0, d_nfr, d_start, d_len, d_w4};
      rows::store_message(rows::row_at<xyws_message>(vmsgs, j), rec);
    }

    // 4. the carry, the view entry, the view row, the result
    if (lane == 0) {
      rows::store_hold_carry(hc, {c_start, c_held, c_nfr, {c_st, c_op}});
      rows::store_reasm_conn(vq, {hbase, hold_cap + out_cap, rq.mc, vmsgs, msg_cap < vmsg_cap ? msg_cap : vmsg_cap});
      rows::store_reasm_result(vr, {ar.out_len, nmsgs, {ar.counts.completed, rst | (s > vmsg_cap ? XYWS_RSM_MSG_CAP : 0u)},
                                           ar.reserved});
      if (res) rows::store_hold_result(res, c_held, delivered ? d_len : 0, st | (c_st & (XYWS_HOLD_ACTIVE | XYWS_HOLD_LOST)));
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

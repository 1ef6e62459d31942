// xyws_broadcast.hip — xyws_broadcast_streams: a sweep's messages framed once
// per room and copied to every member's send range (the reference's
// chat_room::deliver and chat_session::writer,
// example/websocket/websocket_chat.cpp:89-101, 148-175, run once per message
// and member). The semantics are stated in include/xyws.h; this is how they
// are computed. Every table row is read and written through xyws_rows.h, which
// names its words.
//
// Two launches, the room result rows the hand-over between them. No workgroup
// waits for another inside a launch, nothing spins, there are no atomics.
//
// k_room_wire: one workgroup per room, rooms grid-strided. The members are
// taken in tiles of BC_TILE, one member per thread:
//   1. the thread loads its member and its gate (bounds-checked index;
//      load_member, xyws_room.h), walks the stored records, tests each
//      (frame_of) and sums the frame sizes header + head + message;
//   2. a workgroup scan gives each member's offset in the wire; the offsets
//      and what the copy needs of a member go to LDS; the running sum is
//      carried between tiles in a register;
//   3. the copy phase covers the tile's wire range in 16-byte lines
//      (xyws_lines.h), one line per thread per step: item_at finds the member
//      of the line's first byte, the member's records are walked to the frame
//      that holds it, and header, head and message bytes are composed in
//      registers.
// The result row is written once, after the last tile.
//
// k_room_fanout: blockIdx.x strides over the connections, blockIdx.y over
// BC_STEP-byte chunks of the connection's destination range, so a few
// connections with a long wire still fill the machine (the host cannot know
// the wire lengths: the chunks are strided, whatever the length). The copy
// loop is the kernel's own, built from the line primitives (xyws_lines.h): it
// is copy_span's loop, kept here because the shared one measured slower in
// this kernel. The y == 0 workgroup writes the connection's result row.
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

#define BC_TILE BC_WIRE_THREADS  // members per tile of the wire build: one per thread

using namespace xyws_internal;
namespace rows = xyws_rows;

namespace {

__global__ void __launch_bounds__(BC_WIRE_THREADS)
    k_room_wire(const xyws_reasm_conn* __restrict__ reasm, const xyws_reasm_result* __restrict__ rres,
                const xyws_bcast_conn* __restrict__ bconns, uint64_t n, const xyws_room* __restrict__ rooms,
                xyws_room_result* __restrict__ room_results, uint64_t n_rooms, uint32_t flags, uint32_t enc_opts) {
  __shared__ uint64_t s_off[BC_TILE + 1];  // members: start in the wire (and the end after the last)
  __shared__ uint64_t s_msgs[BC_TILE], s_gate[BC_TILE], s_out[BC_TILE], s_ocap[BC_TILE], s_head[BC_TILE],
      s_hlen[BC_TILE];
  __shared__ uint32_t s_stored[BC_TILE];
  __shared__ uint64_t s_w[BC_WIRE_THREADS / BC_WAVE];
  const uint32_t tid = threadIdx.x;
  for (uint64_t ri = blockIdx.x; ri < n_rooms; ri += gridDim.x) {
    const rows::room_row rq = rows::load_room(rooms + ri);
    const uint64_t members = rq.members, nm = rq.n_members, wire = rq.wire, wire_cap = rq.wire_cap;
    g_u8* const wbase = (g_u8*)(wire & ~15ull);
    const uint64_t wlo = wire & 15u;
    const uint64_t wlim = sat_add(wlo, wire_cap);

    uint64_t wpos = 0;                                       // the wire so far (uniform)
    uint32_t c_msgs = 0, c_skip = 0, c_recv = 0, c_st = 0;   // this thread's members
    for (uint64_t base = 0; base < nm; base += BC_TILE) {
      // 1. this thread's member
      member m = {0, 0, 0, 0, 0, 0, 0};
      uint64_t size = 0;
      if (base + tid < nm) {
        const uint64_t ci = ((const XYWS_GLOBAL uint32_t*)members)[base + tid];
        if (ci >= n) {
          c_st |= XYWS_ROOM_BAD_MEMBER;
        } else {
          bool receiver, over_cap;
          load_member(reasm, rres, bconns, ci, m, receiver, over_cap);
          if (over_cap) c_st |= XYWS_ROOM_MSG_CAP;
          c_recv += receiver ? 1u : 0u;
#pragma unroll 1
          for (uint32_t r = 0; r < m.stored; r++) {
            frame_info f;
            if (frame_of(rows::row_at<const xyws_message>(m.msgs, r), m, flags, enc_opts, f)) {
              size += f.h + m.head_len + f.len;
              c_msgs++;
            } else {
              c_skip++;
            }
          }
        }
      }
      // 2. offsets in the wire
      uint64_t total;
      const uint64_t incl = block_scan(size, tid, s_w, total);
      const uint64_t o0 = wpos, o1 = wpos + total;
      s_off[tid] = o0 + (incl - size);
      s_msgs[tid] = m.msgs;
      s_gate[tid] = m.gate;
      s_out[tid] = m.out;
      s_ocap[tid] = m.out_cap;
      s_head[tid] = m.head;
      s_hlen[tid] = m.head_len;
      s_stored[tid] = size ? m.stored : 0u;  // (a member without a frame is not walked)
      if (tid == 0) s_off[BC_TILE] = o1;
      __syncthreads();

      // 3. the tile's bytes [o0, o1)
      const uint64_t P0 = wlo + o0, P1 = wlo + o1;
      const uint64_t wl = P1 < wlim ? P1 : wlim;
      if (wl > P0) {
        for (uint64_t A = ((P0 >> 4) + tid) << 4; A < wl; A += (uint64_t)BC_LINE * BC_WIRE_THREADS) {
          const uint64_t s = A > P0 ? A : P0, e = A + 16 < P1 ? A + 16 : P1;
          uint64_t q = s - wlo;
          uint32_t i = item_at(s_off, BC_TILE, q);  // the member that holds byte q (q < o1)
          bytes16 acc = {0, 0};
          uint32_t a = (uint32_t)(s - A);
          const uint32_t ae = (uint32_t)(e - A);
          while (a < ae && i < BC_TILE) {
            member k;
            k.msgs = s_msgs[i];
            k.gate = s_gate[i];
            k.out = s_out[i];
            k.out_cap = s_ocap[i];
            k.head = s_head[i];
            k.head_len = s_hlen[i];
            k.stored = s_stored[i];
            uint64_t fo = s_off[i];  // the start of the frame under test
#pragma unroll 1
            for (uint32_t r = 0; r < k.stored && a < ae; r++) {
              frame_info f;
              if (!frame_of(rows::row_at<const xyws_message>(k.msgs, r), k, flags, enc_opts, f)) continue;
              const uint64_t fsz = f.h + k.head_len + f.len;
              if (fo + fsz > q) {
                uint64_t rr = q - fo;
                if (rr < f.h) {  // header bytes rr.. at line offset a
                  const uint32_t nb = f.h - (uint32_t)rr < ae - a ? f.h - (uint32_t)rr : ae - a;
                  const bytes16 hd = {(uint64_t)f.hw[0] | ((uint64_t)f.hw[1] << 32), (uint64_t)f.hw[2]};
                  add_bytes(acc, a, q, shr_bytes(hd, (uint32_t)rr), nb);
                  rr += nb;
                }
                if (a < ae && rr < f.h + k.head_len) {  // head bytes
                  const uint64_t left = f.h + k.head_len - rr;
                  const uint32_t nb = left < ae - a ? (uint32_t)left : ae - a;
                  add_bytes(acc, a, q, load_bytes(k.head + (rr - f.h), nb), nb);
                  rr += nb;
                }
                if (a < ae && rr < fsz) {  // message bytes
                  const uint64_t left = fsz - rr;
                  const uint32_t nb = left < ae - a ? (uint32_t)left : ae - a;
                  add_bytes(acc, a, q, load_bytes(k.out + f.off + (rr - f.h - k.head_len), nb), nb);
                }
              }
              fo += fsz;
            }
            i++;
          }
          put_line(wbase, A, s, e, wlo, wlim, acc);
        }
      }
      wpos = o1;
      __syncthreads();  // (LDS is rewritten by the next tile)
    }

    // the result row: the threads' counts summed
    uint64_t t0, t1;
    block_scan(rows::pack_room_counts({c_msgs, c_skip}), tid, s_w, t0);  // (both counts summed as one word)
    block_scan((uint64_t)c_recv, tid, s_w, t1);
    uint32_t st = c_st;
#pragma unroll
    for (uint32_t d = 1; d < BC_WAVE; d <<= 1) st |= (uint32_t)__shfl_xor((int)st, (int)d);
    if ((tid & (BC_WAVE - 1u)) == 0) s_w[tid / BC_WAVE] = st;
    __syncthreads();
    if (tid == 0) {
      st = 0;
      for (uint32_t w = 0; w < BC_WIRE_THREADS / BC_WAVE; w++) st |= (uint32_t)s_w[w];
      if (wpos > wire_cap) st |= XYWS_ROOM_TRUNCATED;
      rows::store_room_result(room_results + ri, wpos, t0, {(uint32_t)t1, st});
    }
    __syncthreads();  // (s_w is reused by the next room)
  }
}

__global__ void __launch_bounds__(BC_THREADS) k_room_fanout(const xyws_bcast_conn* __restrict__ bconns, uint64_t n,
                                                            const xyws_room* __restrict__ rooms,
                                                            const xyws_room_result* __restrict__ room_results,
                                                            uint64_t n_rooms, xyws_bcast_result* __restrict__ results) {
  const uint32_t tid = threadIdx.x;
  for (uint64_t ci = blockIdx.x; ci < n; ci += gridDim.x) {
    const rows::bcast_conn_row bq = rows::load_bcast_conn<true>(bconns + ci);
    const uint64_t out = bq.out, out_cap = bq.out_cap, room = bq.room;
    uint64_t base = 0;
    uint32_t pst = 0;
    if (bq.reply) {
      const rows::reply_result_row rp = rows::load_reply_result<true>((const xyws_reply_result*)bq.reply);
      base = rp.reply_len;
      pst = rp.status;
    }
    uint32_t st = 0;
    uint64_t w = 0, wire = 0;
    if (room >= n_rooms) {  // (XYWS_ROOM_NONE is above every index)
      st = XYWS_BC_NO_ROOM;
    } else if (pst & (XYWS_RPL_CLOSED | XYWS_RPL_OVERFLOW)) {
      st = XYWS_BC_NOT_RECEIVER;
    } else {
      const rows::room_row rq = rows::load_room(rooms + room);
      wire = rq.wire;
      const uint64_t wire_cap = rq.wire_cap, wire_len = rows::load_room_result(room_results + room).wire_len;
      w = wire_len < wire_cap ? wire_len : wire_cap;
    }
    const uint64_t send_len = sat_add(base, w);
    if (send_len > out_cap) st |= XYWS_BC_TRUNCATED;
    if (results && blockIdx.y == 0 && tid == 0) {
      rows::store_bcast_result(results + ci, send_len, w, st);
    }
    if (!w || base >= out_cap) continue;

    // destination positions count from obase (16-byte aligned): out[k] is at olo + k
    g_u8* const obase = (g_u8*)(out & ~15ull);
    const uint64_t olo = out & 15u;
    const uint64_t wlim = sat_add(olo, out_cap);
    const uint64_t P0 = olo + base, P1 = sat_add(P0, w);
    const uint64_t wl = P1 < wlim ? P1 : wlim;
    // (not copy_span: the shared loop measured slower here, profiles/room_rate.jsonl and DESIGN.md 4.9)
    const uint64_t A00 = (P0 >> 4) << 4;
    for (uint64_t A0 = A00 + (uint64_t)blockIdx.y * BC_STEP; A0 < wl; A0 += (uint64_t)gridDim.y * BC_STEP) {
      const uint64_t A = A0 + 16u * tid;
      if (A >= wl) break;
      if (A >= P0 && A + 16 <= wl) {  // a whole line inside the range: wire bytes A - P0 ..
        store_line(obase, A, load_bytes(wire + (A - P0), 16));
      } else {  // the range's first or last line: its own bytes only (put_line's rule with lo = P0, lim = wl)
        const uint64_t s = A > P0 ? A : P0, e = A + 16 < wl ? A + 16 : wl;
        store_edge(obase, A, s, e, shl_bytes(load_bytes(wire + (s - P0), (uint32_t)(e - s)), (uint32_t)(s - A)));
      }
    }
  }
}

}  // namespace

extern "C" {

int xyws_broadcast_streams(xyws_ctx* ctx, const xyws_reasm_conn* dev_reasm, const xyws_reasm_result* dev_reasm_results,
                           const xyws_bcast_conn* dev_bconns, uint64_t n, const xyws_room* dev_rooms,
                           xyws_room_result* dev_room_results, uint64_t n_rooms, uint8_t flags, uint32_t enc_opts,
                           xyws_bcast_result* dev_results, void* stream) {
  if (!ctx || (n && (!dev_reasm || !dev_reasm_results || !dev_bconns))) return XYWS_ERR_INVALID;
  if (n_rooms && (!dev_rooms || !dev_room_results)) return XYWS_ERR_INVALID;
  if (n >= UINT32_MAX) return XYWS_ERR_INVALID;            // (a member index is 32 bits, UINT32_MAX is no index)
  if (flags & XYWS_FLAG_HAS_MASK) return XYWS_ERR_INVALID;  // server role only
  if (enc_opts & ~XYWS_ENC_FRAME_OPCODE) return XYWS_ERR_INVALID;
  if (!n) return XYWS_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  device_guard g(ctx->device);
  if (!g.ok) return XYWS_ERR_HIP;
  if (n_rooms) {
    const uint32_t grid = grid_for(n_rooms, 1, BC_GRID_CAP);
    hipLaunchKernelGGL(k_room_wire, dim3(grid), dim3(BC_WIRE_THREADS), 0, (hipStream_t)stream, dev_reasm,
                       dev_reasm_results, dev_bconns, n, dev_rooms, dev_room_results, n_rooms, (uint32_t)flags, enc_opts);
    const int rc = hip_err(hipGetLastError());
    if (rc != XYWS_OK) return rc;
  }
  const dim3 grid = fanout_grid(n, n_rooms != 0, BC_GRID_CAP, BC_BLOCKS_AIM, BC_SLICES_MAX);
  hipLaunchKernelGGL(k_room_fanout, grid, dim3(BC_THREADS), 0, (hipStream_t)stream, dev_bconns, n, dev_rooms,
                     dev_room_results, n_rooms, dev_results);
  return hip_err(hipGetLastError());
}

// Internal (tests and measurements, no HIP call): the geometry of
// k_room_wire and k_room_fanout. out: {members per tile of the wire build,
// bytes per fan-out step, grid cap, wave size}.
int xyws_debug_broadcast_geometry(uint64_t out[4]) {
  if (!out) return XYWS_ERR_INVALID;
  out[0] = BC_TILE;
  out[1] = BC_STEP;
  out[2] = BC_GRID_CAP;
  out[3] = BC_WAVE;
  return XYWS_OK;
}

}  // extern "C"

// xyws_reply.hip — xyws_reply_streams: the answers to many connections' frames
// written by one launch (the reference's websocket_check_parser_result,
// echo_once and websocket_send_close, example/include/common/websocket.h:70-108
// and example/websocket/websocket_echo.cpp:18-27, run once per coroutine).
// The semantics are stated in include/xyws.h; this is how they are computed.
// Every table row is read and written through xyws_rows.h, which names its words.
//
// As in k_decode_streams (xyws_streams.hip) connections are independent: one
// wave (a 64-thread workgroup) takes one connection, connections are
// grid-strided, no workgroup talks to another and nothing spins.
//
// A connection's table is taken in tiles of REPLY_TILE frames, one frame per
// lane:
//   1. each lane classifies its frame (classify_frame, xyws_frameops.h) and
//      stores the verdict; the first close of the tile comes from a ballot;
//   2. a frame before the close that is to be answered has the reply size
//      header + the payload bytes that lie in this batch; the sizes are
//      scanned across the wave (shuffles), and the tile's items go to LDS:
//      start offset in the reply, header words and length, source offset.
//      Item 0 is the carried prefix (the rest of a frame whose reply an earlier
//      call began; first tile only), items 1..REPLY_TILE the frames, the last
//      item the close frame (a 4-byte header without payload);
//   3. the copy phase covers the tile's output range in 16-byte lines of the
//      send buffer (xyws_lines.h), one line per lane per step: the lane finds
//      the item of its line's first byte (item_at), walks the items that touch
//      the line and composes their header and payload bytes in registers.
// The state between tiles (reply length so far, frame_remaining, echoing,
// answered, first close) is wave-uniform and held in scalars.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>

#include "xyws.h"
#include "xyws_device.h"
#include "xyws_ctx.h"
#include "xyws_frameops.h"
#include "xyws_lines.h"
#include "xyws_rows.h"

#define REPLY_TILE 64u       // frames per tile: one per lane
#define REPLY_LANES 64u      // lanes per connection: one wave
#define REPLY_LINE 16u       // bytes a lane writes per copy step
#define REPLY_GRID_CAP 8192u // 256 CUs x 32 one-wave workgroups; further connections are grid-strided
#define REPLY_ITEMS (REPLY_TILE + 2u)  // the carried prefix, the frames, the close frame
#define REPLY_CLOSE_ITEM (REPLY_TILE + 1u)

using namespace xyws_internal;
namespace rows = xyws_rows;

// The reply bytes [o0, o1) of one tile, whose items are in LDS, into the send
// buffer: reply byte q lives at position olo + q from obase (16-byte aligned);
// positions at or above wlim (olo + out_cap) are not written.
XYWS_DEV void copy_tile(const uint64_t* s_off, const uint64_t* s_soff, const uint64_t* s_h01, const uint32_t* s_h2,
                        uint32_t lane, uint64_t src, g_u8* obase, uint64_t olo, uint64_t wlim, uint64_t o0,
                        uint64_t o1) {
  const uint64_t P0 = olo + o0, P1 = olo + o1;
  const uint64_t wl = P1 < wlim ? P1 : wlim;
  if (wl <= P0) return;
  for (uint64_t A = ((P0 >> 4) + lane) << 4; A < wl; A += (uint64_t)REPLY_LINE * REPLY_LANES) {
    const uint64_t s = A > P0 ? A : P0, e = A + 16 < P1 ? A + 16 : P1;
    uint64_t q = s - olo;
    uint32_t i = item_at(s_off, REPLY_ITEMS, q);  // the item that holds byte q (q < o1)
    bytes16 acc = {0, 0};
    uint32_t a = (uint32_t)(s - A);
    const uint32_t ae = (uint32_t)(e - A);
    while (a < ae && i < REPLY_ITEMS) {
      const uint64_t start = s_off[i], next = s_off[i + 1];
      if (next > q) {
        uint64_t r = q - start;
        const uint32_t h2 = s_h2[i], h = h2 >> 16;
        if (r < h) {  // header bytes r.. at line offset a
          const uint32_t nb = h - (uint32_t)r < ae - a ? h - (uint32_t)r : ae - a;
          add_bytes(acc, a, q, shr_bytes(bytes16{s_h01[i], h2 & 0xFFFFu}, (uint32_t)r), nb);
          r += nb;
        }
        if (a < ae && q < next) {  // payload bytes r - h.. at line offset a
          const uint32_t nb = next - q < ae - a ? (uint32_t)(next - q) : ae - a;
          add_bytes(acc, a, q, load_bytes(src + s_soff[i] + (r - h), nb), nb);
        }
      }
      i++;
    }
    put_line(obase, A, s, e, olo, wlim, acc);
  }
}

__global__ void __launch_bounds__(REPLY_LANES) k_reply_streams(const xyws_conn* __restrict__ conns,
                                                               const uint64_t* __restrict__ nframes,
                                                               const xyws_reply_conn* __restrict__ replies,
                                                               uint64_t n, uint64_t max_payload, uint32_t policy,
                                                               uint32_t flags, uint32_t enc_opts, uint32_t amask,
                                                               xyws_reply_result* __restrict__ results) {
  // one tile's items: start offset in the reply (and the end after the last),
  // source offset of the payload, header bytes 0..7, header bytes 8..9 | length << 16
  __shared__ uint64_t s_off[REPLY_ITEMS + 1];
  __shared__ uint64_t s_soff[REPLY_ITEMS];
  __shared__ uint64_t s_h01[REPLY_ITEMS];
  __shared__ uint32_t s_h2[REPLY_ITEMS];
  const uint32_t lane = threadIdx.x;
  for (uint64_t ci = blockIdx.x; ci < n; ci += gridDim.x) {
    const rows::conn_row cn = rows::load_conn(conns + ci);
    const uint64_t buf = cn.buf, len = cn.len, frames = cn.frames, cap = cn.cap;
    const uint64_t t = uniform64(((const g_u64*)nframes)[ci]);
    const rows::reply_conn_row rq = rows::load_reply_conn(replies + ci);
    const uint64_t out = rq.out, out_cap = rq.out_cap, verd = rq.verdicts;
    xyws_reply_carry* const rc = (xyws_reply_carry*)rq.rc;
    xyws_reply_result* const res = results ? results + ci : nullptr;

    rows::reply_carry_row c = {0, 0, 0, 0, {0, 0, 0}};
    if (rc) c = rows::load_reply_carry(rc);
    const uint32_t code_in = c.state.close_code;
    uint64_t rem = c.frame_remaining;
    uint32_t echoing = c.state.echoing;

    if ((c.state.status & XYWS_RPL_OVERFLOW) || t > cap || (!frames && t)) {  // the table does not cover the stream
      if (lane == 0) {
        if (rc) rows::raise_reply_status(rc, c.state_word, XYWS_RPL_OVERFLOW);
        if (res) rows::store_reply_result(res, 0, XYWS_NPOS, {0, code_in, XYWS_RPL_OVERFLOW});
      }
      continue;
    }
    if (code_in) {  // closed by an earlier call
      if (lane == 0 && res) rows::store_reply_result(res, 0, XYWS_NPOS, {0, code_in, XYWS_RPL_CLOSED});
      continue;
    }

    g_u8* const obase = (g_u8*)(out & ~15ull);
    const uint64_t olo = out & 15u;
    const uint64_t wlim = sat_add(olo, out_cap);

    // the rest of the frame the last batch end cut
    uint64_t pk = 0;
    {
      const uint64_t k = rem < len ? rem : len;
      if (echoing) pk = k;
      rem -= k;
    }

    uint64_t opos = 0, first_close = XYWS_NPOS;
    uint32_t answered = 0, ccode = 0;
    for (uint64_t base = 0; base < t || (base == 0 && pk); base += REPLY_TILE) {
      const uint64_t j = base + lane;
      const bool valid = j < t;
      uint64_t poff = 0, plen = 0;
      uint32_t fflags = 0, fstatus = 0;
      if (valid) {
        const rows::frame_row f = rows::load_frame(rows::row_at<const xyws_frame>(frames, j));
        poff = f.payload_off;
        plen = f.payload_len;
        fflags = f.flags;
        fstatus = f.status;
      }
      xyws_verdict v;
      v.close_code = 0;
      v.peer_code = 0;
      v.action = 0;
      v.reserved[0] = v.reserved[1] = v.reserved[2] = 0;
      if (valid) {
        v = classify_frame(fflags, fstatus, poff, plen, (const g_u8*)buf, len, max_payload, policy);
        if (verd) rows::store_verdict(rows::row_at<xyws_verdict>(verd, j), v);
      }
      const uint64_t closes = __ballot(valid && v.close_code != 0);
      if (first_close != XYWS_NPOS) continue;  // closed in an earlier tile: verdicts only

      // the frames before the first close: lanes below nrep
      uint32_t nrep = t - base < REPLY_TILE ? (uint32_t)(t - base) : REPLY_TILE;
      uint32_t closing = 0;
      if (closes) {
        nrep = (uint32_t)__builtin_ctzll(closes);
        first_close = base + nrep;
        ccode = uniform32((uint32_t)__shfl((int)v.close_code, (int)nrep));
        closing = 1;
      }
      const bool live = lane < nrep;
      const bool ans = live && ((amask >> v.action) & 1u);
      uint64_t inb = 0;
      if (live && poff < len) inb = plen < len - poff ? plen : len - poff;
      uint32_t hw[4] = {0, 0, 0, 0};
      uint32_t h = 0;
      if (ans) h = build_header(reply_flags_of(flags, enc_opts, fflags), plen, false, 0, hw);
      const uint64_t size = ans ? h + inb : 0;
      answered += (uint32_t)__popcll(__ballot(ans));
      if (nrep) {
        rem = uniform64(shfl64(plen - inb, nrep - 1));
        echoing = uniform32((uint32_t)__shfl((int)ans, (int)(nrep - 1)));
      }

      // reply offsets: an inclusive scan of the sizes across the wave
      const uint64_t incl = wave_scan64(size, lane);
      const uint64_t o0 = opos, fstart = opos + pk;
      const uint64_t cstart = fstart + uniform64(shfl64(incl, REPLY_LANES - 1));
      const uint64_t o1 = cstart + 4u * closing;
      s_off[1 + lane] = fstart + (incl - size);
      s_soff[1 + lane] = poff;
      s_h01[1 + lane] = (uint64_t)hw[0] | ((uint64_t)hw[1] << 32);
      s_h2[1 + lane] = (hw[2] & 0xFFFFu) | (h << 16);
      if (lane == 0) {
        s_off[0] = o0;  // the carried prefix: buf[0, pk)
        s_soff[0] = 0;
        s_h01[0] = 0;
        s_h2[0] = 0;
        // websocket_send_close (websocket.h:70-76): FIN | CLOSE, length 2, the code big-endian
        s_off[REPLY_CLOSE_ITEM] = cstart;
        s_soff[REPLY_CLOSE_ITEM] = 0;
        s_h01[REPLY_CLOSE_ITEM] = closing ? 0x0288ull | ((uint64_t)(ccode >> 8) << 16) | ((uint64_t)(ccode & 0xFFu) << 24) : 0;
        s_h2[REPLY_CLOSE_ITEM] = closing ? 4u << 16 : 0;
        s_off[REPLY_ITEMS] = o1;
      }
      pk = 0;
      __syncthreads();
      copy_tile(s_off, s_soff, s_h01, s_h2, lane, buf, obase, olo, wlim, o0, o1);
      opos = o1;
      __syncthreads();  // (LDS is rewritten by the next tile)
    }

    if (lane == 0) {
      if (rc)
        rows::store_reply_carry(rc, rem, c.frames_seen + t, c.replies_total + answered, c.state_word,
                                {ccode, echoing ? 1u : 0u, c.state.status});
      if (res) {
        const uint32_t st = (opos > out_cap ? XYWS_RPL_TRUNCATED : 0u) | (first_close != XYWS_NPOS ? XYWS_RPL_CLOSED : 0u);
        rows::store_reply_result(res, opos, first_close, {answered, ccode, st});
      }
    }
  }
}

extern "C" {

int xyws_reply_streams(xyws_ctx* ctx, const xyws_conn* dev_conns, const uint64_t* dev_nframes,
                       const xyws_reply_conn* dev_replies, uint64_t n, uint64_t max_payload, uint32_t policy,
                       uint8_t flags, uint32_t enc_opts, uint32_t action_mask, xyws_reply_result* dev_results,
                       void* stream) {
  if (!ctx || (n && (!dev_conns || !dev_nframes || !dev_replies))) return XYWS_ERR_INVALID;
  if (flags & XYWS_FLAG_HAS_MASK) return XYWS_ERR_INVALID;  // server role only
  if (enc_opts & ~XYWS_ENC_FRAME_OPCODE) return XYWS_ERR_INVALID;
  if (policy & ~(XYWS_POL_FRAGMENTS | XYWS_POL_UNMASKED | XYWS_POL_STRICT | XYWS_POL_REFERENCE)) return XYWS_ERR_INVALID;
  if (action_mask & ~((2u << XYWS_ACT_CLOSE) - 1u)) return XYWS_ERR_INVALID;
  if (!n) return XYWS_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  device_guard g(ctx->device);
  if (!g.ok) return XYWS_ERR_HIP;
  const uint32_t grid = grid_for(n, 1, REPLY_GRID_CAP);
  hipLaunchKernelGGL(k_reply_streams, dim3(grid), dim3(REPLY_LANES), 0, (hipStream_t)stream, dev_conns, dev_nframes,
                     dev_replies, n, max_payload, policy, (uint32_t)flags, enc_opts, action_mask, dev_results);
  return hip_err(hipGetLastError());
}

// Internal (tests and measurements, no HIP call): the geometry of
// k_reply_streams. out: {frames per tile, bytes per copy step, grid cap,
// wave size}.
int xyws_debug_reply_geometry(uint64_t out[4]) {
  if (!out) return XYWS_ERR_INVALID;
  out[0] = REPLY_TILE;
  out[1] = REPLY_LINE * REPLY_LANES;
  out[2] = REPLY_GRID_CAP;
  out[3] = REPLY_LANES;
  return XYWS_OK;
}

}  // extern "C"

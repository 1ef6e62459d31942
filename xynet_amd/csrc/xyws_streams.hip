// xyws_streams.hip — xyws_decode_streams: the recv buffers of many connections
// decoded by one launch (the reference's per-connection websocket_recv_data
// loop, example/include/common/websocket.h:110-134, run once per coroutine).
//
// Connections are independent, so nothing is speculated and no workgroup
// talks to another: one wave (a 64-thread workgroup) takes one connection and
// chases it exactly from its carry, as k_stream_serial (xyws.hip) states the
// semantics; connections are grid-strided. The speed is in the thousands of
// waves in flight, so a wave keeps little: STREAMS_WINDOW bytes of LDS and the
// window's lines in registers.
//
// A connection is walked in windows of up to STREAMS_WINDOW bytes, each
// starting at the 16-byte line of the current position (a frame start, or the
// next byte of an open payload):
//   1. the lanes load the window's lines (16 bytes each, coalesced: lane l
//      holds lines l, l + 64, ...) and copy them to LDS;
//   2. every lane runs the same chase through LDS on wave-uniform values: a
//      header is read as five dwords at its byte offset and parsed by
//      parse_header_words; lane 0 writes the descriptor; each lane XORs the
//      rotated key into the lines it holds that the payload covers;
//   3. lines that changed go back with 16-byte stores, the connection's first
//      and last line byte by byte within [lo, hi) (two connections cut from
//      one receive slab share such a line).
// The state between windows is the carry itself, held in scalars. A header cut
// by a window end is not consumed: the next window starts at its line (it then
// fits: a header is at most 14 bytes). An open payload that needs no XOR (an
// unmasked frame, a zero key, XYWS_OPT_PARSE_ONLY) is stepped over before a
// window is loaded, so only its part inside the window of its header was read.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>

#include "xyws.h"
#include "xyws_device.h"
#include "xyws_ctx.h"
#include "xyws_rows.h"

#define STREAMS_WINDOW 4096u     // bytes of one window (LDS per workgroup, plus one line of slack)
#define STREAMS_LANES 64u        // lanes per connection: one wave
#define STREAMS_CONNS_PER_WG 1u  // connections a workgroup decodes at a time
#define STREAMS_GRID_CAP 8192u   // 256 CUs x 32 one-wave workgroups; further connections are grid-strided
#define STREAMS_LPL (STREAMS_WINDOW / 16u / STREAMS_LANES)  // lines per lane

// The rotated key kw XORed into the lines this lane holds, over the window's
// bytes [a, b) (offsets from the window start, which is 16-byte aligned: kw is
// aligned_key's for the absolute positions too). Most lines lie outside a
// frame's span and leave at the first test. (A branch-free form, the edge
// lines' masks computed once on the wave-uniform a and b and selected per
// line, measured 8-30 % slower per call on the cells of scripts/streams_rate.py.)
XYWS_DEV void xor_span(u32x4 (&d)[STREAMS_LPL], uint32_t& dirty, uint32_t lane, uint32_t a, uint32_t b,
                       uint32_t kw) {
#pragma unroll
  for (uint32_t t = 0; t < STREAMS_LPL; t++) {
    const uint32_t A = 16u * (lane + STREAMS_LANES * t);
    if (b <= A || a >= A + 16) continue;
    if (a <= A && b >= A + 16) {
      d[t] ^= kw;
    } else {
      d[t].x ^= kw & range_mask(A, a, b);
      d[t].y ^= kw & range_mask(A + 4, a, b);
      d[t].z ^= kw & range_mask(A + 8, a, b);
      d[t].w ^= kw & range_mask(A + 12, a, b);
    }
    dirty |= 1u << t;
  }
}

__global__ void __launch_bounds__(STREAMS_LANES, 6) k_decode_streams(const xyws_conn* __restrict__ conns, uint64_t n,
                                                                  uint64_t* __restrict__ nframes_out,
                                                                  uint32_t parse_only) {
  __shared__ __attribute__((aligned(16))) uint32_t s_w[STREAMS_WINDOW / 4 + 4];
  const uint32_t lane = threadIdx.x;
  for (uint64_t ci = blockIdx.x; ci < n; ci += gridDim.x) {
    const xyws_conn cn = conns[ci];
    if (!cn.len) {  // the connection is left as it is
      if (nframes_out && lane == 0) ((g_u64*)nframes_out)[ci] = 0;
      continue;
    }
    const uint64_t addr = reinterpret_cast<uintptr_t>(cn.buf);
    g_u8* const gbase = (g_u8*)(addr & ~15ull);
    const uint64_t lo = addr & 15u, hi = lo + cn.len;
    xyws_frame* const frames = cn.cap ? cn.frames : nullptr;

    // the carry, in wave-uniform scalars: rem / phase / key of an open payload,
    // chl bytes of an incomplete header in hb
    uint64_t rem = 0, phase = 0;
    uint32_t key = 0, chl = 0;
    bytes16 hb = {0, 0};
    if (cn.carry) {
      const xyws_rows::carry_row c = xyws_rows::load_carry(cn.carry);
      rem = c.payload_remaining;
      phase = c.phase;
      key = c.head.key;
      chl = c.head.hdr_len > 13 ? 13 : c.head.hdr_len;
      hb = low_bytes(bytes16{c.head.hdr_lo, c.head.hdr_hi}, chl);
    }

    uint64_t pos = lo, nf = 0;
    while (pos < hi) {
      if (rem && (parse_only || !key)) {  // an open payload that stays as it is: not loaded
        const uint64_t take = rem < hi - pos ? rem : hi - pos;
        pos += take;
        rem -= take;
        phase += take;
        if (!rem) { phase = 0; key = 0; }
        continue;
      }
      const uint64_t wb = pos & ~15ull, hi16 = (hi + 15) & ~15ull;
      const uint64_t we = hi16 - wb > STREAMS_WINDOW ? wb + STREAMS_WINDOW : hi16;
      const uint32_t nlines = (uint32_t)((we - wb) >> 4);
      const uint64_t vend = we < hi ? we : hi;  // the window's bytes are [pos, vend)
      const g_u32x4* src = reinterpret_cast<const g_u32x4*>(gbase + wb);
      u32x4 d[STREAMS_LPL];
#pragma unroll
      for (uint32_t t = 0; t < STREAMS_LPL; t++) {
        const uint32_t j = lane + STREAMS_LANES * t;
        d[t] = j < nlines ? src[j] : u32x4{0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (uint32_t t = 0; t < STREAMS_LPL; t++) {
        const uint32_t j = lane + STREAMS_LANES * t;
        if (j < nlines) *reinterpret_cast<u32x4*>(&s_w[4 * j]) = d[t];
      }
      __syncthreads();

      // (the chase in 32-bit offsets from the window start: the scalar unit
      // compares no 64-bit magnitudes)
      uint32_t dirty = 0, p = (uint32_t)(pos - wb);
      const uint32_t pv = (uint32_t)(vend - wb);
      while (p < pv) {
        if (rem) {  // payload of the open frame
          const uint32_t room = pv - p;
          const uint32_t take = (uint32_t)(rem >> 32) || (uint32_t)rem > room ? room : (uint32_t)rem;
          if (key && !parse_only) xor_span(d, dirty, lane, p, p + take, aligned_key(key, p, (uint32_t)phase));
          p += take;
          rem -= take;
          phase += take;
          if (!rem) { phase = 0; key = 0; }
          continue;
        }
        // a header at p: 16 bytes from LDS at its byte offset, after the chl carried ones
        const uint32_t q = p >> 2, sh = p & 3u;
        const uint32_t x0 = s_w[q], x1 = s_w[q + 1], x2 = s_w[q + 2], x3 = s_w[q + 3], x4 = s_w[q + 4];
        uint32_t w[4] = {uniform32(__builtin_amdgcn_alignbyte(x1, x0, sh)),
                         uniform32(__builtin_amdgcn_alignbyte(x2, x1, sh)),
                         uniform32(__builtin_amdgcn_alignbyte(x3, x2, sh)),
                         uniform32(__builtin_amdgcn_alignbyte(x4, x3, sh))};
        uint32_t avail = pv - p < 16 ? pv - p : 16;
        const uint32_t h0 = chl;
        if (h0) {
          bytes16 nb = {(uint64_t)w[0] | ((uint64_t)w[1] << 32), (uint64_t)w[2] | ((uint64_t)w[3] << 32)};
          nb = shl_bytes(low_bytes(nb, avail), h0);
          hb.lo |= nb.lo;
          hb.hi |= nb.hi;
          avail = h0 + avail < 16 ? h0 + avail : 16;
          w[0] = (uint32_t)hb.lo; w[1] = (uint32_t)(hb.lo >> 32);
          w[2] = (uint32_t)hb.hi; w[3] = (uint32_t)(hb.hi >> 32);
        }
        const hdr_info h = parse_header_words(w, avail);
        if (!h.hlen) {
          if (vend == hi) {  // cut by the connection's end: its bytes go to the carry
            if (!h0) hb = low_bytes(bytes16{(uint64_t)w[0] | ((uint64_t)w[1] << 32),
                                            (uint64_t)w[2] | ((uint64_t)w[3] << 32)}, avail);
            chl = avail;
            p = pv;
          }
          break;  // (cut by the window's end: the next window starts at its line)
        }
        const uint32_t pp = p + (h.hlen - h0);  // the payload's first byte
        if (frames && nf < cn.cap && lane == 0) {
          const uint64_t ps = wb + pp;
          const uint32_t st = h.status | (sat_add(ps, h.plen) > hi ? XYWS_ST_PAYLOAD_INCOMPLETE : 0u);
          xyws_rows::store_frame(frames + nf, (uint64_t)((int64_t)(wb + p - lo) - (int64_t)h0), ps - lo, h.plen,
                                 {h.key, h.flags, h.hlen, st});
        }
        nf++;
        chl = 0;
        hb = bytes16{0, 0};
        rem = h.plen;
        phase = 0;
        key = h.plen ? h.key : 0u;
        p = pp;
      }
      pos = wb + p;

      if (dirty) {
#pragma unroll
        for (uint32_t t = 0; t < STREAMS_LPL; t++) {
          const uint64_t A = wb + 16u * (lane + STREAMS_LANES * t);
          if ((dirty & (1u << t)) && A >= lo && A + 16 <= hi) *reinterpret_cast<g_u32x4*>(gbase + A) = d[t];
        }
        // the connection's first and last line: its own bytes only
        const uint64_t last = (hi - 1) & ~15ull;
        for (uint32_t e = 0; e < (last ? 2u : 1u); e++) {
          const uint64_t E = e ? last : 0;
          const uint32_t j = (uint32_t)((E - wb) >> 4);
          if (E < wb || E >= we || (j & (STREAMS_LANES - 1)) != lane || !(dirty & (1u << (j / STREAMS_LANES))) ||
              (E >= lo && E + 16 <= hi))
            continue;
          u32x4 v = d[0];
#pragma unroll
          for (uint32_t t = 1; t < STREAMS_LPL; t++)
            if (j / STREAMS_LANES == t) v = d[t];
#pragma unroll 1
          for (uint32_t b = 0; b < 16; b++) {
            const uint32_t wd = b < 4 ? v.x : b < 8 ? v.y : b < 12 ? v.z : v.w;
            if (E + b >= lo && E + b < hi) gbase[E + b] = (uint8_t)(wd >> (8u * (b & 3u)));
          }
        }
      }
      __syncthreads();  // (LDS is rewritten; a line stored here may be the next window's first)
    }

    if (lane == 0) {
      if (cn.carry) xyws_rows::store_carry(cn.carry, rem, phase, nf, {key, chl, hb.lo, hb.hi});
      if (nframes_out) ((g_u64*)nframes_out)[ci] = nf;
    }
  }
}

using namespace xyws_internal;

extern "C" {

int xyws_decode_streams(xyws_ctx* ctx, const xyws_conn* dev_conns, uint64_t n, uint64_t* dev_nframes,
                        uint32_t opts, void* stream) {
  if (!ctx || (!dev_conns && n)) return XYWS_ERR_INVALID;
  if (opts & ~(XYWS_OPT_PARSE_ONLY | XYWS_OPT_UNMASKED_HINT)) return XYWS_ERR_INVALID;
  if (!n) return XYWS_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  device_guard g(ctx->device);
  if (!g.ok) return XYWS_ERR_HIP;
  const uint32_t grid = grid_for(n, STREAMS_CONNS_PER_WG, STREAMS_GRID_CAP);
  hipLaunchKernelGGL(k_decode_streams, dim3(grid), dim3(STREAMS_LANES * STREAMS_CONNS_PER_WG), 0,
                     (hipStream_t)stream, dev_conns, n, dev_nframes, (opts & XYWS_OPT_PARSE_ONLY) ? 1u : 0u);
  return hip_err(hipGetLastError());
}

// Internal (tests and measurements, no HIP call): the geometry of
// k_decode_streams. out: {window bytes, lanes per connection, connections per
// workgroup, grid cap}.
int xyws_debug_streams_geometry(uint64_t out[4]) {
  if (!out) return XYWS_ERR_INVALID;
  out[0] = STREAMS_WINDOW;
  out[1] = STREAMS_LANES;
  out[2] = STREAMS_CONNS_PER_WG;
  out[3] = STREAMS_GRID_CAP;
  return XYWS_OK;
}

}  // extern "C"

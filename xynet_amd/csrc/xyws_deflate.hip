// xyws_deflate.hip — xyws_deflate_streams: the messages a sweep's broadcast
// would frame, compressed once per message on the device (permessage-deflate on
// the send side, RFC 7692 with server_no_context_takeover), in front of
// xyws_broadcast_deflated_streams. The semantics are stated in include/xyws.h;
// this is how they are computed. Every table row is read and
// written through xyws_rows.h; which records are deliverable is load_member's
// and frame_of's answer (xyws_room.h), nobody else's.
//
// As in k_inflate_streams one wave (a 64-thread workgroup) takes one
// connection and its records in order, connections are grid-strided, no
// workgroup talks to another, nothing spins. A record's bytes head | message
// pass through LDS in pieces of DFL_STAGE bytes; the three stages of DEFLATE
// are the wave's:
//   staging  a piece is composed of whole 16-byte lines of the head and the
//            message (load_bytes, xyws_lines.h), one LDS line per lane and step;
//   search   64 positions per step, one per lane: the lane hashes the 4 bytes
//            at its position, takes the newest earlier position with that hash
//            from an LDS table (one position per slot, an LDS atomic max, so
//            the table does not depend on which lane writes last), or the byte
//            before it when that begins a run, and extends the match over LDS
//            words up to 258 bytes. The step's positions enter the table after
//            the step's lookups. Matches never reach behind the piece;
//   choice   the one dependent chain, wave-uniform: a ballot of the lanes with
//            a match of 4 bytes or more; the lowest one at or behind the
//            current position takes its match, the lanes before it are
//            literals, the position jumps past the match; the next step begins
//            where the last token ended;
//   emission each lane holds one token: a literal of 8 or 9 bits or a
//            length/distance pair of at most 31, the fixed code's lengths and
//            bit-reversed codes computed. A wave scan of the bit lengths gives
//            each token its bit offset and the lane ORs it into one or two words
//            of a zeroed LDS stage. The stage goes to global memory as whole
//            16-byte lines, byte stores on the first and last line (put_line).
// A record of one piece is searched once, its bits emitted into LDS while they
// are counted; a longer one is counted first and emitted in a second pass, so
// the fixed form's size is known before a byte leaves LDS. The stored form is
// the staged bytes written out behind 5-byte block headers.
// LDS: 8 KiB piece + 8 KiB table + 9 KiB output stage: six waves per CU on
// gfx950's 160 KiB; the grid cap is that.
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

#define DFL_LANES 64u
#define DFL_STAGE 8192u                        // W: bytes of a record staged, searched and emitted at once
#define DFL_SLOTS 2048u                        // hash slots: the newest position per hash
#define DFL_HASH_BITS 11u
#define DFL_OUT (DFL_STAGE + DFL_STAGE / 8u + 64u)  // the output stage: 9 bits a byte, the block's ends, a flush's read-ahead
#define DFL_GRID_CAP 1536u                     // 256 CUs x 6 one-wave workgroups (LDS); further connections are grid-strided
#define DFL_MIN_MATCH 4u
#define DFL_MAX_MATCH 258u
#define DFL_STORED_MAX 65535u

using namespace xyws_internal;
namespace rows = xyws_rows;

namespace {

static_assert(DFL_SLOTS == 1u << DFL_HASH_BITS && DFL_STAGE <= DFL_STORED_MAX && DFL_STAGE % 16u == 0, "the geometry");

// What one wave keeps in LDS.
struct deflate_lds {
  __attribute__((aligned(16))) uint32_t in[(DFL_STAGE + 32u) / 4u];  // the piece (20 bytes of read-ahead behind it)
  __attribute__((aligned(16))) uint32_t tab[DFL_SLOTS];              // position + 1 of the newest 4 bytes with this hash; 0: none
  __attribute__((aligned(16))) uint32_t out[DFL_OUT / 4u];           // the piece's bits
};

XYWS_DEV uint64_t below(uint32_t p) { return (1ull << p) - 1ull; }  // (p < 64)
XYWS_DEV uint32_t lane_value(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }
XYWS_DEV uint32_t scan32(uint32_t v, uint32_t lane) {  // inclusive, across the wave
#pragma unroll
  for (uint32_t d = 1; d < DFL_LANES; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)v, d);
    if (lane >= d) v += o;
  }
  return v;
}
// The 4 LDS bytes at byte offset o, any alignment (the word behind them is read too).
XYWS_DEV uint32_t rd32(const uint32_t* w, uint32_t o) {
  const uint32_t i = o >> 2;
  return __builtin_amdgcn_alignbyte(w[i + 1], w[i], o & 3u);
}
XYWS_DEV uint32_t log2u(uint32_t v) { return 31u - (uint32_t)__clz((int)v); }  // (v > 0)
XYWS_DEV uint32_t rev(uint32_t code, uint32_t len) { return __brev(code) >> (32u - len); }

// The fixed code of RFC 1951 3.2.6, computed: a Huffman code goes out first bit
// first, so it is bit-reversed; extra bits follow as they are.
XYWS_DEV uint32_t litlen_code(uint32_t s, uint32_t& len) {
  uint32_t c;
  if (s < 144u) c = 0x30u + s, len = 8;
  else if (s < 256u) c = 0x190u + (s - 144u), len = 9;
  else if (s < 280u) c = s - 256u, len = 7;
  else c = 0xC0u + (s - 280u), len = 8;
  return rev(c, len);
}
// A match of mlen bytes (4..258) at distance dist (1..DFL_STAGE): its bits, at most 8 + 5 + 5 + 13.
XYWS_DEV uint32_t match_bits(uint32_t mlen, uint32_t dist, uint32_t& nbits) {
  uint32_t s, e = 0, x = 0;
  const uint32_t l = mlen - 3u;
  if (mlen <= 10u) s = 254u + mlen;
  else if (mlen == DFL_MAX_MATCH) s = 285u;
  else {
    e = log2u(l) - 2u;
    s = 261u + 4u * e + ((l >> e) - 4u);
    x = l & ((1u << e) - 1u);
  }
  uint32_t n;
  uint32_t v = litlen_code(s, n);
  v |= x << n;
  n += e;
  const uint32_t dd = dist - 1u;
  uint32_t ds = dd, de = 0, dx = 0;
  if (dd >= 4u) {
    de = log2u(dd) - 1u;
    ds = 2u * de + 2u + ((dd >> de) & 1u);
    dx = dd & ((1u << de) - 1u);
  }
  v |= rev(ds, 5) << n;
  n += 5u;
  v |= dx << n;
  nbits = n + de;
  return v;
}

// Record bytes [q0, q0 + n) of head[0, hl) | msg to s_in[0, n), whole lines; wave-uniform arguments.
XYWS_DEV void stage_piece(uint32_t* s_in, uint64_t head, uint64_t hl, uint64_t msg, uint64_t q0, uint32_t n, uint32_t lane) {
  __syncthreads();
  for (uint32_t o = 16u * lane; o < n; o += 16u * DFL_LANES) {
    const uint32_t want = n - o < 16u ? n - o : 16u;
    bytes16 acc = {0, 0};
    uint32_t a = 0;
    uint64_t q = q0 + o;
    if (q < hl) {
      const uint32_t nb = hl - q < want ? (uint32_t)(hl - q) : want;
      add_bytes(acc, a, q, load_bytes(head + q, nb), nb);
    }
    if (a < want) {
      const uint32_t nb = want - a;
      add_bytes(acc, a, q, load_bytes(msg + (q - hl), nb), nb);
    }
    *reinterpret_cast<u32x4*>(s_in + (o >> 2)) =
        u32x4{(uint32_t)acc.lo, (uint32_t)(acc.lo >> 32), (uint32_t)acc.hi, (uint32_t)(acc.hi >> 32)};
  }
  __syncthreads();
}

// LDS bytes src[0, nb) to positions [P0, P0 + nb) from dbase (16-byte aligned),
// all of them the record's own and inside the cap: whole lines, byte stores on
// the first and last one. Up to 20 bytes behind src[nb) are read.
XYWS_DEV void flush_stage(const uint32_t* src, uint32_t nb, g_u8* dbase, uint64_t P0, uint32_t lane) {
  __syncthreads();
  const uint64_t P1 = P0 + nb;
  for (uint64_t A = (P0 & ~15ull) + 16u * lane; A < P1; A += 16u * DFL_LANES) {
    const uint64_t s = A > P0 ? A : P0, e = A + 16 < P1 ? A + 16 : P1;
    const uint32_t o = (uint32_t)(s - P0), i = o >> 2, sh = o & 3u;
    const uint32_t w0 = src[i], w1 = src[i + 1], w2 = src[i + 2], w3 = src[i + 3], w4 = src[i + 4];
    bytes16 v = {(uint64_t)__builtin_amdgcn_alignbyte(w1, w0, sh) | ((uint64_t)__builtin_amdgcn_alignbyte(w2, w1, sh) << 32),
                 (uint64_t)__builtin_amdgcn_alignbyte(w3, w2, sh) | ((uint64_t)__builtin_amdgcn_alignbyte(w4, w3, sh) << 32)};
    if (s != A || e != A + 16) v = shl_bytes(low_bytes(v, (uint32_t)(e - s)), (uint32_t)(s - A));
    put_line(dbase, A, s, e, P0, P1, v);
  }
}

// One fixed-Huffman block of the n (1..DFL_STAGE) staged bytes: header, tokens,
// end of block. With emit the bits go to S.out, which is zeroed first and
// begins with the `bit0` (0..7) bits of `carry` that the piece before left
// over. Returns the bit position behind the block (bit0 + its bits).
// Wave-uniform but for the lanes' own tokens.
XYWS_DEV uint32_t fixed_block(deflate_lds& S, uint32_t n, bool emit, uint32_t carry, uint32_t bit0, uint32_t lane) {
  __syncthreads();
  for (uint32_t k = lane; k < DFL_SLOTS / 4u; k += DFL_LANES) reinterpret_cast<u32x4*>(S.tab)[k] = u32x4{0, 0, 0, 0};
  if (emit) {
    const uint32_t lines = (n + n / 8u + 63u) / 16u + 1u;  // (9 n + 25 bits at most, a word of slack; <= DFL_OUT / 16)
    for (uint32_t k = lane; k < lines; k += DFL_LANES)
      reinterpret_cast<u32x4*>(S.out)[k] = u32x4{k == 0 ? carry | (2u << bit0) : 0u, 0, 0, 0};  // BFINAL 0, BTYPE 01
  }
  __syncthreads();
  uint32_t bits = bit0 + 3u;
  for (uint32_t p0 = 0; p0 < n;) {
    // search: this lane's position
    const uint32_t p = p0 + lane;
    uint32_t mlen = 0, dist = 0, word = 0, slot = 0;
    const bool hashed = p + DFL_MIN_MATCH <= n;
    if (p < n) word = rd32(S.in, p);
    if (hashed) {
      slot = (word * 2654435761u) >> (32u - DFL_HASH_BITS);
      uint32_t c = S.tab[slot];                              // (a position of an earlier step: c - 1 < p0)
      if (p && rd32(S.in, p - 1u) == word) c = p;            // a run: the byte before, distance 1
      if (c) {
        c -= 1u;
        const uint32_t maxl = n - p < DFL_MAX_MATCH ? n - p : DFL_MAX_MATCH;
        uint32_t l = 0;
        while (l < maxl) {
          const uint32_t x = rd32(S.in, p + l) ^ rd32(S.in, c + l);
          if (x) {
            l += ((uint32_t)__ffs((int)x) - 1u) >> 3;
            break;
          }
          l += 4u;
        }
        mlen = l < maxl ? l : maxl;
        dist = p - c;
      }
    }
    // choice: the lowest match at or behind the position, literals before it
    const uint32_t lim = n - p0 < DFL_LANES ? n - p0 : DFL_LANES;
    const uint64_t mm = __ballot(mlen >= DFL_MIN_MATCH);
    uint32_t r = 0, kind = 0;  // 1: a literal, 2: a match
    while (r < lim) {
      const uint64_t m = mm & ~below(r);
      if (!m) {
        if (lane >= r && lane < lim) kind = 1;
        r = lim;
        break;
      }
      const uint32_t l = (uint32_t)__ffsll((long long)m) - 1u;  // (l < lim: a match needs 4 bytes in front of n)
      if (lane >= r && lane < l) kind = 1;
      if (lane == l) kind = 2;
      r = l + lane_value(mlen, l);
    }
    // emission
    uint32_t tb = 0, tl = 0;
    if (kind == 1) tb = litlen_code(word & 0xFFu, tl);
    else if (kind == 2) tb = match_bits(mlen, dist, tl);
    const uint32_t incl = scan32(tl, lane);
    __syncthreads();  // (the step's lookups are done)
    if (hashed) atomicMax(&S.tab[slot], p + 1u);
    if (emit && tl) {
      const uint32_t at = bits + incl - tl;
      const uint64_t v = (uint64_t)tb << (at & 31u);
      atomicOr(&S.out[at >> 5], (uint32_t)v);
      if (v >> 32) atomicOr(&S.out[(at >> 5) + 1u], (uint32_t)(v >> 32));
    }
    __syncthreads();
    bits += lane_value(incl, DFL_LANES - 1u);
    p0 += r;
  }
  return bits + 7u;  // end of block: seven zero bits
}

__global__ void __launch_bounds__(DFL_LANES)
    k_deflate_streams(const xyws_reasm_conn* __restrict__ reasm, const xyws_reasm_result* __restrict__ rres,
                      const xyws_bcast_conn* __restrict__ bconns, const xyws_deflate_conn* __restrict__ dconns, uint64_t n,
                      xyws_reasm_conn* __restrict__ view, xyws_reasm_result* __restrict__ vres,
                      xyws_bcast_conn* __restrict__ vbconns, xyws_deflate_result* __restrict__ results) {
  __shared__ deflate_lds S;
  const uint32_t lane = threadIdx.x;
  for (uint64_t ci = blockIdx.x; ci < n; ci += gridDim.x) {
    const rows::deflate_conn_row dq = rows::load_deflate_conn(dconns + ci);
    const uint64_t mc = rows::load_reasm_conn<true>(reasm + ci).mc;
    member m;
    bool receiver, over_cap;
    load_member(reasm, rres, bconns, ci, m, receiver, over_cap);
    const uint64_t msgs = uniform64(m.msgs), mout = uniform64(m.out), head = uniform64(m.head), hl = uniform64(m.head_len);
    const uint32_t stored = rows::load_bcast_room(bconns + ci) == XYWS_ROOM_NONE ? 0u : uniform32(m.stored);
    g_u8* const obase = (g_u8*)(dq.out & ~15ull);
    const uint64_t olo = dq.out & 15u;

    uint64_t opos = 0, in_len = 0, found = 0, kept = 0;  // out_len so far; deliverable records; view records stored
    uint32_t st = 0, n_deflated = 0, n_stored = 0;
    for (uint32_t j = 0; j < stored; j++) {
      const xyws_message* const rp = rows::row_at<const xyws_message>(msgs, j);
      frame_info f;
      if (!frame_of(rp, m, 0, 0, f)) continue;
      if (found++ >= dq.vmsg_cap) {
        st |= XYWS_DFL_MSG_CAP;
        continue;
      }
      const rows::message_row rec = rows::load_message<true>(rp);
      const uint64_t msg = mout + uniform64(f.off), L = hl + uniform64(f.len);
      const uint64_t blocks = (L + DFL_STORED_MAX - 1u) / DFL_STORED_MAX, stored_len = L + 5u * blocks + 1u;
      const bool single = L <= DFL_STAGE;

      // the fixed form's bits: a record of one piece is emitted into LDS on the way
      uint64_t fbits = 0;
      for (uint64_t q0 = 0; q0 < L; q0 += DFL_STAGE) {
        const uint32_t pn = L - q0 < DFL_STAGE ? (uint32_t)(L - q0) : DFL_STAGE;
        stage_piece(S.in, head, hl, msg, q0, pn, lane);
        fbits += fixed_block(S, pn, single, 0, 0, lane);
      }
      const uint64_t fixed_len = (fbits + 3u + 7u) >> 3;  // behind it the empty stored block: 3 bits, then to the byte
      const bool fixed = L && fixed_len < stored_len;
      const uint64_t clen = fixed ? fixed_len : stored_len;
      const bool fits = in_range(opos, clen, dq.out_cap);
      const uint64_t D = olo + opos;  // the record's first byte, from obase

      if (!fits) {
        st |= XYWS_DFL_TOO_LONG;
      } else if (fixed && single) {
        flush_stage(S.out, (uint32_t)clen, obase, D, lane);
      } else if (fixed) {
        uint64_t at = D;
        uint32_t carry = 0, bit0 = 0;
        for (uint64_t q0 = 0; q0 < L; q0 += DFL_STAGE) {
          const uint32_t pn = L - q0 < DFL_STAGE ? (uint32_t)(L - q0) : DFL_STAGE;
          stage_piece(S.in, head, hl, msg, q0, pn, lane);
          const uint32_t end = fixed_block(S, pn, true, carry, bit0, lane);
          const bool last = q0 + pn == L;
          const uint32_t nb = last ? (end + 3u + 7u) >> 3 : end >> 3;
          flush_stage(S.out, nb, obase, at, lane);
          at += nb;
          bit0 = end & 7u;
          carry = uniform32(S.out[nb >> 2] >> (8u * (nb & 3u))) & ((1u << bit0) - 1u);  // (read before the stage is zeroed again)
        }
      } else {
        uint64_t at = D;
        for (uint64_t b0 = 0; b0 < L; b0 += DFL_STORED_MAX) {
          const uint32_t bl = L - b0 < DFL_STORED_MAX ? (uint32_t)(L - b0) : DFL_STORED_MAX;
          if (lane < 5u)  // BFINAL 0, BTYPE 00, to the byte; LEN, NLEN
            obase[at + lane] = (uint8_t)(lane == 0 ? 0u : ((lane < 3u ? bl : ~bl) >> (8u * ((lane - 1u) & 1u))));
          at += 5u;
          for (uint32_t q = 0; q < bl; q += DFL_STAGE) {
            const uint32_t pn = bl - q < DFL_STAGE ? bl - q : DFL_STAGE;
            if (!single) stage_piece(S.in, head, hl, msg, b0 + q, pn, lane);
            flush_stage(S.in, pn, obase, at, lane);
            at += pn;
          }
        }
        if (lane == 0) obase[at] = 0;  // the empty stored block, its 00 00 ff ff left out
      }
      if (fits) {
        in_len += L;
        if (fixed) n_deflated++;
        else n_stored++;
      }
      if (lane == 0)
        rows::store_message(rows::row_at<xyws_message>(dq.vmsgs, kept),
                            {rec.first_frame, rec.nframes, opos, clen,
                             rows::pack_message_meta({XYWS_MSG_COMPLETE | (fits ? 0u : (uint32_t)XYWS_MSG_TRUNCATED),
                                                      rows::unpack_message_meta(rec.meta).opcode})});
      kept++;
      opos += clen;
      __syncthreads();  // (the stages are rewritten by the next record)
    }

    rows::copy_bcast_conn_headless(vbconns + ci, bconns + ci, lane);
    if (lane == 0) {
      rows::store_reasm_conn(view + ci, {dq.out, dq.out_cap, mc, dq.vmsgs, dq.vmsg_cap});
      const uint32_t rst = (opos > dq.out_cap ? XYWS_RSM_TRUNCATED : 0u) | (found > kept ? XYWS_RSM_MSG_CAP : 0u);
      rows::store_reasm_result(vres + ci, {opos, found, {(uint32_t)kept, rst}, 0});
      if (results) rows::store_deflate_result(results + ci, opos, in_len, {n_deflated, n_stored}, st);
    }
  }
}

}  // namespace

extern "C" {

int xyws_deflate_streams(xyws_ctx* ctx, const xyws_reasm_conn* dev_reasm, const xyws_reasm_result* dev_reasm_results,
                         const xyws_bcast_conn* dev_bconns, const xyws_deflate_conn* dev_dconns, uint64_t n, uint32_t opts,
                         xyws_reasm_conn* dev_view, xyws_reasm_result* dev_view_results, xyws_bcast_conn* dev_view_bconns,
                         xyws_deflate_result* dev_results, void* stream) {
  if (!ctx || (n && (!dev_reasm || !dev_reasm_results || !dev_bconns || !dev_dconns || !dev_view || !dev_view_results ||
                     !dev_view_bconns)))
    return XYWS_ERR_INVALID;
  if (opts || n >= UINT32_MAX) return XYWS_ERR_INVALID;
  if (!n) return XYWS_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  device_guard g(ctx->device);
  if (!g.ok) return XYWS_ERR_HIP;
  const uint32_t grid = grid_for(n, 1, DFL_GRID_CAP);
  hipLaunchKernelGGL(k_deflate_streams, dim3(grid), dim3(DFL_LANES), 0, (hipStream_t)stream, dev_reasm, dev_reasm_results,
                     dev_bconns, dev_dconns, n, dev_view, dev_view_results, dev_view_bconns, dev_results);
  return hip_err(hipGetLastError());
}

// Internal (tests and measurements, no HIP call): the geometry of
// k_deflate_streams. out: {stage bytes W, hash slots, grid cap, wave size}.
int xyws_debug_deflate_geometry(uint64_t out[4]) {
  if (!out) return XYWS_ERR_INVALID;
  out[0] = DFL_STAGE;
  out[1] = DFL_SLOTS;
  out[2] = DFL_GRID_CAP;
  out[3] = DFL_LANES;
  static_assert(sizeof(deflate_lds) * (DFL_GRID_CAP / 256u) <= 160u * 1024u, "six waves' LDS per CU");
  return XYWS_OK;
}

}  // extern "C"

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
//
// With XYWS_DFO_DYNAMIC (k_deflate_streams<true>; <false> is the kernel above,
// unchanged) a piece may go out as a dynamic-Huffman block over the same
// tokens. The counting pass adds every token to two LDS histograms (286
// literal/length counters, 30 distance counters); between the passes, when the
// hash table is dead, the wave builds the three codes in the table's 8 KiB
// (build_code: a bitonic sort of the used symbols by (frequency, symbol), the
// two-queue merge, depths top-down, zlib's repair on the counts per length,
// lengths handed out by rank, canonical codes), run-length codes the lengths
// (one position per lane, runs found with ballots) and lays the block's header
// bits down there. The packed table code << 8 | length overwrites the
// histograms: 316 words, the only LDS the option adds. The emitting pass looks
// a token's bits up there: up to 48 bits, ORed into up to three words.
//
// xyws_deflate_windows_streams keeps the server's context: one
// history per room, since every negotiated member inflates the room's whole
// wire. k_room_text lays the sweep's records behind the room's history in wire
// order; k_deflate_streams<false, true> stages DFL_HIST bytes of that text in
// front of every piece, enters the window's positions into the table before
// the first search step and keeps, per piece, the shorter of the blocks
// searched without and with the window; k_room_slide moves the last 32 KiB to
// the front for the next sweep. LDS: 16 KiB window and piece + 8 KiB table +
// 9 KiB output stage: four waves per CU.
//
// With XYWS_DFO_WINDOW_DYNAMIC (k_deflate_streams<true, true>) both hold: the
// window layout and the 316 words of histograms and codes, 35 KiB, still four
// waves per CU. A piece with a window is searched without it and with it, each
// search counted into its own histograms and planned (plan_piece) before the
// next one overwrites them; the shortest of the four blocks is kept in two
// mask bits a piece (wmask: with the window, dmask: dynamic). The emitting pass
// stages the piece again, repeats the chosen search and, where the block is
// dynamic, its count and plan: the codes do not survive the next piece.
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
// xyws_deflate_windows_streams (k_deflate_streams<false, true>): the window in front of the piece
#define DFL_HIST 8192u                         // bytes of window staged in front of a piece (<= 32768, the inflater's)
#define DFL_WIN_GRID_CAP 1024u                 // 256 CUs x 4 one-wave workgroups (LDS)
#define DFL_WIN_PIECES 64u                     // a record's pieces that may use the window (one choice bit each)
#ifndef DFL_WIN_PRIME                          // 0: a measurement build (scripts/deflate_rate.py --noprime-lib) that leaves the
#define DFL_WIN_PRIME 1                        // priming out: the second search then finds what the first found, and runs
#endif                                         // into the window; what it emits still inflates
#define DFL_TEXT_THREADS BC_WIRE_THREADS       // the text build: the wire build's workgroup, a member per thread
#define DFL_SLIDE_THREADS 256u                 // the slide: 4 KiB a step
#define DFL_WIN_TAG 0x5857494E444F5721ull      // ^ the room: marks the text offset the text build left a connection
#define DFL_MIN_MATCH 4u
#define DFL_MAX_MATCH 258u
#define DFL_STORED_MAX 65535u
#define DFL_LITLEN 286u                        // the literal/length alphabet; its table is code[0, 286)
#define DFL_DIST 30u                           // the distance alphabet; its table is code[286, 316)
#define DFL_CLEN 19u                           // the code-length alphabet
// The builder's workspace, in words of the hash table (dead between two passes):
#define WS_KEY 0u                              // 512 sort keys: frequency << 9 | symbol, ~0 for an unused symbol
#define WS_IW 512u                             // 288: the weights of the internal nodes, in the order they are made
#define WS_IP 800u                             // 288: an internal node's parent, then its depth
#define WS_LP 1088u                            // 288: the parent of the leaf of rank r
#define WS_BLC 1376u                           // 16: symbols per length
#define WS_CLF 1392u                           // 20: the code-length alphabet's frequencies, then its packed table
#define WS_SEQ 1412u                           // 316: the run-length coded lengths, symbol | extra << 8, ~0: none here
#define WS_HDR 1728u                           // 76: the block's header bits (17 + 57 + 316 * 7 at most), from bit 0
#define WS_HDR_WORDS 76u
#define WS_RUN WS_IW                           // 316: the first position of the run a position lies in (the trees are done)

using namespace xyws_internal;
namespace rows = xyws_rows;

namespace {

static_assert(DFL_SLOTS == 1u << DFL_HASH_BITS && DFL_STAGE <= DFL_STORED_MAX && DFL_STAGE % 16u == 0, "the geometry");
static_assert(WS_HDR + WS_HDR_WORDS <= DFL_SLOTS && WS_RUN + DFL_LITLEN + DFL_DIST <= WS_BLC &&
                  32u * (WS_HDR_WORDS - 2u) >= 17u + 57u + 7u * (DFL_LITLEN + DFL_DIST) && DFL_STAGE < 1u << 14,
              "the workspace fits the table; a frequency fits its key");

// What one wave keeps in LDS.
struct deflate_lds {
  __attribute__((aligned(16))) uint32_t in[(DFL_STAGE + 32u) / 4u];  // the piece (20 bytes of read-ahead behind it)
  __attribute__((aligned(16))) uint32_t tab[DFL_SLOTS];              // position + 1 of the newest 4 bytes with this hash; 0: none
  __attribute__((aligned(16))) uint32_t out[DFL_OUT / 4u];           // the piece's bits
};

// With XYWS_DFO_DYNAMIC: and the two histograms, then the two codes, code << 8 | length.
struct deflate_lds_dynamic : deflate_lds {
  uint32_t code[DFL_LITLEN + DFL_DIST];
};
// With a window: the piece begins at byte DFL_HIST of `in`, the window ends there.
struct deflate_lds_window {
  __attribute__((aligned(16))) uint32_t in[(DFL_HIST + DFL_STAGE + 32u) / 4u];
  __attribute__((aligned(16))) uint32_t tab[DFL_SLOTS];
  __attribute__((aligned(16))) uint32_t out[DFL_OUT / 4u];
};
static_assert(DFL_HIST % 16u == 0 && DFL_HIST <= XYWS_DFL_WINDOW && DFL_HIST + DFL_STAGE <= XYWS_DFL_WINDOW,
              "a distance is at most DFL_HIST + DFL_STAGE: inside the inflater's window, and syms_of covers it");
template <bool DYN, bool WIN = false>
struct lds_of { typedef deflate_lds type; };
template <>
struct lds_of<true, false> { typedef deflate_lds_dynamic type; };
template <>
struct lds_of<false, true> { typedef deflate_lds_window type; };
// With both (XYWS_DFO_WINDOW_DYNAMIC): the window layout and the dynamic layout's histograms and codes.
struct deflate_lds_window_dynamic : deflate_lds_window {
  uint32_t code[DFL_LITLEN + DFL_DIST];
};
template <>
struct lds_of<true, true> { typedef deflate_lds_window_dynamic type; };

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
// A match of mlen bytes (4..258) at distance dist (1..DFL_STAGE): its length
// symbol s and distance symbol ds, each with e / de extra bits of value x / dx.
struct match_syms { uint32_t s, e, x, ds, de, dx; };
XYWS_DEV match_syms syms_of(uint32_t mlen, uint32_t dist) {
  uint32_t s, e = 0, x = 0;
  const uint32_t l = mlen - 3u;
  if (mlen <= 10u) s = 254u + mlen;
  else if (mlen == DFL_MAX_MATCH) s = 285u;
  else {
    e = log2u(l) - 2u;
    s = 261u + 4u * e + ((l >> e) - 4u);
    x = l & ((1u << e) - 1u);
  }
  const uint32_t dd = dist - 1u;
  uint32_t ds = dd, de = 0, dx = 0;
  if (dd >= 4u) {
    de = log2u(dd) - 1u;
    ds = 2u * de + 2u + ((dd >> de) & 1u);
    dx = dd & ((1u << de) - 1u);
  }
  return {s, e, x, ds, de, dx};
}
// Its bits in the fixed code, at most 8 + 5 + 5 + 13.
XYWS_DEV uint32_t match_bits(uint32_t mlen, uint32_t dist, uint32_t& nbits) {
  const match_syms m = syms_of(mlen, dist);
  const uint32_t e = m.e, x = m.x, ds = m.ds, de = m.de, dx = m.dx;
  uint32_t n;
  uint32_t v = litlen_code(m.s, n);
  v |= x << n;
  n += e;
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

// A room's text bytes [T - H, T + n) to s_in[DFL_HIST - H, DFL_HIST + n): the
// H (<= DFL_HIST, <= T) bytes of window in front of the piece, then the piece.
// Whole LDS lines; the bytes of a line outside the range are zero, no text byte
// outside the range is asked for. Wave-uniform arguments.
XYWS_DEV void stage_text(uint32_t* s_in, uint64_t text, uint64_t T, uint32_t H, uint32_t n, uint32_t lane) {
  __syncthreads();
  const uint32_t lo = DFL_HIST - H, end = DFL_HIST + n;
  const uint64_t src0 = text + T - DFL_HIST;  // the address LDS byte 0 would have (bytes below lo are never formed)
  for (uint32_t A = (lo & ~15u) + 16u * lane; A < end; A += 16u * DFL_LANES) {
    const uint32_t s = A > lo ? A : lo, e = A + 16u < end ? A + 16u : end;
    bytes16 v = load_bytes(src0 + s, e - s);
    if (s != A || e != A + 16u) v = shl_bytes(low_bytes(v, e - s), s - A);
    *reinterpret_cast<u32x4*>(s_in + (A >> 2)) =
        u32x4{(uint32_t)v.lo, (uint32_t)(v.lo >> 32), (uint32_t)v.hi, (uint32_t)(v.hi >> 32)};
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

XYWS_DEV uint32_t wave_sum(uint32_t v, uint32_t lane) { return lane_value(scan32(v, lane), DFL_LANES - 1u); }
XYWS_DEV uint32_t top_bit(uint64_t m) { return 64u - (uint32_t)__clzll((long long)m); }  // 1 + the highest set bit; 0: none

// A length-limited Huffman code over the frequencies fc[0, nsym) (nsym <= 286,
// each below 2^22, limit <= 15, 2^limit >= the used symbols), built by the wave
// in the workspace ws (DFL_SLOTS words). fc[s] becomes code << 8 | length, the
// code canonical (RFC 1951 3.2.2) and bit-reversed; an unused symbol keeps 0, a
// single used one gets length 1. Returns the sum of frequency x length.
XYWS_DEV uint32_t build_code(uint32_t* ws, uint32_t* fc, uint32_t nsym, uint32_t limit, uint32_t lane) {
  __syncthreads();
  // 1. the used symbols sorted by (frequency, symbol): a bitonic sort of N keys
  const uint32_t N = nsym <= 64u ? 64u : nsym <= 128u ? 128u : nsym <= 256u ? 256u : 512u;
  uint32_t m = 0;
  for (uint32_t i = lane; i < N; i += DFL_LANES) {
    const uint32_t f = i < nsym ? fc[i] : 0u;
    ws[WS_KEY + i] = f ? (f << 9) | i : ~0u;
    m += (uint32_t)__popcll(__ballot(f != 0u));
  }
  if (lane < 16u) ws[WS_BLC + lane] = 0;
  __syncthreads();
  for (uint32_t k = 2; k <= N; k <<= 1)
    for (uint32_t j = k >> 1; j; j >>= 1) {
      uint32_t a[4], b[4];  // (a stage's pairs are disjoint: all loads first, so that they overlap)
#pragma unroll
      for (uint32_t u = 0; u < 4u; u++) {
        const uint32_t q = lane + DFL_LANES * u, i = ((q & ~(j - 1u)) << 1) | (q & (j - 1u));
        if (q < N / 2u) a[u] = ws[WS_KEY + i], b[u] = ws[WS_KEY + (i | j)];
      }
#pragma unroll
      for (uint32_t u = 0; u < 4u; u++) {
        const uint32_t q = lane + DFL_LANES * u, i = ((q & ~(j - 1u)) << 1) | (q & (j - 1u));
        if (q < N / 2u && (a[u] > b[u]) == !(i & k)) ws[WS_KEY + i] = b[u], ws[WS_KEY + (i | j)] = a[u];
      }
      __syncthreads();
    }
  if (m < 2u) {
    const uint32_t key = ws[WS_KEY];
    if (m && lane == 0) fc[key & 511u] = 1u;  // length 1, code 0
    __syncthreads();
    return m ? key >> 9 : 0u;
  }
  // 2. the two-queue merge over the sorted leaves: the one serial chain, m - 1
  // steps on one lane. 3. depths top-down: a parent is made after its children.
  if (lane == 0) {
    uint32_t li = 0, ii = 0, lw = ws[WS_KEY] >> 9, iv = ~0u;  // the two queues' heads and their weights; ~0: empty
    for (uint32_t k = 0; k + 1u < m; k++) {
      uint32_t w = 0;
      for (uint32_t t = 0; t < 2u; t++) {
        if (lw <= iv) ws[WS_LP + li++] = k, w += lw, lw = li < m ? ws[WS_KEY + li] >> 9 : ~0u;
        else ws[WS_IP + ii++] = k, w += iv, iv = ii < k ? ws[WS_IW + ii] : ~0u;
      }
      ws[WS_IW + k] = w;
      if (ii == k) iv = w;  // (the node just made is the internal queue's head)
    }
    ws[WS_IP + m - 2u] = 0;
    for (uint32_t k = m - 2u; k-- > 0u;) ws[WS_IP + k] = ws[WS_IP + ws[WS_IP + k]] + 1u;
  }
  __syncthreads();
  // 4. symbols per length, the too long ones at the limit; then zlib's repair
  // on the counts, once per unit of 2^-limit that the Kraft sum is above 1
  for (uint32_t r = lane; r < m; r += DFL_LANES) {
    const uint32_t d = ws[WS_IP + ws[WS_LP + r]] + 1u;
    atomicAdd(&ws[WS_BLC + (d < limit ? d : limit)], 1u);
  }
  __syncthreads();
  if (lane == 0) {
    uint32_t sum = 0;
    for (uint32_t l = 1; l <= limit; l++) sum += ws[WS_BLC + l] << (limit - l);
    for (uint32_t over = sum > 1u << limit ? sum - (1u << limit) : 0u; over; over--) {
      uint32_t b = limit - 1u;
      while (b && !ws[WS_BLC + b]) b--;
      if (!b) break;  // (2^limit < m: no code; not reached by the caller's alphabets)
      ws[WS_BLC + b] -= 1u, ws[WS_BLC + b + 1u] += 2u, ws[WS_BLC + limit] -= 1u;
    }
  }
  __syncthreads();
  // 5. lengths by rank: the rarest symbol gets the longest code
  uint32_t cost = 0;
  for (uint32_t r = lane; r < m; r += DFL_LANES) {
    const uint32_t key = ws[WS_KEY + r];
    uint32_t l = limit;
    for (uint32_t c = ws[WS_BLC + l]; r >= c && l > 1u;) c += ws[WS_BLC + --l];
    fc[key & 511u] = l;
    cost += (key >> 9) * l;
  }
  __syncthreads();
  // 6. canonical codes: next_code on scalar registers, a symbol's place among
  // the symbols of its length by ballot, 64 symbols a step
  uint32_t nc[16];
  nc[0] = 0;
#pragma unroll
  for (uint32_t l = 1; l < 16u; l++) nc[l] = (nc[l - 1u] + (l > 1u ? uniform32(ws[WS_BLC + l - 1u]) : 0u)) << 1;
  for (uint32_t s0 = 0; s0 < nsym; s0 += DFL_LANES) {
    const uint32_t s = s0 + lane, l = s < nsym ? fc[s] : 0u;
    uint32_t code = 0;
#pragma unroll
    for (uint32_t q = 1; q < 16u; q++) {
      const uint64_t b = __ballot(l == q);
      if (l == q) code = nc[q] + (uint32_t)__popcll(b & below(lane));
      nc[q] += (uint32_t)__popcll(b);
    }
    if (l) fc[s] = (rev(code, l) << 8) | l;
  }
  __syncthreads();
  return wave_sum(cost, lane);
}

// The order in which the code-length code's lengths are sent (RFC 1951 3.2.7).
XYWS_DEV uint32_t clen_order(uint32_t i) {
  return (uint32_t)((i < 8u ? 0x0609070800121110ull : i < 16u ? 0x020D030C040B050Aull : 0x0F010Eull) >> (8u * (i & 7u))) & 0xFFu;
}

// After the counting pass of a piece (huff_block<true> without emit, whose
// result is fbits): the two codes from the histograms, into S.code, and where
// the dynamic block can be shorter than the fbits of the fixed one, its header
// bits in the workspace. Returns the header's bits with the dynamic block's
// bits in dbits, or 0 when the fixed block is no longer (a tie goes to it).
template <class LDS>  // deflate_lds_dynamic or deflate_lds_window_dynamic
XYWS_DEV uint32_t plan_piece(LDS& S, uint32_t fbits, uint32_t& dbits, uint32_t lane) {
  uint32_t* const ws = S.tab;
  __syncthreads();
  // HLIT and HDIST end at the last used symbol; the extra bits depend on the symbol alone
  const uint32_t fl = lane < 29u ? S.code[257u + lane] : 0u, fd = lane < DFL_DIST ? S.code[DFL_LITLEN + lane] : 0u;
  const uint32_t hlit = 257u + top_bit(__ballot(fl != 0u)), used_d = top_bit(__ballot(fd != 0u)), hdist = used_d ? used_d : 1u;
  const uint32_t extra = wave_sum(fl * (lane >= 8u && lane < 28u ? (lane - 4u) >> 2 : 0u) + fd * (lane >= 4u ? (lane >> 1) - 1u : 0u), lane);
  uint32_t payload = extra + build_code(ws, S.code, DFL_LITLEN, 15u, lane);
  payload += build_code(ws, S.code + DFL_LITLEN, DFL_DIST, 15u, lane);
  dbits = 0;
  if (17u + 3u * 4u + payload >= fbits) return 0;

  // the lengths, HLIT of the one code and HDIST of the other, are one sequence
  const uint32_t T = hlit + hdist;
  auto len_at = [&](uint32_t t) { return S.code[t < hlit ? t : DFL_LITLEN + t - hlit] & 0xFFu; };
  uint32_t edge = 0;  // the run that reaches this step began there
  for (uint32_t t0 = 0; t0 < T; t0 += DFL_LANES) {
    const uint32_t t = t0 + lane;
    const uint64_t b = __ballot(t < T && (t == 0 || len_at(t) != len_at(t - 1u)));
    const uint64_t mine = b & ((2ull << lane) - 1ull);
    if (t < T) ws[WS_RUN + t] = mine ? t0 + top_bit(mine) - 1u : edge;
    if (b) edge = t0 + top_bit(b) - 1u;
  }
  ws[WS_HDR + lane] = 0, ws[WS_HDR + DFL_LANES + lane] = 0;  // (the header's 76 words; nothing is live up to 128)
  if (lane < 20u) ws[WS_CLF + lane] = 0;
  __syncthreads();
  // a position's symbol, if one begins there: zeros in runs of up to 138 (18:
  // 11 and more, 17: 3 to 10), another length once and then in runs of 3 to 6 (16)
  edge = T;  // the next run behind this step begins there
  for (uint32_t t0 = (T - 1u) & ~(DFL_LANES - 1u);; t0 -= DFL_LANES) {
    const uint32_t t = t0 + lane, st = t < T ? ws[WS_RUN + t] : 0u;
    const uint64_t b = __ballot(t < T && st == t);
    const uint64_t behind = b & ~((2ull << lane) - 1ull);
    const uint32_t en = behind ? t0 + (uint32_t)__ffsll((long long)behind) - 1u : edge;
    if (t < T) {
      const uint32_t v = len_at(t), o = t - st, R = en - st;
      uint32_t sym = ~0u;
      if (v == 0) {
        const uint32_t o2 = o % 138u, c = R - (o - o2) < 138u ? R - (o - o2) : 138u;
        if (c >= 11u) sym = o2 ? ~0u : 18u | ((c - 11u) << 8);
        else if (c >= 3u) sym = o2 ? ~0u : 17u | ((c - 3u) << 8);
        else sym = 0;
      } else if (o == 0) {
        sym = v;
      } else {
        const uint32_t o2 = (o - 1u) % 6u, c = R - (o - o2) < 6u ? R - (o - o2) : 6u;
        if (c >= 3u) sym = o2 ? ~0u : 16u | ((c - 3u) << 8);
        else sym = v;
      }
      ws[WS_SEQ + t] = sym;
      if (sym != ~0u) atomicAdd(&ws[WS_CLF + (sym & 0xFFu)], 1u);
    }
    if (b) edge = t0 + (uint32_t)__ffsll((long long)b) - 1u;
    if (!t0) break;
  }
  __syncthreads();
  // the code-length code: the same builder, 19 symbols, 7 bits; HCLEN ends at the last used one in the sending order
  const uint32_t xbits = 2u * uniform32(ws[WS_CLF + 16u]) + 3u * uniform32(ws[WS_CLF + 17u]) + 7u * uniform32(ws[WS_CLF + 18u]);
  const uint32_t clbits = build_code(ws, ws + WS_CLF, DFL_CLEN, 7u, lane);
  const uint32_t mylen = lane < DFL_CLEN ? ws[WS_CLF + clen_order(lane)] & 0xFFu : 0u;
  const uint32_t last = top_bit(__ballot(mylen != 0u)), hclen = last > 4u ? last : 4u;
  const uint32_t hbits = 17u + 3u * hclen + clbits + xbits;
  dbits = hbits + payload;
  if (dbits >= fbits) return 0;

  // the header: BFINAL 0, BTYPE 10, HLIT, HDIST, HCLEN; the code-length code's lengths; the sequence
  if (lane == 0) ws[WS_HDR] = 4u | ((hlit - 257u) << 3) | ((hdist - 1u) << 8) | ((hclen - 4u) << 13);
  __syncthreads();
  if (lane < hclen && mylen) {
    const uint32_t at = 17u + 3u * lane;
    const uint64_t v = (uint64_t)mylen << (at & 31u);
    atomicOr(&ws[WS_HDR + (at >> 5)], (uint32_t)v);
    if (v >> 32) atomicOr(&ws[WS_HDR + (at >> 5) + 1u], (uint32_t)(v >> 32));
  }
  uint32_t bits = 17u + 3u * hclen;
  for (uint32_t t0 = 0; t0 < T; t0 += DFL_LANES) {
    const uint32_t t = t0 + lane, sym = t < T ? ws[WS_SEQ + t] : ~0u;
    uint32_t tb = 0, tl = 0;
    if (sym != ~0u) {
      const uint32_t c = ws[WS_CLF + (sym & 0xFFu)];
      tb = (c >> 8) | ((sym >> 8) << (c & 0xFFu));
      tl = (c & 0xFFu) + ((sym & 0xFFu) < 16u ? 0u : (sym & 0xFFu) == 16u ? 2u : (sym & 0xFFu) == 17u ? 3u : 7u);
    }
    const uint32_t incl = scan32(tl, lane);
    if (tl) {
      const uint32_t at = bits + incl - tl;
      const uint64_t v = (uint64_t)tb << (at & 31u);
      atomicOr(&ws[WS_HDR + (at >> 5)], (uint32_t)v);
      if (v >> 32) atomicOr(&ws[WS_HDR + (at >> 5) + 1u], (uint32_t)(v >> 32));
    }
    bits += lane_value(incl, DFL_LANES - 1u);
  }
  __syncthreads();
  return hbits;
}

// One fixed-Huffman block of the n (1..DFL_STAGE) staged bytes: header, tokens,
// end of block. With emit the bits go to S.out, which is zeroed first and
// begins with the `bit0` (0..7) bits of `carry` that the piece before left
// over. Returns the bit position behind the block (bit0 + its bits).
// Wave-uniform but for the lanes' own tokens.
//
// DYN (XYWS_DFO_DYNAMIC). Without emit the tokens are also counted into the
// histograms S.code, end of block once. With emit and hbits != 0 the block is
// the dynamic one that plan_piece prepared: its hbits header bits are copied
// from the workspace (before the table is zeroed for the search) and a token's
// bits are looked up in S.code; hbits == 0 emits the fixed block.
//
// WIN (xyws_deflate_windows_streams). The piece lies at byte DFL_HIST of S.in
// and the H bytes in front of it are its window. With prime the window's
// positions enter the table before the first search step, 64 a step, inserts
// only, so a match may begin there: distances reach H + n. Without prime the
// search is the one above over the piece alone, token for token. *hist is set
// when a match's source ends at or before S.in byte `front`, the record's first.
template <bool DYN, bool WIN = false>
XYWS_DEV uint32_t huff_block(typename lds_of<DYN, WIN>::type& S, uint32_t n, bool emit, uint32_t hbits, uint32_t carry,
                             uint32_t bit0, uint32_t lane, uint32_t H = 0, bool prime = false, uint32_t front = 0,
                             uint32_t* hist = nullptr) {
  const bool dyn = DYN && emit && hbits;
  const uint32_t base = WIN ? DFL_HIST : 0u, end = base + n;  // the piece: S.in[base, end)
  const uint32_t lo = WIN && prime ? base - H : base;          // the first byte a match may begin at
  const uint32_t lines = (n + n / 8u + 63u) / 16u + 1u;  // (9 n + 25 bits at most, a word of slack; <= DFL_OUT / 16)
  __syncthreads();
  if constexpr (DYN) {
    if (dyn) {  // (a dynamic block is chosen where it is shorter than the fixed one: the same lines hold it)
      for (uint32_t k = lane; k < lines; k += DFL_LANES) reinterpret_cast<u32x4*>(S.out)[k] = u32x4{k == 0 ? carry : 0u, 0, 0, 0};
      __syncthreads();
      const uint32_t* const hdr = S.tab + WS_HDR;  // (a zero word behind the bits)
      for (uint32_t w = lane; w <= (hbits + 31u) / 32u; w += DFL_LANES)
        S.out[w] |= (uint32_t)((((uint64_t)hdr[w] << 32) | (w ? hdr[w - 1u] : 0u)) >> (32u - bit0));
      __syncthreads();
    } else if (!emit) {
      for (uint32_t k = lane; k < DFL_LITLEN + DFL_DIST; k += DFL_LANES) S.code[k] = k == 256u;
    }
  }
  for (uint32_t k = lane; k < DFL_SLOTS / 4u; k += DFL_LANES) reinterpret_cast<u32x4*>(S.tab)[k] = u32x4{0, 0, 0, 0};
  if (emit && !dyn) {
    for (uint32_t k = lane; k < lines; k += DFL_LANES)
      reinterpret_cast<u32x4*>(S.out)[k] = u32x4{k == 0 ? carry | (2u << bit0) : 0u, 0, 0, 0};  // BFINAL 0, BTYPE 01
  }
  __syncthreads();
  if constexpr (WIN) {
    if (prime && DFL_WIN_PRIME) {  // (a position's 4 bytes lie in front of `end`, as the search's do)
      for (uint32_t q = lo + lane; q < base && q + DFL_MIN_MATCH <= end; q += DFL_LANES)
        atomicMax(&S.tab[(rd32(S.in, q) * 2654435761u) >> (32u - DFL_HASH_BITS)], q + 1u);
      __syncthreads();
    }
  }
  uint32_t bits = bit0 + (dyn ? hbits : 3u);
  for (uint32_t p0 = 0; p0 < n;) {
    // search: this lane's position
    const uint32_t p = base + p0 + lane;
    uint32_t mlen = 0, dist = 0, word = 0, slot = 0;
    const bool hashed = p + DFL_MIN_MATCH <= end;
    if (p < end) word = rd32(S.in, p);
    if (hashed) {
      slot = (word * 2654435761u) >> (32u - DFL_HASH_BITS);
      uint32_t c = S.tab[slot];                              // (a position of an earlier step: c - 1 < p0)
      if (p > lo && rd32(S.in, p - 1u) == word) c = p;       // a run: the byte before, distance 1
      if (c) {
        c -= 1u;
        const uint32_t maxl = end - p < DFL_MAX_MATCH ? end - p : DFL_MAX_MATCH;
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
    if constexpr (WIN) {
      if (hist && __ballot(kind == 2u && p - dist + mlen <= front)) *hist = 1u;
    }
    // emission
    uint32_t tb = 0, tl = 0;
    uint64_t tb64 = 0;  // (DYN: the token's bits, up to 15 + 5 + 15 + 13)
    if constexpr (DYN) {
      if (dyn) {
        if (kind == 1) {
          const uint32_t c = S.code[word & 0xFFu];
          tb64 = c >> 8, tl = c & 0xFFu;
        } else if (kind == 2) {
          const match_syms m = syms_of(mlen, dist);
          const uint32_t cl = S.code[m.s], cd = S.code[DFL_LITLEN + m.ds], ll = (cl & 0xFFu) + m.e, dl = cd & 0xFFu;
          tb64 = (uint64_t)((cl >> 8) | (m.x << (cl & 0xFFu))) | ((uint64_t)(cd >> 8) << ll) | ((uint64_t)m.dx << (ll + dl));
          tl = ll + dl + m.de;
        }
      } else {
        if (kind == 1) tb = litlen_code(word & 0xFFu, tl);
        else if (kind == 2) tb = match_bits(mlen, dist, tl);
        tb64 = tb;
        if (!emit) {  // the histograms
          if (kind == 1) atomicAdd(&S.code[word & 0xFFu], 1u);
          else if (kind == 2) {
            const match_syms m = syms_of(mlen, dist);
            atomicAdd(&S.code[m.s], 1u);
            atomicAdd(&S.code[DFL_LITLEN + m.ds], 1u);
          }
        }
      }
    } else {
      if (kind == 1) tb = litlen_code(word & 0xFFu, tl);
      else if (kind == 2) tb = match_bits(mlen, dist, tl);
    }
    const uint32_t incl = scan32(tl, lane);
    __syncthreads();  // (the step's lookups are done)
    if (hashed) atomicMax(&S.tab[slot], p + 1u);
    if (emit && tl) {
      const uint32_t at = bits + incl - tl;
      if constexpr (DYN) {
        const uint32_t sh = at & 31u;
        const uint64_t v = tb64 << sh;
        const uint32_t top = sh ? (uint32_t)(tb64 >> (64u - sh)) : 0u;
        atomicOr(&S.out[at >> 5], (uint32_t)v);
        if (v >> 32) atomicOr(&S.out[(at >> 5) + 1u], (uint32_t)(v >> 32));
        if (top) atomicOr(&S.out[(at >> 5) + 2u], top);
      } else {
        const uint64_t v = (uint64_t)tb << (at & 31u);
        atomicOr(&S.out[at >> 5], (uint32_t)v);
        if (v >> 32) atomicOr(&S.out[(at >> 5) + 1u], (uint32_t)(v >> 32));
      }
    }
    __syncthreads();
    bits += lane_value(incl, DFL_LANES - 1u);
    p0 += r;
  }
  if constexpr (DYN) {
    if (dyn) {  // end of block: the code of 256, at most 15 bits
      const uint32_t c = S.code[256];
      if (lane == 0) {
        const uint64_t v = (uint64_t)(c >> 8) << (bits & 31u);
        atomicOr(&S.out[bits >> 5], (uint32_t)v);
        if (v >> 32) atomicOr(&S.out[(bits >> 5) + 1u], (uint32_t)(v >> 32));
      }
      return bits + (c & 0xFFu);
    }
  }
  return bits + 7u;  // end of block: seven zero bits
}

// WIN (xyws_deflate_windows_streams, after k_room_text): a connection whose
// room takes over finds the text offset of its first record in its view result
// row, marked with the room's tag. Its records up to the room's cut are staged
// from the room's text with up to DFL_HIST bytes of window in front; each piece
// is searched without the window and with it and takes the shorter block (the
// choices of a record's first DFL_WIN_PIECES pieces are kept in a mask for the
// emitting pass; later pieces go without). Every other record takes the path
// of k_deflate_streams<false>, the piece at byte DFL_HIST of the stage.
// DYN and WIN: each of the two searches is also planned as a dynamic block, and
// every other record takes the path of k_deflate_streams<true>.
template <bool DYN, bool WIN = false>  // XYWS_DFO_DYNAMIC; xyws_deflate_windows_streams
__global__ void __launch_bounds__(DFL_LANES)
    k_deflate_streams(const xyws_reasm_conn* __restrict__ reasm, const xyws_reasm_result* __restrict__ rres,
                      const xyws_bcast_conn* __restrict__ bconns, const xyws_deflate_conn* __restrict__ dconns, uint64_t n,
                      xyws_reasm_conn* __restrict__ view, xyws_reasm_result* __restrict__ vres,
                      xyws_bcast_conn* __restrict__ vbconns, xyws_deflate_result* __restrict__ results,
                      const xyws_deflate_room* __restrict__ drooms = nullptr, xyws_deflate_room_result* droom_results = nullptr,
                      uint64_t n_rooms = 0) {
  __shared__ typename lds_of<DYN, WIN>::type S;
  uint32_t* const s_piece = S.in + (WIN ? DFL_HIST / 4u : 0u);
  const uint32_t lane = threadIdx.x;
  for (uint64_t ci = blockIdx.x; ci < n; ci += gridDim.x) {
    // WIN: the room's text, this connection's place in it, the room's cut and result row
    uint64_t text = 0, tpos = 0, cut = 0;
    xyws_deflate_room_result* rrow = nullptr;
    bool desync = false;
    if constexpr (WIN) {
      const uint64_t room = uniform32(rows::load_bcast_room(bconns + ci));
      if (room < n_rooms) {
        const rows::deflate_room_row dr = rows::load_deflate_room(drooms + room);
        const rows::reasm_result_row mark = rows::load_reasm_result<true>(vres + ci);
        if (dr.text && dr.carry && mark.nmsgs == (DFL_WIN_TAG ^ room)) {
          text = dr.text, tpos = mark.out_len, rrow = droom_results + room;
          cut = rows::load_deflate_room_result(rrow).cut;
        }
      }
    }
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
    uint32_t st = 0, n_deflated = 0, n_stored = 0, n_dynamic = 0;
    for (uint32_t j = 0; j < stored; j++) {
      const xyws_message* const rp = rows::row_at<const xyws_message>(msgs, j);
      frame_info f;
      if (!frame_of(rp, m, 0, 0, f)) continue;
      bool inwin = false;  // WIN: the record lies in the room's text, at offset P
      uint64_t P = 0;
      if constexpr (WIN) {
        if (text) {
          const uint64_t Lt = hl + uniform64(f.len);
          P = tpos, tpos += Lt;
          inwin = P + Lt <= cut;
        }
      }
      if (found++ >= dq.vmsg_cap) {
        st |= XYWS_DFL_MSG_CAP;
        desync |= inwin;
        continue;
      }
      const rows::message_row rec = rows::load_message<true>(rp);
      const uint64_t msg = mout + uniform64(f.off), L = hl + uniform64(f.len);
      const uint64_t blocks = (L + DFL_STORED_MAX - 1u) / DFL_STORED_MAX, stored_len = L + 5u * blocks + 1u;
      const bool single = L <= DFL_STAGE;

      // the Huffman form's bits: a record of one piece is emitted into LDS on the
      // way; under DYN every piece is planned (the shorter of its two blocks), a
      // record of one piece keeps its plan for the emission
      uint64_t fbits = 0;
      uint32_t hbits = 0, dynamic = 0;  // the last piece's dynamic header, 0: fixed; pieces that chose the dynamic block
      uint64_t wmask = 0;               // WIN: bit k: piece k goes out as the block searched with the window
      uint64_t dmask = 0;               // DYN and WIN: bit k: piece k goes out as a dynamic block
      uint32_t hist = 0;                // WIN: such a block has a match whose source lies in front of the record
      bool staged = single;             // the stage holds the record's one block when the counting is done
      bool planned = true;              // DYN and WIN: the plan in LDS (codes, header, hbits) is the chosen block's
      for (uint64_t q0 = 0; q0 < L; q0 += DFL_STAGE) {
        const uint32_t pn = L - q0 < DFL_STAGE ? (uint32_t)(L - q0) : DFL_STAGE;
        if constexpr (DYN && WIN) {
          // four candidates: the search without the window and the one with it, each counted into its
          // own histograms and planned; without before with, fixed before dynamic (plan_piece's tie)
          const uint64_t k = q0 / DFL_STAGE;
          uint32_t H = 0;
          if (inwin) {
            const uint64_t T = P + q0;
            H = T < DFL_HIST ? (uint32_t)T : DFL_HIST;
            stage_text(S.in, text, T, H, pn, lane);
          } else {
            stage_piece(s_piece, head, hl, msg, q0, pn, lane);
          }
          uint32_t db;
          const uint32_t pf = huff_block<true, true>(S, pn, false, 0, 0, 0, lane);
          hbits = plan_piece(S, pf, db, lane);
          uint32_t best = hbits ? db : pf;
          if (H && k < DFL_WIN_PIECES) {
            const uint32_t front = q0 < DFL_HIST ? DFL_HIST - (uint32_t)q0 : 0u;
            uint32_t h = 0;
            const uint32_t wf = huff_block<true, true>(S, pn, false, 0, 0, 0, lane, H, true, front, &h);
            const uint32_t wh = plan_piece(S, wf, db, lane), wbest = wh ? db : wf;
            planned = wbest < best;  // (the codes and the header in LDS are the window's now)
            if (planned) wmask |= 1ull << k, hist |= h, best = wbest, hbits = wh;
          }
          if (hbits && k < DFL_WIN_PIECES) dmask |= 1ull << k;
          fbits += best;
          dynamic += hbits != 0u;
          continue;
        } else if constexpr (WIN) {
          if (inwin) {
            const uint64_t T = P + q0, k = q0 / DFL_STAGE;
            const uint32_t H = T < DFL_HIST ? (uint32_t)T : DFL_HIST;
            stage_text(S.in, text, T, H, pn, lane);
            if (H && k < DFL_WIN_PIECES) {
              const uint32_t front = q0 < DFL_HIST ? DFL_HIST - (uint32_t)q0 : 0u;
              uint32_t h = 0;
              const uint32_t pb = huff_block<false, true>(S, pn, false, 0, 0, 0, lane);
              const uint32_t wb = huff_block<false, true>(S, pn, single, 0, 0, 0, lane, H, true, front, &h);
              if (wb < pb) wmask |= 1ull << k, hist |= h, fbits += wb;
              else staged = false, fbits += pb;
            } else {
              fbits += huff_block<false, true>(S, pn, single, 0, 0, 0, lane);
            }
            continue;
          }
        }
        stage_piece(s_piece, head, hl, msg, q0, pn, lane);
        if constexpr (DYN) {  // (without WIN: with it every piece took the branch at the top)
          const uint32_t fb = huff_block<true, WIN>(S, pn, false, 0, 0, 0, lane);
          uint32_t db;
          hbits = plan_piece(S, fb, db, lane);
          fbits += hbits ? db : fb;
          dynamic += hbits != 0u;
        } else {
          fbits += huff_block<false, WIN>(S, pn, single, 0, 0, 0, lane);
        }
      }
      const uint64_t fixed_len = (fbits + 3u + 7u) >> 3;  // behind it the empty stored block: 3 bits, then to the byte
      const bool fixed = L && fixed_len < stored_len;
      const uint64_t clen = fixed ? fixed_len : stored_len;
      const bool fits = in_range(opos, clen, dq.out_cap);
      const uint64_t D = olo + opos;  // the record's first byte, from obase

      if (!fits) {
        st |= XYWS_DFL_TOO_LONG;
      } else if (!DYN && fixed && staged) {
        flush_stage(S.out, (uint32_t)clen, obase, D, lane);
      } else if (fixed) {
        uint64_t at = D;
        uint32_t carry = 0, bit0 = 0;
        for (uint64_t q0 = 0; q0 < L; q0 += DFL_STAGE) {
          const uint32_t pn = L - q0 < DFL_STAGE ? (uint32_t)(L - q0) : DFL_STAGE;
          bool win = false;  // WIN: this piece's block is the one searched with its window of wh bytes
          uint32_t wh = 0;
          if constexpr (DYN && WIN) {
            // the chosen search again, and its plan where the block is dynamic; a record of one
            // piece is staged still and keeps the plan if the last one made is the chosen block's
            const uint64_t k = q0 / DFL_STAGE;
            if (inwin) {
              const uint64_t T = P + q0;
              wh = T < DFL_HIST ? (uint32_t)T : DFL_HIST;
              if (!single) stage_text(S.in, text, T, wh, pn, lane);
              win = k < DFL_WIN_PIECES && ((wmask >> k) & 1u);
            } else if (!single) {
              stage_piece(s_piece, head, hl, msg, q0, pn, lane);
            }
            if (!single || !planned) {
              hbits = 0;
              if (k >= DFL_WIN_PIECES || ((dmask >> k) & 1u)) {  // (behind the masks: planned again, as without WIN)
                uint32_t db;
                hbits = plan_piece(S, huff_block<true, true>(S, pn, false, 0, 0, 0, lane, wh, win), db, lane);
              }
            }
          } else if constexpr (DYN) {
            if (!single) {  // the piece's plan again: the codes of the one before it are gone
              stage_piece(S.in, head, hl, msg, q0, pn, lane);
              uint32_t db;
              hbits = plan_piece(S, huff_block<true>(S, pn, false, 0, 0, 0, lane), db, lane);
            }
          } else if (WIN && inwin) {
            if constexpr (WIN) {
              const uint64_t T = P + q0, k = q0 / DFL_STAGE;
              const uint32_t H = T < DFL_HIST ? (uint32_t)T : DFL_HIST;
              if (!single) stage_text(S.in, text, T, H, pn, lane);  // (a record of one piece is staged still)
              win = k < DFL_WIN_PIECES && ((wmask >> k) & 1u), wh = H;
            }
          } else {
            stage_piece(s_piece, head, hl, msg, q0, pn, lane);
          }
          const uint32_t end = huff_block<DYN, WIN>(S, pn, true, hbits, carry, bit0, lane, wh, win);
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
            if (!single) {
              if (WIN && inwin) stage_text(S.in, text, P + b0 + q, 0, pn, lane);
              else stage_piece(s_piece, head, hl, msg, b0 + q, pn, lane);
            }
            flush_stage(s_piece, pn, obase, at, lane);
            at += pn;
          }
        }
        if (lane == 0) obase[at] = 0;  // the empty stored block, its 00 00 ff ff left out
      }
      if (fits) {
        in_len += L;
        if (fixed) n_deflated++, n_dynamic += dynamic != 0u;
        else n_stored++;
      }
      if constexpr (WIN) {
        desync |= inwin && !fits;
        if (inwin && fits && fixed && hist && lane == 0) rows::count_deflate_room_history(rrow);
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
    if constexpr (WIN) {
      if (desync && lane == 0) rows::raise_deflate_room_status(rrow, XYWS_DFR_DESYNC);
    }
    if (lane == 0) {
      rows::store_reasm_conn(view + ci, {dq.out, dq.out_cap, mc, dq.vmsgs, dq.vmsg_cap});
      const uint32_t rst = (opos > dq.out_cap ? XYWS_RSM_TRUNCATED : 0u) | (found > kept ? XYWS_RSM_MSG_CAP : 0u);
      rows::store_reasm_result(vres + ci, {opos, found, {(uint32_t)kept, rst}, 0});
      if (results) {
        if constexpr (DYN) rows::store_deflate_result_dynamic(results + ci, opos, in_len, {n_deflated, n_stored}, st, n_dynamic);
        else rows::store_deflate_result(results + ci, opos, in_len, {n_deflated, n_stored}, st);
      }
    }
  }
}

// xyws_deflate_windows_streams, first launch: a room's text. One workgroup per
// room, the members in tiles of one per thread, as k_room_wire walks them
// (load_member and frame_of decide what is deliverable; a record contributes
// head | message, no frame header):
//   1. the thread sizes its member's records; a workgroup scan places the
//      member in the text, behind the history the room begins the call with;
//   2. the member whose range crosses text_cap walks its records once more for
//      the first one that does not fit: the smallest such offset is the room's
//      cut (an LDS atomic min), nothing at or behind it is written;
//   3. each member's view result row gets the text offset of its first record
//      and the room's tag, which the compression reads;
//   4. the tile's bytes go to the text in 16-byte lines (xyws_lines.h), as the
//      wire build composes them.
// The room's result row carries the history's length and the cut on to the
// other two launches. A room without text or carry gets a zero row.
__global__ void __launch_bounds__(DFL_TEXT_THREADS)
    k_room_text(const xyws_reasm_conn* __restrict__ reasm, const xyws_reasm_result* __restrict__ rres,
                const xyws_bcast_conn* __restrict__ bconns, uint64_t n, const xyws_room* __restrict__ rooms,
                const xyws_deflate_room* __restrict__ drooms, const xyws_roster_room_result* __restrict__ last_roster,
                uint64_t n_rooms, xyws_reasm_result* __restrict__ vres, xyws_deflate_room_result* __restrict__ droom_results) {
  constexpr uint32_t TILE = DFL_TEXT_THREADS;
  __shared__ uint64_t s_off[TILE + 1];
  __shared__ uint64_t s_msgs[TILE], s_gate[TILE], s_out[TILE], s_ocap[TILE], s_head[TILE], s_hlen[TILE];
  __shared__ uint32_t s_stored[TILE];
  __shared__ uint64_t s_w[TILE / BC_WAVE];
  __shared__ unsigned long long s_cut;
  const uint32_t tid = threadIdx.x;
  for (uint64_t ri = blockIdx.x; ri < n_rooms; ri += gridDim.x) {
    const rows::room_row rq = rows::load_room(rooms + ri);
    const rows::deflate_room_row dr = rows::load_deflate_room(drooms + ri);
    if (!dr.text || !dr.carry) {
      if (tid == 0) rows::store_deflate_room_result(droom_results + ri, {0, {0, 0}, {0, 0}, 0});
      continue;
    }
    g_u8* const tbase = (g_u8*)(dr.text & ~15ull);
    const uint64_t tlo = dr.text & 15u;
    uint64_t h0 = rows::load_deflate_room_carry((const xyws_deflate_room_carry*)dr.carry).hist_len;
    if (h0 > XYWS_DFL_WINDOW) h0 = XYWS_DFL_WINDOW;
    if (h0 > dr.text_cap) h0 = dr.text_cap;
    uint32_t st = 0;
    if (last_roster && rows::load_roster_joined(last_roster + ri)) h0 = 0, st = XYWS_DFR_RESET;
    if (tid == 0) s_cut = XYWS_NPOS;
    __syncthreads();

    uint64_t wpos = h0;  // the text so far, from `text` (uniform)
    uint32_t c_recs = 0;
    for (uint64_t base = 0; base < rq.n_members; base += TILE) {
      // 1. this thread's member: one of this room's, by its own row too
      member m = {0, 0, 0, 0, 0, 0, 0};
      uint64_t size = 0, ci = n;
      if (base + tid < rq.n_members) {
        ci = ((const XYWS_GLOBAL uint32_t*)rq.members)[base + tid];
        if (ci < n && rows::load_bcast_room(bconns + ci) == ri) {
          bool receiver, over_cap;
          load_member(reasm, rres, bconns, ci, m, receiver, over_cap);
#pragma unroll 1
          for (uint32_t r = 0; r < m.stored; r++) {
            frame_info f;
            if (frame_of(rows::row_at<const xyws_message>(m.msgs, r), m, 0, 0, f)) size += m.head_len + f.len, c_recs++;
          }
        } else {
          ci = n;
        }
      }
      uint64_t total;
      const uint64_t incl = block_scan(size, tid, s_w, total);
      const uint64_t o0 = wpos, o1 = wpos + total, mine = o0 + (incl - size);
      // 2. the cut
      if (ci < n && mine + size > dr.text_cap) {
        uint64_t at = mine;
#pragma unroll 1
        for (uint32_t r = 0; r < m.stored; r++) {
          frame_info f;
          if (!frame_of(rows::row_at<const xyws_message>(m.msgs, r), m, 0, 0, f)) continue;
          if (at + m.head_len + f.len > dr.text_cap) break;
          at += m.head_len + f.len;
        }
        atomicMin(&s_cut, (unsigned long long)at);
      }
      // 3. the member's place, for the compression
      if (ci < n) rows::store_reasm_result(vres + ci, {mine, DFL_WIN_TAG ^ ri, {0, 0}, 0});
      s_off[tid] = mine;
      s_msgs[tid] = m.msgs;
      s_gate[tid] = m.gate;
      s_out[tid] = m.out;
      s_ocap[tid] = m.out_cap;
      s_head[tid] = m.head;
      s_hlen[tid] = m.head_len;
      s_stored[tid] = size ? m.stored : 0u;
      if (tid == 0) s_off[TILE] = o1;
      __syncthreads();

      // 4. the tile's bytes [o0, min(o1, cut))
      const uint64_t cut = s_cut, oe = o1 < cut ? o1 : cut;
      const uint64_t P0 = tlo + o0, P1 = tlo + oe;
      if (oe > o0) {
        for (uint64_t A = ((P0 >> 4) + tid) << 4; A < P1; A += (uint64_t)BC_LINE * TILE) {
          const uint64_t s = A > P0 ? A : P0, e = A + 16 < P1 ? A + 16 : P1;
          uint64_t q = s - tlo;
          uint32_t i = item_at(s_off, TILE, q);
          bytes16 acc = {0, 0};
          uint32_t a = (uint32_t)(s - A);
          const uint32_t ae = (uint32_t)(e - A);
          while (a < ae && i < TILE) {
            member k;
            k.msgs = s_msgs[i];
            k.gate = s_gate[i];
            k.out = s_out[i];
            k.out_cap = s_ocap[i];
            k.head = s_head[i];
            k.head_len = s_hlen[i];
            k.stored = s_stored[i];
            uint64_t fo = s_off[i];  // the start of the record under test
#pragma unroll 1
            for (uint32_t r = 0; r < k.stored && a < ae; r++) {
              frame_info f;
              if (!frame_of(rows::row_at<const xyws_message>(k.msgs, r), k, 0, 0, f)) continue;
              const uint64_t rsz = k.head_len + f.len;
              if (fo + rsz > q) {
                uint64_t rr = q - fo;
                if (rr < k.head_len) {  // head bytes rr.. at line offset a
                  const uint64_t left = k.head_len - rr;
                  const uint32_t nb = left < ae - a ? (uint32_t)left : ae - a;
                  add_bytes(acc, a, q, load_bytes(k.head + rr, nb), nb);
                  rr += nb;
                }
                if (a < ae && rr < rsz) {  // message bytes
                  const uint64_t left = rsz - rr;
                  const uint32_t nb = left < ae - a ? (uint32_t)left : ae - a;
                  add_bytes(acc, a, q, load_bytes(k.out + f.off + (rr - k.head_len), nb), nb);
                }
              }
              fo += rsz;
            }
            i++;
          }
          put_line(tbase, A, s, e, P0, P1, acc);
        }
      }
      wpos = o1;
      __syncthreads();  // (LDS is rewritten by the next tile)
    }

    uint64_t recs;
    block_scan((uint64_t)c_recs, tid, s_w, recs);
    if (tid == 0) {
      const uint64_t cut = s_cut;
      if (cut != XYWS_NPOS) st |= XYWS_DFR_TEXT_CAP;
      rows::store_deflate_room_result(droom_results + ri, {wpos - h0, {(uint32_t)recs, 0}, {st, (uint32_t)h0}, cut});
    }
    __syncthreads();  // (s_cut and s_w are reused by the next room)
  }
}

// xyws_deflate_windows_streams, last launch: the room's history for the next
// sweep. One workgroup per room: the last XYWS_DFL_WINDOW bytes of history and
// text move to the front of the text, ascending, a chunk's loads before its
// stores (source and destination overlap below twice the window); the carry
// gets the new length. After XYWS_DFR_TEXT_CAP or XYWS_DFR_DESYNC the history
// is empty; a room with no record that was not reset keeps text and carry.
__global__ void __launch_bounds__(DFL_SLIDE_THREADS)
    k_room_slide(const xyws_deflate_room* __restrict__ drooms, uint64_t n_rooms, xyws_deflate_room_result* __restrict__ droom_results) {
  const uint32_t tid = threadIdx.x;
  for (uint64_t ri = blockIdx.x; ri < n_rooms; ri += gridDim.x) {
    const rows::deflate_room_row dr = rows::load_deflate_room(drooms + ri);
    if (!dr.text || !dr.carry) continue;
    rows::deflate_room_result_row rr = rows::load_deflate_room_result(droom_results + ri);
    xyws_deflate_room_carry* const carry = (xyws_deflate_room_carry*)dr.carry;
    const uint64_t h0 = rr.state.hist0, total = h0 + rr.text_len;
    const bool empty = (rr.state.status & (XYWS_DFR_TEXT_CAP | XYWS_DFR_DESYNC)) != 0;
    const uint64_t keep = empty ? 0 : total < XYWS_DFL_WINDOW ? total : XYWS_DFL_WINDOW;
    const uint64_t sweeps = h0 ? rows::load_deflate_room_carry(carry).n_sweeps : 0;
    __syncthreads();  // (every thread has the row before it is rewritten)
    if (keep && total > keep) {
      g_u8* const tbase = (g_u8*)(dr.text & ~15ull);
      const uint64_t P0 = dr.text & 15u, P1 = P0 + keep, src = dr.text + (total - keep);
      for (uint64_t A0 = 0; A0 < P1; A0 += 16u * DFL_SLIDE_THREADS) {
        const uint64_t A = A0 + 16u * tid;
        const uint64_t s = A > P0 ? A : P0, e = A + 16 < P1 ? A + 16 : P1;
        bytes16 v = {0, 0};
        if (A < P1) v = shl_bytes(low_bytes(load_bytes(src + (s - P0), (uint32_t)(e - s)), (uint32_t)(e - s)), (uint32_t)(s - A));
        __syncthreads();
        if (A < P1) put_line(tbase, A, s, e, P0, P1, v);
        __syncthreads();
      }
    }
    if (tid == 0) {
      if (rr.counts.n_records || (rr.state.status & XYWS_DFR_RESET))
        rows::store_deflate_room_carry(carry, keep, keep ? sweeps + (rr.counts.n_records ? 1u : 0u) : 0);
      rr.state.hist0 = 0, rr.cut = 0;
      rows::store_deflate_room_result(droom_results + ri, rr);
    }
  }
}

// xyws_debug_deflate_code_lengths: one wave, build_code over the caller's frequencies.
__global__ void __launch_bounds__(DFL_LANES)
    k_code_lengths(const uint32_t* __restrict__ freq, uint32_t nsym, uint32_t limit, uint8_t* __restrict__ lens) {
  __shared__ uint32_t ws[DFL_SLOTS], fc[DFL_LITLEN];
  const uint32_t lane = threadIdx.x;
  for (uint32_t s = lane; s < nsym; s += DFL_LANES) fc[s] = freq[s];
  build_code(ws, fc, nsym, limit, lane);
  for (uint32_t s = lane; s < nsym; s += DFL_LANES) lens[s] = (uint8_t)fc[s];
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
  if ((opts & ~XYWS_DFO_DYNAMIC) || n >= UINT32_MAX) return XYWS_ERR_INVALID;
  if (!n) return XYWS_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  device_guard g(ctx->device);
  if (!g.ok) return XYWS_ERR_HIP;
  const uint32_t grid = grid_for(n, 1, DFL_GRID_CAP);
  if (opts & XYWS_DFO_DYNAMIC)
    hipLaunchKernelGGL(k_deflate_streams<true>, dim3(grid), dim3(DFL_LANES), 0, (hipStream_t)stream, dev_reasm, dev_reasm_results,
                       dev_bconns, dev_dconns, n, dev_view, dev_view_results, dev_view_bconns, dev_results, nullptr, nullptr, 0);
  else
    hipLaunchKernelGGL(k_deflate_streams<false>, dim3(grid), dim3(DFL_LANES), 0, (hipStream_t)stream, dev_reasm, dev_reasm_results,
                       dev_bconns, dev_dconns, n, dev_view, dev_view_results, dev_view_bconns, dev_results, nullptr, nullptr, 0);
  return hip_err(hipGetLastError());
}

int xyws_deflate_windows_streams(xyws_ctx* ctx, const xyws_reasm_conn* dev_reasm, const xyws_reasm_result* dev_reasm_results,
                                 const xyws_bcast_conn* dev_bconns, const xyws_deflate_conn* dev_dconns, uint64_t n,
                                 const xyws_room* dev_rooms, const xyws_deflate_room* dev_drooms,
                                 const xyws_roster_room_result* dev_last_roster, uint64_t n_rooms, uint32_t opts,
                                 xyws_reasm_conn* dev_view, xyws_reasm_result* dev_view_results, xyws_bcast_conn* dev_view_bconns,
                                 xyws_deflate_result* dev_results, xyws_deflate_room_result* dev_droom_results, void* stream) {
  if (!ctx || (n && (!dev_reasm || !dev_reasm_results || !dev_bconns || !dev_dconns || !dev_view || !dev_view_results ||
                     !dev_view_bconns)))
    return XYWS_ERR_INVALID;
  if (n_rooms && (!dev_rooms || !dev_drooms || !dev_droom_results)) return XYWS_ERR_INVALID;
  if ((opts & ~XYWS_DFO_WINDOW_DYNAMIC) || n >= UINT32_MAX || n_rooms >= UINT32_MAX) return XYWS_ERR_INVALID;
  if (!n) return XYWS_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  device_guard g(ctx->device);
  if (!g.ok) return XYWS_ERR_HIP;
  const hipStream_t s = (hipStream_t)stream;
  const auto sibling = opts ? k_deflate_streams<true> : k_deflate_streams<false>;
  const auto windows = opts ? k_deflate_streams<true, true> : k_deflate_streams<false, true>;
  if (!n_rooms) {  // nobody takes over: the sibling's launch
    hipLaunchKernelGGL(sibling, dim3(grid_for(n, 1, DFL_GRID_CAP)), dim3(DFL_LANES), 0, s, dev_reasm, dev_reasm_results,
                       dev_bconns, dev_dconns, n, dev_view, dev_view_results, dev_view_bconns, dev_results, nullptr, nullptr, 0);
    return hip_err(hipGetLastError());
  }
  const uint32_t rgrid = grid_for(n_rooms, 1, BC_GRID_CAP);
  hipLaunchKernelGGL(k_room_text, dim3(rgrid), dim3(DFL_TEXT_THREADS), 0, s, dev_reasm, dev_reasm_results, dev_bconns, n,
                     dev_rooms, dev_drooms, dev_last_roster, n_rooms, dev_view_results, dev_droom_results);
  int rc = hip_err(hipGetLastError());
  if (rc != XYWS_OK) return rc;
  hipLaunchKernelGGL(windows, dim3(grid_for(n, 1, DFL_WIN_GRID_CAP)), dim3(DFL_LANES), 0, s, dev_reasm, dev_reasm_results,
                     dev_bconns, dev_dconns, n, dev_view, dev_view_results, dev_view_bconns, dev_results, dev_drooms,
                     dev_droom_results, n_rooms);
  rc = hip_err(hipGetLastError());
  if (rc != XYWS_OK) return rc;
  hipLaunchKernelGGL(k_room_slide, dim3(rgrid), dim3(DFL_SLIDE_THREADS), 0, s, dev_drooms, n_rooms, dev_droom_results);
  return hip_err(hipGetLastError());
}

// Internal (tests and measurements, no HIP call): the geometry of
// k_deflate_streams<false, true> and <true, true>. out: {stage bytes W, window bytes in front of
// a piece, hash slots, grid cap, wave size, the room's history in bytes}.
int xyws_debug_deflate_windows_geometry(uint64_t out[6]) {
  if (!out) return XYWS_ERR_INVALID;
  out[0] = DFL_STAGE;
  out[1] = DFL_HIST;
  out[2] = DFL_SLOTS;
  out[3] = DFL_WIN_GRID_CAP;
  out[4] = DFL_LANES;
  out[5] = XYWS_DFL_WINDOW;
  static_assert(sizeof(deflate_lds_window) * (DFL_WIN_GRID_CAP / 256u) <= 160u * 1024u, "four waves' LDS per CU");
  static_assert(sizeof(deflate_lds_window_dynamic) * (DFL_WIN_GRID_CAP / 256u) <= 160u * 1024u,
                "and with XYWS_DFO_WINDOW_DYNAMIC: the same grid cap");
  return XYWS_OK;
}

// Internal (tests and measurements): build_code, the device function the
// dynamic blocks' codes come from, by one wave over the frequencies
// dev_freq[0, nsym) (each below 2^22, no more than 2^limit of them non-zero);
// dev_lens[s] is symbol s's code length. The host cannot see the frequencies:
// outside those two conditions the call still returns XYWS_OK and writes
// nothing out of bounds, but the lengths are undefined and may be no code.
int xyws_debug_deflate_code_lengths(xyws_ctx* ctx, const uint32_t* dev_freq, uint32_t nsym, uint32_t limit, uint8_t* dev_lens,
                                    void* stream) {
  if (!ctx || !dev_freq || !dev_lens || !nsym || nsym > DFL_LITLEN || !limit || limit > 15u) return XYWS_ERR_INVALID;
  std::lock_guard<std::mutex> lk(ctx->mu);
  device_guard g(ctx->device);
  if (!g.ok) return XYWS_ERR_HIP;
  hipLaunchKernelGGL(k_code_lengths, dim3(1), dim3(DFL_LANES), 0, (hipStream_t)stream, dev_freq, nsym, limit, dev_lens);
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
  static_assert(sizeof(deflate_lds_dynamic) * (DFL_GRID_CAP / 256u) <= 160u * 1024u, "six waves' LDS per CU");
  return XYWS_OK;
}

}  // extern "C"

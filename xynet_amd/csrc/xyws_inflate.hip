// xyws_inflate.hip — xyws_inflate_streams: the permessage-deflate messages of a
// sweep (RFC 7692, negotiated with no context takeover by XYWS_ACC_DEFLATE)
// inflated on the device between xyws_hold_streams and xyws_broadcast_streams.
// The semantics are stated in include/xyws.h; this is how they are computed
// (DESIGN.md 4.18). Every table row is read and written through xyws_rows.h.
//
// As in its siblings one wave (a 64-thread workgroup) takes one connection,
// connections are grid-strided, no workgroup talks to another, nothing spins,
// there are no atomics. DEFLATE is one dependent chain of bits, so the wave
// walks it together: the bit buffer, the positions and every decision are
// wave-uniform (scalar registers), and the lanes share the parts that are wide:
//   input    the message's bytes come from global memory as whole 16-byte lines
//            (line_of, xyws_lines.h) into a 2 KiB LDS stage, the four tail
//            bytes 00 00 ff ff behind them; the reader refills a 64-bit bit
//            buffer from three staged words, once per symbol;
//   tables   canonical codes: the symbols sorted by (length, symbol) in LDS
//            and, in lane L, the end of the length-L codes on a 15-bit scale
//            and the offset of their symbols. A symbol is one ballot: lanes
//            1..15 compare the next 15 bits (first bit highest) with their end
//            and the lowest lane that is above them is the length. The tables
//            are built by the whole wave: counts per length by ballots, the
//            ends and offsets by a wave scan, the sorted symbols by one lane
//            per symbol. The fixed tables are built the same way, once per
//            wave, from lengths the lanes compute;
//   output   a 32 KiB ring in LDS at the destination's own line offsets, so a
//            finished 16-byte line of the ring is a 16-byte line of global
//            memory: whole-line stores, byte stores on the range's first and
//            last line (put_line). A literal goes to the lane of its place in
//            the run (a compare and a select, no LDS access, no wave-wide
//            step) and a run goes to the ring in one store when a match or the
//            64th literal ends it. A match is copied by all lanes: byte k from
//            start + k when the distance covers the length, from
//            start + k % distance when it repeats. Matches never leave LDS;
//   UTF-8    each lane judges the line it writes out, with the three ring
//            bytes in front of it (the rules of k_reasm_streams).
//   window   xyws_inflate_windows_streams launches the second instantiation,
//            k_inflate_streams<true>: a connection whose client keeps its
//            context has its last 32 KiB of inflated bytes in a window in
//            global memory, the ring's own image. The history is loaded into
//            the ring before the connection's first compressed record, records
//            go on where the history ends (so the ring keeps the history's
//            phase, not the destination's, and write_out funnels each line out
//            of six ring words), and what the call added is stored back at its
//            end. <false> is the code it was: every difference is behind
//            `if constexpr`;
// LDS: 32 KiB ring + 2 KiB stage + 2.3 KiB of code lengths and symbols: four
// waves per CU on gfx950's 160 KiB (one per SIMD); the grid cap is that.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>

#include "xyws.h"
#include "xyws_device.h"
#include "xyws_ctx.h"
#include "xyws_frameops.h"
#include "xyws_lines.h"
#include "xyws_rows.h"

#define INF_LANES 64u
#define INF_LINE 16u
#define INF_STEP (INF_LINE * INF_LANES)  // bytes a connection's wave copies or writes out per step
#define INF_WINDOW 32768u                // the ring: DEFLATE's largest distance
#define INF_STAGE 2048u                  // compressed bytes staged at once
#define INF_FLUSH 8192u                  // ring bytes not yet in global memory that start a write-out
#define INF_GRID_CAP 1024u               // 256 CUs x 4 one-wave workgroups (LDS); further connections are grid-strided
#define INF_NLIT 288u
#define INF_NDIST 32u
#define INF_NCLEN 19u

using namespace xyws_internal;
namespace rows = xyws_rows;

namespace {

constexpr uint32_t RING = INF_WINDOW - 1u;
constexpr uint32_t NO_SYMBOL = 0xFFFFu;
constexpr uint32_t R_BAD = 1u, R_LONG = 2u, R_UTF8 = 4u;  // what inflate_message returns

XYWS_DEV bool is_cont(uint32_t b) { return (b & 0xC0u) == 0x80u; }
XYWS_DEV uint64_t below(uint32_t p) { return (1ull << p) - 1ull; }  // (p < 64)
XYWS_DEV uint32_t scan32(uint32_t v, uint32_t lane) {  // inclusive, across the wave
#pragma unroll
  for (uint32_t d = 1; d < INF_LANES; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)v, d);
    if (lane >= d) v += o;
  }
  return v;
}
XYWS_DEV uint32_t lane_value(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }

// The order in which a dynamic block sends its code-length code lengths
// (RFC 1951 3.2.7), five bits each in two words: no table in memory.
constexpr uint64_t clen_order_word(uint32_t from) {
  constexpr uint8_t ord[INF_NCLEN] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  uint64_t w = 0;
  for (uint32_t i = 0; i < 12 && from + i < INF_NCLEN; i++) w |= (uint64_t)ord[from + i] << (5u * i);
  return w;
}
XYWS_DEV uint32_t clen_order(uint32_t i) {
  constexpr uint64_t lo = clen_order_word(0), hi = clen_order_word(12);
  return (uint32_t)((i < 12 ? lo >> (5u * i) : hi >> (5u * (i - 12))) & 31u);
}

// One canonical code as the lanes hold it: in lane L (1..15) the end of the
// codes of length <= L on the 15-bit scale (the Kraft sum so far, 32768 = a
// complete code) and what is added to a length-L code to find its symbol among
// the sorted ones.
struct code_table {
  uint32_t end;
  int32_t base;
};

// The table of the n code lengths len[0, n) (LDS), its symbols sorted into
// sym[0, coded). Returns the Kraft sum (> 32768: over-subscribed, never
// decoded with); coded: the symbols that have a code.
XYWS_DEV uint32_t build_table(const uint8_t* len, uint32_t n, uint16_t* sym, uint32_t lane, code_table& t, uint32_t& coded) {
  uint32_t cnt = 0;  // lane L: the codes of length L
  for (uint32_t c0 = 0; c0 < n; c0 += INF_LANES) {
    const uint32_t i = c0 + lane, l = i < n ? len[i] : 0u;
#pragma unroll
    for (uint32_t L = 1; L <= 15; L++) {
      const uint32_t c = (uint32_t)__popcll(__ballot(l == L));
      if (lane == L) cnt += c;
    }
  }
  const bool mine = lane >= 1 && lane <= 15;
  t.end = scan32(mine ? cnt << (15u - lane) : 0u, lane);
  const uint32_t upto = scan32(cnt, lane), off = upto - cnt;
  const uint32_t before = (uint32_t)__shfl_up((int)t.end, 1);
  t.base = mine ? (int32_t)off - (int32_t)(before >> (15u - lane)) : 0;  // (lane 1: before is lane 0's, 0)
  uint32_t next = off;
  for (uint32_t c0 = 0; c0 < n; c0 += INF_LANES) {
    const uint32_t i = c0 + lane, l = i < n ? len[i] : 0u;
#pragma unroll
    for (uint32_t L = 1; L <= 15; L++) {
      const uint64_t m = __ballot(l == L);
      const uint32_t at = lane_value(next, L);
      if (l == L) sym[at + (uint32_t)__popcll(m & below(lane))] = (uint16_t)i;  // (at + rank < coded <= n)
      if (lane == L) next += (uint32_t)__popcll(m);
    }
  }
  coded = lane_value(upto, 15);
  return lane_value(t.end, 15);
}

// The symbol that the low bits of bb begin with and its length (NO_SYMBOL: no
// code begins so; the table is not over-subscribed).
XYWS_DEV uint32_t decode(uint64_t bb, const code_table& t, const uint16_t* sym, uint32_t lane, uint32_t& nbits) {
  const uint32_t c = __brev((uint32_t)bb) >> 17;  // the next 15 bits, the first one highest
  const uint64_t hit = __ballot(c < t.end) & 0xFFFEull;
  if (!hit) {
    nbits = 0;
    return NO_SYMBOL;
  }
  const uint32_t L = (uint32_t)__ffsll((long long)hit) - 1u;
  nbits = L;
  const int32_t b = (int32_t)lane_value((uint32_t)t.base, L);
  return uniform32(sym[b + (int32_t)(c >> (15u - L))]);
}

// A complete lit/len or distance code, or the one incomplete form RFC 1951
// allows (a single code of length 1); none: no code at all.
XYWS_DEV bool code_ok(uint32_t kraft, uint32_t coded, bool none_ok) {
  return kraft == 32768u || (kraft == 16384u && coded == 1u) || (none_ok && coded == 0u);
}

// What one wave keeps in LDS.
struct inflate_lds {
  __attribute__((aligned(16))) uint8_t win[INF_WINDOW];
  __attribute__((aligned(16))) uint8_t in[INF_STAGE];
  uint8_t len[INF_NLIT + INF_NDIST];  // a dynamic block's code lengths, lit/len then distance
  uint8_t clen[32];
  uint16_t lsym[INF_NLIT], dsym[INF_NDIST];    // the dynamic block's sorted symbols
  uint16_t flsym[INF_NLIT], fdsym[INF_NDIST];  // the fixed block's
  uint16_t csym[32];
};
static_assert(4 * sizeof(inflate_lds) <= 160 * 1024, "four one-wave workgroups per CU, with or without a window");

// Positions q count from the 16-byte-aligned address at or below the message's
// first byte: the message is [lo, hi), the tail [hi, hi + 4), zeros follow.
// Stages q in [sq, sq + INF_STAGE), sq a multiple of 16.
XYWS_DEV void stage_input(uint8_t* s_in, const g_u8* base, uint64_t lo, uint64_t hi, uint64_t sq, uint32_t lane) {
  __syncthreads();
  for (uint32_t k = lane; k < INF_STAGE / INF_LINE; k += INF_LANES) {
    const uint64_t A = sq + INF_LINE * k;
    bytes16 v = {0, 0};
    if (A < hi && A + 16 > lo) {  // a line that holds one of the message's bytes
      const uint32_t s = A < lo ? (uint32_t)(lo - A) : 0u, e = A + 16 > hi ? (uint32_t)(hi - A) : 16u;
      v = shl_bytes(low_bytes(shr_bytes(line_of(base + A), s), e - s), s);
    }
#pragma unroll
    for (uint32_t t = 2; t < 4; t++) {  // ff ff at hi + 2, hi + 3
      const uint64_t p = hi + t;
      if (p >= A && p < A + 16) {
        const bytes16 f = shl_bytes(bytes16{0xFFull, 0}, (uint32_t)(p - A));
        v.lo |= f.lo;
        v.hi |= f.hi;
      }
    }
    *reinterpret_cast<u32x4*>(s_in + INF_LINE * k) =
        u32x4{(uint32_t)v.lo, (uint32_t)(v.lo >> 32), (uint32_t)v.hi, (uint32_t)(v.hi >> 32)};
  }
  __syncthreads();
}

// The 8 staged bytes at offset o (any alignment; o <= INF_STAGE - 16), wave-uniform.
XYWS_DEV uint64_t staged64(const uint8_t* s_in, uint32_t o) {
  const uint32_t* const w = reinterpret_cast<const uint32_t*>(s_in) + (o >> 2);
  const uint32_t sh = o & 3u, w0 = w[0], w1 = w[1], w2 = w[2];
  return uniform64((uint64_t)__builtin_amdgcn_alignbyte(w1, w0, sh) | ((uint64_t)__builtin_amdgcn_alignbyte(w2, w1, sh) << 32));
}

// Ring positions W count from the 16-byte-aligned address at or below the
// record's first destination byte (dbase): the record is [W0, ..), at most
// [W0, wlim) is written. Writes out [wf, the last finished line), or with
// `final` everything up to we; returns the new wf. utf8: judge the bytes
// written; *bad is each lane's own. With a window (T) the ring keeps the
// history's own phase: position W lies at ring byte W + rd, any alignment, and
// a line is funnelled out of the six ring words that hold it and the four bytes
// in front of it (each word wraps on its own).
template <bool T>
XYWS_DEV uint64_t write_out(const uint8_t* s_win, g_u8* dbase, uint64_t W0, uint64_t wlim, uint64_t wf, uint64_t we,
                            bool final, bool utf8, uint32_t lane, bool* bad, uint32_t rd) {
  const uint64_t upto = final ? we : we & ~15ull;
  if (upto <= wf) return wf;
  const uint64_t wl = upto < wlim ? upto : wlim;
  for (uint64_t A0 = wf & ~15ull; A0 < wl; A0 += INF_STEP) {
    const uint64_t A = A0 + INF_LINE * lane;
    if (A >= wl) break;
    u32x4 x;
    uint32_t pw;  // the 4 ring bytes before the line
    if constexpr (T) {
      const uint32_t i = (uint32_t)A + rd - 4u, sh = i & 3u;
      const uint32_t* const w = reinterpret_cast<const uint32_t*>(s_win);
      uint32_t d[6];
#pragma unroll
      for (uint32_t k = 0; k < 6; k++) d[k] = w[((i >> 2) + k) & (INF_WINDOW / 4u - 1u)];
      pw = __builtin_amdgcn_alignbyte(d[1], d[0], sh);
      x = u32x4{__builtin_amdgcn_alignbyte(d[2], d[1], sh), __builtin_amdgcn_alignbyte(d[3], d[2], sh),
                __builtin_amdgcn_alignbyte(d[4], d[3], sh), __builtin_amdgcn_alignbyte(d[5], d[4], sh)};
    } else {
      x = *reinterpret_cast<const u32x4*>(s_win + ((uint32_t)A & RING));
    }
    bytes16 v = {(uint64_t)x.x | ((uint64_t)x.y << 32), (uint64_t)x.z | ((uint64_t)x.w << 32)};
    const uint64_t s = A > wf ? A : wf, e = A + 16 < upto ? A + 16 : upto;
    put_line(dbase, A, s, e, W0, wlim, v);
    if (!utf8) continue;
    // the line and the 4 ring bytes before it, those in front of the record zero (also where they are history)
    if constexpr (!T) pw = *reinterpret_cast<const uint32_t*>(s_win + ((uint32_t)(A - 4) & RING));
    if (A < W0 + 4) {
      const uint32_t z = (uint32_t)(W0 + 4 - A);  // 1..19 bytes of the 20
      pw = z >= 4 ? 0u : pw & (0xFFFFFFFFu << (8u * z));
      if (z > 4) v = shl_bytes(shr_bytes(v, z - 4), z - 4);
    }
    if (!((v.lo | v.hi | pw) & 0x8080808080808080ull)) continue;  // (ASCII: no rule can fail)
    const uint32_t ja = (uint32_t)(s - A), jb = (uint32_t)((e < wl ? e : wl) - A);
    const uint32_t w0 = pw, w1 = (uint32_t)v.lo, w2 = (uint32_t)(v.lo >> 32), w3 = (uint32_t)v.hi, w4 = (uint32_t)(v.hi >> 32);
    bool b = false;
#pragma unroll
    for (uint32_t q = 0; q < 16; q++) {
      if (q < ja || q >= jb) continue;
      // the byte at q and the 3 before it: bytes q + 1 .. q + 4 of the 20
      const uint32_t k = (q + 1) >> 2, sh = (q + 1) & 3u;
      const uint32_t wl_ = k == 0 ? w0 : k == 1 ? w1 : k == 2 ? w2 : k == 3 ? w3 : w4;
      const uint32_t wh_ = k == 0 ? w1 : k == 1 ? w2 : k == 2 ? w3 : w4;  // (k == 4 comes with sh == 0 only)
      const uint32_t win = sh ? __builtin_amdgcn_alignbyte(wh_, wl_, sh) : wl_;
      if (!(win & 0x80808080u)) continue;
      const uint32_t b3 = win & 0xFFu, b2 = (win >> 8) & 0xFFu, b1 = (win >> 16) & 0xFFu, b0 = win >> 24;
      const uint32_t l1 = lead_len(b1), l2 = lead_len(b2), l3 = lead_len(b3);
      if (is_cont(b0)) b = b || !(l1 > 1 || l2 > 2 || l3 > 3);  // claimed by a lead at most 3 bytes before it
      else if (b0 == 0xC0u || b0 == 0xC1u || b0 >= 0xF5u) b = true;
      // a sequence that ends here is judged whole
      if (l1 == 2) b = b || !is_cont(b0);
      if (l2 == 3) b = b || !is_cont(b1) || !is_cont(b0) || utf8_second_bad(b2, b1);
      if (l3 == 4) b = b || !is_cont(b2) || !is_cont(b1) || !is_cont(b0) || utf8_second_bad(b3, b2);
    }
    if (b) *bad = true;
  }
  return upto;
}

// Inflates the len bytes at src (and the tail) to dbase + [W0, ..), at most
// `room` bytes of them written. *length: the inflated length, room + 1 when it
// does not fit, 0 when the data are bad. Wave-uniform throughout. With a
// window (T) the record's first byte lies at ring byte r0, behind `hist` bytes
// of history that a distance may reach; *reached: one did.
template <bool T>
XYWS_DEV uint32_t inflate_message(inflate_lds& S, uint64_t src, uint64_t len, g_u8* dbase, uint64_t W0, uint64_t room,
                                  bool utf8, bool& have_fixed, code_table& fl, code_table& fd, uint32_t lane,
                                  uint64_t* length, uint32_t r0, uint32_t hist, bool* reached) {
  const g_u8* const base = (const g_u8*)(src & ~15ull);
  const uint64_t lo = src & 15u, hi = lo + len;
  const uint64_t total = 8u * (len + 4u);  // bits of input (len < 2^60: it lies in device memory)
  const uint64_t wlim = sat_add(W0, room);
  uint64_t sq = 0, iq = lo;  // staged from; the next byte to enter the bit buffer
  uint64_t bb = 0;
  uint32_t nb = 0;
  uint64_t op = 0, wf = W0;  // bytes inflated; written out up to
  uint32_t lit = 0, nlit = 0;  // a run of literals: literal k in lane k
  bool bad = false, lng = false, ubad = false;
  const uint32_t rd = T ? r0 - (uint32_t)W0 : 0u;
  auto ring_at = [&](uint32_t k) -> uint32_t {  // the ring byte of the record's byte op + k
    return T ? (r0 + (uint32_t)op + k) & RING : (uint32_t)(W0 + op + k) & RING;
  };

  stage_input(S.in, base, lo, hi, sq, lane);
  auto refill = [&]() {  // 56..63 bits
    if (iq - sq > INF_STAGE - 16u) {
      sq = iq & ~15ull;
      stage_input(S.in, base, lo, hi, sq, lane);
    }
    bb |= staged64(S.in, (uint32_t)(iq - sq)) << nb;
    iq += (63u - nb) >> 3;
    nb |= 56u;
  };
  auto take = [&](uint32_t n) -> uint32_t {  // (n <= 16)
    const uint32_t v = (uint32_t)bb & ((1u << n) - 1u);
    bb >>= n;
    nb -= n;
    return v;
  };
  auto used = [&]() -> uint64_t { return 8u * (iq - lo) - nb; };
  auto put_lits = [&]() {
    if (nlit) {
      if (lane < nlit) S.win[ring_at(lane)] = (uint8_t)lit;
      op += nlit;
      nlit = 0;
    }
  };
  auto after_output = [&]() {  // the cap, and the ring's write-out
    if (op > room) lng = true;
    else if (W0 + op - wf >= INF_FLUSH) {
      __syncthreads();
      wf = write_out<T>(S.win, dbase, W0, wlim, wf, W0 + op, false, utf8, lane, &ubad, rd);
    }
  };

  for (bool last = false; !last && !bad && !lng;) {
    refill();
    if (used() >= total) {  // the input used up at a block boundary
      bad = used() > total;
      break;
    }
    const uint32_t hdr = take(3);
    last = hdr & 1u;
    const uint32_t type = hdr >> 1;
    if (type == 3) {
      bad = true;
    } else if (type == 0) {
      take(nb & 7u);  // to the byte boundary
      const uint32_t blen = take(16), nlen = take(16);
      uint64_t p = iq - (nb >> 3);  // the block's first byte
      if ((blen ^ nlen) != 0xFFFFu || p - lo > len + 4 || blen > len + 4 - (p - lo)) {
        bad = true;
        break;
      }
      for (uint32_t left = blen; left && !lng;) {
        if (p < sq || p >= sq + INF_STAGE) {
          sq = p & ~15ull;
          stage_input(S.in, base, lo, hi, sq, lane);
        }
        const uint64_t have = sq + INF_STAGE - p;
        const uint32_t nn = left < have ? left : (uint32_t)have;
        __syncthreads();
        for (uint32_t k = lane; k < nn; k += INF_LANES) S.win[ring_at(k)] = S.in[(uint32_t)(p - sq) + k];
        op += nn;
        p += nn;
        left -= nn;
        after_output();
      }
      iq = p;
      bb = 0;
      nb = 0;
    } else {
      const uint16_t *lsym, *dsym;
      code_table tl, td;
      if (type == 1) {
        if (!have_fixed) {  // once per wave: lit/len 8, 9, 7, 8 bits, 32 distance codes of 5
          __syncthreads();
          for (uint32_t i = lane; i < INF_NLIT + INF_NDIST; i += INF_LANES)
            S.len[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < INF_NLIT ? 8 : 5);
          __syncthreads();
          uint32_t coded;
          build_table(S.len, INF_NLIT, S.flsym, lane, fl, coded);
          build_table(S.len + INF_NLIT, INF_NDIST, S.fdsym, lane, fd, coded);
          __syncthreads();
          have_fixed = true;
        }
        tl = fl;
        td = fd;
        lsym = S.flsym;
        dsym = S.fdsym;
      } else {
        const uint32_t hlit = take(5) + 257u, hdist = take(5) + 1u, hclen = take(4) + 4u;
        if (hlit > 286u || hdist > 30u) {
          bad = true;
          break;
        }
        __syncthreads();
        if (lane < 32) S.clen[lane] = 0;
        __syncthreads();
        for (uint32_t i = 0; i < hclen; i++) {
          if (!(i & 15u)) refill();
          const uint32_t v = take(3);
          if (lane == 0) S.clen[clen_order(i)] = (uint8_t)v;
        }
        __syncthreads();
        code_table tc;
        uint32_t coded;
        if (build_table(S.clen, INF_NCLEN, S.csym, lane, tc, coded) != 32768u) {
          bad = true;
          break;
        }
        __syncthreads();
        // the code lengths, one dependent chain: they are Huffman-coded themselves
        const uint32_t want = hlit + hdist;
        uint32_t prev = 0;
        for (uint32_t i = 0; i < want && !bad;) {
          refill();
          uint32_t nbits;
          const uint32_t s = decode(bb, tc, S.csym, lane, nbits);
          if (s == NO_SYMBOL) {
            bad = true;
            break;
          }
          take(nbits);
          if (s < 16) {
            if (lane == 0) S.len[i] = (uint8_t)s;
            prev = s;
            i++;
          } else {
            uint32_t rep, val = 0;
            if (s == 16) {
              rep = 3u + take(2);
              val = prev;
              if (!i) bad = true;  // nothing to repeat
            } else if (s == 17) {
              rep = 3u + take(3);
            } else {
              rep = 11u + take(7);
            }
            if (bad || rep > want - i) {
              bad = true;
              break;
            }
            for (uint32_t k = lane; k < rep; k += INF_LANES) S.len[i + k] = (uint8_t)val;
            prev = val;
            i += rep;
          }
          if (used() > total) bad = true;
        }
        if (bad) break;
        __syncthreads();
        if (!uniform32(S.len[256])) {  // no end-of-block code
          bad = true;
          break;
        }
        const uint32_t kl = build_table(S.len, hlit, S.lsym, lane, tl, coded);
        const bool lok = code_ok(kl, coded, false);
        const uint32_t kd = build_table(S.len + hlit, hdist, S.dsym, lane, td, coded);
        if (!lok || !code_ok(kd, coded, true)) {
          bad = true;
          break;
        }
        __syncthreads();
        lsym = S.lsym;
        dsym = S.dsym;
      }
      // the block's symbols
      for (;;) {
        refill();  // enough for a length and a distance with their extra bits: 15 + 5 + 15 + 13
        uint32_t nbits;
        const uint32_t s = decode(bb, tl, lsym, lane, nbits);
        if (s == NO_SYMBOL) {
          bad = true;
          break;
        }
        take(nbits);
        if (s < 256) {
          if (lane == nlit) lit = s;
          if (++nlit == INF_LANES) {
            put_lits();
            after_output();
          }
          if (used() > total) bad = true;
          if (bad || lng) break;
          continue;
        }
        if (s == 256) break;
        if (s >= 286) {
          bad = true;
          break;
        }
        uint32_t mlen;
        if (s < 265) {
          mlen = s - 254u;
        } else if (s == 285) {
          mlen = 258u;
        } else {
          const uint32_t e = (s - 261u) >> 2;
          mlen = 3u + ((4u + ((s - 261u) & 3u)) << e) + take(e);
        }
        const uint32_t d = decode(bb, td, dsym, lane, nbits);
        if (d == NO_SYMBOL || d >= 30) {
          bad = true;
          break;
        }
        take(nbits);
        uint32_t dist;
        if (d < 4) {
          dist = d + 1u;
        } else {
          const uint32_t e = (d >> 1) - 1u;
          dist = 1u + ((2u + (d & 1u)) << e) + take(e);
        }
        put_lits();
        // input ended inside the block; a distance in front of the first byte (of the history's, with a window)
        if (used() > total || (T ? dist > op + hist : dist > op)) {
          bad = true;
          break;
        }
        if constexpr (T) {
          if (dist > op) *reached = true;
        }
        __syncthreads();
        const uint32_t to = T ? r0 + (uint32_t)op : (uint32_t)(W0 + op), from = to - dist;
        for (uint32_t k = lane; k < mlen; k += INF_LANES)
          S.win[(to + k) & RING] = S.win[(from + (dist >= mlen ? k : k % dist)) & RING];
        __syncthreads();
        op += mlen;
        after_output();
        if (lng) break;
      }
      put_lits();
      if (used() > total) bad = true;
      if (!bad && !lng) after_output();
    }
  }

  if (bad) {
    *length = 0;
    return R_BAD;
  }
  __syncthreads();
  wf = write_out<T>(S.win, dbase, W0, wlim, wf, W0 + op, true, utf8 && !lng, lane, &ubad, rd);
  if (lng) {
    *length = room + 1;
    return R_LONG;
  }
  *length = op;
  bool u = __ballot(ubad) != 0;
  if (utf8 && op) {  // a sequence that runs past the message's last byte
    const uint32_t e = T ? r0 + (uint32_t)op : (uint32_t)(W0 + op);
    const uint32_t b0 = S.win[(e - 1) & RING], b1 = op > 1 ? S.win[(e - 2) & RING] : 0u, b2 = op > 2 ? S.win[(e - 3) & RING] : 0u;
    u = u || uniform32(lead_len(b0) > 1 || lead_len(b1) > 2 || lead_len(b2) > 3);
  }
  return u ? R_UTF8 : 0u;
}

// The window of a connection that keeps its client's context is the ring's own
// image: window[i] is ring byte i, and the carry says where the history ends
// (win_pos) and how long it is (win_len). Linear positions below count ring
// bytes from one turn before win_pos, so the history is [e - win_len, e) with
// e = win_pos + INF_WINDOW and nothing is negative.

// The history's bytes from the window into the ring: whole 16-byte lines, the
// bytes of the first and last line that are not history masked off. A history
// within two lines of the full ring may begin and end in the same ring line:
// then every line is taken whole (all of the window is the connection's).
XYWS_DEV void restore_window(uint8_t* s_win, const g_u8* window, uint32_t win_len, uint32_t win_pos, uint32_t lane) {
  const uint32_t e = win_pos + INF_WINDOW, b = e - win_len;
  const bool masks = win_len <= INF_WINDOW - 2u * INF_LINE;
  __syncthreads();
  for (uint32_t A0 = b & ~15u; A0 < e; A0 += INF_STEP) {
    const uint32_t A = A0 + INF_LINE * lane;
    if (A >= e) break;
    const uint32_t o = A & RING;  // (a multiple of 16, <= INF_WINDOW - 16)
    bytes16 v = line_of(window + o);
    if (masks) {
      const uint32_t s = A < b ? b - A : 0u, n = (A + 16u > e ? e - A : 16u) - s;
      v = shl_bytes(low_bytes(shr_bytes(v, s), n), s);
    }
    *reinterpret_cast<u32x4*>(s_win + o) = u32x4{(uint32_t)v.lo, (uint32_t)(v.lo >> 32), (uint32_t)v.hi, (uint32_t)(v.hi >> 32)};
  }
  __syncthreads();
}

// The last `fresh` bytes of the history (what this call added, 1..INF_WINDOW)
// from the ring to the window: whole lines, byte stores on the first and last.
XYWS_DEV void save_window(const uint8_t* s_win, g_u8* window, uint32_t fresh, uint32_t win_pos, uint32_t lane) {
  const uint32_t e = win_pos + INF_WINDOW, b = e - fresh;
  __syncthreads();
  for (uint32_t A0 = b & ~15u; A0 < e; A0 += INF_STEP) {
    const uint32_t A = A0 + INF_LINE * lane;
    if (A >= e) break;
    const uint32_t o = A & RING;
    const u32x4 x = *reinterpret_cast<const u32x4*>(s_win + o);
    const bytes16 v = {(uint64_t)x.x | ((uint64_t)x.y << 32), (uint64_t)x.z | ((uint64_t)x.w << 32)};
    const uint32_t s = A < b ? b - A : 0u, n = A + 16u > e ? e - A : 16u;
    put_line(window, o, o + s, o + n, 0, INF_WINDOW, v);
  }
}

template <bool T>
__global__ void __launch_bounds__(INF_LANES)
    k_inflate_streams(const xyws_conn* __restrict__ conns, const xyws_reasm_conn* __restrict__ in,
                      const xyws_reasm_result* __restrict__ ires, const xyws_hold_result* __restrict__ hres,
                      const xyws_inflate_conn* __restrict__ iconns, uint64_t n, uint32_t opts,
                      xyws_reasm_conn* __restrict__ view, xyws_reasm_result* __restrict__ vres,
                      xyws_inflate_result* __restrict__ results) {
  __shared__ inflate_lds S;
  const uint32_t lane = threadIdx.x;
  bool have_fixed = false;
  code_table fl = {0, 0}, fd = {0, 0};
  for (uint64_t ci = blockIdx.x; ci < n; ci += gridDim.x) {
    const xyws_reasm_conn* const rp = in + ci;
    const xyws_reasm_result* const ap = ires + ci;
    xyws_reasm_conn* const vq = view + ci;
    xyws_reasm_result* const vr = vres + ci;
    xyws_inflate_result* const res = results ? results + ci : nullptr;
    const rows::inflate_conn_row iq = rows::load_inflate_conn(iconns + ci);
    xyws_inflate_carry* const ic = (xyws_inflate_carry*)iq.ic;

    // 1. pass-through: the inputs verbatim
    if (!(iq.flags & XYWS_INFC_NEGOTIATED) || !iq.out || !ic) {
      rows::copy_row(vq, rp, lane);
      rows::copy_row(vr, ap, lane);
      if (res) rows::store_inflate_status(res, XYWS_INF_PASSTHROUGH, lane);
      continue;
    }

    const rows::reasm_conn_row rq = rows::load_reasm_conn<true>(rp);
    const rows::reasm_result_row ar = rows::load_reasm_result<true>(ap);
    const rows::conn_row cq = rows::load_conn(conns + ci);
    const uint64_t ccarry = rows::load_conn_carry(conns + ci);
    const rows::inflate_kept kept = rows::load_inflate_carry(ic);
    const bool delivered = hres && (rows::load_hold_status(hres + ci) & XYWS_HOLD_DELIVERED);
    // the client's context: the history (in the window until a record needs it), what this call added to it
    bool takeover = false, in_ring = false;
    rows::inflate_history hist = {0, 0};
    uint64_t window = 0;
    uint32_t fresh = 0, n_history = 0;
    if constexpr (T) {
      window = rows::load_inflate_window(iconns + ci);
      takeover = (iq.flags & XYWS_INFC_TAKEOVER) && window && !(window & 15u);
      if (takeover) {
        hist = rows::load_inflate_history(ic);
        if (hist.win_len > INF_WINDOW) hist.win_len = 0;  // (no carry this call wrote)
        hist.win_pos &= RING;
      }
    }
    const uint64_t nmsgs = ar.nmsgs, s = nmsgs < rq.msg_cap ? nmsgs : rq.msg_cap;
    const uint64_t vs = s < iq.vmsg_cap ? s : iq.vmsg_cap;
    const uint64_t out = iq.out, out_cap = iq.out_cap;
    uint32_t st = 0, n_inflated = 0, n_bad = 0;

    // 2. whether record j is a compressed message
    auto compressed = [&](uint64_t j, const rows::message_row& rec) -> bool {
      if ((j == 0 && delivered) || (rows::unpack_message_meta(rec.meta).status & XYWS_MSG_CONTINUED))
        return (kept.flags & XYWS_INFK_COMPRESSED) != 0;
      uint32_t b0 = 0x100u;  // byte 0 of its first frame's header
      if (cq.frames && rec.first_frame < cq.cap) {
        const int64_t fo = rows::load_frame_off(rows::row_at<const xyws_frame>(cq.frames, rec.first_frame));
        if (fo < 0) {
          if (kept.flags & XYWS_INFK_HDR0) b0 = kept.hdr0;
        } else if (cq.buf && (uint64_t)fo < cq.len) {
          b0 = uniform32(((const g_u8*)cq.buf)[fo]);
        }
      }
      if (b0 > 0xFFu) {
        st |= XYWS_INF_UNKNOWN;
        return false;
      }
      return (b0 & 0x40u) != 0;
    };

    // 3. the records, in order
    uint64_t opos = 0;
    bool anybad = false, last_compressed = false;
    for (uint64_t j = 0; j < vs; j++) {
      rows::message_row rec = rows::load_message<true>(rows::row_at<const xyws_message>(rq.msgs, j));
      const rows::message_meta m = rows::unpack_message_meta(rec.meta);
      uint32_t ms = m.status;
      const bool comp = compressed(j, rec);
      last_compressed = comp;
      const uint64_t D = out + opos, room = opos < out_cap ? out_cap - opos : 0;
      const bool whole = (ms & XYWS_MSG_COMPLETE) && !(ms & (XYWS_MSG_CONTINUED | XYWS_MSG_TRUNCATED | XYWS_MSG_INTERRUPTED)) &&
                         in_range(rec.out_off, rec.length, rq.out_cap);
      uint64_t L = rec.length;
      if (comp && whole) {
        const bool text = m.opcode == XYWS_FLAG_OP_TEXT;
        bool reached = false;
        if constexpr (T) {
          if (takeover && !in_ring) {
            if (hist.win_len) restore_window(S.win, (const g_u8*)window, hist.win_len, hist.win_pos, lane);
            in_ring = true;
          }
        }
        const uint32_t r = inflate_message<T>(S, rq.out + rec.out_off, rec.length, (g_u8*)(D & ~15ull), D & 15u, room,
                                              (opts & XYWS_INF_UTF8) && text, have_fixed, fl, fd, lane, &L,
                                              takeover ? hist.win_pos : (uint32_t)(D & 15u), takeover ? hist.win_len : 0u, &reached);
        if constexpr (T) {
          if (takeover && (r & (R_BAD | R_LONG))) {  // the context ends: the rest of the call goes without
            takeover = false;
            hist = {0, 0};
            fresh = 0;
          } else if (takeover) {  // (L <= room < 2^60)
            hist.win_len = (uint32_t)(hist.win_len + L < INF_WINDOW ? hist.win_len + L : INF_WINDOW);
            hist.win_pos = (hist.win_pos + (uint32_t)L) & RING;
            fresh = (uint32_t)(fresh + L < INF_WINDOW ? fresh + L : INF_WINDOW);
            if (reached) n_history++;
          }
        }
        ms &= ~(XYWS_MSG_UTF8_BAD | XYWS_MSG_UNCHECKED);
        if (r & R_BAD) {
          ms |= XYWS_MSG_TRUNCATED;
          st |= XYWS_INF_BAD_DATA;
          n_bad++;
        } else if (r & R_LONG) {
          ms |= XYWS_MSG_TRUNCATED;
          st |= XYWS_INF_TOO_LONG;
        } else {
          n_inflated++;
          if (r & R_UTF8) ms |= XYWS_MSG_UTF8_BAD;
        }
      } else {
        // copied: what of its bytes the input's range holds, as far as this one's has room
        const uint64_t readable = rec.out_off < rq.out_cap ? rq.out_cap - rec.out_off : 0;
        uint64_t cl = L < readable ? L : readable;
        if (cl > room) cl = room;
        if (cl) copy_span((g_u8*)(D & ~15ull), D & 15u, (D & 15u) + cl, rq.out + rec.out_off, 0, INF_STEP, lane);
        if (comp && (ms & (XYWS_MSG_COMPLETE | XYWS_MSG_INTERRUPTED))) ms |= XYWS_MSG_TRUNCATED;
        if (L > room) {
          ms |= XYWS_MSG_TRUNCATED;
          st |= XYWS_INF_TOO_LONG;
        }
      }
      if (ms & XYWS_MSG_UTF8_BAD) anybad = true;
      if (lane == 0)
        rows::store_message(rows::row_at<xyws_message>(iq.vmsgs, j),
                            {rec.first_frame, rec.nframes, opos, L, rows::pack_message_meta({ms, m.opcode})});
      opos += L;
    }

    // the carry: the answer of the message open at the end, the first byte of a cut header
    uint32_t kf = 0, hdr0 = 0;
    if ((ar.counts.status & XYWS_RSM_OPEN) && nmsgs && nmsgs - 1 < s) {
      bool c = last_compressed;  // (record nmsgs - 1 is the last of the loop when the view stores it)
      if (nmsgs - 1 >= vs) c = compressed(nmsgs - 1, rows::load_message<true>(rows::row_at<const xyws_message>(rq.msgs, nmsgs - 1)));
      if (c) kf |= XYWS_INFK_COMPRESSED;
    }
    if (ccarry) {
      const rows::carry_head h = rows::load_carry((const xyws_carry*)ccarry).head;
      if (h.hdr_len) {
        kf |= XYWS_INFK_HDR0;
        hdr0 = (uint32_t)(h.hdr_lo & 0xFFu);
      }
    }

    if constexpr (T) {
      if (takeover && fresh) save_window(S.win, (g_u8*)window, fresh, hist.win_pos, lane);
    }
    if (lane == 0) {
      rows::store_inflate_carry(ic, {kf, hdr0}, hist);
      rows::store_reasm_conn(vq, {out, out_cap, rq.mc, iq.vmsgs, rq.msg_cap < iq.vmsg_cap ? rq.msg_cap : iq.vmsg_cap});
      const uint32_t rst = (ar.counts.status & ~XYWS_RSM_UTF8_BAD) | (opos > out_cap ? XYWS_RSM_TRUNCATED : 0u) |
                           (s > iq.vmsg_cap ? XYWS_RSM_MSG_CAP : 0u) | (anybad ? XYWS_RSM_UTF8_BAD : 0u);
      rows::store_reasm_result(vr, {opos, nmsgs, {ar.counts.completed, rst}, ar.reserved});
      if (res) rows::store_inflate_result(res, opos, {n_inflated, n_bad}, {st, n_history});
    }
  }
}

}  // namespace

// Both entry points: the refusals, then one launch of the instantiation asked for.
template <bool T>
static int inflate_call(xyws_ctx* ctx, const xyws_conn* dev_conns, const xyws_reasm_conn* dev_in,
                        const xyws_reasm_result* dev_in_results, const xyws_hold_result* dev_hold_results,
                        const xyws_inflate_conn* dev_iconns, uint64_t n, uint32_t opts, xyws_reasm_conn* dev_view,
                        xyws_reasm_result* dev_view_results, xyws_inflate_result* dev_results, void* stream) {
  if (!ctx || (n && (!dev_conns || !dev_in || !dev_in_results || !dev_iconns || !dev_view || !dev_view_results)))
    return XYWS_ERR_INVALID;
  if ((opts & ~XYWS_INF_UTF8) || n >= UINT32_MAX) return XYWS_ERR_INVALID;
  if (!n) return XYWS_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  device_guard g(ctx->device);
  if (!g.ok) return XYWS_ERR_HIP;
  const uint32_t grid = grid_for(n, 1, INF_GRID_CAP);
  hipLaunchKernelGGL(k_inflate_streams<T>, dim3(grid), dim3(INF_LANES), 0, (hipStream_t)stream, dev_conns, dev_in,
                     dev_in_results, dev_hold_results, dev_iconns, n, opts, dev_view, dev_view_results, dev_results);
  return hip_err(hipGetLastError());
}

extern "C" {

int xyws_inflate_streams(xyws_ctx* ctx, const xyws_conn* dev_conns, const xyws_reasm_conn* dev_in,
                         const xyws_reasm_result* dev_in_results, const xyws_hold_result* dev_hold_results,
                         const xyws_inflate_conn* dev_iconns, uint64_t n, uint32_t opts, xyws_reasm_conn* dev_view,
                         xyws_reasm_result* dev_view_results, xyws_inflate_result* dev_results, void* stream) {
  return inflate_call<false>(ctx, dev_conns, dev_in, dev_in_results, dev_hold_results, dev_iconns, n, opts, dev_view,
                             dev_view_results, dev_results, stream);
}

int xyws_inflate_windows_streams(xyws_ctx* ctx, const xyws_conn* dev_conns, const xyws_reasm_conn* dev_in,
                                 const xyws_reasm_result* dev_in_results, const xyws_hold_result* dev_hold_results,
                                 const xyws_inflate_conn* dev_iconns, uint64_t n, uint32_t opts, xyws_reasm_conn* dev_view,
                                 xyws_reasm_result* dev_view_results, xyws_inflate_result* dev_results, void* stream) {
  return inflate_call<true>(ctx, dev_conns, dev_in, dev_in_results, dev_hold_results, dev_iconns, n, opts, dev_view,
                            dev_view_results, dev_results, stream);
}

// Internal (tests and measurements, no HIP call): the geometry of
// k_inflate_streams. out: {lanes per connection, ring bytes, LDS bytes per
// wave, grid cap}.
int xyws_debug_inflate_geometry(uint64_t out[4]) {
  if (!out) return XYWS_ERR_INVALID;
  out[0] = INF_LANES;
  out[1] = INF_WINDOW;
  out[2] = sizeof(inflate_lds);
  out[3] = INF_GRID_CAP;
  return XYWS_OK;
}

}  // extern "C"

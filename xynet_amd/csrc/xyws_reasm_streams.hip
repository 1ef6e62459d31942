// xyws_reasm_streams.hip — xyws_reassemble_streams: FIN=0 reassembly with
// UTF-8 validation for many connections' frame tables in one launch (what the
// reference's chat server does once per connection and sweep,
// example/websocket/websocket_chat.cpp:177-200). The semantics are those of
// xyws_reassemble_stream per connection, stated in include/xyws.h; this is how
// they are computed. Every table row is read and written through xyws_rows.h,
// which names its words.
//
// As in k_reply_streams (xyws_reply.hip) one wave (a 64-thread workgroup)
// takes one connection, connections are grid-strided, no workgroup talks to
// another and nothing spins. A connection's table is taken in tiles of
// RSM_TILE frames, one frame per lane:
//   1. membership. Whether a message is open changes only at text/binary
//      frames and at FIN continuations; their positions come from ballots, and
//      a loop over those bits alone (wave-uniform, in scalar registers) walks
//      the state (none / open / closing) and leaves four masks: frames that
//      join a message, orphans, starts that interrupt a message, frames that
//      complete one;
//   2. a wave scan of the joined frames' in-batch byte counts gives each item's
//      offset in out; items (out offset, source offset) and the tile's message
//      segments (start in out, message start, flags) go to LDS. Item 0 of the
//      first tile is the carried prefix; segment 0 is the message open at the
//      tile's start;
//   3. the copy phase is k_reply_streams' without headers: a lane per 16-byte
//      line of out (xyws_lines.h), its item from item_at;
//   4. UTF-8 on the composed lines, in registers: a lane looks at its line and
//      the 3 bytes before it (the neighbour lane's, the previous step's, or a
//      wave-uniform tail of the previous tile / the carry's utf8 bytes). Every
//      rule is judged looking back: a sequence where it ends, a continuation
//      byte against the leads before it, a cut sequence at the message's last
//      byte. A bad bit per segment accumulates in LDS;
//   5. the records of the messages that end in the tile are written by one lane
//      each; the message still open goes on in scalars.
// The carry and the result are written once at the end.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>

#include "xyws.h"
#include "xyws_device.h"
#include "xyws_ctx.h"
#include "xyws_frameops.h"
#include "xyws_lines.h"
#include "xyws_rows.h"

#define RSM_TILE 64u       // frames per tile: one per lane
#define RSM_LANES 64u      // lanes per connection: one wave
#define RSM_LINE 16u       // bytes a lane writes per copy step
#define RSM_GRID_CAP 8192u // 256 CUs x 32 one-wave workgroups; further connections are grid-strided
#define RSM_ITEMS (RSM_TILE + 1u)  // the carried prefix, the frames
#define RSM_SEGS (RSM_TILE + 1u)   // the message open at the tile's start, one per start

#define SEG_CHECKED 0x1u  // text, validated in this call
#define SEG_CEND 0x2u     // complete at its end in this tile, all its bytes below out_cap
#define SEG_PL_SHIFT 4u   // bytes of the carried UTF-8 tail before its first byte

using namespace xyws_internal;
namespace rows = xyws_rows;

namespace {

XYWS_DEV uint64_t below(uint32_t p) { return p >= 64 ? ~0ull : (1ull << p) - 1ull; }
XYWS_DEV bool is_cont(uint32_t b) { return (b & 0xC0u) == 0x80u; }

// Byte i (0..18) of a lane's window: the 3 bytes before its line, then the line.
XYWS_DEV uint32_t wbyte(uint32_t prev3, bytes16 v, uint32_t i) {
  if (i < 3) return (prev3 >> (8u * i)) & 0xFFu;
  i -= 3;
  return (uint32_t)((i < 8 ? v.lo >> (8u * i) : v.hi >> (8u * (i - 8))) & 0xFFu);
}

// A lead at out position p of a message that starts at ms is judged when it is
// one of this call's bytes, or the first byte of the carried tail (cs < ms).
template <class T>
XYWS_DEV bool judged(T p, T ms, T cs) { return p >= ms || (cs < ms && p == cs); }

// One tile's bytes [o0, o1) into out (as copy_tile of xyws_reply.hip, items
// without headers), and their UTF-8 rules. tail3: the bytes at out positions
// o0 - 3 .. o0 - 1 (byte k at bits 8k). Returns the same for o1.
XYWS_DEV uint32_t copy_check_tile(const uint64_t* s_off, const uint64_t* s_soff, const uint64_t* s_sstart,
                                  const uint64_t* s_sms, const uint32_t* s_sfl, uint32_t* s_bad, uint32_t* s_tail,
                                  uint32_t lane, uint64_t src, g_u8* obase, uint64_t olo, uint64_t wlim,
                                  uint64_t o0, uint64_t o1, bool utf8on, uint32_t tail3) {
  const uint64_t P0 = olo + o0, P1 = olo + o1;
  const uint64_t wl = P1 < wlim ? P1 : wlim;
  if (wl <= P0) return P1 > P0 ? 0u : tail3;  // (past out_cap nothing is data)
  const uint64_t A00 = (P0 >> 4) << 4;
  uint32_t steptail = 0;
  for (uint64_t A0 = A00; A0 < wl; A0 += (uint64_t)RSM_LINE * RSM_LANES) {
    const uint64_t A = A0 + 16u * lane;
    const bool active = A < wl;
    const uint64_t s = A > P0 ? A : P0, e = A + 16 < P1 ? A + 16 : P1;
    bytes16 acc = {0, 0};
    if (active) {
      uint64_t q = s - olo;
      uint32_t i = item_at(s_off, RSM_ITEMS, q);  // the item that holds byte q
      uint32_t a = (uint32_t)(s - A);
      const uint32_t ae = (uint32_t)(e - A);
      while (a < ae && i < RSM_ITEMS) {
        const uint64_t start = s_off[i], next = s_off[i + 1];
        if (next > q) {
          const uint32_t nb = next - q < ae - a ? (uint32_t)(next - q) : ae - a;
          add_bytes(acc, a, q, load_bytes(src + s_soff[i] + (q - start), nb), nb);
        }
        i++;
      }
      put_line(obase, A, s, e, olo, wlim, acc);
    }
    if (!utf8on) continue;

    // the window: the line, with the 3 bytes before it
    bytes16 v = acc;
    uint32_t prev3 = 0;
    const bool first = A0 == A00 && lane == 0;
    if (first) {  // the bytes before P0: tail3 lies at line offsets sa - 3 .. sa - 1
      const uint32_t sa = (uint32_t)(P0 - A);
      const bytes16 t = {tail3 & 0xFFFFFFu, 0};
      if (sa >= 3) {
        const bytes16 p = shl_bytes(t, sa - 3);
        v.lo |= p.lo;
        v.hi |= p.hi;
      } else {
        v.lo |= shr_bytes(t, 3 - sa).lo;
        prev3 = (tail3 << (8u * sa)) & 0xFFFFFFu;
      }
    }
    const uint32_t hi3 = (uint32_t)(v.hi >> 40);
    const uint32_t up = (uint32_t)__shfl_up((int)hi3, 1);
    if (!first) prev3 = lane ? up : steptail;
    steptail = uniform32((uint32_t)__shfl((int)hi3, (int)(RSM_LANES - 1)));
    if (!active) continue;

    const uint32_t ja = (uint32_t)(s - A);
    const uint32_t jb = (uint32_t)((e < wlim ? e : wlim) - A);
    if (e == P1 && P1 <= wlim) {  // the 3 bytes before P1, for the next tile (window index = line offset + 3)
      const uint32_t je = (uint32_t)(e - A);
      *s_tail = wbyte(prev3, v, je) | (wbyte(prev3, v, je + 1) << 8) | (wbyte(prev3, v, je + 2) << 16);
    }
    // (ASCII in the line and before it: no rule can fail, whatever the segments)
    if (!((v.lo | v.hi | prev3) & 0x8080808080808080ull)) continue;
    // from here on positions are relative to the line's first byte, clamped to [-8, 64] (every byte the
    // rules look at lies in [-3, 16)): 32-bit compares
    const int64_t qbase = (int64_t)A - (int64_t)olo;
    uint32_t seg = item_at(s_sstart, RSM_SEGS, (uint64_t)(qbase + ja));  // the segment of the first byte
    int32_t segend, ms, cs;
    uint32_t fl;
    auto clamp = [](int64_t r) -> int32_t { return r < -8 ? -8 : r > 64 ? 64 : (int32_t)r; };
    auto load_seg = [&]() {
      fl = s_sfl[seg];
      const int64_t m = (int64_t)s_sms[seg] - qbase;
      segend = clamp((int64_t)s_sstart[seg + 1] - qbase);
      ms = clamp(m);
      cs = clamp(m - (int64_t)(fl >> SEG_PL_SHIFT));
    };
    load_seg();
    // the window as five words: bytes 1..3 of w0 are the 3 bytes before the line, w1..w4 the line
    const uint32_t w0 = prev3 << 8, w1 = (uint32_t)v.lo, w2 = (uint32_t)(v.lo >> 32), w3 = (uint32_t)v.hi,
                   w4 = (uint32_t)(v.hi >> 32);
#pragma unroll
    for (int32_t q = 0; q < 16; q++) {
      if ((uint32_t)q < ja || (uint32_t)q >= jb) continue;
      // the byte at q and the 3 before it: window bytes q + 1 .. q + 4
      const uint32_t k = (uint32_t)(q + 1) >> 2, sh = (uint32_t)(q + 1) & 3u;
      const uint32_t wl_ = k == 0 ? w0 : k == 1 ? w1 : k == 2 ? w2 : k == 3 ? w3 : w4;
      const uint32_t wh_ = k == 0 ? w1 : k == 1 ? w2 : k == 2 ? w3 : w4;  // (k == 4 comes with sh == 0 only)
      const uint32_t win = sh ? __builtin_amdgcn_alignbyte(wh_, wl_, sh) : wl_;
      while (q >= segend && seg + 1 < RSM_SEGS) {
        seg++;
        load_seg();
      }
      if (!(fl & SEG_CHECKED) || !(win & 0x80808080u)) continue;  // (four ASCII bytes: no rule can fail)
      const uint32_t b3 = win & 0xFFu, b2 = (win >> 8) & 0xFFu, b1 = (win >> 16) & 0xFFu, b0 = win >> 24;
      const uint32_t l1 = q - 1 >= cs ? lead_len(b1) : 0u, l2 = q - 2 >= cs ? lead_len(b2) : 0u,
                     l3 = q - 3 >= cs ? lead_len(b3) : 0u;
      bool bad = false;
      if (is_cont(b0)) bad = !(l1 > 1 || l2 > 2 || l3 > 3);  // claimed by a lead at most 3 bytes before it
      else if (b0 == 0xC0u || b0 == 0xC1u || b0 >= 0xF5u) bad = true;
      // a sequence that ends here is judged whole
      if (l1 == 2 && judged(q - 1, ms, cs)) bad = bad || !is_cont(b0);
      if (l2 == 3 && judged(q - 2, ms, cs)) bad = bad || !is_cont(b1) || !is_cont(b0) || utf8_second_bad(b2, b1);
      if (l3 == 4 && judged(q - 3, ms, cs))
        bad = bad || !is_cont(b2) || !is_cont(b1) || !is_cont(b0) || utf8_second_bad(b3, b2);
      // the message's last byte: a sequence that runs past it
      if ((fl & SEG_CEND) && q + 1 == segend)
        bad = bad || (lead_len(b0) > 1 && judged(q, ms, cs)) || (l1 > 2 && judged(q - 1, ms, cs)) ||
              (l2 > 3 && judged(q - 2, ms, cs));
      if (bad) s_bad[seg] = 1u;
    }
  }
  return 0xFFFFFFFFu;  // (the caller takes *s_tail after its barrier)
}

__global__ void __launch_bounds__(RSM_LANES) k_reasm_streams(const xyws_conn* __restrict__ conns,
                                                             const uint64_t* __restrict__ nframes,
                                                             const xyws_reasm_conn* __restrict__ reasm, uint64_t n,
                                                             uint32_t opts, xyws_reasm_result* __restrict__ results) {
  __shared__ uint64_t s_off[RSM_ITEMS + 1];   // items: start in out (and the end after the last)
  __shared__ uint64_t s_soff[RSM_ITEMS];      //        source offset
  __shared__ uint64_t s_sstart[RSM_SEGS + 1]; // segments: start in out (unused ones and the end: o1)
  __shared__ uint64_t s_sms[RSM_SEGS];        //           the message's first byte in out
  __shared__ uint32_t s_sfl[RSM_SEGS];        //           SEG_*
  __shared__ uint32_t s_bad[RSM_SEGS];
  __shared__ uint32_t s_tail;
  const uint32_t lane = threadIdx.x;
  const uint64_t lbit = 1ull << lane, lbelow = lbit - 1ull;
  for (uint64_t ci = blockIdx.x; ci < n; ci += gridDim.x) {
    const rows::conn_row cn = rows::load_conn(conns + ci);
    const uint64_t buf = cn.buf, len = cn.len, frames = cn.frames, cap = cn.cap;
    const uint64_t t = uniform64(((const g_u64*)nframes)[ci]);
    const rows::reasm_conn_row rq = rows::load_reasm_conn<true>(reasm + ci);
    const uint64_t out = rq.out, out_cap = rq.out_cap, msgs = rq.msgs, msg_cap = rq.msg_cap;
    xyws_msg_carry* const mc = (xyws_msg_carry*)rq.mc;
    xyws_reasm_result* const res = results ? results + ci : nullptr;

    rows::msg_carry_row c = {0, 0, 0, 0, 0, 0, {0, 0, 0, 0, 0}};
    if (mc) c = rows::load_msg_carry(mc);
    const uint64_t c_len = c.length, c_nfr = c.nframes, c_first = c.first_frame, c_rem = c.frame_remaining,
                   c_seen = c.frames_seen;
    const uint32_t c_status = c.state.status, c_op = c.state.opcode, c_member = c.state.frame_member;

    if ((c_status & XYWS_MSG_OVERFLOW) || t > cap || (!frames && t)) {  // the table does not cover the stream
      if (lane == 0) {
        if (mc) rows::raise_msg_status(mc, c.state_word, XYWS_MSG_OVERFLOW);
        if (res) rows::store_reasm_result(res, {0, 0, {0, XYWS_RSM_OVERFLOW}, 0});
      }
      continue;
    }

    const bool utf8on = (opts & XYWS_REASM_UTF8) && out_cap && msg_cap;
    g_u8* const obase = (g_u8*)(out & ~15ull);
    const uint64_t olo = out & 15u;
    const uint64_t wlim = sat_add(olo, out_cap);

    // the carried tail as the bytes at out positions -3 .. -1
    uint32_t c_pl = 0, tail3 = 0;
    if (c_op == XYWS_FLAG_OP_TEXT) {
      const uint32_t ul = c.state.utf8_len;
      if (ul >= 1 && ul <= 3) {
        c_pl = ul;
        tail3 = (c.state.utf8 << (8u * (3 - ul))) & 0xFFFFFFu;
      }
    }

    // the open message (the record not yet written), wave-uniform
    bool open = c_op != 0, closing = open && (c_status & XYWS_MSG_COMPLETE);
    uint64_t cur_k = 0, cur_first = XYWS_NPOS, cur_nfr = 0, cur_off = 0, cur_len = 0;
    uint32_t cur_st = open ? XYWS_MSG_CONTINUED | (c_status & (XYWS_MSG_UTF8_BAD | XYWS_MSG_UNCHECKED)) : 0u;
    uint32_t cur_op = c_op, cur_bad = 0;
    bool cur_cont = open;
    bool cur_checked = utf8on && cur_op == XYWS_FLAG_OP_TEXT && !(cur_st & (XYWS_MSG_UTF8_BAD | XYWS_MSG_UNCHECKED));
    bool pending = !open && (c_status & XYWS_MSG_ORPHANS);
    uint64_t nrec = open ? 1 : 0;

    // the rest of the frame the last batch end cut
    uint64_t pk = 0;
    const uint64_t hk = c_rem < len ? c_rem : len;
    uint64_t rem = c_rem - hk;
    uint32_t member = rem ? c_member : 0u;
    if (open && c_member) pk = hk;
    bool head_complete = false;
    if (open && closing && rem == 0) {  // the closing message's last byte
      head_complete = true;
      open = closing = false;
    }
    bool cur_live = c_op != 0;

    uint64_t opos = 0;
    uint32_t completed = 0, anybad = 0;
    for (uint64_t base = 0; base < t || base == 0; base += RSM_TILE) {
      const uint64_t j = base + lane;
      const bool valid = j < t;
      uint64_t poff = 0, plen = 0;
      uint32_t fflags = 0;
      if (valid) {
        const rows::frame_row f = rows::load_frame(rows::row_at<const xyws_frame>(frames, j));
        poff = f.payload_off;
        plen = f.payload_len;
        fflags = f.flags;
      }
      const uint32_t op = fflags & XYWS_FLAG_OP_MASK;
      uint64_t avail = 0;
      if (valid && poff < len) avail = plen < len - poff ? plen : len - poff;
      const uint64_t D = __ballot(valid && (op == XYWS_FLAG_OP_TEXT || op == XYWS_FLAG_OP_BINARY));
      const uint64_t C = __ballot(valid && op == XYWS_FLAG_OP_CONTINUE);
      const uint64_t F = __ballot(valid && (fflags & XYWS_FLAG_FIN));
      const uint64_t X = __ballot(valid && plen > avail);

      // 1. membership: a walk over the frames that can change the state
      uint64_t joined = 0, orphans = 0, imask = 0, kmask = 0;
      {
        uint64_t rest = D | (C & F);
        uint32_t cursor = 0;
        for (;;) {
          const uint32_t nx = rest ? (uint32_t)__builtin_ctzll(rest) : 64u;
          const uint64_t range = below(nx) & ~below(cursor);
          if (open && !closing) joined |= C & range;
          else orphans |= C & range;
          if (nx == 64) break;
          const uint64_t bit = 1ull << nx;
          if (D & bit) {
            if (open) imask |= bit;
            joined |= bit;
            open = true;
            closing = false;
            if (F & bit) {
              if (X & bit) closing = true;
              else { open = false; kmask |= bit; }
            }
          } else if (open && !closing) {  // the FIN continuation
            joined |= bit;
            if (X & bit) closing = true;
            else { open = false; kmask |= bit; }
          } else {
            orphans |= bit;
          }
          cursor = nx + 1;
          rest &= rest - 1;
        }
      }
      const uint32_t nvalid = t - base < RSM_TILE ? (uint32_t)(t - base) : RSM_TILE;
      if (nvalid) {
        rem = uniform64(shfl64(plen - avail, nvalid - 1));
        member = rem && ((joined >> (nvalid - 1)) & 1u) ? 1u : 0u;
      }

      // 2. out offsets: an inclusive scan of the joined sizes
      const bool isj = (joined & lbit) != 0;
      const uint64_t size = isj ? avail : 0;
      const uint64_t incl = wave_scan64(size, lane);
      const uint64_t o0 = opos, fstart = opos + pk;
      const uint64_t o1 = fstart + uniform64(shfl64(incl, RSM_LANES - 1));
      const uint64_t myoff = fstart + (incl - size);
      s_off[1 + lane] = myoff;
      s_soff[1 + lane] = poff;

      // the segments: the message open at the tile's start, then one per start
      const bool isD = (D & lbit) != 0;
      const uint32_t nD = (uint32_t)__popcll(D), rank = (uint32_t)__popcll(D & lbelow);
      const uint32_t firstD = D ? (uint32_t)__builtin_ctzll(D) : 64u;
      const uint64_t Dabove = D & ~lbelow & ~lbit;
      const uint32_t p2 = Dabove ? (uint32_t)__builtin_ctzll(Dabove) : 64u;
      const uint64_t range = below(p2) & ~lbelow;  // this start's frames
      const uint64_t nextoff = shfl64(myoff, p2 & 63u);
      const uint64_t mend = p2 < 64 ? nextoff : o1;
      const bool complete = isD && (kmask & range) != 0;
      const bool interrupted = isD && p2 < 64 && ((imask >> p2) & 1u);
      const bool text = op == XYWS_FLAG_OP_TEXT;
      // orphans since the start before this one (or pending at the tile's start)
      const uint64_t Dbelow = D & lbelow;
      const uint32_t pD = Dbelow ? 63u - (uint32_t)__builtin_clzll(Dbelow) : 0u;
      const bool pend = isD && (Dbelow ? (orphans & lbelow & ~below(pD + 1)) != 0 : pending || (orphans & lbelow) != 0);
      if (isD) {
        s_sstart[1 + rank] = myoff;
        s_sms[1 + rank] = myoff;
        s_sfl[1 + rank] = (utf8on && text ? SEG_CHECKED : 0u) | (complete && mend <= out_cap ? SEG_CEND : 0u);
      }
      if (lane >= nD) s_sstart[1 + lane] = o1;
      s_bad[lane] = 0;
      const uint64_t range0 = below(firstD);
      const bool complete0 = cur_live && (head_complete || (kmask & range0) != 0);
      const bool ended0 = cur_live && (complete0 || firstD < 64);
      const uint64_t mend0 = firstD < 64 ? uniform64(shfl64(myoff, firstD & 63u)) : o1;
      if (lane == 0) {
        s_off[0] = o0;  // the carried prefix: buf[0, pk)
        s_soff[0] = 0;
        s_off[RSM_ITEMS] = o1;
        s_sstart[0] = o0;
        s_sstart[RSM_SEGS] = o1;
        s_sms[0] = cur_off;
        s_sfl[0] = (cur_live && cur_checked ? SEG_CHECKED : 0u) | (complete0 && mend0 <= out_cap ? SEG_CEND : 0u) |
                   (cur_live && cur_cont ? c_pl << SEG_PL_SHIFT : 0u);
        s_bad[RSM_TILE] = 0;
      }
      __syncthreads();

      // 3, 4. the bytes and their UTF-8 rules
      // a complete message with no byte in this tile: its last bytes are tail3
      if (cur_live && cur_checked && complete0 && mend0 == o0 && mend0 <= out_cap) {
        const int64_t ms = (int64_t)cur_off, cs = ms - (int64_t)(cur_cont ? c_pl : 0u), e = (int64_t)o0;
        const uint32_t t0 = tail3 & 0xFFu, t1 = (tail3 >> 8) & 0xFFu, t2 = (tail3 >> 16) & 0xFFu;
        if ((e - 1 >= cs && lead_len(t2) > 1 && judged(e - 1, ms, cs)) ||
            (e - 2 >= cs && lead_len(t1) > 2 && judged(e - 2, ms, cs)) ||
            (e - 3 >= cs && lead_len(t0) > 3 && judged(e - 3, ms, cs)))
          cur_bad = 1;
      }
      const uint32_t nt = copy_check_tile(s_off, s_soff, s_sstart, s_sms, s_sfl, s_bad, &s_tail, lane, buf, obase, olo,
                                          wlim, o0, o1, utf8on, tail3);
      __syncthreads();
      tail3 = nt != 0xFFFFFFFFu ? nt : (olo + o1 <= wlim ? uniform32(s_tail) : 0u);

      // 5. the records of the messages that end in this tile
      if (cur_live) {
        cur_nfr += (uint64_t)__popcll(joined & range0);
        cur_len += mend0 - o0;
        cur_bad |= uniform32(s_bad[0]);
        if (ended0) {
          const uint32_t st = cur_st | (complete0 ? XYWS_MSG_COMPLETE : XYWS_MSG_INTERRUPTED) |
                              (cur_off + cur_len > out_cap ? XYWS_MSG_TRUNCATED : 0u) |
                              (cur_checked && cur_bad ? XYWS_MSG_UTF8_BAD : 0u);
          if (cur_k < msg_cap) {
            if (lane == 0)
              rows::store_message(rows::row_at<xyws_message>(msgs, cur_k),
                                  {cur_first, cur_nfr, cur_off, cur_len, rows::pack_message_meta({st, cur_op})});
            if (complete0) completed++;
            if (st & XYWS_MSG_UTF8_BAD) anybad = 1;
          }
          cur_live = false;
        }
      }
      head_complete = false;
      {
        const uint64_t k = nrec + rank;
        const bool ended = isD && (complete || p2 < 64);
        const uint32_t sbad = isD ? s_bad[1 + rank] : 0u;
        const uint32_t st = (pend ? XYWS_MSG_ORPHANS : 0u) | (complete ? XYWS_MSG_COMPLETE : 0u) |
                            (interrupted ? XYWS_MSG_INTERRUPTED : 0u) | (mend > out_cap ? XYWS_MSG_TRUNCATED : 0u) |
                            (utf8on && text && sbad ? XYWS_MSG_UTF8_BAD : 0u);
        const uint64_t nfr = (uint64_t)__popcll(joined & range);
        const bool stored = ended && k < msg_cap;
        if (stored)
          rows::store_message(rows::row_at<xyws_message>(msgs, k),
                              {j, nfr, myoff, mend - myoff, rows::pack_message_meta({st, op})});
        completed += (uint32_t)__popcll(__ballot(stored && complete));
        if (__ballot(stored && (st & XYWS_MSG_UTF8_BAD))) anybad = 1;
        // the last start's message, when it goes on after this tile
        if (nD) {
          const uint32_t lD = 63u - (uint32_t)__builtin_clzll(D);
          const bool lend = uniform32((uint32_t)__shfl((int)ended, (int)lD)) != 0;
          if (!lend) {
            cur_live = true;
            cur_k = nrec + nD - 1;
            cur_first = base + lD;
            cur_nfr = uniform64(shfl64(nfr, lD));
            cur_off = uniform64(shfl64(myoff, lD));
            cur_len = o1 - cur_off;
            cur_st = uniform32((uint32_t)__shfl((int)pend, (int)lD)) ? XYWS_MSG_ORPHANS : 0u;
            cur_op = uniform32((uint32_t)__shfl((int)op, (int)lD));
            cur_cont = false;
            cur_bad = uniform32((uint32_t)__shfl((int)sbad, (int)lD));
            cur_checked = utf8on && cur_op == XYWS_FLAG_OP_TEXT;
          }
        }
      }
      if (D) pending = (orphans & ~below(64u - (uint32_t)__builtin_clzll(D))) != 0;
      else pending = pending || orphans != 0;
      nrec += nD;
      opos = o1;
      pk = 0;
      __syncthreads();  // (LDS is rewritten by the next tile)
    }

    // the record of the message still open, the carry, the result
    uint32_t o_status = pending ? XYWS_MSG_ORPHANS : 0u, o_op = 0, o_member = 0, o_ul = 0, o_u = 0;
    uint64_t o_len = 0, o_nfr = 0, o_first = 0;
    if (cur_live) {
      const bool trunc = cur_off + cur_len > out_cap, stored = cur_k < msg_cap;
      const uint32_t st = cur_st | (trunc ? XYWS_MSG_TRUNCATED : 0u) | (cur_checked && cur_bad ? XYWS_MSG_UTF8_BAD : 0u);
      if (stored) {
        if (lane == 0)
          rows::store_message(rows::row_at<xyws_message>(msgs, cur_k),
                              {cur_first, cur_nfr, cur_off, cur_len, rows::pack_message_meta({st, cur_op})});
        if (st & XYWS_MSG_UTF8_BAD) anybad = 1;
      }
      const bool text = cur_op == XYWS_FLAG_OP_TEXT;
      const bool bad = stored ? (st & XYWS_MSG_UTF8_BAD) != 0 : cur_cont && (c_status & XYWS_MSG_UTF8_BAD);
      const bool unchecked = text && ((cur_cont && (c_status & XYWS_MSG_UNCHECKED)) || !utf8on || trunc || !stored);
      o_op = cur_op;
      o_member = member;
      o_len = (cur_cont ? c_len : 0) + cur_len;
      o_nfr = (cur_cont ? c_nfr : 0) + cur_nfr;
      o_first = cur_cont ? c_first : c_seen + cur_first;
      o_status = (closing ? XYWS_MSG_COMPLETE : 0u) | (bad ? XYWS_MSG_UTF8_BAD : 0u) |
                 (unchecked ? XYWS_MSG_UNCHECKED : 0u);
      if (text && !bad && !unchecked) {
        // from the earliest lead in the message's last 3 bytes whose sequence runs past the end
        const int64_t cs = (int64_t)cur_off - (int64_t)(cur_cont ? c_pl : 0u), e = (int64_t)opos;
        for (uint32_t d = 3; d >= 1; d--) {
          if (e - (int64_t)d < cs) continue;
          if (lead_len((tail3 >> (8u * (3 - d))) & 0xFFu) > d) {
            o_ul = d;
            o_u = (tail3 >> (8u * (3 - d))) & 0xFFFFFFu;
            break;
          }
        }
      }
    }
    if (lane == 0) {
      if (mc) rows::store_msg_carry(mc, o_len, o_nfr, o_first, rem, c_seen + t, {o_status, o_op, o_member, o_ul, o_u});
      if (res) {
        const uint32_t st = (opos > out_cap ? XYWS_RSM_TRUNCATED : 0u) | (nrec > msg_cap ? XYWS_RSM_MSG_CAP : 0u) |
                            (o_op ? XYWS_RSM_OPEN : 0u) | (anybad ? XYWS_RSM_UTF8_BAD : 0u);
        rows::store_reasm_result(res, {opos, nrec, {completed, st}, 0});
      }
    }
  }
}

}  // namespace

extern "C" {

int xyws_reassemble_streams(xyws_ctx* ctx, const xyws_conn* dev_conns, const uint64_t* dev_nframes,
                            const xyws_reasm_conn* dev_reasm, uint64_t n, uint32_t opts,
                            xyws_reasm_result* dev_results, void* stream) {
  if (!ctx || (n && (!dev_conns || !dev_nframes || !dev_reasm))) return XYWS_ERR_INVALID;
  if (opts & ~XYWS_REASM_UTF8) return XYWS_ERR_INVALID;
  if (!n) return XYWS_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  device_guard g(ctx->device);
  if (!g.ok) return XYWS_ERR_HIP;
  const uint32_t grid = grid_for(n, 1, RSM_GRID_CAP);
  hipLaunchKernelGGL(k_reasm_streams, dim3(grid), dim3(RSM_LANES), 0, (hipStream_t)stream, dev_conns, dev_nframes,
                     dev_reasm, n, opts, dev_results);
  return hip_err(hipGetLastError());
}

// Internal (tests and measurements, no HIP call): the geometry of
// k_reasm_streams. out: {frames per tile, bytes per copy step, grid cap,
// wave size}.
int xyws_debug_reasm_streams_geometry(uint64_t out[4]) {
  if (!out) return XYWS_ERR_INVALID;
  out[0] = RSM_TILE;
  out[1] = RSM_LINE * RSM_LANES;
  out[2] = RSM_GRID_CAP;
  out[3] = RSM_LANES;
  return XYWS_OK;
}

}  // extern "C"

// xyws_roster.hip — xyws_roster_streams: every room's member list kept on the
// device, updated from the sweep's own result rows, and the room's welcome and
// farewell notices framed and delivered (the reference's chat_room::join,
// leave, welcome and farewell, example/websocket/websocket_chat.cpp:34-39,
// 49-87). The semantics are stated in include/xyws.h; this is how they are
// computed. Every table row is read and written through xyws_rows.h, which
// names its words.
//
// Three launches, dev_want and the result rows the hand-over between them. No
// workgroup waits for another inside a launch, nothing spins, there are no
// atomics.
//
// k_roster_events: one thread per connection. It decides the connection's
// event from its rows (event_of), writes dev_want[i] (WANT_NONE, WANT_LEAVE or
// the room to join), the whole result row as it stands without the room pass,
// and, where dev_jconns is given, the backlog's word {XYWS_ROOM_NONE, 0}.
//
// k_roster_rooms: one workgroup per room, rooms grid-strided, shaped like the
// broadcast's wire build.
//   A. The members in tiles of RS_TILE, one per thread: the thread loads its
//      entry, copies it into the room's `seen` list where one is named (the
//      list as the broadcast read it, which this sweep's backlog fold walks),
//      bounds-checks it and reads dev_want for the leave mark. One
//      workgroup scan places the kept members (and counts the leavers in the
//      word's upper half), a second one sizes the farewells; the running sums
//      are carried between tiles in registers. The compaction is in place:
//      the scans' barriers end the tile's loads before its stores, and a
//      store's index never exceeds its load's. The leaver's rows are marked
//      and the tile's farewells composed (compose_tile). A tile that nobody
//      leaves, behind tiles nobody left, costs one barrier and no scan.
//   B. dev_want[0 .. n) in steps of RS_SCAN, one word per thread, for the
//      room's joiners in ascending index. First every thread looks at its
//      words of all steps (independent loads) and one barrier says whether
//      anybody joins the room at all: the sweep without an event ends here.
//      Otherwise a step without a joiner costs one barrier more. A pair of
//      scans gives the list position (the admitted are a
//      prefix) and the welcome offset; the joiner's rows are rewritten and
//      the step's welcomes composed.
// compose_tile writes the notices as 16-byte lines (xyws_lines.h): a thread
// takes a line, finds the item that holds its first byte (item_at) and adds
// header, head, name and tail bytes at their line offsets. The text lies in
// LDS as words.
//
// k_roster_deliver: the fan-out's geometry and copy (xyws_room.h, copy_span).
// The source is notes + note_off; base is computed again from the rows (the
// y == 0 workgroup writes send_len while the others copy).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <mutex>

#include "xyws.h"
#include "xyws_device.h"
#include "xyws_ctx.h"
#include "xyws_frameops.h"
#include "xyws_lines.h"
#include "xyws_room.h"
#include "xyws_rows.h"

#define RS_THREADS BC_WIRE_THREADS  // the room pass: the one workgroup a room gets (block_scan's size)
#define RS_TILE RS_THREADS          // members per tile: one per thread
#define RS_SCAN RS_THREADS          // words of dev_want per step of the joiner scan: one per thread
#define RS_EV_THREADS 256u          // the events: connections per workgroup

#define WANT_NONE XYWS_ROOM_NONE          // dev_want[i]: no event
#define WANT_LEAVE (XYWS_ROOM_NONE - 1u)  // ... it leaves; any other value: the room it joins (< n_rooms <= WANT_LEAVE)
#define NOTE_NONE 0xFFFFFFFFu             // an item of a tile without a notice

using namespace xyws_internal;
namespace rows = xyws_rows;

namespace {

// base of 4.: what the earlier calls of the sweep left in the send buffer.
template <bool U>
XYWS_DEV uint64_t base_of(const rows::roster_conn_row& rc, uint32_t& bst, uint32_t& pst, uint32_t& ast) {
  uint64_t base = 0;
  bst = pst = ast = 0;
  if (rc.accept) {
    const rows::accept_brief a = rows::load_accept_brief<U>((const xyws_accept_result*)rc.accept);
    ast = a.status;
    base = (ast & (XYWS_ACC_ACCEPTED | XYWS_ACC_REJECTED)) ? a.resp_len : 0;
  }
  if (rc.reply) {
    const rows::reply_result_row rp = rows::load_reply_result<U>((const xyws_reply_result*)rc.reply);
    pst = rp.status;
    base = rp.reply_len;
  }
  if (rc.bcast) {
    const rows::bcast_result_row bp = U ? rows::load_bcast_result((const xyws_bcast_result*)rc.bcast)
                                        : rows::load_bcast_result_own((const xyws_bcast_result*)rc.bcast);
    bst = bp.status;
    base = bp.send_len;
  }
  return base;
}

// The name's length as the notices count it (1.).
XYWS_DEV uint32_t name_len_of(uint64_t name, uint64_t name_len) {
  return name && name_len <= XYWS_ROSTER_NAME_MAX ? (uint32_t)name_len : 0u;
}

__global__ void __launch_bounds__(RS_EV_THREADS)
    k_roster_events(const xyws_bcast_conn* __restrict__ bconns, const xyws_roster_conn* __restrict__ rconns, uint64_t n,
                    uint64_t n_rooms, xyws_backlog_conn* __restrict__ jconns, uint32_t* __restrict__ want,
                    xyws_roster_result* __restrict__ results) {
  for (uint64_t i = (uint64_t)blockIdx.x * RS_EV_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * RS_EV_THREADS) {
    const rows::roster_conn_row rc = rows::load_roster_conn<false>(rconns + i);
    uint32_t bst, pst, ast;
    const uint64_t base = base_of<false>(rc, bst, pst, ast);
    const uint32_t fl = rc.ask.flags, cur = rows::load_bcast_room(bconns + i);
    const bool is_member = cur < n_rooms;
    const bool leave = (fl & XYWS_RS_LEAVE) || ((fl & XYWS_RS_LEAVE_ON_CLOSE) && rc.reply && (pst & XYWS_RPL_CLOSED));
    const bool on_accept = (fl & XYWS_RS_JOIN_ON_ACCEPT) && rc.accept;
    const bool joins = !leave && rc.ask.room < n_rooms && ((fl & XYWS_RS_JOIN) || (on_accept && (ast & XYWS_ACC_ACCEPTED)));
    bool receiver = !leave && !(pst & (XYWS_RPL_CLOSED | XYWS_RPL_OVERFLOW)) && !(bst & XYWS_BC_NOT_RECEIVER);
    if (on_accept && !(ast & XYWS_ACC_ACCEPTED)) receiver = false;
    uint32_t st = rc.name_len > XYWS_ROSTER_NAME_MAX ? XYWS_RSC_BAD_NAME : 0u;
    uint32_t w = WANT_NONE, room = XYWS_ROOM_NONE;
    if (leave) {
      w = WANT_LEAVE;
    } else {
      if (is_member) {
        st |= XYWS_RSC_MEMBER;
        room = cur;
      }
      if (joins) {
        if (is_member) st |= XYWS_RSC_ALREADY;
        else w = rc.ask.room;
      }
    }
    if (!receiver) st |= XYWS_RSC_NOT_RECEIVER;
    else if (!(st & XYWS_RSC_MEMBER)) st |= XYWS_RSC_NO_ROOM;
    ((XYWS_GLOBAL uint32_t*)want)[i] = w;
    rows::store_roster_result(results + i, base, 0, {st, room}, 0);
    if (jconns) rows::store_backlog_join(jconns + i, {XYWS_ROOM_NONE, 0});
  }
}

// The string of `len` bytes at word w0 of the text in LDS: its bytes from off on, in the low bytes.
XYWS_DEV bytes16 text_bytes(const uint64_t* s_txt, uint32_t w0, uint32_t off) {
  const uint32_t k = w0 + (off >> 3), sh = 8u * (off & 7u);
  const uint64_t a = s_txt[k], b = s_txt[k + 1], c = s_txt[k + 2];  // (two zero words follow the text)
  return sh ? bytes16{(a >> sh) | (b << (64 - sh)), (b >> sh) | (c << (64 - sh))} : bytes16{a, b};
}

// The notices of one tile to wire positions [o0, o1): item i (s_nlen[i] !=
// NOTE_NONE) is header | head | its name | tail at s_off[i]; s_off ascending,
// s_off[RS_TILE] == o1. The wire is addressed from wbase: byte k at wlo + k,
// nothing at or above wlim is written.
XYWS_DEV void compose_tile(g_u8* wbase, uint64_t wlo, uint64_t wlim, uint64_t o0, uint64_t o1, const uint64_t* s_off,
                           const uint64_t* s_name, const uint32_t* s_nlen, const uint64_t* s_txt, uint32_t head_len,
                           uint32_t tail_w0, uint32_t tail_len, uint32_t flags, uint32_t tid) {
  const uint64_t P0 = wlo + o0, P1 = wlo + o1;
  const uint64_t wl = P1 < wlim ? P1 : wlim;
  if (wl <= P0) return;
  for (uint64_t A = ((P0 >> 4) + tid) << 4; A < wl; A += (uint64_t)BC_LINE * RS_THREADS) {
    const uint64_t s = A > P0 ? A : P0, e = A + 16 < P1 ? A + 16 : P1;
    uint64_t q = s - wlo;
    uint32_t i = item_at(s_off, RS_TILE, q);  // the item that holds byte q (q < o1)
    bytes16 acc = {0, 0};
    uint32_t a = (uint32_t)(s - A);
    const uint32_t ae = (uint32_t)(e - A);
    for (; a < ae && i < RS_TILE; i++) {
      const uint32_t nl = s_nlen[i];
      if (nl == NOTE_NONE) continue;
      const uint32_t L = head_len + nl + tail_len;
      uint32_t hw[4];
      const uint32_t h = build_header(flags, L, false, 0, hw);
      uint32_t rr = (uint32_t)(q - s_off[i]);  // (the first item holds q, a later one begins at it)
      if (rr < h) {  // header bytes rr.. at line offset a
        const uint32_t nb = h - rr < ae - a ? h - rr : ae - a;
        add_bytes(acc, a, q, shr_bytes(bytes16{(uint64_t)hw[0] | ((uint64_t)hw[1] << 32), 0}, rr), nb);
        rr += nb;
      }
      if (a < ae && rr < h + head_len) {  // head bytes
        const uint32_t left = h + head_len - rr, nb = left < ae - a ? left : ae - a;
        add_bytes(acc, a, q, text_bytes(s_txt, 0, rr - h), nb);
        rr += nb;
      }
      if (a < ae && rr < h + head_len + nl) {  // name bytes
        const uint32_t left = h + head_len + nl - rr, nb = left < ae - a ? left : ae - a;
        add_bytes(acc, a, q, load_bytes(s_name[i] + (rr - h - head_len), nb), nb);
        rr += nb;
      }
      if (a < ae && rr < h + L) {  // tail bytes
        const uint32_t left = h + L - rr, nb = left < ae - a ? left : ae - a;
        add_bytes(acc, a, q, text_bytes(s_txt, tail_w0, rr - h - head_len - nl), nb);
      }
    }
    put_line(wbase, A, s, e, wlo, wlim, acc);
  }
}

// A notice's size on the wire.
XYWS_DEV uint64_t note_size(uint32_t L) { return (L < 126u ? 2u : 4u) + L; }

__global__ void __launch_bounds__(RS_THREADS)
    k_roster_rooms(xyws_bcast_conn* __restrict__ bconns, const xyws_roster_conn* __restrict__ rconns, uint64_t n,
                   xyws_room* __restrict__ rooms, const xyws_roster_room* __restrict__ rrooms,
                   xyws_roster_room_result* __restrict__ room_results, uint64_t n_rooms, rows::roster_words tx,
                   uint32_t flags, xyws_backlog_conn* __restrict__ jconns, const uint32_t* __restrict__ want,
                   xyws_roster_result* __restrict__ results) {
  __shared__ uint64_t s_off[RS_TILE + 1];  // items: start in the notice wire (and the end after the last)
  __shared__ uint64_t s_name[RS_TILE];
  __shared__ uint32_t s_nlen[RS_TILE];
  __shared__ uint64_t s_w[RS_THREADS / BC_WAVE];
  __shared__ uint64_t s_txt[3 * rows::ROSTER_TEXT_WORDS + 2];
  const uint32_t tid = threadIdx.x;
  if (tid < 3 * rows::ROSTER_TEXT_WORDS + 2) s_txt[tid] = tid < 3 * rows::ROSTER_TEXT_WORDS ? tx.w[tid] : 0;
  __syncthreads();
  const uint32_t head_len = tx.head_len, joined_len = tx.joined_len, left_len = tx.left_len;
  const XYWS_GLOBAL uint32_t* const gwant = (const XYWS_GLOBAL uint32_t*)want;
  for (uint64_t ri = blockIdx.x; ri < n_rooms; ri += gridDim.x) {
    const rows::room_row rq = rows::load_room(rooms + ri);
    const uint64_t nm = rq.n_members;
    XYWS_GLOBAL uint32_t* const members = (XYWS_GLOBAL uint32_t*)rq.members;
    const rows::roster_room_row lq = rows::load_roster_room(rrooms + ri, rq.members != 0);
    const uint64_t cap = lq.member_cap;
    g_u8* const wbase = (g_u8*)(lq.notes & ~15ull);
    const uint64_t wlo = lq.notes & 15u;
    const uint64_t wlim = sat_add(wlo, lq.notes_cap);
    // the list as it stands, for this sweep's backlog fold (5.): the entries that fit member_cap
    xyws_room* const seen = (xyws_room*)lq.seen;
    XYWS_GLOBAL uint32_t* const seen_members = seen ? (XYWS_GLOBAL uint32_t*)rows::load_room_members(seen) : nullptr;
    const uint64_t seen_n = nm < cap ? nm : cap;

    // A. the members: leavers and bad entries out, the farewells
    uint64_t kept = 0, left = 0, wpos = 0;  // (uniform)
    int bad = 0;
    for (uint64_t base = 0; base < nm; base += RS_TILE) {
      uint32_t m = 0, nl = NOTE_NONE;
      uint64_t name = 0, size = 0;
      bool keep = false, leave = false;
      if (base + tid < nm) {
        m = members[base + tid];
        if (seen_members && base + tid < seen_n) seen_members[base + tid] = m;
        if (m >= n) {  // (never dereferenced)
          bad = 1;
        } else if (gwant[m] == WANT_LEAVE) {
          leave = true;
          const rows::roster_name nq = rows::load_roster_name(rconns + m);
          name = nq.name;
          nl = name_len_of(nq.name, nq.name_len);
          size = note_size(head_len + nl + left_len);
        } else {
          keep = true;
        }
      }
      // a tile in which everyone stays, behind tiles in which everyone stayed: nothing moves, nothing is said
      if (!__syncthreads_or((base + tid < nm && !keep) ? 1 : 0) && kept == base) {
        kept += nm - base < RS_TILE ? nm - base : RS_TILE;
        continue;
      }
      uint64_t tc, ts;
      const uint64_t cincl = block_scan((keep ? 1ull : 0ull) | (leave ? 1ull << 32 : 0ull), tid, s_w, tc);
      const uint64_t sincl = block_scan(size, tid, s_w, ts);
      // (the tile's entries are loaded: the scans' barriers)
      if (keep) members[kept + (uint32_t)cincl - 1u] = m;
      if (leave) {
        const rows::roster_result_row row = rows::load_roster_result<false>(results + m);
        rows::store_roster_place(results + m, {row.place.status | XYWS_RSC_LEFT, (uint32_t)ri});
        rows::store_bcast_room(bconns + m, XYWS_ROOM_NONE);
      }
      s_off[tid] = wpos + (sincl - size);
      s_name[tid] = name;
      s_nlen[tid] = nl;
      if (tid == 0) s_off[RS_TILE] = wpos + ts;
      __syncthreads();
      compose_tile(wbase, wlo, wlim, wpos, wpos + ts, s_off, s_name, s_nlen, s_txt, head_len,
                   2 * rows::ROSTER_TEXT_WORDS, left_len, flags, tid);
      kept += (uint32_t)tc;
      left += tc >> 32;
      wpos += ts;
      __syncthreads();  // (LDS is rewritten by the next tile)
    }
    const uint64_t welcome_off = wpos;

    // B. the joiners, in ascending index: the list's tail, the welcomes
    uint64_t joined = 0;  // (uniform)
    bool full = false;
    int mine = 0;  // does anybody join this room at all: independent loads, one barrier
    for (uint64_t j = tid; j < n; j += RS_SCAN) mine |= gwant[j] == ri ? 1 : 0;
    const uint64_t scan_n = __syncthreads_or(mine) ? n : 0;
    for (uint64_t base = 0; base < scan_n; base += RS_SCAN) {
      const uint64_t j = base + tid;
      const bool isj = j < n && gwant[j] == ri;
      if (!__syncthreads_or(isj ? 1 : 0)) continue;
      uint64_t tc, ts;
      const uint64_t cincl = block_scan(isj ? 1ull : 0ull, tid, s_w, tc);
      const uint64_t idx = kept + joined + cincl - 1;  // its place in the list
      const bool adm = isj && idx < cap;
      uint32_t nl = NOTE_NONE;
      uint64_t name = 0, size = 0;
      if (adm) {
        const rows::roster_name nq = rows::load_roster_name(rconns + j);
        name = nq.name;
        nl = name_len_of(nq.name, nq.name_len);
        size = note_size(head_len + nl + joined_len);
      }
      const uint64_t sincl = block_scan(size, tid, s_w, ts);
      const uint64_t off = wpos + (sincl - size);
      if (isj) {
        const rows::roster_result_row row = rows::load_roster_result<false>(results + j);
        if (adm) {
          members[idx] = (uint32_t)j;
          rows::store_roster_place(results + j, {(row.place.status & ~XYWS_RSC_NO_ROOM) | XYWS_RSC_JOINED, (uint32_t)ri});
          rows::store_roster_note_off(results + j, off);
          rows::store_bcast_room(bconns + j, (uint32_t)ri);
          if (jconns) rows::store_backlog_join(jconns + j, {(uint32_t)ri, XYWS_BL_JOIN});
        } else {
          rows::store_roster_place(results + j, {row.place.status | XYWS_RSC_FULL, row.place.room});
        }
      }
      s_off[tid] = off;
      s_name[tid] = name;
      s_nlen[tid] = nl;
      if (tid == 0) s_off[RS_TILE] = wpos + ts;
      __syncthreads();
      compose_tile(wbase, wlo, wlim, wpos, wpos + ts, s_off, s_name, s_nlen, s_txt, head_len, rows::ROSTER_TEXT_WORDS,
                   joined_len, flags, tid);
      const uint64_t room_left = cap > kept + joined ? cap - (kept + joined) : 0;
      if (tc > room_left) full = true;
      joined += tc < room_left ? tc : room_left;
      wpos += ts;
      __syncthreads();  // (LDS is rewritten by the next step)
    }

    const int any_bad = __syncthreads_or(bad);
    if (tid == 0) {
      const uint32_t st = (wpos > lq.notes_cap ? XYWS_RS_TRUNCATED : 0u) | (full ? XYWS_RS_FULL : 0u) |
                          (any_bad ? XYWS_RS_BAD_MEMBER : 0u);
      rows::store_roster_room_result(room_results + ri, wpos, welcome_off, {(uint32_t)joined, (uint32_t)left},
                                     {(uint32_t)(kept + joined), st});
      rows::store_room_count(rooms + ri, kept + joined);
      if (seen) rows::store_room_count(seen, seen_members ? seen_n : 0);
    }
    __syncthreads();  // (s_w is reused by the next room)
  }
}

__global__ void __launch_bounds__(BC_THREADS)
    k_roster_deliver(const xyws_roster_conn* __restrict__ rconns, uint64_t n, const xyws_roster_room* __restrict__ rrooms,
                     const xyws_roster_room_result* __restrict__ room_results, uint64_t n_rooms,
                     xyws_roster_result* __restrict__ results) {
  const uint32_t tid = threadIdx.x;
  for (uint64_t ci = blockIdx.x; ci < n; ci += gridDim.x) {
    const rows::roster_conn_row rc = rows::load_roster_conn<true>(rconns + ci);
    const uint64_t out = rc.out, out_cap = rc.out_cap;
    uint32_t bst, pst, ast;
    const uint64_t base = base_of<true>(rc, bst, pst, ast);
    const rows::roster_result_row row = rows::load_roster_result<true>(results + ci);
    uint32_t st = row.place.status;
    const uint64_t room = row.place.room;
    uint64_t w = 0, src = 0;
    if ((st & (XYWS_RSC_MEMBER | XYWS_RSC_JOINED)) && !(st & XYWS_RSC_NOT_RECEIVER) && room < n_rooms) {
      const rows::roster_room_row lq = rows::load_roster_room(rrooms + room, false);
      const uint64_t notes_len = rows::load_roster_notes_len(room_results + room);
      const uint64_t wv = notes_len < lq.notes_cap ? notes_len : lq.notes_cap;
      if (wv > row.note_off) w = wv - row.note_off;
      src = lq.notes + row.note_off;
    }
    const uint64_t send_len = sat_add(base, w);
    if (send_len > out_cap) st |= XYWS_RSC_TRUNCATED;
    if (blockIdx.y == 0 && tid == 0) rows::store_roster_lengths(results + ci, send_len, w, {st, (uint32_t)room});
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

const xyws_roster_text* reference_text() {
  static const xyws_roster_text t = [] {
    xyws_roster_text r;
    memset(&r, 0, sizeof r);
    static const char head[] = "|        SERVER       |:", joined[] = " has joined the chat\n", left[] = " has left the chat\n";
    static_assert(sizeof head - 1 <= XYWS_ROSTER_TEXT_MAX && sizeof joined - 1 <= XYWS_ROSTER_TEXT_MAX &&
                      sizeof left - 1 <= XYWS_ROSTER_TEXT_MAX, "the reference's strings fit");
    memcpy(r.head, head, sizeof head - 1);
    memcpy(r.joined, joined, sizeof joined - 1);
    memcpy(r.left, left, sizeof left - 1);
    r.head_len = sizeof head - 1;
    r.joined_len = sizeof joined - 1;
    r.left_len = sizeof left - 1;
    return r;
  }();
  return &t;
}

}  // namespace

extern "C" {

int xyws_roster_streams(xyws_ctx* ctx, xyws_bcast_conn* dev_bconns, const xyws_roster_conn* dev_rconns, uint64_t n,
                        xyws_room* dev_rooms, const xyws_roster_room* dev_rrooms,
                        xyws_roster_room_result* dev_room_results, uint64_t n_rooms, const xyws_roster_text* text,
                        uint8_t flags, xyws_backlog_conn* dev_jconns, uint32_t* dev_want, xyws_roster_result* dev_results,
                        void* stream) {
  if (!ctx) return XYWS_ERR_INVALID;
  if (n && (!dev_bconns || !dev_rconns || !dev_want || !dev_results)) return XYWS_ERR_INVALID;
  if (n_rooms && (!dev_rooms || !dev_rrooms || !dev_room_results)) return XYWS_ERR_INVALID;
  if (n >= UINT32_MAX || n_rooms >= UINT32_MAX) return XYWS_ERR_INVALID;  // (indices are 32 bits, UINT32_MAX is none)
  if (flags & XYWS_FLAG_HAS_MASK) return XYWS_ERR_INVALID;                 // server role only
  if (text && (text->head_len > XYWS_ROSTER_TEXT_MAX || text->joined_len > XYWS_ROSTER_TEXT_MAX ||
               text->left_len > XYWS_ROSTER_TEXT_MAX))
    return XYWS_ERR_INVALID;
  if (!n && !n_rooms) return XYWS_OK;
  const rows::roster_words tx = rows::pack_roster_text(text ? *text : *reference_text());
  std::lock_guard<std::mutex> lk(ctx->mu);
  device_guard g(ctx->device);
  if (!g.ok) return XYWS_ERR_HIP;
  if (n) {
    const uint32_t grid = grid_for(n, RS_EV_THREADS, BC_GRID_CAP);
    hipLaunchKernelGGL(k_roster_events, dim3(grid), dim3(RS_EV_THREADS), 0, (hipStream_t)stream, dev_bconns, dev_rconns,
                       n, n_rooms, dev_jconns, dev_want, dev_results);
    const int rc = hip_err(hipGetLastError());
    if (rc != XYWS_OK) return rc;
  }
  if (n_rooms) {
    const uint32_t grid = grid_for(n_rooms, 1, BC_GRID_CAP);
    hipLaunchKernelGGL(k_roster_rooms, dim3(grid), dim3(RS_THREADS), 0, (hipStream_t)stream, dev_bconns, dev_rconns, n,
                       dev_rooms, dev_rrooms, dev_room_results, n_rooms, tx, (uint32_t)flags, dev_jconns, dev_want,
                       dev_results);
    const int rc = hip_err(hipGetLastError());
    if (rc != XYWS_OK) return rc;
  }
  if (!n) return XYWS_OK;
  const dim3 grid = fanout_grid(n, n_rooms != 0, BC_GRID_CAP, BC_BLOCKS_AIM, BC_SLICES_MAX);
  hipLaunchKernelGGL(k_roster_deliver, grid, dim3(BC_THREADS), 0, (hipStream_t)stream, dev_rconns, n, dev_rrooms,
                     dev_room_results, n_rooms, dev_results);
  return hip_err(hipGetLastError());
}

// Internal (tests and measurements, no HIP call): the geometry of
// k_roster_rooms and k_roster_deliver. out: {members per tile of the room
// pass, words of dev_want per step of the joiner scan, bytes per delivery
// step, grid cap}.
int xyws_debug_roster_geometry(uint64_t out[4]) {
  if (!out) return XYWS_ERR_INVALID;
  out[0] = RS_TILE;
  out[1] = RS_SCAN;
  out[2] = BC_STEP;
  out[3] = BC_GRID_CAP;
  return XYWS_OK;
}

}  // extern "C"

// rows_host_check.cpp — the row layouts the sweep kernels use
// (xynet_amd/csrc/xyws_rows.h, its pure part) held against the structs of
// include/xyws.h, as a stand-alone host program built with
// -fsanitize=address,undefined by tests/test_rows_host_check.py. For every row
// type: a struct filled through its named fields, each with its own non-zero
// byte pattern, equals byte for byte the words that XYWS_WORD and the pack
// functions produce; unpacking those words returns every field; a narrow field
// set alone to all-ones changes its own bytes only; reserved bytes come out
// zero (xyws_carry's bytes 43..47 are kept from the word given). Prints one
// line per failed check; exits 0 when there is none.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "xyws.h"
#include "xyws_rows.h"

namespace R = xyws_rows;

static int failures = 0;
static void expect(bool ok, const char* row, const char* what) {
  if (!ok) {
    std::printf("FAIL %s: %s\n", row, what);
    failures++;
  }
}
static void fill_bytes(void* p, size_t n, uint8_t seed) {
  for (size_t i = 0; i < n; i++) static_cast<uint8_t*>(p)[i] = (uint8_t)(seed + i);
}
static uint64_t rd(const void* p, size_t n) {  // a field's value (little-endian, at most 8 bytes)
  uint64_t v = 0;
  std::memcpy(&v, p, n);
  return v;
}
static void wr(void* p, size_t n, uint64_t v) { std::memcpy(p, &v, n); }

#define V(f) rd(&s.f, sizeof s.f)
#define V32(f) ((uint32_t)V(f))
#define SET(f, v) wr(&s.f, sizeof s.f, (v))
#define PUTW(T, f) (w[XYWS_WORD(T, f)] = V(f))  // a field that is a whole word
#define GETW(T, f) SET(f, w[XYWS_WORD(T, f)])
#define FILL(f, seed) fill_bytes(&s.f, sizeof s.f, seed)

// ---------------------------------------------------------------- rows of whole words
static void to_words(const xyws_conn& s, uint64_t* w) {
  PUTW(xyws_conn, buf); PUTW(xyws_conn, len); PUTW(xyws_conn, carry); PUTW(xyws_conn, frames); PUTW(xyws_conn, cap);
}
static void from_words(const uint64_t* w, xyws_conn& s) {
  GETW(xyws_conn, buf); GETW(xyws_conn, len); GETW(xyws_conn, carry); GETW(xyws_conn, frames); GETW(xyws_conn, cap);
}
static void to_words(const xyws_reply_conn& s, uint64_t* w) {
  PUTW(xyws_reply_conn, out); PUTW(xyws_reply_conn, out_cap); PUTW(xyws_reply_conn, rc); PUTW(xyws_reply_conn, verdicts);
}
static void from_words(const uint64_t* w, xyws_reply_conn& s) {
  GETW(xyws_reply_conn, out); GETW(xyws_reply_conn, out_cap); GETW(xyws_reply_conn, rc); GETW(xyws_reply_conn, verdicts);
}
static void to_words(const xyws_reasm_conn& s, uint64_t* w) {
  PUTW(xyws_reasm_conn, out); PUTW(xyws_reasm_conn, out_cap); PUTW(xyws_reasm_conn, mc); PUTW(xyws_reasm_conn, msgs);
  PUTW(xyws_reasm_conn, msg_cap);
}
static void from_words(const uint64_t* w, xyws_reasm_conn& s) {
  GETW(xyws_reasm_conn, out); GETW(xyws_reasm_conn, out_cap); GETW(xyws_reasm_conn, mc); GETW(xyws_reasm_conn, msgs);
  GETW(xyws_reasm_conn, msg_cap);
}
static void to_words(const xyws_hold_conn& s, uint64_t* w) {
  PUTW(xyws_hold_conn, hold_cap); PUTW(xyws_hold_conn, hc); PUTW(xyws_hold_conn, vmsgs); PUTW(xyws_hold_conn, vmsg_cap);
}
static void from_words(const uint64_t* w, xyws_hold_conn& s) {
  GETW(xyws_hold_conn, hold_cap); GETW(xyws_hold_conn, hc); GETW(xyws_hold_conn, vmsgs); GETW(xyws_hold_conn, vmsg_cap);
}
static void to_words(const xyws_room& s, uint64_t* w) {
  PUTW(xyws_room, members); PUTW(xyws_room, n_members); PUTW(xyws_room, wire); PUTW(xyws_room, wire_cap);
}
static void from_words(const uint64_t* w, xyws_room& s) {
  GETW(xyws_room, members); GETW(xyws_room, n_members); GETW(xyws_room, wire); GETW(xyws_room, wire_cap);
}
static void to_words(const xyws_accept_conn& s, uint64_t* w) {
  PUTW(xyws_accept_conn, buf); PUTW(xyws_accept_conn, len); PUTW(xyws_accept_conn, out); PUTW(xyws_accept_conn, out_cap);
}
static void from_words(const uint64_t* w, xyws_accept_conn& s) {
  GETW(xyws_accept_conn, buf); GETW(xyws_accept_conn, len); GETW(xyws_accept_conn, out); GETW(xyws_accept_conn, out_cap);
}

// ---------------------------------------------------------------- rows with shared words
static void to_words(const xyws_frame& s, uint64_t* w) {
  PUTW(xyws_frame, frame_off); PUTW(xyws_frame, payload_off); PUTW(xyws_frame, payload_len);
  w[XYWS_WORD(xyws_frame, key)] = R::pack_frame_meta({V32(key), V32(flags), V32(hdr_len), V32(status)});
}
static void from_words(const uint64_t* w, xyws_frame& s) {
  GETW(xyws_frame, frame_off); GETW(xyws_frame, payload_off); GETW(xyws_frame, payload_len);
  const R::frame_meta m = R::unpack_frame_meta(w[XYWS_WORD(xyws_frame, key)]);
  SET(key, m.key); SET(flags, m.flags); SET(hdr_len, m.hdr_len); SET(status, m.status);
}

static R::carry_head head_of(const xyws_carry& s) {
  return {V32(key), V32(hdr_len), rd(s.hdr, 8), rd(s.hdr + 8, sizeof s.hdr - 8)};
}
static void to_words(const xyws_carry& s, uint64_t* w) {  // (w: the words as found, for the reserved bytes)
  PUTW(xyws_carry, payload_remaining); PUTW(xyws_carry, phase); PUTW(xyws_carry, frames_total);
  R::pack_carry_head(head_of(s), w + XYWS_WORD(xyws_carry, key));
}
static void from_words(const uint64_t* w, xyws_carry& s) {
  GETW(xyws_carry, payload_remaining); GETW(xyws_carry, phase); GETW(xyws_carry, frames_total);
  const uint64_t* const k = w + XYWS_WORD(xyws_carry, key);
  const R::carry_head h = R::unpack_carry_head(k[0], k[1], k[2]);
  SET(key, h.key); SET(hdr_len, h.hdr_len);
  wr(s.hdr, 8, h.hdr_lo);
  wr(s.hdr + 8, sizeof s.hdr - 8, h.hdr_hi);
}

static void to_words(const xyws_verdict& s, uint64_t* w) {
  uint16_t h[4];
  R::pack_verdict(s.close_code, s.peer_code, s.action, h);
  std::memcpy(w, h, sizeof h);
}
static void from_words(const uint64_t* w, xyws_verdict& s) {
  uint16_t h[4];
  std::memcpy(h, w, sizeof h);
  s = R::unpack_verdict(h);
}

static void to_words(const xyws_reply_carry& s, uint64_t* w) {
  PUTW(xyws_reply_carry, frame_remaining); PUTW(xyws_reply_carry, frames_seen); PUTW(xyws_reply_carry, replies_total);
  w[XYWS_WORD(xyws_reply_carry, close_code)] = R::pack_reply_state({V32(close_code), V32(echoing), V32(status)});
}
static void from_words(const uint64_t* w, xyws_reply_carry& s) {
  GETW(xyws_reply_carry, frame_remaining); GETW(xyws_reply_carry, frames_seen); GETW(xyws_reply_carry, replies_total);
  const R::reply_state m = R::unpack_reply_state(w[XYWS_WORD(xyws_reply_carry, close_code)]);
  SET(close_code, m.close_code); SET(echoing, m.echoing); SET(status, m.status);
}
static void to_words(const xyws_reply_result& s, uint64_t* w) {
  PUTW(xyws_reply_result, reply_len); PUTW(xyws_reply_result, first_close);
  w[XYWS_WORD(xyws_reply_result, answered)] = R::pack_reply_counts({V32(answered), V32(close_code), V32(status)});
}
static void from_words(const uint64_t* w, xyws_reply_result& s) {
  GETW(xyws_reply_result, reply_len); GETW(xyws_reply_result, first_close);
  const R::reply_counts m = R::unpack_reply_counts(w[XYWS_WORD(xyws_reply_result, answered)]);
  SET(answered, m.answered); SET(close_code, m.close_code); SET(status, m.status);
}

static void to_words(const xyws_msg_carry& s, uint64_t* w) {
  PUTW(xyws_msg_carry, length); PUTW(xyws_msg_carry, nframes); PUTW(xyws_msg_carry, first_frame);
  PUTW(xyws_msg_carry, frame_remaining); PUTW(xyws_msg_carry, frames_seen);
  R::pack_msg_state({V32(status), V32(opcode), V32(frame_member), V32(utf8_len), V32(utf8)},
                    w + XYWS_WORD(xyws_msg_carry, status));
}
static void from_words(const uint64_t* w, xyws_msg_carry& s) {
  GETW(xyws_msg_carry, length); GETW(xyws_msg_carry, nframes); GETW(xyws_msg_carry, first_frame);
  GETW(xyws_msg_carry, frame_remaining); GETW(xyws_msg_carry, frames_seen);
  const uint64_t* const k = w + XYWS_WORD(xyws_msg_carry, status);
  const R::msg_state m = R::unpack_msg_state(k[0], k[1]);
  SET(status, m.status); SET(opcode, m.opcode); SET(frame_member, m.frame_member); SET(utf8_len, m.utf8_len);
  SET(utf8, m.utf8);
}
static void to_words(const xyws_reasm_result& s, uint64_t* w) {
  PUTW(xyws_reasm_result, out_len); PUTW(xyws_reasm_result, nmsgs);
  w[XYWS_WORD(xyws_reasm_result, completed)] = R::pack_reasm_counts({V32(completed), V32(status)});
}
static void from_words(const uint64_t* w, xyws_reasm_result& s) {
  GETW(xyws_reasm_result, out_len); GETW(xyws_reasm_result, nmsgs);
  const R::reasm_counts m = R::unpack_reasm_counts(w[XYWS_WORD(xyws_reasm_result, completed)]);
  SET(completed, m.completed); SET(status, m.status);
}
static void to_words(const xyws_message& s, uint64_t* w) {
  PUTW(xyws_message, first_frame); PUTW(xyws_message, nframes); PUTW(xyws_message, out_off); PUTW(xyws_message, length);
  w[XYWS_WORD(xyws_message, status)] = R::pack_message_meta({V32(status), V32(opcode)});
}
static void from_words(const uint64_t* w, xyws_message& s) {
  GETW(xyws_message, first_frame); GETW(xyws_message, nframes); GETW(xyws_message, out_off); GETW(xyws_message, length);
  const R::message_meta m = R::unpack_message_meta(w[XYWS_WORD(xyws_message, status)]);
  SET(status, m.status); SET(opcode, m.opcode);
}

static void to_words(const xyws_hold_carry& s, uint64_t* w) {
  PUTW(xyws_hold_carry, start); PUTW(xyws_hold_carry, held); PUTW(xyws_hold_carry, nframes);
  w[XYWS_WORD(xyws_hold_carry, status)] = R::pack_hold_state({V32(status), V32(opcode)});
}
static void from_words(const uint64_t* w, xyws_hold_carry& s) {
  GETW(xyws_hold_carry, start); GETW(xyws_hold_carry, held); GETW(xyws_hold_carry, nframes);
  const R::hold_state m = R::unpack_hold_state(w[XYWS_WORD(xyws_hold_carry, status)]);
  SET(status, m.status); SET(opcode, m.opcode);
}
// (a status alone in its word, behind it reserved0: the storers write the word as the status' value)
static void to_words(const xyws_hold_result& s, uint64_t* w) {
  PUTW(xyws_hold_result, held); PUTW(xyws_hold_result, delivered_len);
  w[XYWS_WORD(xyws_hold_result, status)] = XYWS_PUT(xyws_hold_result, status, s.status);
}
static void from_words(const uint64_t* w, xyws_hold_result& s) {
  GETW(xyws_hold_result, held); GETW(xyws_hold_result, delivered_len);
  SET(status, XYWS_GET(xyws_hold_result, status, w[XYWS_WORD(xyws_hold_result, status)]));
}

static void to_words(const xyws_room_result& s, uint64_t* w) {
  PUTW(xyws_room_result, wire_len);
  w[XYWS_WORD(xyws_room_result, nmsgs)] = R::pack_room_counts({V32(nmsgs), V32(skipped)});
  w[XYWS_WORD(xyws_room_result, receivers)] = R::pack_room_state({V32(receivers), V32(status)});
}
static void from_words(const uint64_t* w, xyws_room_result& s) {
  GETW(xyws_room_result, wire_len);
  const R::room_counts c = R::unpack_room_counts(w[XYWS_WORD(xyws_room_result, nmsgs)]);
  const R::room_state m = R::unpack_room_state(w[XYWS_WORD(xyws_room_result, receivers)]);
  SET(nmsgs, c.nmsgs); SET(skipped, c.skipped); SET(receivers, m.receivers); SET(status, m.status);
}
static void to_words(const xyws_bcast_conn& s, uint64_t* w) {
  PUTW(xyws_bcast_conn, head); PUTW(xyws_bcast_conn, head_len); PUTW(xyws_bcast_conn, out); PUTW(xyws_bcast_conn, out_cap);
  PUTW(xyws_bcast_conn, reply);
  w[XYWS_WORD(xyws_bcast_conn, room)] = XYWS_PUT(xyws_bcast_conn, room, s.room);
}
static void from_words(const uint64_t* w, xyws_bcast_conn& s) {
  GETW(xyws_bcast_conn, head); GETW(xyws_bcast_conn, head_len); GETW(xyws_bcast_conn, out); GETW(xyws_bcast_conn, out_cap);
  GETW(xyws_bcast_conn, reply);
  SET(room, XYWS_GET(xyws_bcast_conn, room, w[XYWS_WORD(xyws_bcast_conn, room)]));
}
static void to_words(const xyws_bcast_result& s, uint64_t* w) {
  PUTW(xyws_bcast_result, send_len); PUTW(xyws_bcast_result, bcast_len);
  w[XYWS_WORD(xyws_bcast_result, status)] = XYWS_PUT(xyws_bcast_result, status, s.status);
}
static void from_words(const uint64_t* w, xyws_bcast_result& s) {
  GETW(xyws_bcast_result, send_len); GETW(xyws_bcast_result, bcast_len);
  SET(status, XYWS_GET(xyws_bcast_result, status, w[XYWS_WORD(xyws_bcast_result, status)]));
}

static void to_words(const xyws_backlog_carry& s, uint64_t* w) {
  w[R::BLC_START] = s.start;
  w[R::BLC_LEN] = s.len;
  w[R::BLC_COUNTS] = R::pack_backlog_counts({s.count, s.gaps});
  w[R::BLC_TOTAL] = s.total;
  for (uint32_t i = 0; i < XYWS_BACKLOG_MAX; i++) w[R::BLC_FLEN + i] = s.flen[i];
}
static void from_words(const uint64_t* w, xyws_backlog_carry& s) {
  const R::backlog_counts c = R::unpack_backlog_counts(w[R::BLC_COUNTS]);
  s.start = w[R::BLC_START];
  s.len = w[R::BLC_LEN];
  s.count = c.count;
  s.gaps = c.gaps;
  s.total = w[R::BLC_TOTAL];
  for (uint32_t i = 0; i < XYWS_BACKLOG_MAX; i++) s.flen[i] = w[R::BLC_FLEN + i];
}
static void to_words(const xyws_backlog_room& s, uint64_t* w) {
  PUTW(xyws_backlog_room, log); PUTW(xyws_backlog_room, log_cap); PUTW(xyws_backlog_room, bc);
  w[XYWS_WORD(xyws_backlog_room, keep)] = XYWS_PUT(xyws_backlog_room, keep, s.keep);
}
static void from_words(const uint64_t* w, xyws_backlog_room& s) {
  GETW(xyws_backlog_room, log); GETW(xyws_backlog_room, log_cap); GETW(xyws_backlog_room, bc);
  SET(keep, XYWS_GET(xyws_backlog_room, keep, w[XYWS_WORD(xyws_backlog_room, keep)]));
}
static void to_words(const xyws_backlog_room_result& s, uint64_t* w) {
  PUTW(xyws_backlog_room_result, len);
  w[XYWS_WORD(xyws_backlog_room_result, count)] = R::pack_backlog_taken({V32(count), V32(folded)});
  w[XYWS_WORD(xyws_backlog_room_result, dropped)] = R::pack_backlog_state({V32(dropped), V32(status)});
}
static void from_words(const uint64_t* w, xyws_backlog_room_result& s) {
  GETW(xyws_backlog_room_result, len);
  const R::backlog_taken t = R::unpack_backlog_taken(w[XYWS_WORD(xyws_backlog_room_result, count)]);
  const R::backlog_state m = R::unpack_backlog_state(w[XYWS_WORD(xyws_backlog_room_result, dropped)]);
  SET(count, t.count); SET(folded, t.folded); SET(dropped, m.dropped); SET(status, m.status);
}
static void to_words(const xyws_backlog_conn& s, uint64_t* w) {
  PUTW(xyws_backlog_conn, out); PUTW(xyws_backlog_conn, out_cap); PUTW(xyws_backlog_conn, bcast);
  PUTW(xyws_backlog_conn, reply);
  w[XYWS_WORD(xyws_backlog_conn, room)] = R::pack_backlog_join({V32(room), V32(flags)});
}
static void from_words(const uint64_t* w, xyws_backlog_conn& s) {
  GETW(xyws_backlog_conn, out); GETW(xyws_backlog_conn, out_cap); GETW(xyws_backlog_conn, bcast);
  GETW(xyws_backlog_conn, reply);
  const R::backlog_join j = R::unpack_backlog_join(w[XYWS_WORD(xyws_backlog_conn, room)]);
  SET(room, j.room); SET(flags, j.flags);
}
static void to_words(const xyws_backlog_result& s, uint64_t* w) {
  PUTW(xyws_backlog_result, send_len); PUTW(xyws_backlog_result, backlog_len);
  w[XYWS_WORD(xyws_backlog_result, status)] = XYWS_PUT(xyws_backlog_result, status, s.status);
}
static void from_words(const uint64_t* w, xyws_backlog_result& s) {
  GETW(xyws_backlog_result, send_len); GETW(xyws_backlog_result, backlog_len);
  SET(status, XYWS_GET(xyws_backlog_result, status, w[XYWS_WORD(xyws_backlog_result, status)]));
}

static void to_words(const xyws_accept_result& s, uint64_t* w) {
  R::pack_accept({s.status, s.http_status, s.reason, s.consumed, s.resp_len, s.path_off, s.path_len, s.key_off}, w);
}
static void from_words(const uint64_t* w, xyws_accept_result& s) {
  const R::accept_fields a = R::unpack_accept(w);
  SET(status, a.status); SET(http_status, a.http_status); SET(reason, a.reason); SET(consumed, a.consumed);
  SET(resp_len, a.resp_len); SET(path_off, a.path_off); SET(path_len, a.path_len); SET(key_off, a.key_off);
}

// ---------------------------------------------------------------- the checks
// fill: every named field its own non-zero pattern; the reserved ones stay zero.
template <class T, class Fill>
static void check_row(const char* row, Fill fill) {
  T s{};
  fill(s);
  uint64_t w[sizeof(T) / 8] = {};
  to_words(s, w);
  expect(!std::memcmp(&s, w, sizeof(T)), row, "the packed words are the struct's bytes");
  T back{};
  from_words(w, back);
  expect(!std::memcmp(&s, &back, sizeof(T)), row, "unpacking returns every field");
}
// One narrow field all-ones, everything else zero: exactly that field's bytes are set.
template <class T, class Set>
static void check_ones(const char* what, Set set) {
  T s{};
  set(s);
  uint64_t w[sizeof(T) / 8] = {};
  to_words(s, w);
  expect(!std::memcmp(&s, w, sizeof(T)), what, "all-ones spills into a neighbour");
  T back{};
  from_words(w, back);
  expect(!std::memcmp(&s, &back, sizeof(T)), what, "all-ones does not come back");
}
#define ROW(T, ...) check_row<T>(#T, [](T& s) { __VA_ARGS__; })
#define ONES(T, f) check_ones<T>(#T "." #f, [](T& s) { std::memset(&s.f, 0xFF, sizeof s.f); })

// xyws_carry: hdr straddles three words; the reserved bytes 43..47 come from the word given.
static void check_carry_header() {
  for (uint32_t hl : {0u, 1u, 13u, 14u}) {
    xyws_carry s{};
    fill_bytes(s.key, 4, 0x11);
    s.hdr_len = (uint8_t)hl;
    fill_bytes(s.hdr, sizeof s.hdr, 0xC1);  // 14 distinct bytes, whatever hdr_len says
    uint64_t w[sizeof(xyws_carry) / 8] = {};
    uint8_t found[8] = {0x5A, 0x5B, 0x5C, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5};  // bytes 40..47 before the call
    std::memcpy(&w[XYWS_WORD(xyws_carry, key) + 2], found, 8);
    to_words(s, w);
    const uint8_t* const b = reinterpret_cast<const uint8_t*>(w);
    expect(!std::memcmp(b, &s, offsetof(xyws_carry, reserved)), "xyws_carry", "key, hdr_len and hdr[14] in place");
    expect(!std::memcmp(b + 43, found + 3, 5), "xyws_carry", "bytes 43..47 are kept");
    xyws_carry back{};
    from_words(w, back);
    expect(back.hdr_len == hl && !std::memcmp(back.hdr, s.hdr, sizeof s.hdr) && !std::memcmp(back.key, s.key, 4),
           "xyws_carry", "the header comes back");
  }
}

int main() {
  ROW(xyws_frame, FILL(frame_off, 0x10); FILL(payload_off, 0x20); FILL(payload_len, 0x30); FILL(key, 0x40);
      FILL(flags, 0x50); FILL(hdr_len, 0x60); FILL(status, 0x70));
  ONES(xyws_frame, key); ONES(xyws_frame, flags); ONES(xyws_frame, hdr_len); ONES(xyws_frame, status);

  ROW(xyws_carry, FILL(payload_remaining, 0x10); FILL(phase, 0x20); FILL(frames_total, 0x30); FILL(key, 0x40);
      FILL(hdr_len, 0x50); FILL(hdr, 0x60));
  ONES(xyws_carry, key); ONES(xyws_carry, hdr_len); ONES(xyws_carry, hdr);
  check_carry_header();

  ROW(xyws_conn, FILL(buf, 0x10); FILL(len, 0x20); FILL(carry, 0x30); FILL(frames, 0x40); FILL(cap, 0x50));
  ROW(xyws_verdict, FILL(close_code, 0x10); FILL(peer_code, 0x20); FILL(action, 0x30));
  ONES(xyws_verdict, close_code); ONES(xyws_verdict, peer_code); ONES(xyws_verdict, action);

  ROW(xyws_reply_conn, FILL(out, 0x10); FILL(out_cap, 0x20); FILL(rc, 0x30); FILL(verdicts, 0x40));
  ROW(xyws_reply_carry, FILL(frame_remaining, 0x10); FILL(frames_seen, 0x20); FILL(replies_total, 0x30);
      FILL(close_code, 0x40); FILL(echoing, 0x50); FILL(status, 0x60));
  ONES(xyws_reply_carry, close_code); ONES(xyws_reply_carry, echoing); ONES(xyws_reply_carry, status);
  ROW(xyws_reply_result, FILL(reply_len, 0x10); FILL(first_close, 0x20); FILL(answered, 0x30); FILL(close_code, 0x40);
      FILL(status, 0x50));
  ONES(xyws_reply_result, answered); ONES(xyws_reply_result, close_code); ONES(xyws_reply_result, status);

  ROW(xyws_reasm_conn, FILL(out, 0x10); FILL(out_cap, 0x20); FILL(mc, 0x30); FILL(msgs, 0x40); FILL(msg_cap, 0x50));
  ROW(xyws_msg_carry, FILL(length, 0x10); FILL(nframes, 0x20); FILL(first_frame, 0x30); FILL(frame_remaining, 0x40);
      FILL(frames_seen, 0x50); FILL(status, 0x60); FILL(opcode, 0x70); FILL(frame_member, 0x80); FILL(utf8_len, 0x90);
      FILL(utf8, 0xA0));
  ONES(xyws_msg_carry, status); ONES(xyws_msg_carry, opcode); ONES(xyws_msg_carry, frame_member);
  ONES(xyws_msg_carry, utf8_len); ONES(xyws_msg_carry, utf8);
  ROW(xyws_reasm_result, FILL(out_len, 0x10); FILL(nmsgs, 0x20); FILL(completed, 0x30); FILL(status, 0x40));
  ONES(xyws_reasm_result, completed); ONES(xyws_reasm_result, status);
  ROW(xyws_message, FILL(first_frame, 0x10); FILL(nframes, 0x20); FILL(out_off, 0x30); FILL(length, 0x40);
      FILL(status, 0x50); FILL(opcode, 0x60));
  ONES(xyws_message, status); ONES(xyws_message, opcode);

  ROW(xyws_hold_conn, FILL(hold_cap, 0x10); FILL(hc, 0x20); FILL(vmsgs, 0x30); FILL(vmsg_cap, 0x40));
  ROW(xyws_hold_carry, FILL(start, 0x10); FILL(held, 0x20); FILL(nframes, 0x30); FILL(status, 0x40); FILL(opcode, 0x50));
  ONES(xyws_hold_carry, status); ONES(xyws_hold_carry, opcode);
  ROW(xyws_hold_result, FILL(held, 0x10); FILL(delivered_len, 0x20); FILL(status, 0x30));
  ONES(xyws_hold_result, status);

  ROW(xyws_room, FILL(members, 0x10); FILL(n_members, 0x20); FILL(wire, 0x30); FILL(wire_cap, 0x40));
  ROW(xyws_room_result, FILL(wire_len, 0x10); FILL(nmsgs, 0x20); FILL(skipped, 0x30); FILL(receivers, 0x40);
      FILL(status, 0x50));
  ONES(xyws_room_result, nmsgs); ONES(xyws_room_result, skipped); ONES(xyws_room_result, receivers);
  ONES(xyws_room_result, status);
  ROW(xyws_bcast_conn, FILL(head, 0x10); FILL(head_len, 0x20); FILL(out, 0x30); FILL(out_cap, 0x40); FILL(reply, 0x50);
      FILL(room, 0x60));
  ONES(xyws_bcast_conn, room);
  ROW(xyws_bcast_result, FILL(send_len, 0x10); FILL(bcast_len, 0x20); FILL(status, 0x30));
  ONES(xyws_bcast_result, status);

  ROW(xyws_backlog_room, FILL(log, 0x10); FILL(log_cap, 0x20); FILL(bc, 0x30); FILL(keep, 0x40));
  ONES(xyws_backlog_room, keep);
  ROW(xyws_backlog_carry, FILL(start, 0x10); FILL(len, 0x20); FILL(count, 0x30); FILL(gaps, 0x40); FILL(total, 0x50);
      FILL(flen, 0x60));
  ONES(xyws_backlog_carry, count); ONES(xyws_backlog_carry, gaps);
  ROW(xyws_backlog_room_result, FILL(len, 0x10); FILL(count, 0x20); FILL(folded, 0x30); FILL(dropped, 0x40);
      FILL(status, 0x50));
  ONES(xyws_backlog_room_result, count); ONES(xyws_backlog_room_result, folded);
  ONES(xyws_backlog_room_result, dropped); ONES(xyws_backlog_room_result, status);
  ROW(xyws_backlog_conn, FILL(out, 0x10); FILL(out_cap, 0x20); FILL(bcast, 0x30); FILL(reply, 0x40); FILL(room, 0x50);
      FILL(flags, 0x60));
  ONES(xyws_backlog_conn, room); ONES(xyws_backlog_conn, flags);
  ROW(xyws_backlog_result, FILL(send_len, 0x10); FILL(backlog_len, 0x20); FILL(status, 0x30));
  ONES(xyws_backlog_result, status);

  ROW(xyws_accept_conn, FILL(buf, 0x10); FILL(len, 0x20); FILL(out, 0x30); FILL(out_cap, 0x40));
  ROW(xyws_accept_result, FILL(status, 0x10); FILL(http_status, 0x20); FILL(reason, 0x30); FILL(consumed, 0x40);
      FILL(resp_len, 0x50); FILL(path_off, 0x60); FILL(path_len, 0x70); FILL(key_off, 0x80));
  ONES(xyws_accept_result, status); ONES(xyws_accept_result, http_status); ONES(xyws_accept_result, reason);
  ONES(xyws_accept_result, consumed); ONES(xyws_accept_result, resp_len); ONES(xyws_accept_result, path_off);
  ONES(xyws_accept_result, path_len); ONES(xyws_accept_result, key_off);

  std::printf("%d failed\n", failures);
  return failures ? 1 : 0;
}

// xyws_rows.h — internal: the rows of the connection sweep's tables
// (xyws_decode_streams .. xyws_roster_streams), each stated once for every
// kernel that reads or writes it. include/xyws.h declares the rows as C
// structs; the kernels move them as 64-bit words, and this header is the one
// place that says which word and which bits a field is: every index and shift
// comes from offsetof, none is a literal.
//
// The pure part (word indices, pack and unpack of every word that holds more
// than one field, and the asserts that make "these fields share a word" true)
// needs nothing of HIP: a plain C++ compiler takes it
// (tests/cpp/rows_host_check.cpp). The device part (loaders and storers on
// global pointers) is compiled by hipcc only. A packed value must fit its
// field: pack does not mask.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "xyws.h"

#if defined(__HIPCC__)
#define XYWS_HD __host__ __device__ inline __attribute__((always_inline))
#define XYWS_HD_UNROLL _Pragma("unroll")
#else
#define XYWS_HD inline
#define XYWS_HD_UNROLL
#endif

// Field f of row type T: its 64-bit word, its first bit in that word, its value
// taken from / placed into the word.
#define XYWS_WORD(T, f) (offsetof(T, f) / 8)
#define XYWS_SHIFT(T, f) (8u * (uint32_t)(offsetof(T, f) % 8))
#define XYWS_GET(T, f, w) ((uint32_t)(((w) >> XYWS_SHIFT(T, f)) & ::xyws_rows::mask_of(sizeof(((T*)0)->f))))
#define XYWS_PUT(T, f, v) ((uint64_t)(v) << XYWS_SHIFT(T, f))
// The fields first..last of T lie in one word, and T is whole words.
#define XYWS_ONE_WORD(T, first, last)                                                                     \
  static_assert(XYWS_WORD(T, first) == (offsetof(T, last) + sizeof(((T*)0)->last) - 1) / 8 && sizeof(T) % 8 == 0, \
                #T ": " #first " .. " #last " share a word")

namespace xyws_rows {

constexpr uint64_t mask_of(size_t bytes) { return bytes >= 8 ? ~0ull : (1ull << (8 * bytes)) - 1ull; }

// ---------------------------------------------------------------- xyws_frame
struct frame_meta { uint32_t key, flags, hdr_len, status; };  // (key: the wire bytes, little-endian)
XYWS_ONE_WORD(xyws_frame, key, reserved);
XYWS_HD uint64_t pack_frame_meta(frame_meta m) {
  return XYWS_PUT(xyws_frame, key, m.key) | XYWS_PUT(xyws_frame, flags, m.flags) |
         XYWS_PUT(xyws_frame, hdr_len, m.hdr_len) | XYWS_PUT(xyws_frame, status, m.status);
}
XYWS_HD frame_meta unpack_frame_meta(uint64_t w) {
  return {XYWS_GET(xyws_frame, key, w), XYWS_GET(xyws_frame, flags, w), XYWS_GET(xyws_frame, hdr_len, w),
          XYWS_GET(xyws_frame, status, w)};
}

// ---------------------------------------------------------------- xyws_carry
// key, hdr_len and hdr[14] over three words (w[0] is the word of key); header
// byte i is byte i of hdr_lo (i < 8) or byte i - 8 of hdr_hi. The reserved
// bytes behind hdr in w[2] are kept as found.
struct carry_head { uint32_t key, hdr_len; uint64_t hdr_lo, hdr_hi; };
constexpr uint32_t CARRY_HDR_SHIFT = XYWS_SHIFT(xyws_carry, hdr);  // hdr[0] in w[0]
constexpr uint64_t CARRY_HDR_TAIL = mask_of(sizeof(((xyws_carry*)0)->hdr) - 8 - (64 - CARRY_HDR_SHIFT) / 8);  // hdr in w[2]
XYWS_ONE_WORD(xyws_carry, key, hdr_len);
static_assert(XYWS_WORD(xyws_carry, hdr) == XYWS_WORD(xyws_carry, key) && CARRY_HDR_SHIFT != 0 &&
                  (offsetof(xyws_carry, hdr) + sizeof(((xyws_carry*)0)->hdr) - 1) / 8 == XYWS_WORD(xyws_carry, key) + 2,
              "xyws_carry: hdr begins in the word of key and ends two words on");
XYWS_HD void pack_carry_head(carry_head h, uint64_t w[3]) {
  w[0] = XYWS_PUT(xyws_carry, key, h.key) | XYWS_PUT(xyws_carry, hdr_len, h.hdr_len) | (h.hdr_lo << CARRY_HDR_SHIFT);
  w[1] = (h.hdr_lo >> (64 - CARRY_HDR_SHIFT)) | (h.hdr_hi << CARRY_HDR_SHIFT);
  w[2] = ((h.hdr_hi >> (64 - CARRY_HDR_SHIFT)) & CARRY_HDR_TAIL) | (w[2] & ~CARRY_HDR_TAIL);
}
XYWS_HD carry_head unpack_carry_head(uint64_t w0, uint64_t w1, uint64_t w2) {
  return {XYWS_GET(xyws_carry, key, w0), XYWS_GET(xyws_carry, hdr_len, w0),
          (w0 >> CARRY_HDR_SHIFT) | (w1 << (64 - CARRY_HDR_SHIFT)),
          (w1 >> CARRY_HDR_SHIFT) | ((w2 & CARRY_HDR_TAIL) << (64 - CARRY_HDR_SHIFT))};
}

// ---------------------------------------------------------------- xyws_verdict
// (2-byte aligned: four half-words, the reserved bytes zero)
static_assert(sizeof(xyws_verdict) == 8 && offsetof(xyws_verdict, action) % 2 == 0, "xyws_verdict: four half-words");
XYWS_HD void pack_verdict(uint32_t close_code, uint32_t peer_code, uint32_t action, uint16_t h[4]) {
  h[0] = h[1] = h[2] = h[3] = 0;
  h[offsetof(xyws_verdict, close_code) / 2] = (uint16_t)close_code;
  h[offsetof(xyws_verdict, peer_code) / 2] = (uint16_t)peer_code;
  h[offsetof(xyws_verdict, action) / 2] = (uint16_t)action;
}
XYWS_HD xyws_verdict unpack_verdict(const uint16_t h[4]) {
  xyws_verdict v = {h[offsetof(xyws_verdict, close_code) / 2], h[offsetof(xyws_verdict, peer_code) / 2],
                    (uint8_t)h[offsetof(xyws_verdict, action) / 2], {0, 0, 0}};
  return v;
}

// ---------------------------------------------------------------- xyws_reply_carry, xyws_reply_result
struct reply_state { uint32_t close_code, echoing, status; };  // (the storer keeps the carry's reserved bytes)
XYWS_ONE_WORD(xyws_reply_carry, close_code, reserved);
XYWS_HD uint64_t pack_reply_state(reply_state s) {
  return XYWS_PUT(xyws_reply_carry, close_code, s.close_code) | XYWS_PUT(xyws_reply_carry, echoing, s.echoing) |
         XYWS_PUT(xyws_reply_carry, status, s.status);
}
XYWS_HD reply_state unpack_reply_state(uint64_t w) {
  return {XYWS_GET(xyws_reply_carry, close_code, w), XYWS_GET(xyws_reply_carry, echoing, w),
          XYWS_GET(xyws_reply_carry, status, w)};
}
constexpr uint64_t REPLY_STATE_BITS = mask_of(offsetof(xyws_reply_carry, reserved) % 8);  // the word without reserved

struct reply_counts { uint32_t answered, close_code, status; };
XYWS_ONE_WORD(xyws_reply_result, answered, status);
XYWS_HD uint64_t pack_reply_counts(reply_counts c) {
  return XYWS_PUT(xyws_reply_result, answered, c.answered) | XYWS_PUT(xyws_reply_result, close_code, c.close_code) |
         XYWS_PUT(xyws_reply_result, status, c.status);
}
XYWS_HD reply_counts unpack_reply_counts(uint64_t w) {
  return {XYWS_GET(xyws_reply_result, answered, w), XYWS_GET(xyws_reply_result, close_code, w),
          XYWS_GET(xyws_reply_result, status, w)};
}

// ---------------------------------------------------------------- xyws_msg_carry, xyws_reasm_result, xyws_message
// status .. utf8[3] over two words (w[0] is the word of status); utf8: the
// three bytes, byte i at bits 8i. The reserved bytes behind them are zero.
struct msg_state { uint32_t status, opcode, frame_member, utf8_len, utf8; };
constexpr uint32_t MSG_UTF8_SHIFT = XYWS_SHIFT(xyws_msg_carry, utf8);
XYWS_ONE_WORD(xyws_msg_carry, status, utf8_len);
static_assert(XYWS_WORD(xyws_msg_carry, utf8) == XYWS_WORD(xyws_msg_carry, status) && MSG_UTF8_SHIFT != 0 &&
                  XYWS_WORD(xyws_msg_carry, reserved) == XYWS_WORD(xyws_msg_carry, status) + 1,
              "xyws_msg_carry: utf8 begins in the word of status and ends in the next");
XYWS_HD void pack_msg_state(msg_state s, uint64_t w[2]) {
  w[0] = XYWS_PUT(xyws_msg_carry, status, s.status) | XYWS_PUT(xyws_msg_carry, opcode, s.opcode) |
         XYWS_PUT(xyws_msg_carry, frame_member, s.frame_member) | XYWS_PUT(xyws_msg_carry, utf8_len, s.utf8_len) |
         ((uint64_t)s.utf8 << MSG_UTF8_SHIFT);
  w[1] = (uint64_t)s.utf8 >> (64 - MSG_UTF8_SHIFT);
}
XYWS_HD msg_state unpack_msg_state(uint64_t w0, uint64_t w1) {
  return {XYWS_GET(xyws_msg_carry, status, w0), XYWS_GET(xyws_msg_carry, opcode, w0),
          XYWS_GET(xyws_msg_carry, frame_member, w0), XYWS_GET(xyws_msg_carry, utf8_len, w0),
          (uint32_t)(((w0 >> MSG_UTF8_SHIFT) | (w1 << (64 - MSG_UTF8_SHIFT))) & mask_of(sizeof(((xyws_msg_carry*)0)->utf8)))};
}

struct reasm_counts { uint32_t completed, status; };
XYWS_ONE_WORD(xyws_reasm_result, completed, status);
XYWS_HD uint64_t pack_reasm_counts(reasm_counts c) {
  return XYWS_PUT(xyws_reasm_result, completed, c.completed) | XYWS_PUT(xyws_reasm_result, status, c.status);
}
XYWS_HD reasm_counts unpack_reasm_counts(uint64_t w) {
  return {XYWS_GET(xyws_reasm_result, completed, w), XYWS_GET(xyws_reasm_result, status, w)};
}

struct message_meta { uint32_t status, opcode; };
XYWS_ONE_WORD(xyws_message, status, reserved);
XYWS_HD uint64_t pack_message_meta(message_meta m) {
  return XYWS_PUT(xyws_message, status, m.status) | XYWS_PUT(xyws_message, opcode, m.opcode);
}
XYWS_HD message_meta unpack_message_meta(uint64_t w) {
  return {XYWS_GET(xyws_message, status, w), XYWS_GET(xyws_message, opcode, w)};
}

// ---------------------------------------------------------------- xyws_hold_carry, xyws_hold_result
struct hold_state { uint32_t status, opcode; };
XYWS_ONE_WORD(xyws_hold_carry, status, reserved);
XYWS_HD uint64_t pack_hold_state(hold_state s) {
  return XYWS_PUT(xyws_hold_carry, status, s.status) | XYWS_PUT(xyws_hold_carry, opcode, s.opcode);
}
XYWS_HD hold_state unpack_hold_state(uint64_t w) {
  return {XYWS_GET(xyws_hold_carry, status, w), XYWS_GET(xyws_hold_carry, opcode, w)};
}
XYWS_ONE_WORD(xyws_hold_result, status, reserved0);

// ---------------------------------------------------------------- xyws_room_result, xyws_bcast_conn, xyws_bcast_result
struct room_counts { uint32_t nmsgs, skipped; };
struct room_state { uint32_t receivers, status; };
XYWS_ONE_WORD(xyws_room_result, nmsgs, skipped);
XYWS_ONE_WORD(xyws_room_result, receivers, status);
XYWS_HD uint64_t pack_room_counts(room_counts c) {
  return XYWS_PUT(xyws_room_result, nmsgs, c.nmsgs) | XYWS_PUT(xyws_room_result, skipped, c.skipped);
}
XYWS_HD room_counts unpack_room_counts(uint64_t w) {
  return {XYWS_GET(xyws_room_result, nmsgs, w), XYWS_GET(xyws_room_result, skipped, w)};
}
XYWS_HD uint64_t pack_room_state(room_state s) {
  return XYWS_PUT(xyws_room_result, receivers, s.receivers) | XYWS_PUT(xyws_room_result, status, s.status);
}
XYWS_HD room_state unpack_room_state(uint64_t w) {
  return {XYWS_GET(xyws_room_result, receivers, w), XYWS_GET(xyws_room_result, status, w)};
}
XYWS_ONE_WORD(xyws_bcast_conn, room, reserved0);
XYWS_ONE_WORD(xyws_bcast_result, status, reserved0);

// ---------------------------------------------------------------- the backlog's rows
struct backlog_counts { uint32_t count, gaps; };  // xyws_backlog_carry
XYWS_ONE_WORD(xyws_backlog_carry, count, gaps);
XYWS_HD uint64_t pack_backlog_counts(backlog_counts c) {
  return XYWS_PUT(xyws_backlog_carry, count, c.count) | XYWS_PUT(xyws_backlog_carry, gaps, c.gaps);
}
XYWS_HD backlog_counts unpack_backlog_counts(uint64_t w) {
  return {XYWS_GET(xyws_backlog_carry, count, w), XYWS_GET(xyws_backlog_carry, gaps, w)};
}
// (the fold keeps a copy of the carry in LDS and writes it back one word per thread)
constexpr uint32_t BLC_START = XYWS_WORD(xyws_backlog_carry, start), BLC_LEN = XYWS_WORD(xyws_backlog_carry, len),
                   BLC_COUNTS = XYWS_WORD(xyws_backlog_carry, count), BLC_TOTAL = XYWS_WORD(xyws_backlog_carry, total),
                   BLC_FLEN = XYWS_WORD(xyws_backlog_carry, flen), BLC_WORDS = sizeof(xyws_backlog_carry) / 8;
XYWS_ONE_WORD(xyws_backlog_room, keep, reserved0);

struct backlog_taken { uint32_t count, folded; };  // xyws_backlog_room_result
struct backlog_state { uint32_t dropped, status; };
XYWS_ONE_WORD(xyws_backlog_room_result, count, folded);
XYWS_ONE_WORD(xyws_backlog_room_result, dropped, status);
XYWS_HD uint64_t pack_backlog_taken(backlog_taken t) {
  return XYWS_PUT(xyws_backlog_room_result, count, t.count) | XYWS_PUT(xyws_backlog_room_result, folded, t.folded);
}
XYWS_HD backlog_taken unpack_backlog_taken(uint64_t w) {
  return {XYWS_GET(xyws_backlog_room_result, count, w), XYWS_GET(xyws_backlog_room_result, folded, w)};
}
XYWS_HD uint64_t pack_backlog_state(backlog_state s) {
  return XYWS_PUT(xyws_backlog_room_result, dropped, s.dropped) | XYWS_PUT(xyws_backlog_room_result, status, s.status);
}
XYWS_HD backlog_state unpack_backlog_state(uint64_t w) {
  return {XYWS_GET(xyws_backlog_room_result, dropped, w), XYWS_GET(xyws_backlog_room_result, status, w)};
}

struct backlog_join { uint32_t room, flags; };  // xyws_backlog_conn
XYWS_ONE_WORD(xyws_backlog_conn, room, flags);
XYWS_HD uint64_t pack_backlog_join(backlog_join j) {
  return XYWS_PUT(xyws_backlog_conn, room, j.room) | XYWS_PUT(xyws_backlog_conn, flags, j.flags);
}
XYWS_HD backlog_join unpack_backlog_join(uint64_t w) {
  return {XYWS_GET(xyws_backlog_conn, room, w), XYWS_GET(xyws_backlog_conn, flags, w)};
}
XYWS_ONE_WORD(xyws_backlog_result, status, reserved0);

// ---------------------------------------------------------------- the roster's rows
struct roster_ask { uint32_t room, flags; };  // xyws_roster_conn
XYWS_ONE_WORD(xyws_roster_conn, room, flags);
XYWS_HD uint64_t pack_roster_ask(roster_ask a) {
  return XYWS_PUT(xyws_roster_conn, room, a.room) | XYWS_PUT(xyws_roster_conn, flags, a.flags);
}
XYWS_HD roster_ask unpack_roster_ask(uint64_t w) {
  return {XYWS_GET(xyws_roster_conn, room, w), XYWS_GET(xyws_roster_conn, flags, w)};
}

struct roster_counts { uint32_t joined, left; };  // xyws_roster_room_result
struct roster_state { uint32_t n_members, status; };
XYWS_ONE_WORD(xyws_roster_room_result, joined, left);
XYWS_ONE_WORD(xyws_roster_room_result, n_members, status);
XYWS_HD uint64_t pack_roster_counts(roster_counts c) {
  return XYWS_PUT(xyws_roster_room_result, joined, c.joined) | XYWS_PUT(xyws_roster_room_result, left, c.left);
}
XYWS_HD roster_counts unpack_roster_counts(uint64_t w) {
  return {XYWS_GET(xyws_roster_room_result, joined, w), XYWS_GET(xyws_roster_room_result, left, w)};
}
XYWS_HD uint64_t pack_roster_state(roster_state s) {
  return XYWS_PUT(xyws_roster_room_result, n_members, s.n_members) | XYWS_PUT(xyws_roster_room_result, status, s.status);
}
XYWS_HD roster_state unpack_roster_state(uint64_t w) {
  return {XYWS_GET(xyws_roster_room_result, n_members, w), XYWS_GET(xyws_roster_room_result, status, w)};
}

struct roster_place { uint32_t status, room; };  // xyws_roster_result
XYWS_ONE_WORD(xyws_roster_result, status, room);
XYWS_HD uint64_t pack_roster_place(roster_place p) {
  return XYWS_PUT(xyws_roster_result, status, p.status) | XYWS_PUT(xyws_roster_result, room, p.room);
}
XYWS_HD roster_place unpack_roster_place(uint64_t w) {
  return {XYWS_GET(xyws_roster_result, status, w), XYWS_GET(xyws_roster_result, room, w)};
}
// A roster row read as a broadcast row (xyws_backlog_conn.bcast may name one): the
// words and the status field's place agree, and so do the bits the backlog tests.
static_assert(XYWS_WORD(xyws_roster_result, send_len) == XYWS_WORD(xyws_bcast_result, send_len) &&
                  XYWS_WORD(xyws_roster_result, note_len) == XYWS_WORD(xyws_bcast_result, bcast_len) &&
                  offsetof(xyws_roster_result, status) == offsetof(xyws_bcast_result, status) &&
                  sizeof(((xyws_roster_result*)0)->status) == sizeof(((xyws_bcast_result*)0)->status) &&
                  sizeof(xyws_roster_result) == sizeof(xyws_bcast_result),
              "xyws_roster_result: send_len, note_len and status lie as xyws_bcast_result's send_len, bcast_len and status");
static_assert(XYWS_RSC_TRUNCATED == XYWS_BC_TRUNCATED && XYWS_RSC_NOT_RECEIVER == XYWS_BC_NOT_RECEIVER &&
                  XYWS_RSC_NO_ROOM == XYWS_BC_NO_ROOM,
              "xyws_roster_result: the first three status bits are xyws_bcast_result's");

// xyws_roster_text as the kernels take it: the three strings as 64-bit words
// (byte i of a string = byte i % 8 of its word i / 8), then the lengths.
constexpr uint32_t ROSTER_TEXT_WORDS = XYWS_ROSTER_TEXT_MAX / 8;
static_assert(XYWS_ROSTER_TEXT_MAX % 8 == 0 && offsetof(xyws_roster_text, head) == 0 &&
                  offsetof(xyws_roster_text, joined) == XYWS_ROSTER_TEXT_MAX &&
                  offsetof(xyws_roster_text, left) == 2 * XYWS_ROSTER_TEXT_MAX &&
                  offsetof(xyws_roster_text, head_len) == 3 * XYWS_ROSTER_TEXT_MAX,
              "xyws_roster_text: three strings of whole words, then the lengths");
struct roster_words {
  uint64_t w[3 * ROSTER_TEXT_WORDS];  // head, joined, left
  uint32_t head_len, joined_len, left_len;
};
XYWS_HD roster_words pack_roster_text(const xyws_roster_text& t) {
  roster_words r;
  const uint8_t* const b = reinterpret_cast<const uint8_t*>(&t);  // (the strings come first: the assert above)
  for (uint32_t k = 0; k < 3 * ROSTER_TEXT_WORDS; k++) {
    uint64_t v = 0;
    for (uint32_t i = 0; i < 8; i++) v |= (uint64_t)b[8 * k + i] << (8 * i);
    r.w[k] = v;
  }
  r.head_len = t.head_len;
  r.joined_len = t.joined_len;
  r.left_len = t.left_len;
  return r;
}

// ---------------------------------------------------------------- xyws_accept_result
// Four words of two or three fields each, w[0] the word of status.
struct accept_fields { uint32_t status, http_status, reason, consumed, resp_len, path_off, path_len, key_off; };
XYWS_ONE_WORD(xyws_accept_result, status, reason);
XYWS_ONE_WORD(xyws_accept_result, consumed, resp_len);
XYWS_ONE_WORD(xyws_accept_result, path_off, path_len);
XYWS_ONE_WORD(xyws_accept_result, key_off, reserved);
static_assert(XYWS_WORD(xyws_accept_result, key_off) == 3 * XYWS_WORD(xyws_accept_result, consumed) &&
                  XYWS_WORD(xyws_accept_result, path_off) == 2 * XYWS_WORD(xyws_accept_result, consumed) &&
                  sizeof(xyws_accept_result) == 4 * 8,
              "xyws_accept_result: four words in the order of pack_accept");
XYWS_HD void pack_accept(accept_fields a, uint64_t w[4]) {
  // (http_status and reason joined in 32 bits first: placed apart, k_accept_streams keeps four more scalars spilled)
  w[XYWS_WORD(xyws_accept_result, status)] =
      XYWS_PUT(xyws_accept_result, status, a.status) |
      XYWS_PUT(xyws_accept_result, http_status,
               a.http_status | (a.reason << (XYWS_SHIFT(xyws_accept_result, reason) - XYWS_SHIFT(xyws_accept_result, http_status))));
  w[XYWS_WORD(xyws_accept_result, consumed)] =
      XYWS_PUT(xyws_accept_result, consumed, a.consumed) | XYWS_PUT(xyws_accept_result, resp_len, a.resp_len);
  w[XYWS_WORD(xyws_accept_result, path_off)] =
      XYWS_PUT(xyws_accept_result, path_off, a.path_off) | XYWS_PUT(xyws_accept_result, path_len, a.path_len);
  w[XYWS_WORD(xyws_accept_result, key_off)] = XYWS_PUT(xyws_accept_result, key_off, a.key_off);
}
XYWS_HD accept_fields unpack_accept(const uint64_t w[4]) {
  const uint64_t a = w[XYWS_WORD(xyws_accept_result, status)], b = w[XYWS_WORD(xyws_accept_result, consumed)],
                 c = w[XYWS_WORD(xyws_accept_result, path_off)], d = w[XYWS_WORD(xyws_accept_result, key_off)];
  return {XYWS_GET(xyws_accept_result, status, a),   XYWS_GET(xyws_accept_result, http_status, a),
          XYWS_GET(xyws_accept_result, reason, a),   XYWS_GET(xyws_accept_result, consumed, b),
          XYWS_GET(xyws_accept_result, resp_len, b), XYWS_GET(xyws_accept_result, path_off, c),
          XYWS_GET(xyws_accept_result, path_len, c), XYWS_GET(xyws_accept_result, key_off, d)};
}

// ---------------------------------------------------------------- xyws_route_conn, xyws_route_result
// Three words of two fields each (key_len with reserved[0], which is zero), then a reserved word.
struct route_place { uint32_t status, room; };
struct route_key { uint32_t route, key_off; };
XYWS_ONE_WORD(xyws_route_conn, rconn, reserved);
XYWS_ONE_WORD(xyws_route_result, status, room);
XYWS_ONE_WORD(xyws_route_result, route, key_off);
static_assert(XYWS_SHIFT(xyws_route_result, key_len) == 0 && XYWS_WORD(xyws_route_result, key_len) + 2 == sizeof(xyws_route_result) / 8,
              "xyws_route_result: key_len begins the third of four words");
XYWS_HD uint64_t pack_route_place(route_place p) {
  return XYWS_PUT(xyws_route_result, status, p.status) | XYWS_PUT(xyws_route_result, room, p.room);
}
XYWS_HD route_place unpack_route_place(uint64_t w) {
  return {XYWS_GET(xyws_route_result, status, w), XYWS_GET(xyws_route_result, room, w)};
}
XYWS_HD uint64_t pack_route_key(route_key k) {
  return XYWS_PUT(xyws_route_result, route, k.route) | XYWS_PUT(xyws_route_result, key_off, k.key_off);
}
XYWS_HD route_key unpack_route_key(uint64_t w) {
  return {XYWS_GET(xyws_route_result, route, w), XYWS_GET(xyws_route_result, key_off, w)};
}
// xyws_roster_conn.room as a 32-bit word of its row: what xyws_route_streams stores alone.
constexpr uint32_t ROSTER_ROOM_HALF = offsetof(xyws_roster_conn, room) / 4;
static_assert(offsetof(xyws_roster_conn, room) % 4 == 0 && sizeof(((xyws_roster_conn*)0)->room) == 4,
              "xyws_roster_conn: room is one aligned 32-bit word");

// ---------------------------------------------------------------- xyws_outbox_conn, xyws_outbox_entry, xyws_outbox_summary
// The conn row is six whole words. An entry is four words, the first of them
// conn and flags; the summary's counts are two words of two fields each.
struct outbox_tag { uint32_t conn, flags; };             // xyws_outbox_entry
struct outbox_counts { uint32_t n_close, n_truncated; };  // xyws_outbox_summary
struct outbox_state { uint32_t n_deferred, status; };
XYWS_ONE_WORD(xyws_outbox_entry, conn, flags);
XYWS_ONE_WORD(xyws_outbox_summary, n_close, n_truncated);
XYWS_ONE_WORD(xyws_outbox_summary, n_deferred, status);
constexpr uint32_t OBE_WORDS = sizeof(xyws_outbox_entry) / 8, OBS_WORDS = sizeof(xyws_outbox_summary) / 8;
static_assert(XYWS_WORD(xyws_outbox_conn, reserved) == 6 * XYWS_WORD(xyws_outbox_conn, out_cap) &&
                  sizeof(xyws_outbox_conn) == 8 * 8 && XYWS_WORD(xyws_outbox_summary, reserved) + 2 == OBS_WORDS,
              "xyws_outbox_conn: six words and two reserved; xyws_outbox_summary: two reserved words end it");
XYWS_HD uint64_t pack_outbox_tag(outbox_tag t) {
  return XYWS_PUT(xyws_outbox_entry, conn, t.conn) | XYWS_PUT(xyws_outbox_entry, flags, t.flags);
}
XYWS_HD outbox_tag unpack_outbox_tag(uint64_t w) {
  return {XYWS_GET(xyws_outbox_entry, conn, w), XYWS_GET(xyws_outbox_entry, flags, w)};
}
XYWS_HD uint64_t pack_outbox_counts(outbox_counts c) {
  return XYWS_PUT(xyws_outbox_summary, n_close, c.n_close) | XYWS_PUT(xyws_outbox_summary, n_truncated, c.n_truncated);
}
XYWS_HD outbox_counts unpack_outbox_counts(uint64_t w) {
  return {XYWS_GET(xyws_outbox_summary, n_close, w), XYWS_GET(xyws_outbox_summary, n_truncated, w)};
}
XYWS_HD uint64_t pack_outbox_state(outbox_state s) {
  return XYWS_PUT(xyws_outbox_summary, n_deferred, s.n_deferred) | XYWS_PUT(xyws_outbox_summary, status, s.status);
}
XYWS_HD outbox_state unpack_outbox_state(uint64_t w) {
  return {XYWS_GET(xyws_outbox_summary, n_deferred, w), XYWS_GET(xyws_outbox_summary, status, w)};
}
// A whole entry and a whole summary as the words the kernels store, one word per thread.
struct outbox_entry_fields { outbox_tag tag; uint64_t off, len, full_len; };
XYWS_HD void pack_outbox_entry(const outbox_entry_fields& e, uint64_t w[OBE_WORDS]) {
  w[XYWS_WORD(xyws_outbox_entry, conn)] = pack_outbox_tag(e.tag);
  w[XYWS_WORD(xyws_outbox_entry, off)] = e.off;
  w[XYWS_WORD(xyws_outbox_entry, len)] = e.len;
  w[XYWS_WORD(xyws_outbox_entry, full_len)] = e.full_len;
}
struct outbox_summary_fields { uint64_t n_entries, pack_len, packed_len, send_bytes; outbox_counts counts; outbox_state state; };
XYWS_HD void pack_outbox_summary(const outbox_summary_fields& s, uint64_t w[OBS_WORDS]) {
  XYWS_HD_UNROLL
  for (uint32_t i = 0; i < OBS_WORDS; i++) w[i] = 0;  // (the reserved words)
  w[XYWS_WORD(xyws_outbox_summary, n_entries)] = s.n_entries;
  w[XYWS_WORD(xyws_outbox_summary, pack_len)] = s.pack_len;
  w[XYWS_WORD(xyws_outbox_summary, packed_len)] = s.packed_len;
  w[XYWS_WORD(xyws_outbox_summary, send_bytes)] = s.send_bytes;
  w[XYWS_WORD(xyws_outbox_summary, n_close)] = pack_outbox_counts(s.counts);
  w[XYWS_WORD(xyws_outbox_summary, n_deferred)] = pack_outbox_state(s.state);
}

// ---------------------------------------------------------------- the inbox's rows
// Head, entry, carry and result are four words each, the conn row and the
// summary eight. Every word that holds two fields is stated here.
struct inbox_tag { uint32_t conn, flags; };            // xyws_inbox_entry
struct inbox_state { uint32_t state, status; };        // xyws_inbox_carry
struct inbox_flags { uint32_t flags, reserved0; };     // xyws_inbox_conn
struct inbox_counts { uint32_t n_entries, status; };   // xyws_inbox_result
struct inbox_conns { uint32_t n_conns, n_opened; };    // xyws_inbox_summary
struct inbox_ends { uint32_t n_eof, n_broken; };
struct inbox_bad { uint32_t n_bad_entries, status; };
XYWS_ONE_WORD(xyws_inbox_entry, conn, flags);
XYWS_ONE_WORD(xyws_inbox_carry, state, status);
XYWS_ONE_WORD(xyws_inbox_conn, flags, reserved0);
XYWS_ONE_WORD(xyws_inbox_result, n_entries, status);
XYWS_ONE_WORD(xyws_inbox_summary, n_conns, n_opened);
XYWS_ONE_WORD(xyws_inbox_summary, n_eof, n_broken);
XYWS_ONE_WORD(xyws_inbox_summary, n_bad_entries, status);
constexpr uint32_t IBS_WORDS = sizeof(xyws_inbox_summary) / 8;
static_assert(sizeof(xyws_inbox_head) == 4 * 8 && sizeof(xyws_inbox_entry) == 4 * 8 && sizeof(xyws_inbox_carry) == 4 * 8 &&
                  sizeof(xyws_inbox_conn) == 8 * 8 && sizeof(xyws_inbox_result) == 4 * 8 &&
                  XYWS_WORD(xyws_inbox_summary, reserved) + 3 == IBS_WORDS &&
                  XYWS_WORD(xyws_inbox_result, reserved) == 3 * XYWS_WORD(xyws_inbox_result, lead),
              "the inbox's rows: whole words, the summary ends with three reserved ones, a result row with one");
XYWS_HD uint64_t pack_inbox_tag(inbox_tag t) {
  return XYWS_PUT(xyws_inbox_entry, conn, t.conn) | XYWS_PUT(xyws_inbox_entry, flags, t.flags);
}
XYWS_HD inbox_tag unpack_inbox_tag(uint64_t w) {
  return {XYWS_GET(xyws_inbox_entry, conn, w), XYWS_GET(xyws_inbox_entry, flags, w)};
}
XYWS_HD uint64_t pack_inbox_state(inbox_state s) {
  return XYWS_PUT(xyws_inbox_carry, state, s.state) | XYWS_PUT(xyws_inbox_carry, status, s.status);
}
XYWS_HD inbox_state unpack_inbox_state(uint64_t w) {
  return {XYWS_GET(xyws_inbox_carry, state, w), XYWS_GET(xyws_inbox_carry, status, w)};
}
XYWS_HD uint64_t pack_inbox_flags(inbox_flags f) {
  return XYWS_PUT(xyws_inbox_conn, flags, f.flags) | XYWS_PUT(xyws_inbox_conn, reserved0, f.reserved0);
}
XYWS_HD inbox_flags unpack_inbox_flags(uint64_t w) {
  return {XYWS_GET(xyws_inbox_conn, flags, w), XYWS_GET(xyws_inbox_conn, reserved0, w)};
}
XYWS_HD uint64_t pack_inbox_counts(inbox_counts c) {
  return XYWS_PUT(xyws_inbox_result, n_entries, c.n_entries) | XYWS_PUT(xyws_inbox_result, status, c.status);
}
XYWS_HD inbox_counts unpack_inbox_counts(uint64_t w) {
  return {XYWS_GET(xyws_inbox_result, n_entries, w), XYWS_GET(xyws_inbox_result, status, w)};
}
XYWS_HD uint64_t pack_inbox_conns(inbox_conns c) {
  return XYWS_PUT(xyws_inbox_summary, n_conns, c.n_conns) | XYWS_PUT(xyws_inbox_summary, n_opened, c.n_opened);
}
XYWS_HD inbox_conns unpack_inbox_conns(uint64_t w) {
  return {XYWS_GET(xyws_inbox_summary, n_conns, w), XYWS_GET(xyws_inbox_summary, n_opened, w)};
}
XYWS_HD uint64_t pack_inbox_ends(inbox_ends e) {
  return XYWS_PUT(xyws_inbox_summary, n_eof, e.n_eof) | XYWS_PUT(xyws_inbox_summary, n_broken, e.n_broken);
}
XYWS_HD inbox_ends unpack_inbox_ends(uint64_t w) {
  return {XYWS_GET(xyws_inbox_summary, n_eof, w), XYWS_GET(xyws_inbox_summary, n_broken, w)};
}
XYWS_HD uint64_t pack_inbox_bad(inbox_bad b) {
  return XYWS_PUT(xyws_inbox_summary, n_bad_entries, b.n_bad_entries) | XYWS_PUT(xyws_inbox_summary, status, b.status);
}
XYWS_HD inbox_bad unpack_inbox_bad(uint64_t w) {
  return {XYWS_GET(xyws_inbox_summary, n_bad_entries, w), XYWS_GET(xyws_inbox_summary, status, w)};
}
// A whole summary as the words the summary pass stores, one word per thread.
struct inbox_summary_fields { uint64_t n_entries, bytes; inbox_conns conns; inbox_ends ends; inbox_bad bad; };
XYWS_HD void pack_inbox_summary(const inbox_summary_fields& s, uint64_t w[IBS_WORDS]) {
  XYWS_HD_UNROLL
  for (uint32_t i = 0; i < IBS_WORDS; i++) w[i] = 0;  // (the reserved words)
  w[XYWS_WORD(xyws_inbox_summary, n_entries)] = s.n_entries;
  w[XYWS_WORD(xyws_inbox_summary, bytes)] = s.bytes;
  w[XYWS_WORD(xyws_inbox_summary, n_conns)] = pack_inbox_conns(s.conns);
  w[XYWS_WORD(xyws_inbox_summary, n_eof)] = pack_inbox_ends(s.ends);
  w[XYWS_WORD(xyws_inbox_summary, n_bad_entries)] = pack_inbox_bad(s.bad);
}

}  // namespace xyws_rows

// ================================================================ the device part
#if defined(__HIPCC__)
#include "xyws_device.h"

typedef XYWS_GLOBAL uint16_t g_u16;

namespace xyws_rows {

// Field f (a whole word, or the word that holds it) of the row at p: U = true
// takes it wave-uniform, in scalar registers; U = false is each thread's own load.
template <bool U>
XYWS_DEV uint64_t load_word(const void* p, size_t w) {
  const uint64_t v = ((const g_u64*)p)[w];
  return U ? uniform64(v) : v;
}
#define XYWS_LD(U, T, p, f) ::xyws_rows::load_word<U>(p, XYWS_WORD(T, f))
#define XYWS_ST(T, p, f, v) (((g_u64*)(p))[XYWS_WORD(T, f)] = (v))

// Row i of the table of T at device address base.
template <class T>
XYWS_DEV T* row_at(uint64_t base, uint64_t i) { return (T*)(base + sizeof(T) * i); }

// A whole row copied as it is, one word per lane.
template <class T>
XYWS_DEV void copy_row(T* dst, const T* src, uint32_t lane) {
  if (lane < sizeof(T) / 8) ((g_u64*)dst)[lane] = ((const g_u64*)src)[lane];
}

// ---- xyws_conn (wave-uniform), xyws_frame (one per thread), xyws_carry, xyws_verdict
struct conn_row { uint64_t buf, len, frames, cap; };
XYWS_DEV conn_row load_conn(const xyws_conn* p) {
  return {XYWS_LD(true, xyws_conn, p, buf), XYWS_LD(true, xyws_conn, p, len), XYWS_LD(true, xyws_conn, p, frames),
          XYWS_LD(true, xyws_conn, p, cap)};
}

struct frame_row { uint64_t payload_off, payload_len; uint32_t flags, status; };
XYWS_DEV frame_row load_frame(const xyws_frame* p) {
  const frame_meta m = unpack_frame_meta(XYWS_LD(false, xyws_frame, p, key));
  return {XYWS_LD(false, xyws_frame, p, payload_off), XYWS_LD(false, xyws_frame, p, payload_len), m.flags, m.status};
}
XYWS_DEV void store_frame(xyws_frame* p, uint64_t frame_off, uint64_t payload_off, uint64_t payload_len, frame_meta m) {
  XYWS_ST(xyws_frame, p, frame_off, frame_off);
  XYWS_ST(xyws_frame, p, payload_off, payload_off);
  XYWS_ST(xyws_frame, p, payload_len, payload_len);
  XYWS_ST(xyws_frame, p, key, pack_frame_meta(m));
}

struct carry_row { uint64_t payload_remaining, phase; carry_head head; };
XYWS_DEV carry_row load_carry(const xyws_carry* p) {
  const size_t k = XYWS_WORD(xyws_carry, key);
  return {XYWS_LD(true, xyws_carry, p, payload_remaining), XYWS_LD(true, xyws_carry, p, phase),
          unpack_carry_head(load_word<true>(p, k), load_word<true>(p, k + 1), load_word<true>(p, k + 2))};
}
// (frames_total grows by nframes; the reserved bytes behind hdr stay)
XYWS_DEV void store_carry(xyws_carry* p, uint64_t payload_remaining, uint64_t phase, uint64_t nframes, carry_head head) {
  g_u64* const row = (g_u64*)p;
  const size_t k = XYWS_WORD(xyws_carry, key);
  XYWS_ST(xyws_carry, p, payload_remaining, payload_remaining);
  XYWS_ST(xyws_carry, p, phase, phase);
  row[XYWS_WORD(xyws_carry, frames_total)] += nframes;
  uint64_t h[3] = {0, 0, row[k + 2]};
  pack_carry_head(head, h);
#pragma unroll
  for (uint32_t i = 0; i < 3; i++) row[k + i] = h[i];
}

XYWS_DEV void store_verdict(xyws_verdict* p, const xyws_verdict& v) {
  uint16_t h[4];
  pack_verdict(v.close_code, v.peer_code, v.action, h);
#pragma unroll
  for (uint32_t i = 0; i < 4; i++) ((g_u16*)p)[i] = h[i];
}

// ---- xyws_reply_conn, xyws_reply_carry (wave-uniform), xyws_reply_result
struct reply_conn_row { uint64_t out, out_cap, rc, verdicts; };
XYWS_DEV reply_conn_row load_reply_conn(const xyws_reply_conn* p) {
  return {XYWS_LD(true, xyws_reply_conn, p, out), XYWS_LD(true, xyws_reply_conn, p, out_cap),
          XYWS_LD(true, xyws_reply_conn, p, rc), XYWS_LD(true, xyws_reply_conn, p, verdicts)};
}

struct reply_carry_row { uint64_t frame_remaining, frames_seen, replies_total, state_word; reply_state state; };
XYWS_DEV reply_carry_row load_reply_carry(const xyws_reply_carry* p) {
  const uint64_t w = XYWS_LD(true, xyws_reply_carry, p, close_code);
  return {XYWS_LD(true, xyws_reply_carry, p, frame_remaining), XYWS_LD(true, xyws_reply_carry, p, frames_seen),
          XYWS_LD(true, xyws_reply_carry, p, replies_total), w, unpack_reply_state(w)};
}
// Status bits set in the word of close_code as loaded (state_word); nothing else is written.
XYWS_DEV void raise_reply_status(xyws_reply_carry* p, uint64_t state_word, uint32_t bits) {
  XYWS_ST(xyws_reply_carry, p, close_code, state_word | XYWS_PUT(xyws_reply_carry, status, bits));
}
// The whole carry; the reserved bytes stay as state_word has them.
XYWS_DEV void store_reply_carry(xyws_reply_carry* p, uint64_t frame_remaining, uint64_t frames_seen,
                                uint64_t replies_total, uint64_t state_word, reply_state s) {
  XYWS_ST(xyws_reply_carry, p, frame_remaining, frame_remaining);
  XYWS_ST(xyws_reply_carry, p, frames_seen, frames_seen);
  XYWS_ST(xyws_reply_carry, p, replies_total, replies_total);
  XYWS_ST(xyws_reply_carry, p, close_code, (state_word & ~REPLY_STATE_BITS) | pack_reply_state(s));
}

struct reply_result_row { uint64_t reply_len, first_close; uint32_t status; };
template <bool U>
XYWS_DEV reply_result_row load_reply_result(const xyws_reply_result* p) {
  return {XYWS_LD(U, xyws_reply_result, p, reply_len), XYWS_LD(U, xyws_reply_result, p, first_close),
          unpack_reply_counts(XYWS_LD(U, xyws_reply_result, p, answered)).status};
}
XYWS_DEV void store_reply_result(xyws_reply_result* p, uint64_t reply_len, uint64_t first_close, reply_counts c) {
  XYWS_ST(xyws_reply_result, p, reply_len, reply_len);
  XYWS_ST(xyws_reply_result, p, first_close, first_close);
  XYWS_ST(xyws_reply_result, p, answered, pack_reply_counts(c));
  XYWS_ST(xyws_reply_result, p, reserved, 0);
}

// ---- xyws_reasm_conn, xyws_msg_carry (wave-uniform), xyws_reasm_result, xyws_message
// (out_cap counts as 0 without out, msg_cap without msgs: then neither is loaded)
struct reasm_conn_row { uint64_t out, out_cap, mc, msgs, msg_cap; };
template <bool U>
XYWS_DEV reasm_conn_row load_reasm_conn(const xyws_reasm_conn* p) {
  reasm_conn_row r;
  r.out = XYWS_LD(U, xyws_reasm_conn, p, out);
  r.out_cap = r.out ? XYWS_LD(U, xyws_reasm_conn, p, out_cap) : 0;
  r.mc = XYWS_LD(U, xyws_reasm_conn, p, mc);
  r.msgs = XYWS_LD(U, xyws_reasm_conn, p, msgs);
  r.msg_cap = r.msgs ? XYWS_LD(U, xyws_reasm_conn, p, msg_cap) : 0;
  return r;
}
XYWS_DEV void store_reasm_conn(xyws_reasm_conn* p, const reasm_conn_row& r) {
  XYWS_ST(xyws_reasm_conn, p, out, r.out);
  XYWS_ST(xyws_reasm_conn, p, out_cap, r.out_cap);
  XYWS_ST(xyws_reasm_conn, p, mc, r.mc);
  XYWS_ST(xyws_reasm_conn, p, msgs, r.msgs);
  XYWS_ST(xyws_reasm_conn, p, msg_cap, r.msg_cap);
  for (size_t w = XYWS_WORD(xyws_reasm_conn, reserved); w < sizeof(xyws_reasm_conn) / 8; w++) ((g_u64*)p)[w] = 0;
}

// (state_word: the word of status as loaded)
struct msg_carry_row { uint64_t length, nframes, first_frame, frame_remaining, frames_seen, state_word; msg_state state; };
XYWS_DEV msg_carry_row load_msg_carry(const xyws_msg_carry* p) {
  const size_t k = XYWS_WORD(xyws_msg_carry, status);
  const uint64_t w = load_word<true>(p, k);
  return {XYWS_LD(true, xyws_msg_carry, p, length),      XYWS_LD(true, xyws_msg_carry, p, nframes),
          XYWS_LD(true, xyws_msg_carry, p, first_frame), XYWS_LD(true, xyws_msg_carry, p, frame_remaining),
          XYWS_LD(true, xyws_msg_carry, p, frames_seen), w, unpack_msg_state(w, load_word<true>(p, k + 1))};
}
// Status bits set in the word of status as loaded; nothing else is written.
XYWS_DEV void raise_msg_status(xyws_msg_carry* p, uint64_t state_word, uint32_t bits) {
  XYWS_ST(xyws_msg_carry, p, status, state_word | XYWS_PUT(xyws_msg_carry, status, bits));
}
// The whole carry, the reserved bytes zero.
XYWS_DEV void store_msg_carry(xyws_msg_carry* p, uint64_t length, uint64_t nframes, uint64_t first_frame,
                              uint64_t frame_remaining, uint64_t frames_seen, msg_state state) {
  const size_t k = XYWS_WORD(xyws_msg_carry, status);
  uint64_t w[2];
  pack_msg_state(state, w);
  XYWS_ST(xyws_msg_carry, p, length, length);
  XYWS_ST(xyws_msg_carry, p, nframes, nframes);
  XYWS_ST(xyws_msg_carry, p, first_frame, first_frame);
  XYWS_ST(xyws_msg_carry, p, frame_remaining, frame_remaining);
  XYWS_ST(xyws_msg_carry, p, frames_seen, frames_seen);
  ((g_u64*)p)[k] = w[0];
  ((g_u64*)p)[k + 1] = w[1];
  for (size_t r = k + 2; r < sizeof(xyws_msg_carry) / 8; r++) ((g_u64*)p)[r] = 0;
}

// (reserved: the view of xyws_hold_streams hands the input's word on)
struct reasm_result_row { uint64_t out_len, nmsgs; reasm_counts counts; uint64_t reserved; };
template <bool U>
XYWS_DEV reasm_result_row load_reasm_result(const xyws_reasm_result* p) {
  return {XYWS_LD(U, xyws_reasm_result, p, out_len), XYWS_LD(U, xyws_reasm_result, p, nmsgs),
          unpack_reasm_counts(XYWS_LD(U, xyws_reasm_result, p, completed)), XYWS_LD(U, xyws_reasm_result, p, reserved)};
}
XYWS_DEV void store_reasm_result(xyws_reasm_result* p, const reasm_result_row& r) {
  XYWS_ST(xyws_reasm_result, p, out_len, r.out_len);
  XYWS_ST(xyws_reasm_result, p, nmsgs, r.nmsgs);
  XYWS_ST(xyws_reasm_result, p, completed, pack_reasm_counts(r.counts));
  XYWS_ST(xyws_reasm_result, p, reserved, r.reserved);
}

// (meta: the word of status and opcode as it is, pack_message_meta's; a copied record keeps it whole)
struct message_row { uint64_t first_frame, nframes, out_off, length, meta; };
template <bool U>
XYWS_DEV message_row load_message(const xyws_message* p) {
  return {XYWS_LD(U, xyws_message, p, first_frame), XYWS_LD(U, xyws_message, p, nframes),
          XYWS_LD(U, xyws_message, p, out_off), XYWS_LD(U, xyws_message, p, length), XYWS_LD(U, xyws_message, p, status)};
}
XYWS_DEV void store_message(xyws_message* p, const message_row& m) {
  XYWS_ST(xyws_message, p, first_frame, m.first_frame);
  XYWS_ST(xyws_message, p, nframes, m.nframes);
  XYWS_ST(xyws_message, p, out_off, m.out_off);
  XYWS_ST(xyws_message, p, length, m.length);
  XYWS_ST(xyws_message, p, status, m.meta);
}

// ---- xyws_hold_conn, xyws_hold_carry (wave-uniform), xyws_hold_result
struct hold_conn_row { uint64_t hold_cap, hc, vmsgs, vmsg_cap; };  // (vmsg_cap counts as 0 without vmsgs)
XYWS_DEV hold_conn_row load_hold_conn(const xyws_hold_conn* p) {
  hold_conn_row r;
  r.hold_cap = XYWS_LD(true, xyws_hold_conn, p, hold_cap);
  r.hc = XYWS_LD(true, xyws_hold_conn, p, hc);
  r.vmsgs = XYWS_LD(true, xyws_hold_conn, p, vmsgs);
  r.vmsg_cap = r.vmsgs ? XYWS_LD(true, xyws_hold_conn, p, vmsg_cap) : 0;
  return r;
}

struct hold_carry_row { uint64_t start, held, nframes; hold_state state; };
XYWS_DEV hold_carry_row load_hold_carry(const xyws_hold_carry* p) {
  return {XYWS_LD(true, xyws_hold_carry, p, start), XYWS_LD(true, xyws_hold_carry, p, held),
          XYWS_LD(true, xyws_hold_carry, p, nframes), unpack_hold_state(XYWS_LD(true, xyws_hold_carry, p, status))};
}
XYWS_DEV void store_hold_carry(xyws_hold_carry* p, const hold_carry_row& c) {
  XYWS_ST(xyws_hold_carry, p, start, c.start);
  XYWS_ST(xyws_hold_carry, p, held, c.held);
  XYWS_ST(xyws_hold_carry, p, nframes, c.nframes);
  XYWS_ST(xyws_hold_carry, p, status, pack_hold_state(c.state));
}
XYWS_DEV void store_hold_result(xyws_hold_result* p, uint64_t held, uint64_t delivered_len, uint32_t status) {
  XYWS_ST(xyws_hold_result, p, held, held);
  XYWS_ST(xyws_hold_result, p, delivered_len, delivered_len);
  XYWS_ST(xyws_hold_result, p, status, status);
  XYWS_ST(xyws_hold_result, p, reserved, 0);
}
// The row {0, 0, status}, one word per lane.
XYWS_DEV void store_hold_status(xyws_hold_result* p, uint32_t status, uint32_t lane) {
  if (lane < sizeof(xyws_hold_result) / 8) ((g_u64*)p)[lane] = lane == XYWS_WORD(xyws_hold_result, status) ? (uint64_t)status : 0;
}

// ---- xyws_room, xyws_room_result (wave-uniform), xyws_bcast_conn, xyws_bcast_result
// (n_members counts as 0 without members, wire_cap without wire: then neither is loaded)
struct room_row { uint64_t members, n_members, wire, wire_cap; };
XYWS_DEV room_row load_room(const xyws_room* p) {
  room_row r;
  r.members = XYWS_LD(true, xyws_room, p, members);
  r.n_members = r.members ? XYWS_LD(true, xyws_room, p, n_members) : 0;
  r.wire = XYWS_LD(true, xyws_room, p, wire);
  r.wire_cap = r.wire ? XYWS_LD(true, xyws_room, p, wire_cap) : 0;
  return r;
}
struct room_result_row { uint64_t wire_len; uint32_t nmsgs, status; };
XYWS_DEV room_result_row load_room_result(const xyws_room_result* p) {
  return {XYWS_LD(true, xyws_room_result, p, wire_len), unpack_room_counts(XYWS_LD(true, xyws_room_result, p, nmsgs)).nmsgs,
          unpack_room_state(XYWS_LD(true, xyws_room_result, p, receivers)).status};
}
// (counts: pack_room_counts' word, which the wire build sums as one)
XYWS_DEV void store_room_result(xyws_room_result* p, uint64_t wire_len, uint64_t counts, room_state s) {
  XYWS_ST(xyws_room_result, p, wire_len, wire_len);
  XYWS_ST(xyws_room_result, p, nmsgs, counts);
  XYWS_ST(xyws_room_result, p, receivers, pack_room_state(s));
  XYWS_ST(xyws_room_result, p, reserved, 0);
}

// (head_len counts as 0 without head, out_cap without out: then neither is loaded)
struct bcast_conn_row { uint64_t head, head_len, out, out_cap, reply, room; };
template <bool U>
XYWS_DEV bcast_conn_row load_bcast_conn(const xyws_bcast_conn* p) {
  bcast_conn_row r;
  r.head = XYWS_LD(U, xyws_bcast_conn, p, head);
  r.head_len = r.head ? XYWS_LD(U, xyws_bcast_conn, p, head_len) : 0;
  r.out = XYWS_LD(U, xyws_bcast_conn, p, out);
  r.out_cap = r.out ? XYWS_LD(U, xyws_bcast_conn, p, out_cap) : 0;
  r.reply = XYWS_LD(U, xyws_bcast_conn, p, reply);
  r.room = XYWS_GET(xyws_bcast_conn, room, XYWS_LD(U, xyws_bcast_conn, p, room));
  return r;
}
struct bcast_result_row { uint64_t send_len; uint32_t status; };
XYWS_DEV bcast_result_row load_bcast_result(const xyws_bcast_result* p) {
  return {XYWS_LD(true, xyws_bcast_result, p, send_len),
          XYWS_GET(xyws_bcast_result, status, XYWS_LD(true, xyws_bcast_result, p, status))};
}
XYWS_DEV void store_bcast_result(xyws_bcast_result* p, uint64_t send_len, uint64_t bcast_len, uint32_t status) {
  XYWS_ST(xyws_bcast_result, p, send_len, send_len);
  XYWS_ST(xyws_bcast_result, p, bcast_len, bcast_len);
  XYWS_ST(xyws_bcast_result, p, status, status);
  XYWS_ST(xyws_bcast_result, p, reserved, 0);
}

// ---- the backlog's rows (wave-uniform)
struct backlog_room_row { uint64_t log, log_cap, bc; uint32_t keep; };
XYWS_DEV backlog_room_row load_backlog_room(const xyws_backlog_room* p) {
  return {XYWS_LD(true, xyws_backlog_room, p, log), XYWS_LD(true, xyws_backlog_room, p, log_cap),
          XYWS_LD(true, xyws_backlog_room, p, bc),
          uniform32(XYWS_GET(xyws_backlog_room, keep, XYWS_LD(false, xyws_backlog_room, p, keep)))};
}
struct backlog_span { uint64_t start, len; };  // of xyws_backlog_carry, what the delivery reads
XYWS_DEV backlog_span load_backlog_span(const xyws_backlog_carry* p) {
  return {XYWS_LD(true, xyws_backlog_carry, p, start), XYWS_LD(true, xyws_backlog_carry, p, len)};
}
XYWS_DEV void store_backlog_room_result(xyws_backlog_room_result* p, uint64_t len, backlog_taken t, backlog_state s) {
  XYWS_ST(xyws_backlog_room_result, p, len, len);
  XYWS_ST(xyws_backlog_room_result, p, count, pack_backlog_taken(t));
  XYWS_ST(xyws_backlog_room_result, p, dropped, pack_backlog_state(s));
  XYWS_ST(xyws_backlog_room_result, p, reserved, 0);
}
struct backlog_conn_row { uint64_t out, out_cap, bcast, reply; backlog_join join; };  // (out_cap: 0 without out)
XYWS_DEV backlog_conn_row load_backlog_conn(const xyws_backlog_conn* p) {
  backlog_conn_row r;
  r.out = XYWS_LD(true, xyws_backlog_conn, p, out);
  r.out_cap = r.out ? XYWS_LD(true, xyws_backlog_conn, p, out_cap) : 0;
  r.bcast = XYWS_LD(true, xyws_backlog_conn, p, bcast);
  r.reply = XYWS_LD(true, xyws_backlog_conn, p, reply);
  r.join = unpack_backlog_join(XYWS_LD(true, xyws_backlog_conn, p, room));
  return r;
}
XYWS_DEV void store_backlog_result(xyws_backlog_result* p, uint64_t send_len, uint64_t backlog_len, uint32_t status) {
  XYWS_ST(xyws_backlog_result, p, send_len, send_len);
  XYWS_ST(xyws_backlog_result, p, backlog_len, backlog_len);
  XYWS_ST(xyws_backlog_result, p, status, status);
  XYWS_ST(xyws_backlog_result, p, reserved, 0);
}

// ---- the roster's rows, and the words of other rows that xyws_roster_streams rewrites
// (name_len counts as 0 without name, out_cap without out: then neither is loaded)
struct roster_conn_row { uint64_t name, name_len, out, out_cap, bcast, reply, accept; roster_ask ask; };
template <bool U>
XYWS_DEV roster_conn_row load_roster_conn(const xyws_roster_conn* p) {
  roster_conn_row r;
  r.name = XYWS_LD(U, xyws_roster_conn, p, name);
  r.name_len = r.name ? XYWS_LD(U, xyws_roster_conn, p, name_len) : 0;
  r.out = XYWS_LD(U, xyws_roster_conn, p, out);
  r.out_cap = r.out ? XYWS_LD(U, xyws_roster_conn, p, out_cap) : 0;
  r.bcast = XYWS_LD(U, xyws_roster_conn, p, bcast);
  r.reply = XYWS_LD(U, xyws_roster_conn, p, reply);
  r.accept = XYWS_LD(U, xyws_roster_conn, p, accept);
  r.ask = unpack_roster_ask(XYWS_LD(U, xyws_roster_conn, p, room));
  return r;
}
// What the notices take of a connection: its name (each thread's own load).
struct roster_name { uint64_t name, name_len; };
XYWS_DEV roster_name load_roster_name(const xyws_roster_conn* p) {
  return {XYWS_LD(false, xyws_roster_conn, p, name), XYWS_LD(false, xyws_roster_conn, p, name_len)};
}
// (member_cap counts as 0 without the room's members, notes_cap without notes)
struct roster_room_row { uint64_t member_cap, notes, notes_cap, seen; };
XYWS_DEV roster_room_row load_roster_room(const xyws_roster_room* p, bool has_members) {
  roster_room_row r;
  r.member_cap = has_members ? XYWS_LD(true, xyws_roster_room, p, member_cap) : 0;
  r.notes = XYWS_LD(true, xyws_roster_room, p, notes);
  r.notes_cap = r.notes ? XYWS_LD(true, xyws_roster_room, p, notes_cap) : 0;
  r.seen = XYWS_LD(true, xyws_roster_room, p, seen);
  return r;
}
// The member array an xyws_room row names (the roster's `seen` row: only this and the count are touched).
XYWS_DEV uint64_t load_room_members(const xyws_room* p) { return XYWS_LD(true, xyws_room, p, members); }
// A broadcast row as each thread's own load (load_bcast_result takes it wave-uniform).
XYWS_DEV bcast_result_row load_bcast_result_own(const xyws_bcast_result* p) {
  return {XYWS_LD(false, xyws_bcast_result, p, send_len),
          XYWS_GET(xyws_bcast_result, status, XYWS_LD(false, xyws_bcast_result, p, status))};
}
XYWS_DEV uint64_t load_roster_notes_len(const xyws_roster_room_result* p) {
  return XYWS_LD(true, xyws_roster_room_result, p, notes_len);
}
XYWS_DEV void store_roster_room_result(xyws_roster_room_result* p, uint64_t notes_len, uint64_t welcome_off,
                                       roster_counts c, roster_state s) {
  XYWS_ST(xyws_roster_room_result, p, notes_len, notes_len);
  XYWS_ST(xyws_roster_room_result, p, welcome_off, welcome_off);
  XYWS_ST(xyws_roster_room_result, p, joined, pack_roster_counts(c));
  XYWS_ST(xyws_roster_room_result, p, n_members, pack_roster_state(s));
}
struct roster_result_row { uint64_t note_off; roster_place place; };  // what the later launches read of a row
template <bool U>
XYWS_DEV roster_result_row load_roster_result(const xyws_roster_result* p) {
  return {XYWS_LD(U, xyws_roster_result, p, note_off), unpack_roster_place(XYWS_LD(U, xyws_roster_result, p, status))};
}
XYWS_DEV void store_roster_result(xyws_roster_result* p, uint64_t send_len, uint64_t note_len, roster_place pl,
                                  uint64_t note_off) {
  XYWS_ST(xyws_roster_result, p, send_len, send_len);
  XYWS_ST(xyws_roster_result, p, note_len, note_len);
  XYWS_ST(xyws_roster_result, p, status, pack_roster_place(pl));
  XYWS_ST(xyws_roster_result, p, note_off, note_off);
}
// The room pass's part of a row: its place, and for a joiner where its welcome begins.
XYWS_DEV void store_roster_place(xyws_roster_result* p, roster_place pl) {
  XYWS_ST(xyws_roster_result, p, status, pack_roster_place(pl));
}
XYWS_DEV void store_roster_note_off(xyws_roster_result* p, uint64_t note_off) {
  XYWS_ST(xyws_roster_result, p, note_off, note_off);
}
// The delivery's part: the lengths, and the row's place again with the bits it adds.
XYWS_DEV void store_roster_lengths(xyws_roster_result* p, uint64_t send_len, uint64_t note_len, roster_place pl) {
  XYWS_ST(xyws_roster_result, p, send_len, send_len);
  XYWS_ST(xyws_roster_result, p, note_len, note_len);
  XYWS_ST(xyws_roster_result, p, status, pack_roster_place(pl));
}
// xyws_bcast_conn.room alone (each thread's own): the other half of its word stays as found.
XYWS_DEV uint32_t load_bcast_room(const xyws_bcast_conn* p) {
  return XYWS_GET(xyws_bcast_conn, room, XYWS_LD(false, xyws_bcast_conn, p, room));
}
XYWS_DEV void store_bcast_room(xyws_bcast_conn* p, uint32_t room) {
  const uint64_t field = XYWS_PUT(xyws_bcast_conn, room, mask_of(sizeof(((xyws_bcast_conn*)0)->room)));
  XYWS_ST(xyws_bcast_conn, p, room, (XYWS_LD(false, xyws_bcast_conn, p, room) & ~field) | XYWS_PUT(xyws_bcast_conn, room, room));
}
// xyws_room.n_members alone, and the word of xyws_backlog_conn's room and flags.
XYWS_DEV void store_room_count(xyws_room* p, uint64_t n_members) { XYWS_ST(xyws_room, p, n_members, n_members); }
XYWS_DEV void store_backlog_join(xyws_backlog_conn* p, backlog_join j) {
  XYWS_ST(xyws_backlog_conn, p, room, pack_backlog_join(j));
}
// What the roster reads of an accept row: status and resp_len.
struct accept_brief { uint32_t status, resp_len; };
template <bool U>
XYWS_DEV accept_brief load_accept_brief(const xyws_accept_result* p) {
  return {XYWS_GET(xyws_accept_result, status, XYWS_LD(U, xyws_accept_result, p, status)),
          XYWS_GET(xyws_accept_result, resp_len, XYWS_LD(U, xyws_accept_result, p, resp_len))};
}

// ---- xyws_accept_conn (wave-uniform), xyws_accept_result
struct accept_conn_row { uint64_t buf, len, out, out_cap; };
XYWS_DEV accept_conn_row load_accept_conn(const xyws_accept_conn* p) {
  return {XYWS_LD(true, xyws_accept_conn, p, buf), XYWS_LD(true, xyws_accept_conn, p, len),
          XYWS_LD(true, xyws_accept_conn, p, out), XYWS_LD(true, xyws_accept_conn, p, out_cap)};
}
XYWS_DEV void store_accept_result(xyws_accept_result* p, accept_fields a) {
  uint64_t w[4];
  pack_accept(a, w);
#pragma unroll
  for (uint32_t i = 0; i < 4; i++) ((g_u64*)p)[i] = w[i];
}

// ---- xyws_route_conn, xyws_route_result (wave-uniform), and what xyws_route_streams takes of other rows
typedef XYWS_GLOBAL uint32_t g_u32;
XYWS_DEV uint32_t load_route_conn(const xyws_route_conn* p) {
  return XYWS_GET(xyws_route_conn, rconn, XYWS_LD(true, xyws_route_conn, p, rconn));
}
// What the route call reads of an accept row: whether it was accepted, where its request ends and its target lies.
struct accept_target { uint32_t status, consumed, path_off, path_len; };
XYWS_DEV accept_target load_accept_target(const xyws_accept_result* p) {
  const uint64_t c = XYWS_LD(true, xyws_accept_result, p, path_off);
  return {XYWS_GET(xyws_accept_result, status, XYWS_LD(true, xyws_accept_result, p, status)),
          XYWS_GET(xyws_accept_result, consumed, XYWS_LD(true, xyws_accept_result, p, consumed)),
          XYWS_GET(xyws_accept_result, path_off, c), XYWS_GET(xyws_accept_result, path_len, c)};
}
XYWS_DEV void store_route_result(xyws_route_result* p, route_place pl, route_key k, uint32_t key_len) {
  XYWS_ST(xyws_route_result, p, status, pack_route_place(pl));
  XYWS_ST(xyws_route_result, p, route, pack_route_key(k));
  XYWS_ST(xyws_route_result, p, key_len, (uint64_t)key_len);
  ((g_u64*)p)[XYWS_WORD(xyws_route_result, key_len) + 1] = 0;
}
// xyws_roster_conn.room alone, by one 32-bit store: no other byte of the row is written.
XYWS_DEV void store_roster_room(xyws_roster_conn* p, uint32_t room) { ((g_u32*)p)[ROSTER_ROOM_HALF] = room; }

// ---- xyws_outbox_conn, and what xyws_outbox_streams takes of the sweep's result rows
// (out_cap counts as 0 without out: then it is not loaded)
struct outbox_conn_row { uint64_t out, out_cap, backlog, bcast, reply, accept; };
template <bool U>
XYWS_DEV outbox_conn_row load_outbox_conn(const xyws_outbox_conn* p) {
  outbox_conn_row r;
  r.out = XYWS_LD(U, xyws_outbox_conn, p, out);
  r.out_cap = r.out ? XYWS_LD(U, xyws_outbox_conn, p, out_cap) : 0;
  r.backlog = XYWS_LD(U, xyws_outbox_conn, p, backlog);
  r.bcast = XYWS_LD(U, xyws_outbox_conn, p, bcast);
  r.reply = XYWS_LD(U, xyws_outbox_conn, p, reply);
  r.accept = XYWS_LD(U, xyws_outbox_conn, p, accept);
  return r;
}
// The send buffer alone (wave-uniform): what the pack pass reads of a row.
XYWS_DEV uint64_t load_outbox_out(const xyws_outbox_conn* p) { return XYWS_LD(true, xyws_outbox_conn, p, out); }
// A backlog row's send_len (each thread's own load).
XYWS_DEV uint64_t load_backlog_send_len(const xyws_backlog_result* p) {
  return XYWS_LD(false, xyws_backlog_result, p, send_len);
}
// Word w of the entry at p / of the summary at p, one word per thread that calls it.
XYWS_DEV void store_outbox_entry_word(xyws_outbox_entry* p, uint32_t w, uint64_t v) { ((g_u64*)p)[w] = v; }
XYWS_DEV void store_outbox_summary_word(xyws_outbox_summary* p, uint32_t w, uint64_t v) { ((g_u64*)p)[w] = v; }

// ---- the inbox's rows, and the words of other rows that xyws_inbox_streams reads or rewrites
struct inbox_head_row { uint64_t m, pack_len; };
XYWS_DEV inbox_head_row load_inbox_head(const xyws_inbox_head* p) {
  return {XYWS_LD(false, xyws_inbox_head, p, m), XYWS_LD(false, xyws_inbox_head, p, pack_len)};
}
struct inbox_entry_row { inbox_tag tag; uint64_t off, len, at; };  // (each thread's own entry)
XYWS_DEV inbox_entry_row load_inbox_entry(const xyws_inbox_entry* p) {
  return {unpack_inbox_tag(XYWS_LD(false, xyws_inbox_entry, p, conn)), XYWS_LD(false, xyws_inbox_entry, p, off),
          XYWS_LD(false, xyws_inbox_entry, p, len), XYWS_LD(false, xyws_inbox_entry, p, at)};
}
struct inbox_conn_row { uint64_t buf, cap, carry, conn, aconn, aresult; uint32_t flags; };
XYWS_DEV inbox_conn_row load_inbox_conn(const xyws_inbox_conn* p) {
  return {XYWS_LD(false, xyws_inbox_conn, p, buf),   XYWS_LD(false, xyws_inbox_conn, p, cap),
          XYWS_LD(false, xyws_inbox_conn, p, carry), XYWS_LD(false, xyws_inbox_conn, p, conn),
          XYWS_LD(false, xyws_inbox_conn, p, aconn), XYWS_LD(false, xyws_inbox_conn, p, aresult),
          unpack_inbox_flags(XYWS_LD(false, xyws_inbox_conn, p, flags)).flags};
}
// The receive range alone (wave-uniform): what the copy pass reads of a row.
XYWS_DEV uint64_t load_inbox_buf(const xyws_inbox_conn* p) { return XYWS_LD(true, xyws_inbox_conn, p, buf); }
struct inbox_carry_row { uint64_t http_len, bytes_total; inbox_state state; };
XYWS_DEV inbox_carry_row load_inbox_carry(const xyws_inbox_carry* p) {
  return {XYWS_LD(false, xyws_inbox_carry, p, http_len), XYWS_LD(false, xyws_inbox_carry, p, bytes_total),
          unpack_inbox_state(XYWS_LD(false, xyws_inbox_carry, p, state))};
}
// (the carry's reserved word stays the caller's)
XYWS_DEV void store_inbox_carry(xyws_inbox_carry* p, const inbox_carry_row& c) {
  XYWS_ST(xyws_inbox_carry, p, http_len, c.http_len);
  XYWS_ST(xyws_inbox_carry, p, bytes_total, c.bytes_total);
  XYWS_ST(xyws_inbox_carry, p, state, pack_inbox_state(c.state));
}
XYWS_DEV void store_inbox_result(xyws_inbox_result* p, uint64_t len, uint64_t lead, inbox_counts c) {
  XYWS_ST(xyws_inbox_result, p, len, len);
  XYWS_ST(xyws_inbox_result, p, lead, lead);
  XYWS_ST(xyws_inbox_result, p, n_entries, pack_inbox_counts(c));
  XYWS_ST(xyws_inbox_result, p, reserved, 0);
}
XYWS_DEV void store_inbox_summary_word(xyws_inbox_summary* p, uint32_t w, uint64_t v) { ((g_u64*)p)[w] = v; }
// What the inbox reads of an accept row (each thread's own): the verdict and where the request ends.
struct accept_end { uint32_t status, consumed; };
XYWS_DEV accept_end load_accept_end(const xyws_accept_result* p) {
  return {XYWS_GET(xyws_accept_result, status, XYWS_LD(false, xyws_accept_result, p, status)),
          XYWS_GET(xyws_accept_result, consumed, XYWS_LD(false, xyws_accept_result, p, consumed))};
}
// The buf and len words of a decode row and of an accept row: no other word of the row is written.
XYWS_DEV void store_conn_recv(xyws_conn* p, uint64_t buf, uint64_t len) {
  XYWS_ST(xyws_conn, p, buf, buf);
  XYWS_ST(xyws_conn, p, len, len);
}
XYWS_DEV void store_accept_recv(xyws_accept_conn* p, uint64_t buf, uint64_t len) {
  XYWS_ST(xyws_accept_conn, p, buf, buf);
  XYWS_ST(xyws_accept_conn, p, len, len);
}

}  // namespace xyws_rows
#endif  // __HIPCC__

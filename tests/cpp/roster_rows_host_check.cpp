// roster_rows_host_check.cpp — the rows of xyws_roster_streams as the kernels
// pack and unpack them (xynet_amd/csrc/xyws_rows.h, its pure part) held against
// the structs of include/xyws.h: a stand-alone host program built with
// -fsanitize=address,undefined by tests/test_roster_rows_text.py, the
// companion of rows_host_check.cpp for the rows that call adds. For every
// packed word: a struct filled through its named fields equals byte for byte
// the words XYWS_WORD and the pack function produce; unpacking returns every
// field; a field set alone to all-ones changes its own bytes only. The text's
// words hold its strings byte for byte. A roster result row read through
// xyws_bcast_result's fields gives send_len, note_len and status. Prints one
// line per failed check; exits 0 when there is none.
#include <cstdint>
#include <cstdio>
#include <cstring>

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

template <class T>
static void words_of(const T& s, uint64_t* w) { std::memcpy(w, &s, sizeof s); }

// One word of two 32-bit fields a, b of row type T: pack, unpack, all-ones in either.
#define PAIR(T, a, b, PACK, UNPACK, fa, fb)                                                          \
  do {                                                                                               \
    for (int k = 0; k < 3; k++) {                                                                    \
      T s;                                                                                           \
      std::memset(&s, 0, sizeof s);                                                                  \
      s.a = k == 1 ? 0xFFFFFFFFu : 0x11223344u;                                                      \
      s.b = k == 2 ? 0xFFFFFFFFu : 0x55667788u;                                                      \
      uint64_t w[sizeof(T) / 8];                                                                     \
      words_of(s, w);                                                                                \
      expect(XYWS_WORD(T, a) == XYWS_WORD(T, b), #T, #a " and " #b " share a word");                  \
      expect(PACK({(uint32_t)s.a, (uint32_t)s.b}) == w[XYWS_WORD(T, a)], #T, "pack " #a ", " #b);     \
      const auto u = UNPACK(w[XYWS_WORD(T, a)]);                                                     \
      expect(u.fa == s.a && u.fb == s.b, #T, "unpack " #a ", " #b);                                  \
    }                                                                                                \
  } while (0)

int main() {
  PAIR(xyws_roster_conn, room, flags, R::pack_roster_ask, R::unpack_roster_ask, room, flags);
  PAIR(xyws_roster_room_result, joined, left, R::pack_roster_counts, R::unpack_roster_counts, joined, left);
  PAIR(xyws_roster_room_result, n_members, status, R::pack_roster_state, R::unpack_roster_state, n_members, status);
  PAIR(xyws_roster_result, status, room, R::pack_roster_place, R::unpack_roster_place, status, room);

  {  // every other field of the four rows is a whole word of its own
    expect(sizeof(xyws_roster_conn) == 64 && sizeof(xyws_roster_room) == 32 && sizeof(xyws_roster_room_result) == 32 &&
               sizeof(xyws_roster_result) == 32, "roster rows", "sizes");
    xyws_roster_conn c;
    std::memset(&c, 0, sizeof c);
    c.name = (const void*)0x1111111111111111ull;
    c.name_len = 0x2222222222222222ull;
    c.out = (void*)0x3333333333333333ull;
    c.out_cap = 0x4444444444444444ull;
    c.bcast = (const xyws_bcast_result*)0x5555555555555555ull;
    c.reply = (const xyws_reply_result*)0x6666666666666666ull;
    c.accept = (const xyws_accept_result*)0x7777777777777777ull;
    uint64_t w[8];
    words_of(c, w);
    expect(w[XYWS_WORD(xyws_roster_conn, name)] == 0x1111111111111111ull &&
               w[XYWS_WORD(xyws_roster_conn, name_len)] == 0x2222222222222222ull &&
               w[XYWS_WORD(xyws_roster_conn, out)] == 0x3333333333333333ull &&
               w[XYWS_WORD(xyws_roster_conn, out_cap)] == 0x4444444444444444ull &&
               w[XYWS_WORD(xyws_roster_conn, bcast)] == 0x5555555555555555ull &&
               w[XYWS_WORD(xyws_roster_conn, reply)] == 0x6666666666666666ull &&
               w[XYWS_WORD(xyws_roster_conn, accept)] == 0x7777777777777777ull,
           "xyws_roster_conn", "whole-word fields");
    xyws_roster_room r = {0x1111111111111111ull, (void*)0x2222222222222222ull, 0x3333333333333333ull,
                          (xyws_room*)0x4444444444444444ull};
    uint64_t v[4];
    words_of(r, v);
    expect(v[XYWS_WORD(xyws_roster_room, member_cap)] == 0x1111111111111111ull &&
               v[XYWS_WORD(xyws_roster_room, notes)] == 0x2222222222222222ull &&
               v[XYWS_WORD(xyws_roster_room, notes_cap)] == 0x3333333333333333ull &&
               v[XYWS_WORD(xyws_roster_room, seen)] == 0x4444444444444444ull,
           "xyws_roster_room", "whole-word fields");
  }

  {  // a roster row where the backlog reads a broadcast row
    xyws_roster_result s;
    std::memset(&s, 0, sizeof s);
    s.send_len = 0x0102030405060708ull;
    s.note_len = 0x1112131415161718ull;
    s.status = XYWS_RSC_NOT_RECEIVER | XYWS_RSC_LEFT;
    s.room = 0xFFFFFFFFu;
    s.note_off = 0x2122232425262728ull;
    xyws_bcast_result b;
    std::memcpy(&b, &s, sizeof b);
    expect(b.send_len == s.send_len && b.bcast_len == s.note_len && b.status == s.status, "xyws_roster_result",
           "read as xyws_bcast_result");
    expect((b.status & XYWS_BC_NOT_RECEIVER) != 0 && !(b.status & (XYWS_BC_TRUNCATED | XYWS_BC_NO_ROOM)),
           "xyws_roster_result", "the broadcast's bits");
    expect(XYWS_RSC_TRUNCATED == XYWS_BC_TRUNCATED && XYWS_RSC_NOT_RECEIVER == XYWS_BC_NOT_RECEIVER &&
               XYWS_RSC_NO_ROOM == XYWS_BC_NO_ROOM, "xyws_roster_result", "bit values");
  }

  {  // the text as words
    xyws_roster_text t;
    std::memset(&t, 0, sizeof t);
    for (unsigned i = 0; i < XYWS_ROSTER_TEXT_MAX; i++) {
      t.head[i] = (uint8_t)(0x10 + i);
      t.joined[i] = (uint8_t)(0x40 + i);
      t.left[i] = (uint8_t)(0x80 + i);
    }
    t.head_len = 32;
    t.joined_len = 7;
    t.left_len = 0;
    const R::roster_words q = R::pack_roster_text(t);
    uint8_t bytes[3 * XYWS_ROSTER_TEXT_MAX];
    std::memcpy(bytes, q.w, sizeof bytes);  // (little-endian words: byte i of a string is byte i % 8 of word i / 8)
    expect(std::memcmp(bytes, t.head, 32) == 0 && std::memcmp(bytes + 32, t.joined, 32) == 0 &&
               std::memcmp(bytes + 64, t.left, 32) == 0, "xyws_roster_text", "strings as words");
    expect(q.head_len == 32 && q.joined_len == 7 && q.left_len == 0, "xyws_roster_text", "lengths");
    expect(sizeof q.w == 3 * XYWS_ROSTER_TEXT_MAX && R::ROSTER_TEXT_WORDS * 8 == XYWS_ROSTER_TEXT_MAX, "xyws_roster_text",
           "word count");
  }

  std::printf("%d failed\n", failures);
  return failures ? 1 : 0;
}

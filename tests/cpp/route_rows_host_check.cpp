// route_rows_host_check.cpp — the rows of xyws_route_streams as the kernel packs
// and unpacks them (xynet_amd/csrc/xyws_rows.h, its pure part) held against the
// structs of include/xyws.h: a stand-alone host program built with
// -fsanitize=address,undefined by tests/test_route_rows_text.py, the companion
// of roster_rows_host_check.cpp for the rows that call adds. For every packed
// word: a struct filled through its named fields equals byte for byte the word
// XYWS_WORD and the pack function produce; unpacking returns every field; a
// field set alone to all-ones changes its own bytes only. The roster row's room
// is the 32-bit word the kernel stores alone. Prints one line per failed check;
// exits 0 when there is none.
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
  PAIR(xyws_route_result, status, room, R::pack_route_place, R::unpack_route_place, status, room);
  PAIR(xyws_route_result, route, key_off, R::pack_route_key, R::unpack_route_key, route, key_off);

  expect(sizeof(xyws_route) == 24 && sizeof(xyws_route_conn) == 8 && sizeof(xyws_route_result) == 32, "route rows",
         "sizes");
  {  // key_len is the low half of the third word, the reserved fields the rest of the row
    xyws_route_result s;
    std::memset(&s, 0, sizeof s);
    s.key_len = 0xFFFFFFFFu;
    uint64_t w[4];
    words_of(s, w);
    expect(w[XYWS_WORD(xyws_route_result, key_len)] == 0xFFFFFFFFull && w[0] == 0 && w[1] == 0 && w[3] == 0,
           "xyws_route_result", "key_len alone");
    expect(XYWS_WORD(xyws_route_result, key_len) == 2 && XYWS_WORD(xyws_route_result, reserved) == 2,
           "xyws_route_result", "the third word");
  }
  {  // rconn is the low half of its row's only word
    xyws_route_conn c = {0xFFFFFFFFu, 0};
    uint64_t w[1];
    words_of(c, w);
    expect(w[0] == 0xFFFFFFFFull && XYWS_GET(xyws_route_conn, rconn, w[0]) == XYWS_ROUTE_NO_ROW, "xyws_route_conn", "rconn");
  }
  {  // the roster row's room as a 32-bit word: storing it changes bytes 56..59 alone
    xyws_roster_conn c;
    std::memset(&c, 0xA5, sizeof c);
    uint32_t halves[sizeof c / 4];
    std::memcpy(halves, &c, sizeof c);
    halves[R::ROSTER_ROOM_HALF] = 0x01020304u;
    xyws_roster_conn d;
    std::memcpy(&d, halves, sizeof d);
    expect(d.room == 0x01020304u && d.flags == 0xA5A5A5A5u && d.accept == c.accept && d.name == c.name &&
               d.out_cap == c.out_cap, "xyws_roster_conn", "room as a 32-bit word");
    std::memset(&c, 0, sizeof c);
    c.room = 0xFFFFFFFFu;
    std::memcpy(halves, &c, sizeof c);
    unsigned set = 0;
    for (unsigned i = 0; i < sizeof c / 4; i++) set += halves[i] != 0;
    expect(set == 1 && halves[R::ROSTER_ROOM_HALF] == 0xFFFFFFFFu, "xyws_roster_conn", "room alone");
  }

  std::printf("%d failed\n", failures);
  return failures ? 1 : 0;
}

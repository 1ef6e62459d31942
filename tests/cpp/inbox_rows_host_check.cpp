// inbox_rows_host_check.cpp — the rows of xyws_inbox_streams as the kernels
// pack them (xynet_amd/csrc/xyws_rows.h, its pure part) held against the
// structs of include/xyws.h: a stand-alone host program built with
// -fsanitize=address,undefined by tests/test_inbox_rows_text.py, the companion
// of outbox_rows_host_check.cpp for the rows this call adds. For every packed
// word: a struct filled through its named fields equals byte for byte the word
// XYWS_WORD and the pack function produce; unpacking returns every field; a
// field set alone to all-ones changes its own bytes only. A whole summary
// packed as words equals the struct, and the words of the decode and accept
// rows that the call rewrites are buf and len alone. Prints one line per
// failed check; exits 0 when there is none.
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
      for (size_t i = 0; i < sizeof(T) / 8; i++)                                                     \
        expect(i == XYWS_WORD(T, a) || w[i] == 0, #T, #a ", " #b " change their own word only");      \
    }                                                                                                \
  } while (0)

// Field f of row type T is one whole word: set alone to all-ones, it is that word and no other.
#define WHOLE(T, f)                                                                                  \
  do {                                                                                               \
    T s;                                                                                             \
    std::memset(&s, 0, sizeof s);                                                                    \
    std::memset(&s.f, 0xFF, sizeof s.f);                                                             \
    uint64_t w[sizeof(T) / 8];                                                                       \
    words_of(s, w);                                                                                  \
    unsigned set = 0;                                                                                \
    for (size_t i = 0; i < sizeof(T) / 8; i++) set += w[i] != 0;                                     \
    expect(sizeof s.f == 8 && set == 1 && w[XYWS_WORD(T, f)] == ~0ull, #T, #f " is one whole word");  \
  } while (0)

int main() {
  PAIR(xyws_inbox_entry, conn, flags, R::pack_inbox_tag, R::unpack_inbox_tag, conn, flags);
  PAIR(xyws_inbox_carry, state, status, R::pack_inbox_state, R::unpack_inbox_state, state, status);
  PAIR(xyws_inbox_conn, flags, reserved0, R::pack_inbox_flags, R::unpack_inbox_flags, flags, reserved0);
  PAIR(xyws_inbox_result, n_entries, status, R::pack_inbox_counts, R::unpack_inbox_counts, n_entries, status);
  PAIR(xyws_inbox_summary, n_conns, n_opened, R::pack_inbox_conns, R::unpack_inbox_conns, n_conns, n_opened);
  PAIR(xyws_inbox_summary, n_eof, n_broken, R::pack_inbox_ends, R::unpack_inbox_ends, n_eof, n_broken);
  PAIR(xyws_inbox_summary, n_bad_entries, status, R::pack_inbox_bad, R::unpack_inbox_bad, n_bad_entries, status);

  expect(sizeof(xyws_inbox_head) == 32 && sizeof(xyws_inbox_entry) == 32 && sizeof(xyws_inbox_carry) == 32 &&
             sizeof(xyws_inbox_conn) == 64 && sizeof(xyws_inbox_result) == 32 && sizeof(xyws_inbox_summary) == 64,
         "inbox rows", "sizes");
  expect(R::IBS_WORDS == 8, "inbox rows", "word counts");

  WHOLE(xyws_inbox_head, m);
  WHOLE(xyws_inbox_head, pack_len);
  WHOLE(xyws_inbox_entry, off);
  WHOLE(xyws_inbox_entry, len);
  WHOLE(xyws_inbox_entry, at);
  WHOLE(xyws_inbox_carry, http_len);
  WHOLE(xyws_inbox_carry, bytes_total);
  WHOLE(xyws_inbox_carry, reserved);
  WHOLE(xyws_inbox_conn, buf);
  WHOLE(xyws_inbox_conn, cap);
  WHOLE(xyws_inbox_conn, carry);
  WHOLE(xyws_inbox_conn, conn);
  WHOLE(xyws_inbox_conn, aconn);
  WHOLE(xyws_inbox_conn, aresult);
  WHOLE(xyws_inbox_result, len);
  WHOLE(xyws_inbox_result, lead);
  WHOLE(xyws_inbox_result, reserved);
  // the words of other rows that the call rewrites: buf and len, each a whole word of its row
  WHOLE(xyws_conn, buf);
  WHOLE(xyws_conn, len);
  WHOLE(xyws_accept_conn, buf);
  WHOLE(xyws_accept_conn, len);
  expect(XYWS_WORD(xyws_conn, buf) != XYWS_WORD(xyws_conn, carry) && XYWS_WORD(xyws_conn, len) != XYWS_WORD(xyws_conn, carry) &&
             XYWS_WORD(xyws_accept_conn, len) != XYWS_WORD(xyws_accept_conn, out),
         "xyws_conn, xyws_accept_conn", "buf and len share no word with a field that stays the caller's");
  {  // what the call reads of an accept row: status and consumed come back from a packed row
    uint64_t w[4];
    R::pack_accept({XYWS_ACC_ACCEPTED, 101, 0, 0x01020304u, 129, 4, 5, 77}, w);
    xyws_accept_result r;
    std::memcpy(&r, w, sizeof r);
    expect(r.status == XYWS_ACC_ACCEPTED && r.consumed == 0x01020304u, "xyws_accept_result", "status and consumed");
  }
  {  // a whole summary, the reserved words zero
    xyws_inbox_summary s;
    std::memset(&s, 0, sizeof s);
    s.n_entries = 0x0101010101010101ull;
    s.bytes = 0x0202020202020202ull;
    s.n_conns = 0x03030303u;
    s.n_opened = 0x04040404u;
    s.n_eof = 0x05050505u;
    s.n_broken = 0x06060606u;
    s.n_bad_entries = 0xFFFFFFFFu;
    s.status = XYWS_IBM_BAD_ENTRIES | XYWS_IBM_BROKEN | XYWS_IBM_CLIPPED;
    uint64_t w[R::IBS_WORDS], p[R::IBS_WORDS];
    words_of(s, w);
    std::memset(p, 0xA5, sizeof p);
    R::pack_inbox_summary({s.n_entries, s.bytes, {s.n_conns, s.n_opened}, {s.n_eof, s.n_broken},
                           {s.n_bad_entries, s.status}}, p);
    expect(std::memcmp(w, p, sizeof w) == 0, "xyws_inbox_summary", "a whole summary as words");
  }

  std::printf("%d failed\n", failures);
  return failures ? 1 : 0;
}

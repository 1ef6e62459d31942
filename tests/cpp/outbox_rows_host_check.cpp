// outbox_rows_host_check.cpp — the rows of xyws_outbox_streams as the kernels
// pack them (xynet_amd/csrc/xyws_rows.h, its pure part) held against the
// structs of include/xyws.h: a stand-alone host program built with
// -fsanitize=address,undefined by tests/test_outbox_rows_text.py, the companion
// of route_rows_host_check.cpp for the rows this call adds. For every packed
// word: a struct filled through its named fields equals byte for byte the word
// XYWS_WORD and the pack function produce; unpacking returns every field; a
// field set alone to all-ones changes its own bytes only. A whole entry and a
// whole summary packed as words equal the structs. Prints one line per failed
// check; exits 0 when there is none.
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

int main() {
  PAIR(xyws_outbox_entry, conn, flags, R::pack_outbox_tag, R::unpack_outbox_tag, conn, flags);
  PAIR(xyws_outbox_summary, n_close, n_truncated, R::pack_outbox_counts, R::unpack_outbox_counts, n_close, n_truncated);
  PAIR(xyws_outbox_summary, n_deferred, status, R::pack_outbox_state, R::unpack_outbox_state, n_deferred, status);

  expect(sizeof(xyws_outbox_conn) == 64 && sizeof(xyws_outbox_entry) == 32 && sizeof(xyws_outbox_summary) == 64,
         "outbox rows", "sizes");
  expect(R::OBE_WORDS == 4 && R::OBS_WORDS == 8, "outbox rows", "word counts");
  {  // the conn row: six whole words in the header's order, then the reserved ones
    expect(XYWS_WORD(xyws_outbox_conn, out) == 0 && XYWS_WORD(xyws_outbox_conn, out_cap) == 1 &&
               XYWS_WORD(xyws_outbox_conn, backlog) == 2 && XYWS_WORD(xyws_outbox_conn, bcast) == 3 &&
               XYWS_WORD(xyws_outbox_conn, reply) == 4 && XYWS_WORD(xyws_outbox_conn, accept) == 5 &&
               XYWS_WORD(xyws_outbox_conn, reserved) == 6,
           "xyws_outbox_conn", "word order");
    xyws_outbox_conn c;
    std::memset(&c, 0, sizeof c);
    c.out_cap = ~0ull;
    uint64_t w[8];
    words_of(c, w);
    unsigned set = 0;
    for (unsigned i = 0; i < 8; i++) set += w[i] != 0;
    expect(set == 1 && w[XYWS_WORD(xyws_outbox_conn, out_cap)] == ~0ull, "xyws_outbox_conn", "out_cap alone");
  }
  {  // a whole entry
    xyws_outbox_entry e = {0x01020304u, XYWS_OB_CLOSE | XYWS_OB_DEFERRED, 0x1111111111111110ull, 0x2222222222222222ull,
                           0x3333333333333333ull};
    uint64_t w[R::OBE_WORDS], p[R::OBE_WORDS];
    words_of(e, w);
    R::pack_outbox_entry({{e.conn, e.flags}, e.off, e.len, e.full_len}, p);
    expect(std::memcmp(w, p, sizeof w) == 0, "xyws_outbox_entry", "a whole entry as words");
  }
  {  // a whole summary, the reserved words zero
    xyws_outbox_summary s;
    std::memset(&s, 0, sizeof s);
    s.n_entries = 0x0101010101010101ull;
    s.pack_len = 0x0202020202020200ull;
    s.packed_len = 0x0303030303030300ull;
    s.send_bytes = 0x0404040404040404ull;
    s.n_close = 0x05050505u;
    s.n_truncated = 0x06060606u;
    s.n_deferred = 0xFFFFFFFFu;
    s.status = XYWS_OBS_DEFERRED | XYWS_OBS_TRUNCATED;
    uint64_t w[R::OBS_WORDS], p[R::OBS_WORDS];
    words_of(s, w);
    std::memset(p, 0xA5, sizeof p);
    R::pack_outbox_summary({s.n_entries, s.pack_len, s.packed_len, s.send_bytes, {s.n_close, s.n_truncated},
                            {s.n_deferred, s.status}}, p);
    expect(std::memcmp(w, p, sizeof w) == 0, "xyws_outbox_summary", "a whole summary as words");
  }
  // the rows the length chain reads: send_len lies in a backlog row, a bcast row and a roster row alike
  expect(XYWS_WORD(xyws_backlog_result, send_len) == XYWS_WORD(xyws_bcast_result, send_len) &&
             XYWS_WORD(xyws_bcast_result, send_len) == XYWS_WORD(xyws_roster_result, send_len),
         "send_len", "the same word in the three rows");

  std::printf("%d failed\n", failures);
  return failures ? 1 : 0;
}

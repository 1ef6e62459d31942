// xyws_route.h — internal: the route table and its lookup, stated once for the
// host and the device (include/xyws.h states the semantics): the blob's layout,
// the hash, the key of a request target, which prefixes of it are candidates,
// the probe and the verdict. xyws_route_streams' kernel (xyws_route.hip) runs
// the candidates of one target on the lanes of a wave; xyws_route_lookup is
// lookup() below, one candidate after the other over host memory, and
// xyws_route_build is build(). The header needs nothing of HIP: a plain C++
// compiler takes it as it is (tests/cpp/route_host_check.cpp).
//
// The blob, little-endian 32-bit words, nothing in it a pointer:
//   header (HEADER_BYTES): magic, version, slots (a power of two), n_routes,
//     keys_off, keys_len, total (the blob's size), 0;
//   slots x SLOT_BYTES: hash, key_off (from the blob's start), key_len,
//     flags (SLOT_USED | XYWS_ROUTE_PREFIX), room, route (the index given to
//     build); open addressing, linear probing from home(hash), and since
//     slots > n_routes a chain always ends at an unused slot;
//   the keys in normal form, one after the other.
// The hash of a key is the polynomial sum((c_i + 1) * B^(n-1-i)) mod 2^32: the
// hash of a string and of its extension compose (hash_step), and so do the
// hashes of two halves (hash_join), which is what lets a wave take the hashes
// of all prefixes of a target from one scan.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "xyws.h"

#if defined(__HIPCC__)
#define XYWS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define XYWS_HD inline
#endif

namespace xyws_routing {

constexpr uint32_t MAGIC = 0x54525958u;  // "XYRT"
constexpr uint32_t VERSION = 1;
constexpr uint32_t HEADER_BYTES = 32, SLOT_BYTES = 24;
constexpr uint32_t H_MAGIC = 0, H_VERSION = 4, H_SLOTS = 8, H_ROUTES = 12, H_KEYS_OFF = 16, H_KEYS_LEN = 20, H_TOTAL = 24;
constexpr uint32_t S_HASH = 0, S_KEY_OFF = 4, S_KEY_LEN = 8, S_FLAGS = 12, S_ROOM = 16, S_ROUTE = 20;
constexpr uint32_t SLOT_USED = 0x80000000u;
constexpr uint32_t HASH_B = 0x01000193u;
constexpr uint32_t WINDOW = XYWS_ROUTE_KEY_MAX + 1;  // the bytes of a target that are looked at
constexpr uint32_t NO_ROUTE = 0xFFFFFFFFu;
constexpr uint32_t POLICY_BITS = XYWS_RT_MISS_404;
constexpr uint32_t RESP_404_LEN = 64;

// B^n mod 2^32.
constexpr uint32_t hash_pow(uint32_t n) {
  uint32_t p = 1, b = HASH_B;
  for (; n; n >>= 1, b *= b)
    if (n & 1) p *= b;
  return p;
}
// The hash of s + c from the hash of s; of s + t from theirs, t of n bytes (pow_n = B^n).
XYWS_HD uint32_t hash_step(uint32_t h, uint32_t c) { return h * HASH_B + c + 1u; }
XYWS_HD uint32_t hash_join(uint32_t hs, uint32_t ht, uint32_t pow_n) { return hs * pow_n + ht; }
// Where a chain begins (the hash's high bits decide: the low ones depend on the last bytes only).
XYWS_HD uint32_t home(uint32_t h, uint32_t slots) { return (uint32_t)(((uint64_t)(h * 0x9E3779B1u) * slots) >> 32); }

XYWS_HD uint32_t rd32(const uint8_t* t, uint64_t off) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *reinterpret_cast<const uint32_t*>(t + off);  // (open() has checked the alignment)
#else
  uint32_t v;
  memcpy(&v, t + off, 4);
  return v;
#endif
}

// Target bytes: p[i] for i below the length given with it only.
struct host_bytes {
  const uint8_t* p;
  XYWS_HD uint8_t operator[](uint32_t i) const { return p[i]; }
};

// ---------------------------------------------------------------- the table
struct table {
  const uint8_t* t;
  uint64_t len;
  uint32_t slots;  // 0: nothing to probe
  bool bad;        // bytes were given and are no table
};
XYWS_HD table open(const void* blob, uint64_t len) {
  table tb = {(const uint8_t*)blob, len, 0, false};
  if (!len) return tb;
  tb.bad = true;
  if (len < HEADER_BYTES || ((uintptr_t)blob & 3u)) return tb;
  if (rd32(tb.t, H_MAGIC) != MAGIC || rd32(tb.t, H_VERSION) != VERSION || rd32(tb.t, H_TOTAL) != len) return tb;
  const uint32_t slots = rd32(tb.t, H_SLOTS);
  if (!slots || (slots & (slots - 1)) || HEADER_BYTES + (uint64_t)SLOT_BYTES * slots > len) return tb;
  tb.slots = slots;
  tb.bad = false;
  return tb;
}

// The route whose key is p[0, j) and hashes to h: exact, or one with
// XYWS_ROUTE_PREFIX. Every slot lies inside the blob (open), every key range is
// checked before its bytes are read, and the walk ends after `slots` steps.
template <class R>
XYWS_HD bool probe(const table& tb, uint32_t h, const R& p, uint32_t j, bool exact, uint32_t& room, uint32_t& route) {
  uint32_t i = home(h, tb.slots);
  for (uint32_t n = 0; n < tb.slots; n++, i = (i + 1) & (tb.slots - 1)) {
    const uint64_t s = HEADER_BYTES + (uint64_t)SLOT_BYTES * i;
    const uint32_t fl = rd32(tb.t, s + S_FLAGS);
    if (!(fl & SLOT_USED)) return false;
    if (rd32(tb.t, s + S_HASH) != h || rd32(tb.t, s + S_KEY_LEN) != j) continue;
    const uint64_t ko = rd32(tb.t, s + S_KEY_OFF);
    if (ko + j > tb.len) continue;  // (a damaged blob)
    bool same = true;
    for (uint32_t k = 0; k < j && same; k++) same = tb.t[ko + k] == p[k];
    if (!same) continue;
    if (!exact && !(fl & XYWS_ROUTE_PREFIX)) return false;  // (the key is in the table once)
    room = rd32(tb.t, s + S_ROOM);
    route = rd32(tb.t, s + S_ROUTE);
    return true;
  }
  return false;
}

// ---------------------------------------------------------------- the key of a target, its candidates
XYWS_HD bool ends_key(uint32_t c) { return c == '?' || c == '#'; }
// The length of the key P of a target of `len` bytes whose first `?` or `#`
// within its first min(len, WINDOW) bytes is at `cut` (none: cut >= that
// window), before a trailing `/` is dropped; and whether one may be: then byte
// plen0 - 1 lies in the window and is looked at.
XYWS_HD uint32_t key_len_before_slash(uint32_t len, uint32_t cut) {
  const uint32_t w = len < WINDOW ? len : WINDOW;
  return cut < w ? cut : len;
}
XYWS_HD bool slash_may_drop(uint32_t plen0, uint32_t len) {
  return plen0 > 1 && plen0 <= (len < WINDOW ? len : WINDOW);
}
// p[0, j) is a candidate of the key of plen bytes: P itself, or a prefix in
// front of a `/` (next = p[j], first = p[0]); exact: only a route without
// XYWS_ROUTE_PREFIX's extension is asked for.
XYWS_HD bool is_candidate(uint32_t j, uint32_t plen, uint32_t next, uint32_t first, bool& exact) {
  exact = j == plen;
  if (j == 0 || j > plen || j > XYWS_ROUTE_KEY_MAX) return false;
  return exact || next == '/' || (j == 1 && first == '/');
}

// What the lookup found, before the caller's policy: best = the length of the
// longest matching key, 0 for none.
struct found {
  uint32_t best, room, route, key_len;
};
XYWS_HD uint32_t match_status(const table& tb, const found& f) {
  return (f.best ? XYWS_RT_MATCHED | (f.best < f.key_len ? XYWS_RT_BY_PREFIX : 0u) : XYWS_RT_MISS) |
         (tb.bad ? XYWS_RT_BAD_TABLE : 0u);
}

// The lookup of the target p[0, len), one candidate after the other.
template <class R>
XYWS_HD found lookup(const table& tb, const R& p, uint32_t len) {
  const uint32_t w = len < WINDOW ? len : WINDOW;
  uint32_t cut = 0;
  while (cut < w && !ends_key(p[cut])) cut++;
  uint32_t plen = key_len_before_slash(len, cut);
  if (slash_may_drop(plen, len) && p[plen - 1] == '/') plen--;
  found f = {0, XYWS_ROOM_NONE, NO_ROUTE, plen};
  if (!tb.slots) return f;
  const uint32_t e = plen < XYWS_ROUTE_KEY_MAX ? plen : XYWS_ROUTE_KEY_MAX;
  uint32_t h = 0;
  for (uint32_t j = 1; j <= e; j++) {
    h = hash_step(h, p[j - 1]);
    bool exact;
    if (!is_candidate(j, plen, j < plen ? p[j] : 0u, p[0], exact)) continue;
    uint32_t room, route;
    if (probe(tb, h, p, j, exact, room, route)) f = {j, room, route, plen};
  }
  return f;
}

// A miss's room and status bits under the caller's policy.
XYWS_HD bool args_ok(uint32_t policy) { return !(policy & ~POLICY_BITS); }
XYWS_HD void settle_miss(uint32_t default_room, uint32_t policy, uint32_t& status, uint32_t& room) {
  if (policy & XYWS_RT_MISS_404) {
    status |= XYWS_RT_NOT_FOUND;
    room = XYWS_ROOM_NONE;
  } else {
    room = default_room;
  }
}
// Byte i of the 404.
XYWS_HD uint8_t resp_404(uint32_t i) {
  return (uint8_t)"HTTP/1.1 404 Not Found\r\nConnection: close\r\nContent-Length: 0\r\n\r\n"[i];
}

// xyws_route_lookup (include/xyws.h).
inline int lookup_target(const void* host_table, uint64_t table_len, const void* target, uint64_t len,
                         xyws_route_result* res) {
  if (!res || (table_len && !host_table) || (len && !target)) return XYWS_ERR_INVALID;
  const table tb = open(host_table, table_len);
  const found f = lookup(tb, host_bytes{(const uint8_t*)target}, len < 0xFFFFFFFFull ? (uint32_t)len : 0xFFFFFFFFu);
  *res = xyws_route_result{match_status(tb, f), f.room, f.route, 0, f.key_len, {0, 0, 0}};
  return XYWS_OK;
}

// ---------------------------------------------------------------- xyws_route_build (host only)
inline void wr32(uint8_t* t, uint64_t off, uint32_t v) { memcpy(t + off, &v, 4); }

inline int build(const xyws_route* routes, uint32_t n, uint32_t slots, void* host_table, uint64_t cap, uint64_t* need) {
  if (need) *need = 0;
  if ((n && !routes) || n >= (1u << 30)) return XYWS_ERR_INVALID;
  if (slots && ((slots & (slots - 1)) || slots <= n)) return XYWS_ERR_INVALID;
  uint64_t keys_len = 0;
  std::vector<uint32_t> klen(n);
  for (uint32_t r = 0; r < n; r++) {
    const uint8_t* const k = (const uint8_t*)routes[r].key;
    const uint32_t l = routes[r].key_len;
    if (!k || l == 0 || l > XYWS_ROUTE_KEY_MAX || (routes[r].flags & ~XYWS_ROUTE_PREFIX)) return XYWS_ERR_INVALID;
    for (uint32_t i = 0; i < l; i++)
      if (ends_key(k[i])) return XYWS_ERR_INVALID;
    klen[r] = l > 1 && k[l - 1] == '/' ? l - 1 : l;
    keys_len += klen[r];
  }
  if (!slots)
    for (slots = 2; slots < 2ull * n; slots <<= 1) {}
  const uint64_t keys_off = HEADER_BYTES + (uint64_t)SLOT_BYTES * slots, total = keys_off + keys_len;
  if (total > 0xFFFFFFFFull) return XYWS_ERR_INVALID;
  std::vector<uint8_t> blob(total, 0);
  uint8_t* const t = blob.data();
  wr32(t, H_MAGIC, MAGIC);
  wr32(t, H_VERSION, VERSION);
  wr32(t, H_SLOTS, slots);
  wr32(t, H_ROUTES, n);
  wr32(t, H_KEYS_OFF, (uint32_t)keys_off);
  wr32(t, H_KEYS_LEN, (uint32_t)keys_len);
  wr32(t, H_TOTAL, (uint32_t)total);
  uint64_t at = keys_off;
  for (uint32_t r = 0; r < n; r++) {
    const uint8_t* const k = (const uint8_t*)routes[r].key;
    uint32_t h = 0;
    for (uint32_t i = 0; i < klen[r]; i++) h = hash_step(h, k[i]);
    uint32_t i = home(h, slots);
    for (;; i = (i + 1) & (slots - 1)) {  // (slots > n: an unused slot is met)
      const uint64_t s = HEADER_BYTES + (uint64_t)SLOT_BYTES * i;
      if (!(rd32(t, s + S_FLAGS) & SLOT_USED)) break;
      if (rd32(t, s + S_HASH) == h && rd32(t, s + S_KEY_LEN) == klen[r] &&
          !memcmp(t + rd32(t, s + S_KEY_OFF), k, klen[r]))
        return XYWS_ERR_INVALID;  // two keys equal in normal form
    }
    const uint64_t s = HEADER_BYTES + (uint64_t)SLOT_BYTES * i;
    memcpy(t + at, k, klen[r]);
    wr32(t, s + S_HASH, h);
    wr32(t, s + S_KEY_OFF, (uint32_t)at);
    wr32(t, s + S_KEY_LEN, klen[r]);
    wr32(t, s + S_FLAGS, SLOT_USED | routes[r].flags);
    wr32(t, s + S_ROOM, routes[r].room);
    wr32(t, s + S_ROUTE, r);
    at += klen[r];
  }
  if (need) *need = total;
  if (cap < total) return XYWS_ERR_CAPACITY;
  if (!host_table) return XYWS_ERR_INVALID;
  memcpy(host_table, t, total);
  return XYWS_OK;
}

}  // namespace xyws_routing

// xyws_directory.h — internal: the room directory of xyws_open_streams, stated
// once for the host and the device (include/xyws.h states the semantics): the
// blob's layout, how it is opened, the probe over a blob at rest, and the host
// calls xyws_directory_init / _lookup / _get / _stat. The kernels
// (xyws_open.hip) insert into the same slots concurrently; what they add to the
// probe (PENDING slots, the claim) is stated there. The hash, its composition
// and the chain's first slot are xyws_route.h's, and a key is the window a
// route row names, in the normal form the route call already applied. The
// header needs nothing of HIP: a plain C++ compiler takes it as it is
// (tests/cpp/directory_host_check.cpp).
//
// The blob, little-endian 32-bit words, nothing in it a pointer, 16-byte aligned
// on the device (a slot's first two words are one 64-bit compare-and-swap, its
// last four one 16-byte load):
//   header (HEADER_BYTES): magic, version, slots (a power of two), room_base,
//     room_cap, n_open, keys_off, keys_cap, keys_used, dead, total, 0 ..;
//   slots x SLOT_BYTES: state, claimer, first, 0, hash, key_off (from the
//     blob's start), key_len, room; open addressing, linear probing from
//     home(hash); a slot never becomes EMPTY again, so a key sits before the
//     first EMPTY slot of its chain;
//   the key arena of keys_cap bytes: the keys one after the other, the first
//     keys_used bytes in use.
// States: EMPTY (first = UINT32_MAX); PENDING, between the launches of one call
// only: claimed by row `claimer`, whose request bytes are the key, `first` the
// lowest row that names it; USED: hash .. room are valid; DEAD: claimed by a
// key that found no room: walked past, never matched.
// The directory is closed (opens nothing more) once n_open == room_cap,
// keys_used == keys_cap, or a key has been refused (dead != 0): the admitted
// keys of a directory are a prefix of all the keys it was ever asked for.
#pragma once
#include <stdint.h>
#include <string.h>

#include "xyws.h"
#include "xyws_route.h"

namespace xyws_directory {

using xyws_routing::hash_step;
using xyws_routing::home;
using xyws_routing::rd32;

constexpr uint32_t MAGIC = 0x44525958u;  // "XYRD"
constexpr uint32_t VERSION = 1;
constexpr uint32_t HEADER_BYTES = 64, SLOT_BYTES = 32, ALIGN = 16;
constexpr uint32_t H_MAGIC = 0, H_VERSION = 4, H_SLOTS = 8, H_ROOM_BASE = 12, H_ROOM_CAP = 16, H_N_OPEN = 20;
constexpr uint32_t H_KEYS_OFF = 24, H_KEYS_CAP = 28, H_KEYS_USED = 32, H_DEAD = 36, H_TOTAL = 40;
constexpr uint32_t S_STATE = 0, S_CLAIMER = 4, S_FIRST = 8, S_HASH = 16, S_KEY_OFF = 20, S_KEY_LEN = 24, S_ROOM = 28;
constexpr uint32_t EMPTY = 0, PENDING = 1, USED = 2, DEAD = 3;
constexpr uint32_t NO_ROW = 0xFFFFFFFFu;

XYWS_HD uint64_t slot_at(uint32_t i) { return HEADER_BYTES + (uint64_t)SLOT_BYTES * i; }

// ---------------------------------------------------------------- the blob, opened
struct dir {
  const uint8_t* t;
  uint64_t len;
  uint32_t slots;  // 0: the bytes are no directory (bad)
  uint32_t room_base, room_cap, n_open, keys_off, keys_cap, keys_used, dead;
  bool bad;
};
XYWS_HD bool closed(const dir& d) { return d.n_open >= d.room_cap || d.keys_used >= d.keys_cap || d.dead != 0; }
// A call over n rows may claim: every row could name a key of its own, and each must find a slot, or which
// keys find one would be a matter of scheduling. (n_open + dead <= slots: every one of them took a slot.)
XYWS_HD bool may_claim(const dir& d, uint64_t n) {
  return !closed(d) && (uint64_t)d.n_open + d.dead <= d.slots && n <= (uint64_t)d.slots - d.n_open - d.dead;
}

XYWS_HD dir open(const void* blob, uint64_t len) {
  dir d = {(const uint8_t*)blob, len, 0, 0, 0, 0, 0, 0, 0, 0, true};
  if (!blob || len < HEADER_BYTES) return d;
#if defined(__HIP_DEVICE_COMPILE__)
  if ((uintptr_t)blob & (ALIGN - 1)) return d;  // (the host reads bytes: any alignment)
#endif
  if (rd32(d.t, H_MAGIC) != MAGIC || rd32(d.t, H_VERSION) != VERSION || rd32(d.t, H_TOTAL) != len) return d;
  const uint32_t slots = rd32(d.t, H_SLOTS), keys_off = rd32(d.t, H_KEYS_OFF), keys_cap = rd32(d.t, H_KEYS_CAP);
  const uint32_t room_base = rd32(d.t, H_ROOM_BASE), room_cap = rd32(d.t, H_ROOM_CAP);
  if (!slots || (slots & (slots - 1)) || slot_at(slots) != keys_off || (uint64_t)keys_off + keys_cap != len) return d;
  if ((uint64_t)room_base + room_cap > 0xFFFFFFFFull || 2ull * room_cap > slots) return d;
  d.n_open = rd32(d.t, H_N_OPEN);
  d.keys_used = rd32(d.t, H_KEYS_USED);
  d.dead = rd32(d.t, H_DEAD);
  if (d.n_open > room_cap || d.keys_used > keys_cap) return d;
  d.slots = slots;
  d.room_base = room_base;
  d.room_cap = room_cap;
  d.keys_off = keys_off;
  d.keys_cap = keys_cap;
  d.bad = false;
  return d;
}

// A USED slot's key range lies in the arena's used part and its room is one the directory hands out.
XYWS_HD bool slot_ok(const dir& d, uint32_t key_off, uint32_t key_len, uint32_t room) {
  return key_len >= 1 && key_len <= XYWS_ROUTE_KEY_MAX && key_off >= d.keys_off &&
         (uint64_t)key_off + key_len <= (uint64_t)d.keys_off + d.keys_used && room >= d.room_base &&
         room - d.room_base < d.n_open;
}

// The room of the key p[0, n) with hash h in a blob at rest (no PENDING slot is
// matched): every slot lies inside the blob (open), every key range is checked
// before its bytes are read, and the walk ends after `slots` steps.
template <class R>
XYWS_HD bool probe(const dir& d, uint32_t h, const R& p, uint32_t n, uint32_t& room) {
  uint32_t i = home(h, d.slots);
  for (uint32_t step = 0; step < d.slots; step++, i = (i + 1) & (d.slots - 1)) {
    const uint64_t s = slot_at(i);
    const uint32_t state = rd32(d.t, s + S_STATE);
    if (state == EMPTY) return false;
    if (state != USED || rd32(d.t, s + S_HASH) != h || rd32(d.t, s + S_KEY_LEN) != n) continue;
    const uint32_t ko = rd32(d.t, s + S_KEY_OFF), r = rd32(d.t, s + S_ROOM);
    if (!slot_ok(d, ko, n, r)) continue;  // (a damaged blob)
    bool same = true;
    for (uint32_t k = 0; k < n && same; k++) same = d.t[ko + k] == p[k];
    if (!same) continue;
    room = r;
    return true;
  }
  return false;
}

// ---------------------------------------------------------------- the host calls (include/xyws.h)
inline int init(uint32_t slots, uint32_t room_base, uint32_t room_cap, uint32_t keys_cap, void* host_blob, uint64_t cap,
                uint64_t* need) {
  if (need) *need = 0;
  if ((uint64_t)room_base + room_cap > 0xFFFFFFFFull || room_cap >= (1u << 30)) return XYWS_ERR_INVALID;
  if (slots && ((slots & (slots - 1)) || slots < 2ull * room_cap || slots < 2)) return XYWS_ERR_INVALID;
  if (!slots)
    for (slots = 2; slots < 2ull * room_cap; slots <<= 1) {}
  const uint64_t keys_off = slot_at(slots), total = keys_off + keys_cap;
  if (total > 0xFFFFFFFFull) return XYWS_ERR_INVALID;
  if (need) *need = total;
  if (cap < total) return XYWS_ERR_CAPACITY;
  if (!host_blob) return XYWS_ERR_INVALID;
  uint8_t* const t = (uint8_t*)host_blob;
  memset(t, 0, total);
  using xyws_routing::wr32;
  wr32(t, H_MAGIC, MAGIC);
  wr32(t, H_VERSION, VERSION);
  wr32(t, H_SLOTS, slots);
  wr32(t, H_ROOM_BASE, room_base);
  wr32(t, H_ROOM_CAP, room_cap);
  wr32(t, H_KEYS_OFF, (uint32_t)keys_off);
  wr32(t, H_KEYS_CAP, keys_cap);
  wr32(t, H_TOTAL, (uint32_t)total);
  for (uint32_t i = 0; i < slots; i++) wr32(t, slot_at(i) + S_FIRST, NO_ROW);
  return XYWS_OK;
}

inline int lookup(const void* host_blob, uint64_t len, const void* key, uint32_t key_len, uint32_t* room) {
  if (!host_blob || !room || (key_len && !key)) return XYWS_ERR_INVALID;
  const dir d = open(host_blob, len);
  if (d.bad) return XYWS_ERR_INVALID;
  *room = XYWS_ROOM_NONE;
  if (key_len < 1 || key_len > XYWS_ROUTE_KEY_MAX) return XYWS_OK;
  uint32_t h = 0;
  for (uint32_t i = 0; i < key_len; i++) h = hash_step(h, ((const uint8_t*)key)[i]);
  uint32_t r;
  if (probe(d, h, xyws_routing::host_bytes{(const uint8_t*)key}, key_len, r)) *room = r;
  return XYWS_OK;
}

// The first USED slot at or behind slot `from` (a slot whose ranges a damaged blob broke is passed over);
// *next: the slot behind it, from which a listing goes on. One pass over the slots lists a directory.
inline int get(const void* host_blob, uint64_t len, uint32_t from, uint32_t* key_off, uint32_t* key_len, uint32_t* room,
               uint32_t* next) {
  if (!host_blob || !key_off || !key_len || !room) return XYWS_ERR_INVALID;
  const dir d = open(host_blob, len);
  if (d.bad) return XYWS_ERR_INVALID;
  for (uint32_t s = from; s < d.slots; s++) {
    const uint64_t at = slot_at(s);
    if (rd32(d.t, at + S_STATE) != USED) continue;
    const uint32_t ko = rd32(d.t, at + S_KEY_OFF), kl = rd32(d.t, at + S_KEY_LEN), r = rd32(d.t, at + S_ROOM);
    if (!slot_ok(d, ko, kl, r)) continue;
    *key_off = ko;
    *key_len = kl;
    *room = r;
    if (next) *next = s + 1;
    return XYWS_OK;
  }
  return XYWS_ERR_INVALID;
}

inline int stat(const void* host_blob, uint64_t len, xyws_directory_info* info) {
  if (!host_blob || !info) return XYWS_ERR_INVALID;
  const dir d = open(host_blob, len);
  if (d.bad) return XYWS_ERR_INVALID;
  *info = xyws_directory_info{d.slots, d.room_base, d.room_cap, d.n_open, d.keys_cap, d.keys_used, d.dead, 0};
  return XYWS_OK;
}

}  // namespace xyws_directory

// directory_host_check.cpp — the room directory's host side (xynet_amd/csrc/
// xyws_directory.h, shared by the kernels and xyws_directory_lookup) as a
// stand-alone host program, built with -fsanitize=address,undefined by
// tests/test_open_abi.py: init, a directory filled the way the kernels leave it
// (USED slots by linear probing, one DEAD slot), lookup over heap copies of the
// exact sizes, get and stat; then blobs with one damaged slot each, which must not match.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "xyws_directory.h"

namespace D = xyws_directory;
using xyws_routing::wr32;

static unsigned failed = 0;
#define CHECK(c) ((c) ? (void)0 : (void)(failed++, std::printf("line %d: %s\n", __LINE__, #c)))

// What the kernels leave for one admitted (room != XYWS_ROOM_NONE) or refused key.
static void insert(std::vector<uint8_t>& b, const std::string& key, uint32_t room) {
  uint8_t* const t = b.data();
  const uint32_t slots = D::rd32(t, D::H_SLOTS);
  uint32_t h = 0;
  for (unsigned char c : key) h = D::hash_step(h, c);
  uint32_t i = D::home(h, slots);
  while (D::rd32(t, D::slot_at(i) + D::S_STATE) != D::EMPTY) i = (i + 1) & (slots - 1);
  const uint64_t s = D::slot_at(i);
  const uint32_t used = D::rd32(t, D::H_KEYS_USED), at = D::rd32(t, D::H_KEYS_OFF) + used, dead = room == XYWS_ROOM_NONE;
  wr32(t, s + D::S_FIRST, 0);
  wr32(t, s + D::S_HASH, h);
  wr32(t, s + D::S_KEY_LEN, (uint32_t)key.size());
  wr32(t, s + D::S_ROOM, room);
  wr32(t, s + D::S_STATE, dead ? D::DEAD : D::USED);
  wr32(t, D::H_DEAD, D::rd32(t, D::H_DEAD) + dead);
  if (dead) return;
  std::memcpy(t + at, key.data(), key.size());
  wr32(t, s + D::S_KEY_OFF, at);
  wr32(t, D::H_KEYS_USED, used + (uint32_t)key.size());
  wr32(t, D::H_N_OPEN, D::rd32(t, D::H_N_OPEN) + 1);
}

// lookup with the blob and the key in heap buffers of their exact sizes.
static int lookup_exact(const std::vector<uint8_t>& blob, const std::string& key, uint32_t* room) {
  const std::vector<uint8_t> tb(blob.begin(), blob.end()), tk(key.begin(), key.end());
  return D::lookup(tb.data(), tb.size(), tk.data(), (uint32_t)tk.size(), room);
}

int main() {
  uint64_t need = 7;
  CHECK(D::init(7, 10, 2, 0, nullptr, 0, &need) == XYWS_ERR_INVALID && need == 0);
  std::vector<std::string> keys = {"/", "/rooms/a", "/rooms/a/b", "/rooms/b", std::string(256, 'k'), std::string(255, 'k')};
  for (int i = 0; i < 9; i++) keys.push_back("/k/" + std::to_string(i * 7919));
  std::vector<uint8_t> blob(64 + 32 * 32 + 1024, 0xEE);
  CHECK(D::init(32, 10, 16, 1024, blob.data(), blob.size(), &need) == XYWS_OK && need == blob.size());
  uint32_t room = 5, ko, kl;
  CHECK(lookup_exact(blob, "/", &room) == XYWS_OK && room == XYWS_ROOM_NONE);
  CHECK(D::get(blob.data(), blob.size(), 0, &ko, &kl, &room, nullptr) == XYWS_ERR_INVALID);
  for (size_t i = 0; i < keys.size(); i++) insert(blob, keys[i], 10 + (uint32_t)i);
  insert(blob, "/refused", XYWS_ROOM_NONE);

  xyws_directory_info info;
  CHECK(D::stat(blob.data(), blob.size(), &info) == XYWS_OK && info.n_open == keys.size() && info.dead == 1 &&
        info.slots == 32 && info.room_base == 10 && info.room_cap == 16 && info.keys_cap == 1024);
  for (size_t i = 0; i < keys.size(); i++) CHECK(lookup_exact(blob, keys[i], &room) == XYWS_OK && room == 10 + i);
  for (const std::string& absent : {std::string("/refused"), std::string("/rooms"), std::string("/rooms/a/"), std::string(),
                                    std::string(257, 'k')})
    CHECK(lookup_exact(blob, absent, &room) == XYWS_OK && room == XYWS_ROOM_NONE);
  uint32_t at = 0, seen = 0;  // (seen: one bit per room)
  for (uint32_t i = 0; i < keys.size(); i++) {
    CHECK(D::get(blob.data(), blob.size(), at, &ko, &kl, &room, &at) == XYWS_OK && room - 10 < keys.size() &&
          std::string((const char*)blob.data() + ko, kl) == keys[room - 10] && !(seen >> (room - 10) & 1));
    seen |= 1u << ((room - 10) & 31);
  }
  CHECK(D::get(blob.data(), blob.size(), at, &ko, &kl, &room, &at) == XYWS_ERR_INVALID);
  std::vector<uint8_t> bad = blob;  // bytes that are no directory, null arguments
  bad.pop_back();
  CHECK(lookup_exact(bad, "/", &room) == XYWS_ERR_INVALID && D::stat(bad.data(), bad.size(), &info) == XYWS_ERR_INVALID);
  CHECK(D::lookup(nullptr, 64, "/", 1, &room) == XYWS_ERR_INVALID && D::lookup(blob.data(), blob.size(), nullptr, 1, &room) ==
                                                                         XYWS_ERR_INVALID);

  // damaged blobs (the header kept right, so they open): a key range that ends past the arena's used part or past
  // the blob, a length past the key's, a room the directory never gave, a PENDING slot at rest: never matched
  for (uint32_t field : {D::S_KEY_OFF, D::S_KEY_LEN, D::S_ROOM, D::S_STATE})
    for (uint32_t slot = 0; slot < 32; slot++) {
      std::vector<uint8_t> b = blob;
      const uint32_t v = field == D::S_STATE ? D::PENDING : field == D::S_KEY_LEN ? 300u : (uint32_t)b.size() - (slot & 7);
      if (D::rd32(b.data(), D::slot_at(slot) + D::S_STATE) != D::USED) continue;
      const uint32_t was = D::rd32(b.data(), D::slot_at(slot) + D::S_ROOM) - 10;
      wr32(b.data(), D::slot_at(slot) + field, v);
      CHECK(lookup_exact(b, keys[was], &room) == XYWS_OK && room == XYWS_ROOM_NONE);
    }
  std::printf("%u failed\n", failed);
  return failed ? 1 : 0;
}

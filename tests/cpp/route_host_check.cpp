// route_host_check.cpp — the route table and its lookup (xynet_amd/csrc/
// xyws_route.h, the source xyws_route_lookup and the kernel share) as a
// stand-alone host program, built with -fsanitize=address,undefined by
// tests/test_route_host_check.py. The file named on the command line holds
// the routes (u32 count; per route u32 length, the key, u32 room, u32 flags)
// and the targets (u32 count; per target u32 length, the bytes). The table is
// built with the size the library chooses and with the smallest it takes, and
// held in a heap buffer of exactly its size; every target is looked up from a
// heap buffer of exactly its size, so a read past either is caught. One line
// per table and target: the result row. Then every target is looked up in a
// few thousand blobs damaged by seeded byte flips and truncations, each again
// in a buffer of its exact size: a damaged table may misroute, so only the
// clean exit counts there.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "xyws_route.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}

static bool read_u32(std::FILE* f, uint32_t* v) { return std::fread(v, 4, 1, f) == 1; }
static bool read_bytes(std::FILE* f, std::vector<uint8_t>* v, uint32_t n) {
  v->resize(n);
  return !n || std::fread(v->data(), 1, n, f) == n;
}

// The lookup with both ranges in heap buffers of their exact sizes.
static int lookup_exact(const uint8_t* blob, size_t blob_len, const std::vector<uint8_t>& target, xyws_route_result* r) {
  uint8_t* const tb = static_cast<uint8_t*>(std::malloc(blob_len ? blob_len : 1));
  uint8_t* const tg = static_cast<uint8_t*>(std::malloc(target.size() ? target.size() : 1));
  if (blob_len) std::memcpy(tb, blob, blob_len);
  if (!target.empty()) std::memcpy(tg, target.data(), target.size());
  const int rc = xyws_routing::lookup_target(blob_len ? tb : nullptr, blob_len, target.empty() ? nullptr : tg,
                                             target.size(), r);
  std::free(tg);
  std::free(tb);
  return rc;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  const uint32_t damaged = (uint32_t)std::strtoul(argv[2], nullptr, 10);
  uint32_t n_routes, n_targets;
  if (!read_u32(f, &n_routes)) return 2;
  std::vector<std::vector<uint8_t>> keys(n_routes), targets;
  std::vector<xyws_route> routes(n_routes);
  for (uint32_t i = 0; i < n_routes; i++) {
    uint32_t len;
    if (!read_u32(f, &len) || !read_bytes(f, &keys[i], len) || !read_u32(f, &routes[i].room) ||
        !read_u32(f, &routes[i].flags))
      return 2;
    routes[i].key = keys[i].data();
    routes[i].key_len = len;
    routes[i].reserved = 0;
  }
  if (!read_u32(f, &n_targets)) return 2;
  targets.resize(n_targets);
  for (uint32_t i = 0; i < n_targets; i++) {
    uint32_t len;
    if (!read_u32(f, &len) || !read_bytes(f, &targets[i], len)) return 2;
  }
  std::fclose(f);

  uint32_t smallest = 1;
  while (smallest <= n_routes) smallest <<= 1;
  const uint32_t sizes[] = {0, smallest};
  std::vector<std::vector<uint8_t>> blobs;
  for (uint32_t s = 0; s < 2; s++) {
    uint64_t need = 0;
    if (xyws_routing::build(routes.data(), n_routes, sizes[s], nullptr, 0, &need) != XYWS_ERR_CAPACITY || !need) return 3;
    std::vector<uint8_t> blob(need);
    if (xyws_routing::build(routes.data(), n_routes, sizes[s], blob.data(), need, &need) != XYWS_OK) return 3;
    for (uint32_t t = 0; t < n_targets; t++) {
      xyws_route_result r;
      if (lookup_exact(blob.data(), blob.size(), targets[t], &r) != XYWS_OK) return 4;
      std::printf("%u %u %u %u %u %u %u\n", s, t, r.status, r.room, r.route, r.key_off, r.key_len);
    }
    blobs.push_back(blob);
  }

  unsigned matched = 0;
  for (uint32_t d = 0; d < damaged; d++) {
    std::vector<uint8_t> blob = blobs[d & 1];
    const uint32_t kind = rnd() % 4;
    uint32_t n_slots;
    std::memcpy(&n_slots, blob.data() + 8, 4);  // (of the blob as built)
    if (kind == 0) {
      blob.resize(rnd() % blob.size());  // a truncation (the size word no longer fits: no table)
    } else {
      // flips anywhere; kinds 2 and 3 aim at the header's slot count and at the slots, where the offsets are
      const uint32_t flips = 1 + rnd() % 8;
      for (uint32_t k = 0; k < flips; k++) {
        const size_t span = kind == 1 ? blob.size() : kind == 2 ? 32 : 32 + 24 * (size_t)n_slots;
        blob[rnd() % (span < blob.size() ? span : blob.size())] ^= (uint8_t)(1u << (rnd() % 8));
      }
      if (kind == 3 && (rnd() & 1)) {  // a slot whose key range runs past the blob, the size word kept right
        const size_t at = 32 + 24 * (size_t)(rnd() % n_slots) + 4;
        const uint32_t off = (uint32_t)blob.size() - rnd() % 3;
        if (at + 4 <= blob.size()) std::memcpy(blob.data() + at, &off, 4);
      }
    }
    for (uint32_t t = 0; t < n_targets; t++) {
      xyws_route_result r;
      if (lookup_exact(blob.data(), blob.size(), targets[t], &r) != XYWS_OK) return 5;
      matched += (r.status & XYWS_RT_MATCHED) != 0;
    }
  }
  std::printf("damaged %u matched %u\n", damaged, matched);
  return 0;
}

// accept_host_check.cpp — the handshake grammar (xynet_amd/csrc/xyws_accept.h,
// the source xyws_accept_request and the kernel share) as a stand-alone host
// program, built with -fsanitize=address,undefined by
// tests/test_accept_host_check.py: every input of the file named on the
// command line (u32 length + bytes, repeated), at every truncation length,
// under both policies, each time in a heap buffer of exactly that many bytes
// and with a send buffer of exactly out_cap bytes, so a read past len or a
// write past out_cap is caught. Prints, per input and policy, the verdict of
// the whole input and how its truncations were answered.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "xyws_accept.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<std::vector<uint8_t>> inputs;
  for (uint32_t n; std::fread(&n, 4, 1, f) == 1;) {
    std::vector<uint8_t> v(n);
    if (n && std::fread(v.data(), 1, n, f) != n) return 2;
    inputs.push_back(v);
  }
  std::fclose(f);
  const uint64_t caps[] = {0, 25, 26, 128, 129, 130};
  const uint32_t policies[] = {0, XYWS_ACC_REFERENCE};
  for (size_t i = 0; i < inputs.size(); i++) {
    const std::vector<uint8_t>& in = inputs[i];
    for (uint32_t policy : policies) {
      unsigned incomplete = 0, accepted = 0, rejected = 0;
      xyws_accept_result whole{};
      for (size_t k = 0; k <= in.size(); k++) {
        uint8_t* req = static_cast<uint8_t*>(std::malloc(k ? k : 1));
        if (k) std::memcpy(req, in.data(), k);
        for (uint64_t cap : caps) {
          uint8_t* out = static_cast<uint8_t*>(std::malloc(cap ? cap : 1));
          xyws_accept_result r;
          // (max_request: above, at and below the input, so the cut at max_request is walked too)
          const uint32_t mrs[] = {XYWS_ACCEPT_MAX_REQUEST, k ? (uint32_t)k : 1u, k > 1 ? (uint32_t)k - 1 : 1u};
          for (uint32_t mr : mrs) {
            if (mr > XYWS_ACCEPT_MAX_REQUEST) continue;
            if (xyws_accept::accept_request(k ? req : nullptr, k, mr, policy, cap ? out : nullptr, cap, &r) != XYWS_OK)
              return 3;
            if (mr == XYWS_ACCEPT_MAX_REQUEST && cap == 130) {
              if (r.status & XYWS_ACC_ACCEPTED) accepted++;
              else if (r.status & XYWS_ACC_REJECTED) rejected++;
              else incomplete++;
              if (k == in.size()) whole = r;
            }
          }
          std::free(out);
        }
        std::free(req);
      }
      std::printf("%zu %u %u %u %u %u %u %u %u %u\n", i, policy, whole.status, (unsigned)whole.http_status,
                  (unsigned)whole.reason, whole.consumed, whole.resp_len, incomplete, accepted, rejected);
    }
  }
  return 0;
}

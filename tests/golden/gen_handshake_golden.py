#!/usr/bin/env python3
"""What the reference's websocket_request_handler answers to the requests of
tests/accept_cases.py (tests/golden/handshake.json).

CONTAINER-ONLY test infrastructure, like gen_golden.py: it needs the xynet
reference tree (XYNET_REFERENCE, default /root/reference), g++ and libcrypto.
It writes a small driver of its own into a temporary directory, compiles it
against the reference's headers and runs it; nothing of the reference or
compiled from it is kept. The driver feeds each input to a fresh
websocket_request_handler and records parse()'s return and
generate_response()'s bytes. Each input is handed over in a buffer with one
extra non-space byte behind it: the reference reads *buf once past the end
while it skips spaces, and this keeps that read defined.

Every case is recorded whole; the cases in accept_cases.TRUNCATED at every
length 0..len as well ({"of": name, "len": k}).

Re-run with:  python tests/golden/gen_handshake_golden.py
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import accept_cases as AC  # noqa: E402

REFERENCE = os.environ.get("XYNET_REFERENCE", "/root/reference")

DRIVER = r"""
#include <array>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <span>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>
#include "xynet/http/websocket_request_handler.h"

static int hexval(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {  // one input per line, in hex ("-": empty)
    std::vector<char> buf;
    if (line != "-")
      for (size_t i = 0; i + 1 < line.size(); i += 2) buf.push_back((char)(hexval(line[i]) * 16 + hexval(line[i + 1])));
    const size_t len = buf.size();
    buf.push_back('#');
    xynet::websocket_request_handler h;
    const int ret = h.parse(std::string_view{buf.data(), len});
    const auto resp = h.generate_response();
    std::printf("%d ", ret);
    for (std::byte b : resp) std::printf("%02x", (unsigned)b);
    std::printf("\n");
  }
  return 0;
}
"""


def main():
    entries, inputs = [], []
    for name, req in AC.CASES:
        entries.append({"name": name, "req": req.hex()})
        inputs.append(req)
    for name in AC.TRUNCATED:
        req = AC.BY_NAME[name]
        for k in range(len(req) + 1):
            entries.append({"of": name, "len": k})
            inputs.append(req[:k])
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.run(["g++", "-std=c++20", "-O1", "-I" + os.path.join(REFERENCE, "include"), src, "-o", exe,
                        "-lcrypto"], check=True)
        out = subprocess.run([exe], input="".join((r.hex() or "-") + "\n" for r in inputs), capture_output=True,
                             text=True, check=True).stdout.splitlines()
    assert len(out) == len(entries)
    for e, line in zip(entries, out):
        ret, _, resp = line.partition(" ")
        e["parse"], e["resp"] = int(ret), resp
    path = os.path.join(HERE, "handshake.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e) for e in entries) + "\n]\n")
    print(path, len(entries), "entries", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

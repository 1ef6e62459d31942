"""CPU checks of xyws_accept_streams' boundary: declared in include/xyws.h and
exported, struct layouts and flag values as the header states them, the
kernel's geometry readable, the argument refusals given without a device, and
xyws_accept_request (the kernel's grammar compiled for the host) equal to the
Python model on every case of tests/accept_cases.py, under both policies, at
every truncation length and at the response capacities around the two
response lengths. The C++ shim's handler runs the reference's handshake loop."""
import ctypes as C
import os
import re
import subprocess

import pytest

import accept_cases as AC
import accept_model as M
import xynet_amd._lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_CAPS = (0, 25, 26, 128, 129, 130)
GUARD = 0xA5


def exported():
    out = subprocess.run(["nm", "-D", "--defined-only", L.lib_path()], capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_declared_and_exported():
    names = {"xyws_accept_streams", "xyws_accept_request"}
    assert names <= set(L.declared_symbols())
    lib = L.load()
    assert names | {"xyws_debug_accept_geometry"} <= exported()
    assert lib.xyws_abi_version() == 2
    assert "xyws_debug_accept_geometry" not in L.declared_symbols()  # internal: not part of the public header


def offsets(cls):
    return {f[0]: getattr(cls, f[0]).offset for f in cls._fields_}


def header_fields(name):
    src = open(L.HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.search(r"(\w+)(\[\d+\])?\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]


def test_struct_layouts_and_values_match_header():
    assert C.sizeof(L.AcceptConn) == 32 and C.sizeof(L.AcceptResult) == 32
    assert offsets(L.AcceptConn) == {"buf": 0, "len": 8, "out": 16, "out_cap": 24}
    assert offsets(L.AcceptResult) == {"status": 0, "http_status": 4, "reason": 6, "consumed": 8, "resp_len": 12,
                                       "path_off": 16, "path_len": 20, "key_off": 24, "reserved": 28}
    for cls, name in ((L.AcceptConn, "xyws_accept_conn"), (L.AcceptResult, "xyws_accept_result")):
        assert [f[0] for f in cls._fields_] == header_fields(name), name
    src = open(L.HEADER).read()

    def define(name):
        return int(re.search(r"#define %s\s+(0x[0-9a-fA-F]+|\d+)u?\b" % name, src).group(1), 0)

    for name, val in (("ACCEPTED", L.ACC_ACCEPTED), ("REJECTED", L.ACC_REJECTED), ("TRUNCATED", L.ACC_TRUNCATED),
                      ("REFERENCE", L.ACC_REFERENCE)):
        assert define("XYWS_ACC_" + name) == val
    assert (L.ACC_ACCEPTED, L.ACC_REJECTED, L.ACC_TRUNCATED) == (M.ACCEPTED, M.REJECTED, M.TRUNCATED) == (1, 2, 4)
    assert L.ACC_REFERENCE == M.REFERENCE and not L.ACC_REFERENCE & 7
    order = ["NONE", "PARSE", "TOO_LONG", "METHOD", "VERSION", "FOLDED", "HOST", "UPGRADE", "CONNECTION", "KEY",
             "WS_VERSION"]
    for i, name in enumerate(order):
        assert define("XYWS_ACR_" + name) == i == getattr(L, "ACR_" + name) == getattr(M, "R_" + name)
    assert define("XYWS_ACCEPT_MAX_REQUEST") == L.ACCEPT_MAX_REQUEST == M.MAX_REQUEST == 8192
    assert "never negotiated" in src  # subprotocols and extensions: stated in the header


def test_geometry_without_a_device():
    lib = L.load()
    assert lib.xyws_debug_accept_geometry(None) == -1
    g = (C.c_uint64 * 4)()
    assert lib.xyws_debug_accept_geometry(g) == 0
    lanes, lds, lines, grid = g
    assert lanes == 64 and lines == 64      # one wave per connection, one 16-byte line per lane per step
    assert 8192 + 15 + 129 <= lds <= 16384  # a whole request at any alignment and the response: one wave's LDS
    assert 256 <= grid <= 65536


def test_argument_refusals_without_a_device():
    """Every refusal is decided on the arguments alone, before the context is
    used: a placeholder context (never dereferenced) gets the same answers on
    a host without a GPU."""
    lib = L.load()
    fake = C.create_string_buffer(4096)
    ctx, p = C.cast(fake, C.c_void_p), C.cast(fake, C.c_void_p)
    ok = dict(conns=p, n=1, maxr=1024, policy=0, res=None)

    def call(c=ctx, **kw):
        a = dict(ok, **kw)
        return lib.xyws_accept_streams(c, a["conns"], a["n"], a["maxr"], a["policy"], a["res"], None)

    assert call(c=None) == -1 and call(c=None, n=0) == -1
    assert call(conns=None) == -1
    assert call(maxr=0) == -1 and call(maxr=8193) == -1 and call(maxr=0xFFFFFFFF) == -1
    assert call(policy=1) == -1 and call(policy=L.ACC_REFERENCE | 0x200) == -1 and call(policy=0x80000000) == -1
    assert call(n=0, maxr=0) == -1 and call(n=0, policy=2) == -1
    # n == 0: OK and nothing launched, whatever the tables (no device needed)
    assert call(n=0, conns=None) == 0
    assert call(n=0, conns=None, maxr=8192, policy=L.ACC_REFERENCE, res=p) == 0
    # the host call refuses the same arguments
    r = L.AcceptResult()
    assert lib.xyws_accept_request(b"x", 1, 0, 0, None, 0, C.byref(r)) == -1
    assert lib.xyws_accept_request(b"x", 1, 8193, 0, None, 0, C.byref(r)) == -1
    assert lib.xyws_accept_request(b"x", 1, 1024, 1, None, 0, C.byref(r)) == -1
    assert lib.xyws_accept_request(None, 1, 1024, 0, None, 0, C.byref(r)) == -1
    assert lib.xyws_accept_request(b"x", 1, 1024, 0, None, 1, C.byref(r)) == -1
    assert lib.xyws_accept_request(None, 0, 1024, 0, None, 0, None) == 0


def host_accept(lib, req, length, policy, max_request, out_cap):
    """(the 32 result bytes, the out buffer's bytes with a guard behind out_cap)."""
    out = (C.c_uint8 * (out_cap + 16))(*([GUARD] * (out_cap + 16)))
    r = L.AcceptResult()
    C.memset(C.byref(r), GUARD, 32)
    assert lib.xyws_accept_request(req, length, max_request, policy, out, out_cap, C.byref(r)) == 0
    return bytes(r), bytes(out)


@pytest.mark.parametrize("policy", [0, M.REFERENCE])
def test_host_call_equals_the_model_at_every_truncation(policy):
    lib = L.load()
    for name, req in AC.CASES:
        for k in range(len(req) + 1):
            res, resp = M.accept(req[:k], policy, max_request=M.MAX_REQUEST)
            want = M.pack_result(res)
            # (the bytes behind k stay in the buffer: nothing behind len may change the answer)
            got, out = host_accept(lib, req, k, policy, M.MAX_REQUEST, 130)
            assert got == want, (name, k)
            assert out == resp + bytes([GUARD]) * (146 - len(resp)), (name, k)


@pytest.mark.parametrize("policy", [0, M.REFERENCE])
def test_host_call_capacities_and_max_request(policy):
    lib = L.load()
    for name, req in AC.CASES:
        for cap in OUT_CAPS:
            res, resp = M.accept(req, policy, max_request=M.MAX_REQUEST, out_cap=cap)
            got, out = host_accept(lib, req, len(req), policy, M.MAX_REQUEST, cap)
            assert got == M.pack_result(res), (name, cap)
            assert out == resp + bytes([GUARD]) * (cap + 16 - len(resp)), (name, cap)
        # max_request at, one below and one above the request's own end (TOO_LONG below it)
        end = M.accept(req, policy, max_request=M.MAX_REQUEST)[0]["consumed"] or len(req)
        for mr in {max(end - 1, 1), max(end, 1), end + 1, 1, 16}:
            res, resp = M.accept(req, policy, max_request=mr)
            got, out = host_accept(lib, req, len(req), policy, mr, 130)
            assert got == M.pack_result(res) and out[:len(resp)] == resp, (name, mr)
    res = M.accept(AC.RFC, policy, max_request=len(AC.RFC) - 1)[0]
    assert res["reason"] == M.R_TOO_LONG


def test_host_call_random_keys_against_hashlib():
    lib = L.load()
    for key in AC.random_keys(64):
        req = AC.browser(key)
        got, out = host_accept(lib, req, len(req), 0, 1024, 129)
        assert out[:129] == M.response_101(key)
        assert int.from_bytes(got[24:28], "little") == req.index(key)


SHIM_PROG = r"""
#include <array>
#include <cstdio>
#include <cstring>
#include <string>
#include "xyws/websocket.hpp"
using namespace xynet;
using namespace std;
static_assert(sizeof(xyws_accept_conn) == 32 && sizeof(xyws_accept_result) == 32);
inline constexpr static const uint16_t MAX_HTTP_REQUEST_SIZE = 1024;

// websocket_handshake (example/include/common/websocket.h:40-68) without its socket: the request arrives in `recvs`
static string handshake(const char* wire, const size_t* recvs, size_t n_recvs) {
  array<byte, MAX_HTTP_REQUEST_SIZE> buf{};
  auto parser = websocket_request_handler{};
  auto recv_bytes = std::size_t{};
  for (size_t r = 0; r < n_recvs && recv_bytes < MAX_HTTP_REQUEST_SIZE; r++) {
    memcpy(buf.data() + recv_bytes, wire + recv_bytes, recvs[r]);
    recv_bytes += recvs[r];
    auto ret = parser.parse(std::span{buf.data(), recv_bytes});
    if (ret == -1) continue;
    auto response = parser.generate_response();
    printf("ret %d path %.*s\n", ret, (int)parser.get_path().size(), parser.get_path().data());
    return string(reinterpret_cast<const char*>(response.data()), response.size());
  }
  return "";
}

int main(int argc, char** argv) {
  const char* wire = argv[1];
  const size_t whole[] = {strlen(wire)};
  fputs(handshake(wire, whole, 1).c_str(), stdout);
  websocket_request_handler rfc{0, 1024};
  const int ret = rfc.parse(string_view{wire});
  printf("rfc %d %s", ret, string(rfc.response_view()).c_str());
  printf("bad %zu\n", rfc.bad_request_response().size());
  if (argc > 9) {  // (named, never run: the device call of the same shim)
    xyws::context ctx(0);
    xyws::accept_streams(ctx, nullptr, 0);
    xyws::accept_streams(ctx, nullptr, 0, nullptr, XYWS_ACC_REFERENCE, 2048, nullptr);
  }
  return 0;
}
"""


def test_shim_handler_runs_the_reference_handshake(tmp_path):
    src = tmp_path / "shim.cpp"
    src.write_text(SHIM_PROG)
    exe = tmp_path / "shim"
    libdir = os.path.dirname(L.lib_path())
    inc = os.path.join(ROOT, "include")
    r = subprocess.run(["g++", "-std=c++20", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", inc, str(src), "-o", str(exe), "-L",
                        libdir, "-lxyws", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), AC.RFC.decode()], capture_output=True)
    assert r.returncode == 0, r.stderr
    want = M.response_101(AC.RFC_KEY)
    assert r.stdout == (b"ret %d path /chat\n" % len(AC.RFC)) + want + (b"rfc %d " % len(AC.RFC)) + want + b"bad 26\n"

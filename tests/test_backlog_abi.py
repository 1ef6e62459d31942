"""CPU checks of xyws_backlog_streams' boundary: declared in include/xyws.h
and exported, struct layouts and flag values as the header states them, the
kernels' geometry readable, the argument refusals and the nothing-to-launch
case answered without a device, and the C++ shim's wrapper compiling."""
import ctypes as C
import os
import re
import subprocess

import xynet_amd._lib as L
from test_reply_abi import exported, offsets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_fields(name):
    """Field names of a struct in include/xyws.h, in order (an array's extent may be a macro)."""
    src = open(L.HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.search(r"(\w+)(\[\w+\])?\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]


def test_declared_and_exported():
    assert "xyws_backlog_streams" in L.declared_symbols()
    lib = L.load()
    assert hasattr(lib, "xyws_backlog_streams") and hasattr(lib, "xyws_debug_backlog_geometry")
    assert {"xyws_backlog_streams", "xyws_debug_backlog_geometry"} <= exported()
    assert lib.xyws_abi_version() == 2
    # internal: not part of the public header
    assert "xyws_debug_backlog_geometry" not in L.declared_symbols()


def test_struct_layouts_match_header():
    assert C.sizeof(L.BacklogCarry) == 192 and C.sizeof(L.BacklogRoom) == 32
    assert C.sizeof(L.BacklogRoomResult) == 32 and C.sizeof(L.BacklogConn) == 64 and C.sizeof(L.BacklogResult) == 32
    assert offsets(L.BacklogCarry) == {"start": 0, "len": 8, "count": 16, "gaps": 20, "total": 24, "flen": 32,
                                       "reserved": 160}
    assert offsets(L.BacklogRoom) == {"log": 0, "log_cap": 8, "bc": 16, "keep": 24, "reserved0": 28}
    assert offsets(L.BacklogRoomResult) == {"len": 0, "count": 8, "folded": 12, "dropped": 16, "status": 20,
                                            "reserved": 24}
    assert offsets(L.BacklogConn) == {"out": 0, "out_cap": 8, "bcast": 16, "reply": 24, "room": 32, "flags": 36,
                                      "reserved": 40}
    assert offsets(L.BacklogResult) == {"send_len": 0, "backlog_len": 8, "status": 16, "reserved0": 20,
                                        "reserved": 24}
    for cls, name in ((L.BacklogCarry, "xyws_backlog_carry"), (L.BacklogRoom, "xyws_backlog_room"),
                      (L.BacklogRoomResult, "xyws_backlog_room_result"), (L.BacklogConn, "xyws_backlog_conn"),
                      (L.BacklogResult, "xyws_backlog_result")):
        assert [f[0] for f in cls._fields_] == header_fields(name), name
    src = open(L.HEADER).read()
    for name in ("BL_PASSTHROUGH", "BL_BAD_CARRY", "BL_MISMATCH", "BL_GAP", "BL_EVICTED", "BL_TOO_LONG", "BL_JOIN",
                 "BLC_JOINED", "BLC_TRUNCATED", "BLC_NO_ROOM", "BLC_NOT_RECEIVER"):
        assert int(re.search(r"#define XYWS_%s\s+(0x[0-9a-fA-F]+)u" % name, src).group(1), 16) == getattr(L, name), name
    assert (L.BL_PASSTHROUGH, L.BL_BAD_CARRY, L.BL_MISMATCH, L.BL_GAP, L.BL_EVICTED, L.BL_TOO_LONG) == \
        (1, 2, 4, 8, 16, 32)
    assert (L.BLC_JOINED, L.BLC_TRUNCATED, L.BLC_NO_ROOM, L.BLC_NOT_RECEIVER) == (1, 2, 4, 8) and L.BL_JOIN == 1
    assert re.search(r"#define XYWS_BACKLOG_MAX\s+16u", src) and L.BACKLOG_MAX == 16
    assert re.search(r"#define XYWS_ABI_VERSION 2\b", src)


def test_geometry_without_a_device():
    lib = L.load()
    assert lib.xyws_debug_backlog_geometry(None) == -1
    g = (C.c_uint64 * 4)()
    assert lib.xyws_debug_backlog_geometry(g) == 0
    tile, step, grid, wave = g
    assert wave == 64 and tile % wave == 0 and 64 <= tile <= 1024  # one member per thread of a workgroup
    assert step % 16 == 0 and step >= 16 * wave                   # whole 16-byte lines, at least one per lane
    assert 256 <= grid <= 65535


def test_argument_refusals_without_a_device():
    """Every refusal is decided on the arguments alone, before the context is
    used: a placeholder context (never dereferenced) gets the same answers on
    a host without a GPU."""
    lib = L.load()
    fake = C.create_string_buffer(4096)
    ctx, p = C.cast(fake, C.c_void_p), C.cast(fake, C.c_void_p)
    ok = dict(rsm=p, rres=p, bc=p, n=1, rooms=p, rr=p, br=p, brr=p, nr=1, jc=p, res=p)

    def call(c=ctx, **kw):
        a = dict(ok, **kw)
        return lib.xyws_backlog_streams(c, a["rsm"], a["rres"], a["bc"], a["n"], a["rooms"], a["rr"], a["br"],
                                        a["brr"], a["nr"], a["jc"], a["res"], None)

    assert call(c=None) == -1
    assert call(c=None, n=0, nr=0) == -1
    assert call(rsm=None) == -1 and call(rres=None) == -1 and call(bc=None) == -1
    assert call(rooms=None) == -1 and call(rr=None) == -1 and call(br=None) == -1
    assert call(n=0, rooms=None) == -1 and call(n=0, rr=None) == -1 and call(n=0, br=None) == -1
    assert call(n=0xFFFFFFFF) == -1 and call(n=1 << 32) == -1 and call(n=1 << 63) == -1
    assert call(n=0xFFFFFFFF, nr=0) == -1
    # nothing to launch: OK whatever the tables (no device needed)
    assert call(n=0, nr=0) == 0
    assert call(n=0, nr=0, rsm=None, rres=None, bc=None, rooms=None, rr=None, br=None, brr=None, jc=None,
                res=None) == 0
    # no room to fold and nobody to deliver to
    assert call(nr=0, jc=None, rsm=None, rres=None, bc=None, rooms=None, rr=None, br=None) == 0


SHIM_PROG = r"""
#include <cstdio>
#include "xyws/websocket.hpp"
using namespace xyws;
static_assert(sizeof(xyws_backlog_carry) == 192 && sizeof(xyws_backlog_room) == 32);
static_assert(sizeof(xyws_backlog_room_result) == 32 && sizeof(xyws_backlog_conn) == 64);
static_assert(sizeof(xyws_backlog_result) == 32 && XYWS_BACKLOG_MAX == 16);
int main() {
  try {
    context ctx(0);
    backlog_streams(ctx, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0);
    backlog_streams(ctx, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr,
                    nullptr);
    std::puts("device");
    return 0;
  } catch (const error& e) {
    std::printf("error %d\n", e.code());
    return 0;
  }
}
"""


def test_shim_wrapper_compiles(tmp_path):
    src = tmp_path / "shim.cpp"
    src.write_text(SHIM_PROG)
    exe = tmp_path / "shim"
    libdir = os.path.dirname(L.lib_path())
    r = subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe), "-L", libdir, "-lxyws", f"-Wl,-rpath,{libdir}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

"""CPU checks of xyws_broadcast_streams' boundary: declared in include/xyws.h
and exported, struct layouts as the header states them, the kernels' geometry
readable, the argument refusals given without a device, and the C++ shim's
wrapper compiling."""
import ctypes as C
import os
import re
import subprocess

import xynet_amd._lib as L
from test_reply_abi import exported, header_fields, offsets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_and_exported():
    assert "xyws_broadcast_streams" in L.declared_symbols()
    lib = L.load()
    assert hasattr(lib, "xyws_broadcast_streams") and hasattr(lib, "xyws_debug_broadcast_geometry")
    assert {"xyws_broadcast_streams", "xyws_debug_broadcast_geometry"} <= exported()
    assert lib.xyws_abi_version() == 2
    # internal: not part of the public header
    assert "xyws_debug_broadcast_geometry" not in L.declared_symbols()


def test_struct_layouts_match_header():
    assert C.sizeof(L.Room) == 32 and C.sizeof(L.RoomResult) == 32
    assert C.sizeof(L.BcastConn) == 64 and C.sizeof(L.BcastResult) == 32
    assert offsets(L.Room) == {"members": 0, "n_members": 8, "wire": 16, "wire_cap": 24}
    assert offsets(L.RoomResult) == {"wire_len": 0, "nmsgs": 8, "skipped": 12, "receivers": 16, "status": 20,
                                     "reserved": 24}
    assert offsets(L.BcastConn) == {"head": 0, "head_len": 8, "out": 16, "out_cap": 24, "reply": 32, "room": 40,
                                    "reserved0": 44, "reserved": 48}
    assert offsets(L.BcastResult) == {"send_len": 0, "bcast_len": 8, "status": 16, "reserved0": 20, "reserved": 24}
    for cls, name in ((L.Room, "xyws_room"), (L.RoomResult, "xyws_room_result"), (L.BcastConn, "xyws_bcast_conn"),
                      (L.BcastResult, "xyws_bcast_result")):
        assert [f[0] for f in cls._fields_] == header_fields(name), name
    src = open(L.HEADER).read()
    for name, val in (("ROOM_TRUNCATED", L.ROOM_TRUNCATED), ("ROOM_BAD_MEMBER", L.ROOM_BAD_MEMBER),
                      ("ROOM_MSG_CAP", L.ROOM_MSG_CAP), ("BC_TRUNCATED", L.BC_TRUNCATED),
                      ("BC_NOT_RECEIVER", L.BC_NOT_RECEIVER), ("BC_NO_ROOM", L.BC_NO_ROOM)):
        assert int(re.search(r"#define XYWS_%s\s+(0x[0-9a-fA-F]+)u" % name, src).group(1), 16) == val, name
    assert (L.ROOM_TRUNCATED, L.ROOM_BAD_MEMBER, L.ROOM_MSG_CAP) == (1, 2, 4)
    assert (L.BC_TRUNCATED, L.BC_NOT_RECEIVER, L.BC_NO_ROOM) == (1, 2, 4)
    assert re.search(r"#define XYWS_ROOM_NONE\s+UINT32_MAX", src) and L.ROOM_NONE == 0xFFFFFFFF
    assert re.search(r"#define XYWS_ABI_VERSION 2\b", src)


def test_geometry_without_a_device():
    lib = L.load()
    assert lib.xyws_debug_broadcast_geometry(None) == -1
    g = (C.c_uint64 * 4)()
    assert lib.xyws_debug_broadcast_geometry(g) == 0
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
    ok = dict(rsm=p, rres=p, bc=p, n=1, rooms=p, rr=p, nr=1, flags=0x11, enc=0, res=None)

    def call(c=ctx, **kw):
        a = dict(ok, **kw)
        return lib.xyws_broadcast_streams(c, a["rsm"], a["rres"], a["bc"], a["n"], a["rooms"], a["rr"], a["nr"],
                                          a["flags"], a["enc"], a["res"], None)

    assert call(c=None) == -1
    assert call(c=None, n=0) == -1
    assert call(rsm=None) == -1 and call(rres=None) == -1 and call(bc=None) == -1
    assert call(rooms=None) == -1 and call(rr=None) == -1
    assert call(n=0, rooms=None) == -1 and call(n=0, rr=None) == -1
    assert call(n=0xFFFFFFFF) == -1 and call(n=1 << 32) == -1 and call(n=1 << 63) == -1
    assert call(flags=0x31) == -1 and call(flags=0x20) == -1 and call(n=0, flags=0x21) == -1
    assert call(enc=2) == -1 and call(enc=L.ENC_FRAME_OPCODE | 0x80000000) == -1 and call(n=0, enc=2) == -1
    # n == 0: OK and nothing launched, whatever the tables (no device needed)
    assert call(n=0, rsm=None, rres=None, bc=None) == 0
    assert call(n=0, rsm=None, rres=None, bc=None, rooms=None, rr=None, nr=0) == 0
    assert call(n=0, enc=L.ENC_FRAME_OPCODE) == 0 and call(n=0, flags=0x12) == 0


SHIM_PROG = r"""
#include <cstdio>
#include "xyws/websocket.hpp"
using namespace xyws;
static_assert(sizeof(xyws_room) == 32 && sizeof(xyws_room_result) == 32);
static_assert(sizeof(xyws_bcast_conn) == 64 && sizeof(xyws_bcast_result) == 32);
int main() {
  try {
    context ctx(0);
    broadcast_streams(ctx, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0);
    broadcast_streams(ctx, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0,
                      websocket_flags::WS_FINAL_FRAME | websocket_flags::WS_OP_TEXT, XYWS_ENC_FRAME_OPCODE, nullptr,
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

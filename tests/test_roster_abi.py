"""CPU checks of xyws_roster_streams' boundary: declared in include/xyws.h and
exported, struct layouts and flag values as the header states them, a roster
result row readable as a broadcast row, the kernels' geometry readable, the
argument refusals and the nothing-to-launch case answered without a device, and
the C++ shim's wrapper compiling."""
import ctypes as C
import os
import re
import subprocess

import xynet_amd._lib as L
from test_backlog_abi import header_fields
from test_reply_abi import exported, offsets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_and_exported():
    assert "xyws_roster_streams" in L.declared_symbols()
    lib = L.load()
    assert hasattr(lib, "xyws_roster_streams") and hasattr(lib, "xyws_debug_roster_geometry")
    assert {"xyws_roster_streams", "xyws_debug_roster_geometry"} <= exported()
    assert lib.xyws_abi_version() == 2  # (a function more breaks no caller)
    # internal: not part of the public header
    assert "xyws_debug_roster_geometry" not in L.declared_symbols()


def test_struct_layouts_match_header():
    assert C.sizeof(L.RosterConn) == 64 and C.sizeof(L.RosterRoom) == 32 and C.sizeof(L.RosterRoomResult) == 32
    assert C.sizeof(L.RosterResult) == 32 and C.sizeof(L.RosterText) == 104
    assert offsets(L.RosterConn) == {"name": 0, "name_len": 8, "out": 16, "out_cap": 24, "bcast": 32, "reply": 40,
                                     "accept": 48, "room": 56, "flags": 60}
    assert offsets(L.RosterRoom) == {"member_cap": 0, "notes": 8, "notes_cap": 16, "seen": 24}
    assert offsets(L.RosterRoomResult) == {"notes_len": 0, "welcome_off": 8, "joined": 16, "left": 20, "n_members": 24,
                                           "status": 28}
    assert offsets(L.RosterResult) == {"send_len": 0, "note_len": 8, "status": 16, "room": 20, "note_off": 24}
    assert offsets(L.RosterText) == {"head": 0, "joined": 32, "left": 64, "head_len": 96, "joined_len": 97,
                                     "left_len": 98, "reserved": 99}
    for cls, name in ((L.RosterConn, "xyws_roster_conn"), (L.RosterRoom, "xyws_roster_room"),
                      (L.RosterRoomResult, "xyws_roster_room_result"), (L.RosterResult, "xyws_roster_result")):
        assert [f[0] for f in cls._fields_] == header_fields(name), name
    src = open(L.HEADER).read()
    names = ("RS_JOIN", "RS_LEAVE", "RS_JOIN_ON_ACCEPT", "RS_LEAVE_ON_CLOSE", "RS_TRUNCATED", "RS_FULL", "RS_BAD_MEMBER",
             "RSC_TRUNCATED", "RSC_NOT_RECEIVER", "RSC_NO_ROOM", "RSC_MEMBER", "RSC_JOINED", "RSC_LEFT", "RSC_FULL",
             "RSC_ALREADY", "RSC_BAD_NAME")
    for name in names:
        assert int(re.search(r"#define XYWS_%s\s+(0x[0-9a-fA-F]+)u" % name, src).group(1), 16) == getattr(L, name), name
    assert (L.RS_JOIN, L.RS_LEAVE, L.RS_JOIN_ON_ACCEPT, L.RS_LEAVE_ON_CLOSE) == (1, 2, 4, 8)
    assert (L.RS_TRUNCATED, L.RS_FULL, L.RS_BAD_MEMBER) == (0x10, 0x20, 0x40)
    bits = [getattr(L, n) for n in names[7:]]
    assert bits == [1 << k for k in range(9)]
    assert re.search(r"#define XYWS_ROSTER_NAME_MAX\s+256u", src) and L.ROSTER_NAME_MAX == 256
    assert re.search(r"#define XYWS_ROSTER_TEXT_MAX\s+32u", src) and L.ROSTER_TEXT_MAX == 32
    assert re.search(r"#define XYWS_ABI_VERSION 2\b", src)


def test_a_roster_row_reads_as_a_broadcast_row():
    """xyws_backlog_conn.bcast may point at a roster row: send_len, note_len
    and status lie where the broadcast row has send_len, bcast_len and status,
    and the three bits the backlog and the fan-out test have the same values."""
    a, b = offsets(L.RosterResult), offsets(L.BcastResult)
    assert (a["send_len"], a["note_len"], a["status"]) == (b["send_len"], b["bcast_len"], b["status"])
    assert C.sizeof(L.RosterResult) == C.sizeof(L.BcastResult)
    assert dict(L.RosterResult._fields_)["status"] is dict(L.BcastResult._fields_)["status"]
    assert (L.RSC_TRUNCATED, L.RSC_NOT_RECEIVER, L.RSC_NO_ROOM) == (L.BC_TRUNCATED, L.BC_NOT_RECEIVER, L.BC_NO_ROOM)
    row = L.RosterResult(send_len=77, note_len=5, status=L.RSC_NOT_RECEIVER | L.RSC_LEFT, room=3, note_off=9)
    seen = L.BcastResult.from_buffer_copy(bytes(row))
    assert (seen.send_len, seen.bcast_len) == (77, 5) and seen.status & L.BC_NOT_RECEIVER
    # the header says so, and xyws_rows.h asserts it for the kernels
    rows_h = open(os.path.join(L.PKG, "csrc", "xyws_rows.h")).read()
    assert "XYWS_RSC_TRUNCATED == XYWS_BC_TRUNCATED" in rows_h
    assert "offsetof(xyws_roster_result, status) == offsetof(xyws_bcast_result, status)" in rows_h


def test_geometry_without_a_device():
    lib = L.load()
    assert lib.xyws_debug_roster_geometry(None) == -1
    g = (C.c_uint64 * 4)()
    assert lib.xyws_debug_roster_geometry(g) == 0
    tile, scan, step, grid = g
    assert tile % 64 == 0 and 64 <= tile <= 1024  # one member per thread of a workgroup
    assert scan % 64 == 0 and 64 <= scan <= 4096  # whole waves of dev_want words
    assert step % 16 == 0 and step >= 16 * 64     # whole 16-byte lines, at least one per lane
    assert 256 <= grid <= 65535
    b = (C.c_uint64 * 4)()
    assert lib.xyws_debug_backlog_geometry(b) == 0 and b[1] == step and b[2] == grid  # the fan-out's geometry


def test_argument_refusals_without_a_device():
    """Every refusal is decided on the arguments alone, before the context is
    used: a placeholder context (never dereferenced) gets the same answers on
    a host without a GPU."""
    lib = L.load()
    fake = C.create_string_buffer(4096)
    ctx, p = C.cast(fake, C.c_void_p), C.cast(fake, C.c_void_p)
    ok = dict(bc=p, rc=p, n=1, rooms=p, rr=p, rres=p, nr=1, text=None, flags=0x11, jc=p, want=p, res=p)

    def call(c=ctx, **kw):
        a = dict(ok, **kw)
        return lib.xyws_roster_streams(c, a["bc"], a["rc"], a["n"], a["rooms"], a["rr"], a["rres"], a["nr"], a["text"],
                                       a["flags"], a["jc"], a["want"], a["res"], None)

    assert call(c=None) == -1
    assert call(c=None, n=0, nr=0) == -1
    assert call(bc=None) == -1 and call(rc=None) == -1 and call(want=None) == -1 and call(res=None) == -1
    assert call(nr=0, bc=None) == -1 and call(nr=0, want=None) == -1
    assert call(rooms=None) == -1 and call(rr=None) == -1 and call(rres=None) == -1
    assert call(n=0, rooms=None) == -1 and call(n=0, rr=None) == -1 and call(n=0, rres=None) == -1
    assert call(n=0xFFFFFFFF) == -1 and call(n=1 << 32) == -1 and call(n=1 << 63) == -1
    assert call(n=0xFFFFFFFF, nr=0) == -1 and call(nr=0xFFFFFFFF) == -1
    assert call(flags=0x20 | 0x11) == -1 and call(flags=0x20, n=0, nr=0) == -1
    for field in ("head_len", "joined_len", "left_len"):
        t = L.RosterText(head_len=32, joined_len=32, left_len=32)
        assert call(text=C.byref(t), n=0, nr=0) == 0   # 32 is allowed
        setattr(t, field, 33)
        assert call(text=C.byref(t)) == -1 and call(text=C.byref(t), n=0, nr=0) == -1
    # nothing to launch: OK whatever the tables (no device needed)
    assert call(n=0, nr=0) == 0
    assert call(n=0, nr=0, bc=None, rc=None, rooms=None, rr=None, rres=None, jc=None, want=None, res=None) == 0


SHIM_PROG = r"""
#include <cstdio>
#include "xyws/websocket.hpp"
using namespace xyws;
static_assert(sizeof(xyws_roster_conn) == 64 && sizeof(xyws_roster_room) == 32);
static_assert(sizeof(xyws_roster_room_result) == 32 && sizeof(xyws_roster_result) == 32);
static_assert(sizeof(xyws_roster_text) == 104 && XYWS_ROSTER_NAME_MAX == 256);
int main() {
  try {
    context ctx(0);
    roster_streams(ctx, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr);
    xyws_roster_text text = {};
    roster_streams(ctx, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                   XYWS_FLAG_FIN | XYWS_FLAG_OP_BINARY, &text, nullptr);
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

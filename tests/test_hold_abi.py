"""CPU checks of xyws_hold_streams' boundary: declared in include/xyws.h and
exported, struct layouts as the header states them, the kernel's geometry
readable, the argument refusals given without a device, and the C++ shim's
wrapper compiling."""
import ctypes as C
import os
import re
import subprocess

import hold_model as HM
import xynet_amd._lib as L
from test_reply_abi import exported, header_fields, offsets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_and_exported():
    assert "xyws_hold_streams" in L.declared_symbols()
    lib = L.load()
    assert hasattr(lib, "xyws_hold_streams") and hasattr(lib, "xyws_debug_hold_geometry")
    assert {"xyws_hold_streams", "xyws_debug_hold_geometry"} <= exported()
    assert lib.xyws_abi_version() == 2
    # internal: not part of the public header
    assert "xyws_debug_hold_geometry" not in L.declared_symbols()


def test_struct_layouts_match_header():
    assert C.sizeof(L.HoldConn) == 32 and C.sizeof(L.HoldCarry) == 32 and C.sizeof(L.HoldResult) == 32
    assert offsets(L.HoldConn) == {"hold_cap": 0, "hc": 8, "vmsgs": 16, "vmsg_cap": 24}
    assert offsets(L.HoldCarry) == {"start": 0, "held": 8, "nframes": 16, "status": 24, "opcode": 28, "reserved": 29}
    assert offsets(L.HoldResult) == {"held": 0, "delivered_len": 8, "status": 16, "reserved0": 20, "reserved": 24}
    for cls, name in ((L.HoldConn, "xyws_hold_conn"), (L.HoldCarry, "xyws_hold_carry"),
                      (L.HoldResult, "xyws_hold_result")):
        assert [f[0] for f in cls._fields_] == header_fields(name), name
    src = open(L.HEADER).read()
    for name, val, model in (("DELIVERED", L.HOLD_DELIVERED, HM.DELIVERED), ("ACTIVE", L.HOLD_ACTIVE, HM.ACTIVE),
                             ("LOST", L.HOLD_LOST, HM.LOST), ("DROPPED", L.HOLD_DROPPED, HM.DROPPED),
                             ("TOO_LONG", L.HOLD_TOO_LONG, HM.TOO_LONG),
                             ("PASSTHROUGH", L.HOLD_PASSTHROUGH, HM.PASSTHROUGH)):
        assert int(re.search(r"#define XYWS_HOLD_%s\s+(0x[0-9a-fA-F]+)u" % name, src).group(1), 16) == val == model
    assert (L.HOLD_DELIVERED, L.HOLD_ACTIVE, L.HOLD_LOST, L.HOLD_DROPPED, L.HOLD_TOO_LONG, L.HOLD_PASSTHROUGH) == \
        (0x1, 0x2, 0x4, 0x8, 0x10, 0x20)
    assert re.search(r"#define XYWS_ABI_VERSION 2\b", src)
    # the model's packings are the structs'
    c = HM.Carry(16, 5, 3, HM.ACTIVE, 2)
    s = L.HoldCarry.from_buffer_copy(c.pack())
    assert (s.start, s.held, s.nframes, s.status, s.opcode) == c.key()
    r = L.HoldResult.from_buffer_copy(HM.pack_result(dict(held=7, delivered_len=9, status=0x13)))
    assert (r.held, r.delivered_len, r.status, r.reserved0, r.reserved) == (7, 9, 0x13, 0, 0)


def test_geometry_without_a_device():
    lib = L.load()
    assert lib.xyws_debug_hold_geometry(None) == -1
    g = (C.c_uint64 * 4)()
    assert lib.xyws_debug_hold_geometry(g) == 0
    lanes, line, step, grid = g
    assert lanes == 64 and line == 16 and step == lanes * line  # one wave, a 16-byte line per lane and step
    assert 256 <= grid <= 65535


def test_argument_refusals_without_a_device():
    """Every refusal is decided on the arguments alone, before the context is
    used: a placeholder context (never dereferenced) gets the same answers on
    a host without a GPU."""
    lib = L.load()
    fake = C.create_string_buffer(4096)
    ctx, p = C.cast(fake, C.c_void_p), C.cast(fake, C.c_void_p)
    ok = dict(rsm=p, rres=p, hold=p, n=1, view=p, vres=p, res=None)

    def call(c=ctx, **kw):
        a = dict(ok, **kw)
        return lib.xyws_hold_streams(c, a["rsm"], a["rres"], a["hold"], a["n"], a["view"], a["vres"], a["res"], None)

    assert call(c=None) == -1  # (a null ctx first)
    assert call(c=None, n=0) == -1
    assert call(c=None, rsm=None) == -1
    assert call(rsm=None) == -1 and call(rres=None) == -1 and call(hold=None) == -1
    assert call(view=None) == -1 and call(vres=None) == -1
    assert call(view=None, res=p) == -1 and call(rsm=None, rres=None, hold=None, view=None, vres=None) == -1
    # n == 0: OK and nothing launched, whatever the tables (no device needed)
    assert call(n=0) == 0
    assert call(n=0, rsm=None, rres=None, hold=None, view=None, vres=None) == 0
    assert call(n=0, res=p) == 0


SHIM_PROG = r"""
#include <cstdio>
#include "xyws/websocket.hpp"
using namespace xyws;
static_assert(sizeof(xyws_hold_conn) == 32 && sizeof(xyws_hold_carry) == 32 && sizeof(xyws_hold_result) == 32);
static_assert(offsetof(xyws_hold_carry, status) == 24 && offsetof(xyws_hold_carry, opcode) == 28);
int main() {
  try {
    context ctx(0);
    hold_streams(ctx, nullptr, nullptr, nullptr, 0, nullptr, nullptr);
    hold_streams(ctx, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
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

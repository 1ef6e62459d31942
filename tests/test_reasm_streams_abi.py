"""CPU checks of xyws_reassemble_streams' boundary: declared in include/xyws.h
and exported, struct layouts as the header states them, the kernel's geometry
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
    assert "xyws_reassemble_streams" in L.declared_symbols()
    lib = L.load()
    assert hasattr(lib, "xyws_reassemble_streams") and hasattr(lib, "xyws_debug_reasm_streams_geometry")
    assert {"xyws_reassemble_streams", "xyws_debug_reasm_streams_geometry"} <= exported()
    assert lib.xyws_abi_version() == 2
    # internal: not part of the public header
    assert "xyws_debug_reasm_streams_geometry" not in L.declared_symbols()


def test_struct_layouts_match_header():
    assert C.sizeof(L.ReasmConn) == 64 and C.sizeof(L.ReasmResult) == 32
    assert offsets(L.ReasmConn) == {"out": 0, "out_cap": 8, "mc": 16, "msgs": 24, "msg_cap": 32, "reserved": 40}
    assert offsets(L.ReasmResult) == {"out_len": 0, "nmsgs": 8, "completed": 16, "status": 20, "reserved": 24}
    for cls, name in ((L.ReasmConn, "xyws_reasm_conn"), (L.ReasmResult, "xyws_reasm_result")):
        assert [f[0] for f in cls._fields_] == header_fields(name), name
    src = open(L.HEADER).read()
    for name, val in (("RSM_TRUNCATED", L.RSM_TRUNCATED), ("RSM_MSG_CAP", L.RSM_MSG_CAP),
                      ("RSM_OVERFLOW", L.RSM_OVERFLOW), ("RSM_OPEN", L.RSM_OPEN), ("RSM_UTF8_BAD", L.RSM_UTF8_BAD),
                      ("MSG_OVERFLOW", L.MSG_OVERFLOW)):
        assert int(re.search(r"#define XYWS_%s\s+(0x[0-9a-fA-F]+)u" % name, src).group(1), 16) == val, name
    assert (L.RSM_TRUNCATED, L.RSM_MSG_CAP, L.RSM_OVERFLOW, L.RSM_OPEN, L.RSM_UTF8_BAD) == (1, 2, 4, 8, 16)
    assert L.MSG_OVERFLOW == 0x80
    # the sticky bit is none of xyws_reassemble_stream's status bits
    assert not L.MSG_OVERFLOW & (L.MSG_COMPLETE | L.MSG_UTF8_BAD | L.MSG_INTERRUPTED | L.MSG_TRUNCATED |
                                 L.MSG_ORPHANS | L.MSG_CONTINUED | L.MSG_UNCHECKED)


def test_geometry_without_a_device():
    lib = L.load()
    assert lib.xyws_debug_reasm_streams_geometry(None) == -1
    g = (C.c_uint64 * 4)()
    assert lib.xyws_debug_reasm_streams_geometry(g) == 0
    tile, step, grid, wave = g
    assert wave == 64 and tile == wave  # one frame per lane
    assert step == 16 * wave            # one 16-byte line per lane per step
    assert 256 <= grid <= 65536


def test_argument_refusals_without_a_device():
    """Every refusal is decided on the arguments alone, before the context is
    used: a placeholder context (never dereferenced) gets the same answers on
    a host without a GPU."""
    lib = L.load()
    fake = C.create_string_buffer(4096)
    ctx, p = C.cast(fake, C.c_void_p), C.cast(fake, C.c_void_p)
    ok = dict(conns=p, nf=p, rsm=p, n=1, opts=L.REASM_UTF8, res=None)

    def call(c=ctx, **kw):
        a = dict(ok, **kw)
        return lib.xyws_reassemble_streams(c, a["conns"], a["nf"], a["rsm"], a["n"], a["opts"], a["res"], None)

    assert call(c=None) == -1
    assert call(c=None, n=0) == -1
    assert call(conns=None) == -1 and call(nf=None) == -1 and call(rsm=None) == -1
    assert call(opts=2) == -1 and call(opts=L.REASM_UTF8 | 0x80000000) == -1
    assert call(n=0, opts=2) == -1
    # n == 0: OK and nothing launched, whatever the tables (no device needed)
    assert call(n=0, conns=None, nf=None, rsm=None) == 0
    assert call(n=0, opts=0) == 0 and call(n=0) == 0


SHIM_PROG = r"""
#include <cstdio>
#include "xyws/websocket.hpp"
using namespace xyws;
static_assert(sizeof(xyws_reasm_conn) == 64 && sizeof(xyws_reasm_result) == 32);
int main() {
  try {
    context ctx(0);
    reassemble_streams(ctx, nullptr, nullptr, nullptr, 0);
    reassemble_streams(ctx, nullptr, nullptr, nullptr, 0, XYWS_REASM_UTF8, nullptr, nullptr);
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

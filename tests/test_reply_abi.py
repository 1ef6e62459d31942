"""CPU checks of xyws_reply_streams' boundary: declared in include/xyws.h and
exported, struct layouts as the header states them, the kernel's geometry
readable and the argument refusals given without a device."""
import ctypes as C
import re
import subprocess

import xynet_amd._lib as L


def exported():
    out = subprocess.run(["nm", "-D", "--defined-only", L.lib_path()], capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_declared_and_exported():
    assert "xyws_reply_streams" in L.declared_symbols()
    lib = L.load()
    assert hasattr(lib, "xyws_reply_streams") and hasattr(lib, "xyws_debug_reply_geometry")
    assert {"xyws_reply_streams", "xyws_debug_reply_geometry"} <= exported()
    assert lib.xyws_abi_version() == 2
    # internal: not part of the public header
    assert "xyws_debug_reply_geometry" not in L.declared_symbols()


def offsets(cls):
    return {f[0]: getattr(cls, f[0]).offset for f in cls._fields_}


def header_fields(name):
    """Field names of a struct in include/xyws.h, in order."""
    src = open(L.HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.search(r"(\w+)(\[\d+\])?\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]


def test_struct_layouts_match_header():
    assert C.sizeof(L.ReplyCarry) == 32 and C.sizeof(L.ReplyConn) == 32 and C.sizeof(L.ReplyResult) == 32
    assert offsets(L.ReplyCarry) == {"frame_remaining": 0, "frames_seen": 8, "replies_total": 16, "close_code": 24,
                                     "echoing": 26, "status": 27, "reserved": 28}
    assert offsets(L.ReplyConn) == {"out": 0, "out_cap": 8, "rc": 16, "verdicts": 24}
    assert offsets(L.ReplyResult) == {"reply_len": 0, "first_close": 8, "answered": 16, "close_code": 20,
                                      "status": 22, "reserved": 24}
    for cls, name in ((L.ReplyCarry, "xyws_reply_carry"), (L.ReplyConn, "xyws_reply_conn"),
                      (L.ReplyResult, "xyws_reply_result")):
        assert [f[0] for f in cls._fields_] == header_fields(name), name
    src = open(L.HEADER).read()
    for name, val in (("TRUNCATED", L.RPL_TRUNCATED), ("CLOSED", L.RPL_CLOSED), ("OVERFLOW", L.RPL_OVERFLOW)):
        assert int(re.search(r"#define XYWS_RPL_%s\s+(0x[0-9a-fA-F]+)u" % name, src).group(1), 16) == val
    assert (L.RPL_TRUNCATED, L.RPL_CLOSED, L.RPL_OVERFLOW) == (1, 2, 4)


def test_geometry_without_a_device():
    lib = L.load()
    assert lib.xyws_debug_reply_geometry(None) == -1
    g = (C.c_uint64 * 4)()
    assert lib.xyws_debug_reply_geometry(g) == 0
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
    ok = dict(conns=p, nf=p, rep=p, n=1, maxp=1 << 20, policy=0, flags=0x11, enc=0, amask=1, res=None)

    def call(c=ctx, **kw):
        a = dict(ok, **kw)
        return lib.xyws_reply_streams(c, a["conns"], a["nf"], a["rep"], a["n"], a["maxp"], a["policy"], a["flags"],
                                      a["enc"], a["amask"], a["res"], None)

    assert call(c=None) == -1
    assert call(c=None, n=0) == -1
    assert call(conns=None) == -1 and call(nf=None) == -1 and call(rep=None) == -1
    assert call(flags=0x11 | 0x20) == -1  # XYWS_FLAG_HAS_MASK: server role only
    assert call(enc=2) == -1 and call(enc=L.ENC_FRAME_OPCODE | 0x80000000) == -1
    assert call(policy=0x10) == -1 and call(policy=0x80000000) == -1
    assert call(amask=1 << (L.ACT_CLOSE + 1)) == -1 and call(amask=0x80000000) == -1
    # n == 0: OK and nothing launched, whatever the tables (no device needed)
    assert call(n=0, conns=None, nf=None, rep=None) == 0
    assert call(n=0, policy=0xF, enc=L.ENC_FRAME_OPCODE, amask=0xF) == 0

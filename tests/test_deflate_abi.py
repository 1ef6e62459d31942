"""CPU checks of xyws_deflate_streams' and xyws_broadcast_deflated_streams' boundary: the two rows' sizes and offsets
as the header states them, the geometry, and every refusal decided on the arguments alone, before the context is used
(no device)."""
import ctypes as C

import pytest

import xynet_amd._lib as L

LAYOUT = {
    L.DeflateConn: (64, dict(out=0, out_cap=8, vmsgs=16, vmsg_cap=24, flags=32, reserved0=36, reserved=40)),
    L.DeflateResult: (32, dict(out_len=0, in_len=8, n_deflated=16, n_stored=20, status=24, reserved0=28)),
}


@pytest.mark.parametrize("struct", LAYOUT, ids=lambda s: s.__name__)
def test_row_layout(struct):
    size, offs = LAYOUT[struct]
    assert C.sizeof(struct) == size and {n: getattr(struct, n).offset for n, _ in struct._fields_} == offs


def test_symbols_and_geometry():
    assert {"xyws_deflate_streams", "xyws_broadcast_deflated_streams"} <= set(L.declared_symbols())
    g = (C.c_uint64 * 4)()
    assert L.load().xyws_debug_deflate_geometry(g) == 0 and L.load().xyws_debug_deflate_geometry(None) == -1
    W, slots, cap, wave = g
    assert wave == 64 and W % 16 == 0 and 1024 <= W <= 65535 and slots & (slots - 1) == 0
    assert cap % 256 == 0 and cap // 256 * (W + 4 * slots + W * 9 // 8) <= 160 * 1024  # the stages of a CU's waves fit its LDS


def test_refusals_without_a_device():
    lib = L.load()
    fake = C.create_string_buffer(4096)
    ctx = p = C.cast(fake, C.c_void_p)
    ok = dict(tin=p, tres=p, bc=p, dc=p, n=1, opts=0, view=p, vres=p, vbc=p, res=p)

    def call(c=ctx, **kw):
        a = dict(ok, **kw)
        return lib.xyws_deflate_streams(c, a["tin"], a["tres"], a["bc"], a["dc"], a["n"], a["opts"], a["view"], a["vres"],
                                        a["vbc"], a["res"], None)

    assert call(c=None) == -1 and call(c=None, n=0) == -1
    for name in ("tin", "tres", "bc", "dc", "view", "vres", "vbc"):
        assert call(**{name: None}) == -1, name
    assert call(opts=1) == -1 and call(n=0, opts=0x80000000) == -1
    assert call(n=0xFFFFFFFF) == -1 and call(n=1 << 40) == -1
    assert call(n=0) == 0 and call(n=0, tin=None, tres=None, bc=None, dc=None, view=None, vres=None, vbc=None, res=None) == 0

    okb = dict(tin=p, tres=p, bc=p, n=1, rooms=p, rres=p, nr=1, flags=0x11, enc=0, res=p, view=p, vres=p, vbc=p, dc=p, zr=p, zres=p)

    def bcast(c=ctx, **kw):
        a = dict(okb, **kw)
        return lib.xyws_broadcast_deflated_streams(c, a["tin"], a["tres"], a["bc"], a["n"], a["rooms"], a["rres"], a["nr"],
                                                   a["flags"], a["enc"], a["res"], a["view"], a["vres"], a["vbc"], a["dc"],
                                                   a["zr"], a["zres"], None)

    assert bcast(c=None) == -1
    for name in ("tin", "tres", "bc", "rooms", "rres", "view", "vres", "vbc", "dc", "zr", "zres"):
        assert bcast(**{name: None}) == -1, name
    assert bcast(flags=0x11 | L.FLAG_RSV1) == -1 and bcast(flags=0x31) == -1 and bcast(enc=2) == -1 and bcast(n=0xFFFFFFFF) == -1
    assert bcast(n=0, flags=0x51) == -1 and bcast(n=0) == 0 and bcast(n=0, nr=0, zr=None, zres=None, rooms=None, rres=None) == 0

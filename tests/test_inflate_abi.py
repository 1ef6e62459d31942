"""CPU checks of xyws_inflate_streams' boundary: the three rows' sizes and offsets as the header states them, and
every refusal decided on the arguments alone, before the context is used (no device)."""
import ctypes as C

import pytest

import xynet_amd._lib as L

LAYOUT = {
    L.InflateConn: (64, dict(out=0, out_cap=8, vmsgs=16, vmsg_cap=24, ic=32, flags=40, reserved0=44, reserved=48)),
    L.InflateCarry: (32, dict(flags=0, hdr0=4, reserved0=5, reserved=8)),
    L.InflateResult: (32, dict(out_len=0, n_inflated=8, n_bad=12, status=16, reserved0=20, reserved=24)),
}


@pytest.mark.parametrize("struct", LAYOUT, ids=lambda s: s.__name__)
def test_row_layout(struct):
    size, offs = LAYOUT[struct]
    assert C.sizeof(struct) == size and {n: getattr(struct, n).offset for n, _ in struct._fields_} == offs


def test_symbols_and_geometry():
    assert "xyws_inflate_streams" in L.declared_symbols()
    g = (C.c_uint64 * 4)()
    assert L.load().xyws_debug_inflate_geometry(g) == 0 and L.load().xyws_debug_inflate_geometry(None) == -1
    assert g[0] == 64 and g[1] == 32768 and g[1] < g[2] <= 160 * 1024 // 4 and g[3] == 1024  # four waves' LDS per CU


def test_refusals_without_a_device():
    lib = L.load()
    fake = C.create_string_buffer(4096)
    ctx = p = C.cast(fake, C.c_void_p)
    ok = dict(conns=p, tin=p, tres=p, hold=p, ic=p, n=1, opts=0, view=p, vres=p, res=p)

    def call(c=ctx, **kw):
        a = dict(ok, **kw)
        return lib.xyws_inflate_streams(c, a["conns"], a["tin"], a["tres"], a["hold"], a["ic"], a["n"], a["opts"], a["view"],
                                        a["vres"], a["res"], None)

    assert call(c=None) == -1 and call(c=None, n=0) == -1
    for name in ("conns", "tin", "tres", "ic", "view", "vres"):
        assert call(**{name: None}) == -1, name
    assert call(opts=2) == -1 and call(opts=0x80000001) == -1 and call(n=0, opts=2) == -1
    assert call(n=0xFFFFFFFF) == -1 and call(n=1 << 40) == -1
    # n == 0: OK and nothing launched, whatever the tables (the fake context is never used)
    assert call(n=0) == 0 and call(n=0, opts=1, conns=None, tin=None, tres=None, hold=None, ic=None, view=None, vres=None,
                                   res=None) == 0

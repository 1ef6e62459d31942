"""xyws_deflate_windows_streams' boundary on the CPU: its rows, the geometry, the refusals decided on the arguments alone."""
import ctypes as C

import pytest

import xynet_amd._lib as L

LAYOUT = {
    L.DeflateRoomCarry: dict(hist_len=0, n_sweeps=8, flags=16, reserved0=20, reserved=24),
    L.DeflateRoom: dict(text=0, text_cap=8, carry=16, reserved=24),
    L.DeflateRoomResult: dict(text_len=0, n_records=8, n_history=12, status=16, reserved0=20, reserved=24),
}


@pytest.mark.parametrize("struct", LAYOUT, ids=lambda s: s.__name__)
def test_row_layout(struct):
    assert C.sizeof(struct) == 32 and {n: getattr(struct, n).offset for n, _ in struct._fields_} == LAYOUT[struct]


def test_symbol_and_geometry():
    assert "xyws_deflate_windows_streams" in L.declared_symbols()
    assert (L.DFR_RESET, L.DFR_TEXT_CAP, L.DFR_DESYNC, L.ACC_DEFLATE_SERVER_TAKEOVER, L.ACC_SERVER_TAKEOVER) == (1, 2, 4, 0x800, 0x20)
    g, lib = (C.c_uint64 * 6)(), L.load()
    assert lib.xyws_debug_deflate_windows_geometry(g) == 0 and lib.xyws_debug_deflate_windows_geometry(None) == -1
    W, hist, slots, cap, wave, window = g
    assert wave == 64 and W % 16 == 0 and slots & (slots - 1) == 0 and window == L.DFL_WINDOW == 32768
    assert hist % 16 == 0 and 0 < hist and hist + W <= window  # every distance is one the inflater's window holds
    assert cap % 256 == 0 and cap // 256 * (hist + W + 4 * slots + W * 9 // 8) <= 160 * 1024  # a CU's waves fit its LDS


def test_refusals_without_a_device():
    lib, ctx = L.load(), (p := C.cast(C.create_string_buffer(4096), C.c_void_p))
    ok = dict(tin=p, tres=p, bc=p, dc=p, n=1, rooms=p, dr=p, ro=None, nr=1, opts=0, view=p, vres=p, vbc=p, res=None, drres=p)

    def call(c=ctx, **kw):
        a = dict(ok, **kw)
        return lib.xyws_deflate_windows_streams(c, a["tin"], a["tres"], a["bc"], a["dc"], a["n"], a["rooms"], a["dr"], a["ro"],
                                                a["nr"], a["opts"], a["view"], a["vres"], a["vbc"], a["res"], a["drres"], None)

    assert call(c=None) == -1 and call(c=None, n=0) == -1
    for name in ("tin", "tres", "bc", "dc", "view", "vres", "vbc", "rooms", "dr", "drres"):
        assert call(**{name: None}) == -1, name
    assert call(opts=L.DFO_DYNAMIC) == -1 and call(opts=1) == -1 and call(n=0, opts=L.DFO_DYNAMIC) == -1
    assert call(n=0xFFFFFFFF) == -1 and call(nr=0xFFFFFFFF) == -1 and call(n=0, nr=1 << 40) == -1
    assert call(n=0) == 0 and call(n=0, ro=p) == 0
    assert call(n=0, nr=0, tin=None, tres=None, bc=None, dc=None, view=None, vres=None, vbc=None, rooms=None, dr=None, drres=None) == 0

"""CPU checks of the boundary of xyws_unsent_streams and xyws_unsent_view_streams:
declared in include/xyws.h and exported, the debug symbol exported and not
declared, row sizes, offsets and values as the header states them, and every
refusal given on the arguments alone, without a device."""
import ctypes as C

import unsent_model as M
import xynet_amd._lib as L
from test_outbox_abi import exported, header_fields, offsets


def test_declared_and_exported():
    names = {"xyws_unsent_streams", "xyws_unsent_view_streams", "xyws_unsent_scratch_bytes"}
    assert names <= set(L.declared_symbols())
    assert names | {"xyws_debug_unsent_geometry"} <= exported()
    assert "xyws_debug_unsent_geometry" not in L.declared_symbols()


def test_rows_match_the_header():
    want = {
        L.UnsentConn: ("xyws_unsent_conn", 32, {"out": 0, "pend_cap": 8, "carry": 16, "reserved": 24}),
        L.UnsentCarry: ("xyws_unsent_carry", 32, {"pend_len": 0, "last_len": 8, "sweep": 16, "flags": 20, "reserved": 24}),
        L.UnsentReport: ("xyws_unsent_report", 8, {"sent": 0, "sweep": 4}),
        L.UnsentHead: ("xyws_unsent_head", 16, {"sweep": 0, "reserved0": 4, "reserved": 8}),
        L.UnsentResult: ("xyws_unsent_result", 32, {"pend_len": 0, "moved": 8, "status": 16, "reserved0": 20, "reserved": 24}),
    }
    for cls, (name, size, offs) in want.items():
        assert C.sizeof(cls) == size and offsets(cls) == offs, name
        assert [f[0] for f in cls._fields_] == header_fields(name), name
    src = open(L.HEADER).read()
    for name, val, model in (("KEPT", L.US_KEPT, M.KEPT), ("OVERFLOW", L.US_OVERFLOW, M.OVERFLOW),
                             ("BAD_REPORT", L.US_BAD_REPORT, M.BAD_REPORT)):
        assert "#define XYWS_US_%s" % name in src and val == model, name
        assert int(src.split("#define XYWS_US_%s" % name)[1].split("u")[0], 0) == val, name


def test_geometry_and_scratch_without_a_device():
    lib = L.load()
    g = (C.c_uint64 * 4)()
    assert lib.xyws_debug_unsent_geometry(None) == -1 and lib.xyws_debug_unsent_geometry(g) == 0
    tile, step, waves, record = g
    assert tile == 64 * waves and step == 16 * 64 and record % 8 == 0
    assert lib.xyws_unsent_scratch_bytes(0) == 0
    assert [lib.xyws_unsent_scratch_bytes(n) for n in (1, tile, tile + 1)] == [record, record * tile, record * (tile + 1)]


def test_refusals_without_a_device():
    """A placeholder context (never dereferenced) gets the same answers on a host without a GPU."""
    lib = L.load()
    fake = C.create_string_buffer(4096)
    ctx = p = C.c_void_p(C.addressof(fake))
    need = lib.xyws_unsent_scratch_bytes(3)
    ok = dict(c=ctx, uconns=p, n=3, reports=p, head=p, results=p, scratch=p, sb=need)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.xyws_unsent_streams(a["c"], a["uconns"], a["n"], a["reports"], a["head"], a["results"], a["scratch"],
                                       a["sb"], None)

    assert call(c=None) == -1 and call(c=None, n=0) == -1
    assert call(uconns=None) == -1 and call(head=None) == -1 and call(scratch=None) == -1
    assert call(sb=need - 1) == -1 and call(sb=0) == -1
    assert call(n=0xFFFFFFFF, sb=1 << 62) == -1 and call(n=1 << 32, sb=1 << 62) == -1
    assert call(n=0, sb=0) == 0 and call(n=0, uconns=None, reports=None, head=None, results=None, scratch=None, sb=0) == 0

    def view(c=ctx, uconns=p, conns=p, n=3, out=p, rows=p):
        return lib.xyws_unsent_view_streams(c, uconns, conns, n, out, rows, None)

    assert view(c=None) == -1 and view(c=None, n=0) == -1
    assert view(uconns=None) == -1 and view(conns=None) == -1 and view(out=None) == -1 and view(rows=None) == -1
    assert view(n=0xFFFFFFFF) == -1 and view(n=1 << 32) == -1
    assert view(n=0) == 0 and view(n=0, uconns=None, conns=None, out=None, rows=None) == 0

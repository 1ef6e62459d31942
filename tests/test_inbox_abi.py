"""CPU checks of xyws_inbox_streams' boundary: declared in include/xyws.h and
exported, struct layouts and values as the header states them, the kernels'
geometry readable, every refusal given without a device, and the scratch size
monotone and 8-aligned."""
import ctypes as C
import re

import inbox_model as M
import xynet_amd._lib as L
from test_outbox_abi import exported, header_fields, offsets


def test_declared_and_exported():
    names = {"xyws_inbox_streams", "xyws_inbox_scratch_bytes"}
    assert names <= set(L.declared_symbols())
    lib = L.load()
    internal = {"xyws_debug_inbox_geometry", "xyws_debug_inbox_host_scatter"}
    assert names | internal <= exported()
    assert lib.xyws_abi_version() == 2
    assert not internal & set(L.declared_symbols())


def test_struct_layouts_and_values_match_header():
    sizes = {L.InboxHead: 32, L.InboxEntry: 32, L.InboxCarry: 32, L.InboxConn: 64, L.InboxResult: 32, L.InboxSummary: 64}
    for cls, size in sizes.items():
        assert C.sizeof(cls) == size, cls
    assert offsets(L.InboxHead) == {"m": 0, "pack_len": 8, "reserved": 16}
    assert offsets(L.InboxEntry) == {"conn": 0, "flags": 4, "off": 8, "len": 16, "at": 24}
    assert offsets(L.InboxCarry) == {"http_len": 0, "bytes_total": 8, "state": 16, "status": 20, "reserved": 24}
    assert offsets(L.InboxConn) == {"buf": 0, "cap": 8, "carry": 16, "conn": 24, "aconn": 32, "aresult": 40, "flags": 48,
                                    "reserved0": 52, "reserved": 56}
    assert offsets(L.InboxResult) == {"len": 0, "lead": 8, "n_entries": 16, "status": 20, "reserved": 24}
    assert offsets(L.InboxSummary) == {"n_entries": 0, "bytes": 8, "n_conns": 16, "n_opened": 20, "n_eof": 24,
                                       "n_broken": 28, "n_bad_entries": 32, "status": 36, "reserved": 40}
    for cls, name in ((L.InboxHead, "xyws_inbox_head"), (L.InboxEntry, "xyws_inbox_entry"),
                      (L.InboxCarry, "xyws_inbox_carry"), (L.InboxConn, "xyws_inbox_conn"),
                      (L.InboxResult, "xyws_inbox_result"), (L.InboxSummary, "xyws_inbox_summary")):
        assert [f[0] for f in cls._fields_] == header_fields(name), name
    src = open(L.HEADER).read()

    def define(name):
        return int(re.search(r"#define %s\s+(0x[0-9a-fA-F]+|\d+)u?\b" % name, src).group(1), 0)

    for name, val, model in (
            ("IBE_EOF", L.IBE_EOF, M.EOF_E), ("IBC_NO_HANDSHAKE", L.IBC_NO_HANDSHAKE, M.NO_HANDSHAKE),
            ("IB_HTTP", L.IB_HTTP, M.HTTP), ("IB_OPEN", L.IB_OPEN, M.OPEN), ("IB_DEAD", L.IB_DEAD, M.DEAD),
            ("IBR_EOF", L.IBR_EOF, M.R_EOF), ("IBR_DROPPED", L.IBR_DROPPED, M.R_DROPPED),
            ("IBR_REFUSED", L.IBR_REFUSED, M.R_REFUSED), ("IBR_BAD_TILING", L.IBR_BAD_TILING, M.R_BAD_TILING),
            ("IBR_OVERFLOW", L.IBR_OVERFLOW, M.R_OVERFLOW), ("IBR_BAD_RANGE", L.IBR_BAD_RANGE, M.R_BAD_RANGE),
            ("IBR_BAD_CONSUMED", L.IBR_BAD_CONSUMED, M.R_BAD_CONSUMED), ("IBR_OPENED", L.IBR_OPENED, M.R_OPENED),
            ("IBM_BAD_ENTRIES", L.IBM_BAD_ENTRIES, M.S_BAD_ENTRIES), ("IBM_BROKEN", L.IBM_BROKEN, M.S_BROKEN),
            ("IBM_CLIPPED", L.IBM_CLIPPED, M.S_CLIPPED), ("ACC_ACCEPTED", L.ACC_ACCEPTED, M.ACC_ACCEPTED),
            ("ACC_REJECTED", L.ACC_REJECTED, M.ACC_REJECTED)):
        assert define("XYWS_" + name) == val == model, name
    assert len(re.findall(r"#define (XYWS_IB[ERCM]?_\w+)", src)) == 16
    # the sticky bits of the model are those the header calls sticky
    sticky = 0
    for name in re.findall(r"#define (XYWS_IBR_\w+)\s+\S+\s*/\* sticky", src):
        sticky |= define(name)
    assert sticky == M.STICKY


def geometry():
    g = (C.c_uint64 * 5)()
    assert L.load().xyws_debug_inbox_geometry(g) == 0
    return tuple(g)


def test_geometry_without_a_device():
    assert L.load().xyws_debug_inbox_geometry(None) == -1
    tile, step, gx, gy, ge = geometry()
    assert tile % 64 == 0 and 64 <= tile <= 1024     # whole waves, one workgroup
    assert step % 16 == 0 and step == 1024           # one wave per 1 KiB chunk
    assert 256 <= gx <= 65536 and 1 <= gy <= 65535 and 1 <= ge <= 65536


def test_scratch_bytes_monotone_and_aligned():
    lib = L.load()
    tile = geometry()[0]
    prev = 0
    for n in list(range(0, 2 * tile + 3)) + [16384, 1 << 20, (1 << 32) - 2]:
        b = lib.xyws_inbox_scratch_bytes(n, 0)
        assert b % 8 == 0 and b >= prev and b >= 32 * n, n
        prev = b
    prev = 0
    for m in list(range(0, 70)) + [16384, 1 << 20, (1 << 32) - 2]:
        b = lib.xyws_inbox_scratch_bytes(7, m)
        assert b % 8 == 0 and b >= prev and b >= 32 * m, m
        prev = b
    assert lib.xyws_inbox_scratch_bytes(tile + 1, 5) > lib.xyws_inbox_scratch_bytes(tile, 5) > 0
    assert lib.xyws_inbox_scratch_bytes(5, 6) > lib.xyws_inbox_scratch_bytes(5, 5)


def test_streams_refusals_without_a_device():
    """Every refusal is decided on the arguments alone, before the context is
    used: a placeholder context (never dereferenced) gets the same answers on
    a host without a GPU."""
    lib = L.load()
    fake = C.create_string_buffer(4096 + 16)
    ctx = p = C.c_void_p((C.addressof(fake) + 15) & ~15)
    need = lib.xyws_inbox_scratch_bytes(1, 4)
    ok = dict(iconns=p, n=1, head=p, entries=p, m_cap=4, pack=p, pack_cap=64, results=p, summary=p, scratch=p, sb=need)

    def call(c=ctx, **kw):
        a = dict(ok, **kw)
        return lib.xyws_inbox_streams(c, a["iconns"], a["n"], a["head"], a["entries"], a["m_cap"], a["pack"],
                                      a["pack_cap"], a["results"], a["summary"], a["scratch"], a["sb"], None)

    assert call(c=None) == -1 and call(c=None, n=0, sb=0) == -1
    assert call(iconns=None) == -1 and call(head=None) == -1 and call(summary=None) == -1
    assert call(scratch=None) == -1
    assert call(entries=None) == -1 and call(entries=None, n=0) == -1
    assert call(pack=None) == -1 and call(pack=None, n=0) == -1
    assert call(sb=need - 1) == -1 and call(sb=0) == -1
    assert call(m_cap=5) == -1 and call(n=2) == -1
    for k in range(1, 8):   # (64-bit atomics: the scratch is 8-byte aligned)
        assert call(scratch=C.c_void_p(p.value + k), sb=need + 64) == -1, k
    assert call(scratch=C.c_void_p(p.value + 3), n=0, sb=0) == 0
    assert call(n=0xFFFFFFFF, sb=1 << 62) == -1 and call(n=1 << 32, sb=1 << 62) == -1
    assert call(m_cap=0xFFFFFFFF, sb=1 << 62) == -1 and call(m_cap=1 << 32, sb=1 << 62) == -1
    # n == 0: OK and nothing launched, whatever the tables (no device needed)
    assert call(n=0, sb=0) == 0
    assert call(n=0, iconns=None, head=None, entries=None, m_cap=0, pack=None, pack_cap=0, results=None, summary=None,
                scratch=None, sb=0) == 0

"""CPU checks of xyws_outbox_streams' boundary: declared in include/xyws.h and
exported, struct layouts and values as the header states them, the kernels'
geometry readable, every refusal given without a device, and the scratch size
monotone and 8-aligned."""
import ctypes as C
import re
import subprocess

import outbox_model as M
import xynet_amd._lib as L


def exported():
    out = subprocess.run(["nm", "-D", "--defined-only", L.lib_path()], capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_declared_and_exported():
    names = {"xyws_outbox_streams", "xyws_outbox_scratch_bytes", "xyws_outbox_map", "xyws_notifier_enqueue"}
    assert names <= set(L.declared_symbols())
    lib = L.load()
    internal = {"xyws_debug_outbox_geometry", "xyws_debug_outbox_host_fetch"}
    assert names | internal <= exported()
    assert lib.xyws_abi_version() == 2
    assert not internal & set(L.declared_symbols())


def offsets(cls):
    return {f[0]: getattr(cls, f[0]).offset for f in cls._fields_}


def header_fields(name):
    src = open(L.HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for d in body.split(";"):
        if d.strip():  # `uint32_t a, b, c` declares three
            names += [re.search(r"(\w+)(\[\d+\])?\s*$", part.strip()).group(1) for part in d.split(",")]
    return names


def test_struct_layouts_and_values_match_header():
    assert (C.sizeof(L.OutboxConn), C.sizeof(L.OutboxEntry), C.sizeof(L.OutboxSummary)) == (64, 32, 64)
    assert offsets(L.OutboxConn) == {"out": 0, "out_cap": 8, "backlog": 16, "bcast": 24, "reply": 32, "accept": 40,
                                     "reserved": 48}
    assert offsets(L.OutboxEntry) == {"conn": 0, "flags": 4, "off": 8, "len": 16, "full_len": 24}
    assert offsets(L.OutboxSummary) == {"n_entries": 0, "pack_len": 8, "packed_len": 16, "send_bytes": 24, "n_close": 32,
                                        "n_truncated": 36, "n_deferred": 40, "status": 44, "reserved": 48}
    for cls, name in ((L.OutboxConn, "xyws_outbox_conn"), (L.OutboxEntry, "xyws_outbox_entry"),
                      (L.OutboxSummary, "xyws_outbox_summary")):
        assert [f[0] for f in cls._fields_] == header_fields(name), name
    src = open(L.HEADER).read()

    def define(name):
        return int(re.search(r"#define %s\s+(0x[0-9a-fA-F]+|\d+)u?\b" % name, src).group(1), 0)

    for name, val, model in (("OB_CLOSE", L.OB_CLOSE, M.CLOSE), ("OB_OVERFLOW", L.OB_OVERFLOW, M.OVERFLOW),
                             ("OB_TRUNCATED", L.OB_TRUNCATED, M.TRUNCATED), ("OB_DEFERRED", L.OB_DEFERRED, M.DEFERRED),
                             ("OBS_DEFERRED", L.OBS_DEFERRED, M.S_DEFERRED),
                             ("OBS_TRUNCATED", L.OBS_TRUNCATED, M.S_TRUNCATED),
                             ("RPL_CLOSED", L.RPL_CLOSED, M.RPL_CLOSED), ("RPL_OVERFLOW", L.RPL_OVERFLOW, M.RPL_OVERFLOW),
                             ("ACC_ACCEPTED", L.ACC_ACCEPTED, M.ACC_ACCEPTED),
                             ("ACC_REJECTED", L.ACC_REJECTED, M.ACC_REJECTED)):
        assert define("XYWS_" + name) == val == model, name
    assert sorted(re.findall(r"#define (XYWS_OBS?_\w+)", src)) == [
        "XYWS_OBS_DEFERRED", "XYWS_OBS_TRUNCATED", "XYWS_OB_CLOSE", "XYWS_OB_DEFERRED", "XYWS_OB_OVERFLOW",
        "XYWS_OB_TRUNCATED"]


def geometry():
    g = (C.c_uint64 * 4)()
    assert L.load().xyws_debug_outbox_geometry(g) == 0
    return tuple(g)


def test_geometry_without_a_device():
    assert L.load().xyws_debug_outbox_geometry(None) == -1
    tile, step, gx, gy = geometry()
    assert tile % 64 == 0 and 64 <= tile <= 1024     # whole waves, one workgroup
    assert step % 16 == 0 and 16 <= step <= 16384    # whole lines
    assert 256 <= gx <= 65536 and 1 <= gy <= 65535


def test_scratch_bytes_monotone_and_aligned():
    lib = L.load()
    tile = geometry()[0]
    assert lib.xyws_outbox_scratch_bytes(0) == 0
    prev = 0
    for n in list(range(1, 3 * tile + 3)) + [16384, 1 << 20, (1 << 32) - 2]:
        b = lib.xyws_outbox_scratch_bytes(n)
        assert b % 8 == 0 and b >= prev and b >= 8 * n, n
        prev = b
    assert lib.xyws_outbox_scratch_bytes(tile + 1) > lib.xyws_outbox_scratch_bytes(tile) > 0


def test_streams_refusals_without_a_device():
    """Every refusal is decided on the arguments alone, before the context is
    used: a placeholder context (never dereferenced) gets the same answers on
    a host without a GPU."""
    lib = L.load()
    fake = C.create_string_buffer(4096 + 16)
    base = (C.addressof(fake) + 15) & ~15
    ctx = p = C.c_void_p(base)
    need = lib.xyws_outbox_scratch_bytes(1)
    ok = dict(conns=p, n=1, pack=p, cap=64, entries=p, summary=p, scratch=p, sb=need)

    def call(c=ctx, **kw):
        a = dict(ok, **kw)
        return lib.xyws_outbox_streams(c, a["conns"], a["n"], a["pack"], a["cap"], a["entries"], a["summary"],
                                       a["scratch"], a["sb"], None)

    assert call(c=None) == -1 and call(c=None, n=0, sb=0) == -1
    assert call(conns=None) == -1 and call(entries=None) == -1 and call(summary=None) == -1
    assert call(scratch=None) == -1
    assert call(sb=need - 1) == -1 and call(sb=0) == -1
    assert call(n=5, sb=lib.xyws_outbox_scratch_bytes(5) - 1) == -1
    for k in range(1, 16):
        assert call(pack=C.c_void_p(base + k)) == -1, k
        assert call(pack=C.c_void_p(base + k), n=0) == -1, k
    assert call(n=0xFFFFFFFF, sb=1 << 62) == -1 and call(n=1 << 32, sb=1 << 62) == -1
    # n == 0: OK and nothing launched, whatever the tables (no device needed)
    assert call(n=0, sb=0) == 0
    assert call(n=0, conns=None, entries=None, summary=None, scratch=None, pack=None, cap=0, sb=0) == 0


def test_map_refusals_without_a_device():
    lib = L.load()
    d = C.c_void_p(0x1234)
    assert lib.xyws_outbox_map(None, C.byref(d)) == -1 and d.value is None
    assert lib.xyws_outbox_map(C.c_void_p(0x1000), None) == -1
    # plain host memory is not mapped for any device: refused, and no address comes back
    buf = C.create_string_buffer(64)
    d = C.c_void_p(0x1234)
    assert lib.xyws_outbox_map(C.cast(buf, C.c_void_p), C.byref(d)) == -1 and d.value is None


def test_notifier_enqueue_refuses_a_null_notifier():
    assert L.load().xyws_notifier_enqueue(None, 0, None) == -1

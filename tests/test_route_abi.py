"""CPU checks of xyws_route_streams' boundary: declared in include/xyws.h and
exported, struct layouts and values as the header states them, the kernel's
geometry readable, every refusal of xyws_route_build and xyws_route_streams
given without a device, and xyws_route_lookup (the kernel's lookup compiled for
the host) equal to the Python model on every case of tests/route_cases.py, for
the table size the library chooses and for the smallest it takes."""
import ctypes as C
import re
import subprocess

import pytest

import route_cases as RC
import route_model as M
import xynet_amd._lib as L
from xynet_amd import websocket as W

GUARD = 0xA5


def exported():
    out = subprocess.run(["nm", "-D", "--defined-only", L.lib_path()], capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_declared_and_exported():
    names = {"xyws_route_build", "xyws_route_lookup", "xyws_route_streams"}
    assert names <= set(L.declared_symbols())
    lib = L.load()
    internal = {"xyws_debug_route_geometry", "xyws_debug_route_home", "xyws_debug_route_host"}
    assert names | internal <= exported()
    assert lib.xyws_abi_version() == 2
    assert not internal & set(L.declared_symbols())


def offsets(cls):
    return {f[0]: getattr(cls, f[0]).offset for f in cls._fields_}


def header_fields(name):
    src = open(L.HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.search(r"(\w+)(\[\d+\])?\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]


def test_struct_layouts_and_values_match_header():
    assert (C.sizeof(L.Route), C.sizeof(L.RouteConn), C.sizeof(L.RouteResult)) == (24, 8, 32)
    assert offsets(L.Route) == {"key": 0, "key_len": 8, "room": 12, "flags": 16, "reserved": 20}
    assert offsets(L.RouteConn) == {"rconn": 0, "reserved": 4}
    assert offsets(L.RouteResult) == {"status": 0, "room": 4, "route": 8, "key_off": 12, "key_len": 16, "reserved": 20}
    for cls, name in ((L.Route, "xyws_route"), (L.RouteConn, "xyws_route_conn"), (L.RouteResult, "xyws_route_result")):
        assert [f[0] for f in cls._fields_] == header_fields(name), name
    src = open(L.HEADER).read()

    def define(name):
        return int(re.search(r"#define %s\s+(0x[0-9a-fA-F]+|\d+)u?\b" % name, src).group(1), 0)

    for name, val, model in (("MATCHED", L.RT_MATCHED, M.MATCHED), ("BY_PREFIX", L.RT_BY_PREFIX, M.BY_PREFIX),
                             ("MISS", L.RT_MISS, M.MISS), ("NOT_FOUND", L.RT_NOT_FOUND, M.NOT_FOUND),
                             ("NOT_ACCEPTED", L.RT_NOT_ACCEPTED, M.NOT_ACCEPTED), ("BAD_ROW", L.RT_BAD_ROW, M.BAD_ROW),
                             ("BAD_TABLE", L.RT_BAD_TABLE, M.BAD_TABLE), ("MISS_404", L.RT_MISS_404, M.MISS_404)):
        assert define("XYWS_RT_" + name) == val == model, name
    assert define("XYWS_ROUTE_KEY_MAX") == L.ROUTE_KEY_MAX == M.KEY_MAX == 256
    assert define("XYWS_ROUTE_PREFIX") == L.ROUTE_PREFIX == M.PREFIX == 1
    assert define("XYWS_ACR_NOT_FOUND") == L.ACR_NOT_FOUND == M.R_NOT_FOUND == 11
    assert re.search(r"#define XYWS_ROUTE_NO_ROW\s+UINT32_MAX", src) and L.ROUTE_NO_ROW == M.NO_ROW == 0xFFFFFFFF
    assert L.ROOM_NONE == M.ROOM_NONE


def test_geometry_without_a_device():
    lib = L.load()
    assert lib.xyws_debug_route_geometry(None) == -1
    g = (C.c_uint64 * 4)()
    assert lib.xyws_debug_route_geometry(g) == 0
    lanes, step, stage, grid = g
    assert lanes == 64 and lanes * step == M.KEY_MAX  # one wave per connection, every byte of the key window on a lane
    assert 15 + M.WINDOW <= stage <= 17 * 16          # the window at any alignment: at most 17 lines
    assert 256 <= grid <= 65536


def routes_of(triples):
    rows = (L.Route * max(len(triples), 1))()
    keep = [C.create_string_buffer(k, max(len(k), 1)) for k, _, _ in triples]
    for row, buf, (k, room, flags) in zip(rows, keep, triples):
        row.key, row.key_len, row.room, row.flags = C.addressof(buf), len(k), room, flags
    return rows, keep


def build(triples, slots=0, cap=None, table=True):
    lib = L.load()
    rows, keep = routes_of(triples)
    need = C.c_uint64(0x1234)
    blob = C.create_string_buffer(1 << 16)
    rc = lib.xyws_route_build(rows, len(triples), slots, blob if table else None, (1 << 16) if cap is None else cap,
                              C.byref(need))
    return rc, need.value, blob.raw[:need.value]


def test_build_refusals_and_need():
    two = [(b"/a", 0, 0), (b"/b", 1, 0)]
    for bad in ([(b"", 0, 0)], [(b"/" + b"x" * 256, 0, 0)], [(b"/a?b", 0, 0)], [(b"#", 0, 0)],
                [(b"/a", 0, 0), (b"/a/", 1, L.ROUTE_PREFIX)], [(b"/", 0, 0), (b"/", 1, 0)], [(b"/a", 0, 2)],
                [(b"/a", 0, 0x80000000)]):
        assert build(bad) == (-1, 0, b""), bad
        with pytest.raises(ValueError):
            M.table(bad)
    for slots in (3, 1, 2, 6, 0x80000001):
        assert build(two, slots)[:2] == (-1, 0)
    lib = L.load()
    need = C.c_uint64(7)
    assert lib.xyws_route_build(None, 1, 0, None, 0, C.byref(need)) == -1 and need.value == 0
    rows, keep = routes_of(two)
    rows[1].key = None
    assert lib.xyws_route_build(rows, 2, 0, None, 0, C.byref(need)) == -1
    # need is written whatever cap; nothing else is when it does not suffice
    rc, need4, blob = build(two, 4)
    assert rc == 0 and need4 == len(blob) > 0
    assert build(two, 4, cap=0)[:2] == (-4, need4) and build(two, 4, cap=need4 - 1)[:2] == (-4, need4)
    assert build(two, 4, cap=need4)[0] == 0
    assert build(two, 4, table=False)[0] == -1           # room enough, and nowhere to put it
    assert build(two, 4, cap=0, table=False)[:2] == (-4, need4)
    assert lib.xyws_route_build(routes_of(two)[0], 2, 4, None, 0, None) == -4  # need is nullable
    assert build(two, 8)[1] > need4 and build(two, 0)[0] == 0
    assert build([], 0)[0] == 0 and build([], 1)[0] == 0 and build([], 3)[0] == -1
    # the blob begins with a magic and a version word and holds no pointer: two builds are equal bytes
    assert blob[:4] == b"XYRT" and int.from_bytes(blob[4:8], "little") == 1
    assert build(two, 4)[2] == blob


def test_streams_refusals_without_a_device():
    """Every refusal is decided on the arguments alone, before the context is
    used: a placeholder context (never dereferenced) gets the same answers on
    a host without a GPU."""
    lib = L.load()
    fake = C.create_string_buffer(4096)
    ctx, p = C.cast(fake, C.c_void_p), C.cast(fake, C.c_void_p)
    ok = dict(ac=p, ar=p, rt=p, n=1, tab=p, tl=64, rc=p, nrc=1, dflt=0, policy=0, res=None)

    def call(c=ctx, **kw):
        a = dict(ok, **kw)
        return lib.xyws_route_streams(c, a["ac"], a["ar"], a["rt"], a["n"], a["tab"], a["tl"], a["rc"], a["nrc"],
                                      a["dflt"], a["policy"], a["res"], None)

    assert call(c=None) == -1 and call(c=None, n=0) == -1
    assert call(ac=None) == -1 and call(ar=None) == -1 and call(rt=None) == -1
    assert call(tab=None) == -1 and call(rc=None) == -1
    assert call(policy=2) == -1 and call(policy=0x80000001) == -1
    assert call(n=0, tab=None) == -1 and call(n=0, rc=None) == -1 and call(n=0, policy=4) == -1
    # n == 0: OK and nothing launched, whatever the tables (no device needed)
    assert call(n=0, ac=None, ar=None, rt=None) == 0
    assert call(n=0, ac=None, ar=None, rt=None, tab=None, tl=0, rc=None, nrc=0, policy=L.RT_MISS_404, res=p) == 0
    # the host call
    r = L.RouteResult()
    assert lib.xyws_route_lookup(None, 1, b"/", 1, C.byref(r)) == -1
    assert lib.xyws_route_lookup(None, 0, None, 1, C.byref(r)) == -1
    assert lib.xyws_route_lookup(None, 0, b"/", 1, None) == -1
    assert lib.xyws_route_lookup(None, 0, None, 0, C.byref(r)) == 0 and r.status == L.RT_MISS


def host_lookup(blob, target, length=None):
    lib = L.load()
    r = L.RouteResult()
    C.memset(C.byref(r), GUARD, 32)
    assert lib.xyws_route_lookup(blob, len(blob), target, len(target) if length is None else length, C.byref(r)) == 0
    return bytes(r)


@pytest.mark.parametrize("smallest", [False, True])
@pytest.mark.parametrize("name", list(RC.TABLES))
def test_host_lookup_equals_the_model_on_every_case(name, smallest):
    routes = RC.TABLES[name]
    tab = M.table(routes)
    blob = L.route_table_of(routes, RC.smallest_slots(len(routes)) if smallest else 0)
    for tname, target in RC.TARGETS:
        assert host_lookup(blob, target) == M.pack_result(M.lookup(tab, target)), (name, tname)
        # (the bytes behind len stay in the buffer: nothing behind it may change the answer)
        for k in (0, 1, len(target) // 2):
            assert host_lookup(blob, target, k) == M.pack_result(M.lookup(tab, target[:k])), (name, tname, k)
    # no table at all, and bytes that are none
    for tname, target in RC.TARGETS[:8]:
        assert host_lookup(b"", target) == M.pack_result(M.lookup(None, target))
        for bad in (blob[:31], blob[:-1], b"\0" + blob[1:], blob[:4] + b"\2" + blob[5:], blob + b"\0"):
            assert host_lookup(bad, target) == M.pack_result(M.lookup(tab, target, bad_table=True)), tname


def test_long_chains_and_random_keys():
    lib = L.load()
    keys = RC.random_keys(300)
    routes = [(k, i, L.ROUTE_PREFIX if i % 3 == 0 else 0) for i, k in enumerate(keys)]
    tab = M.table(routes)
    for slots in (0, RC.smallest_slots(len(routes))):
        blob = L.route_table_of(routes, slots)
        for k in keys:
            for target in (k, k + b"/", k + b"/below?x", k + b"x", k[:-1]):
                assert host_lookup(blob, target) == M.pack_result(M.lookup(tab, target)), (slots, target)
    # 64 keys whose chains begin in one slot of the smallest table
    chain = [k for k in RC.random_keys(20000, seed=7) if lib.xyws_debug_route_home(k, len(k), 128) == 5][:64]
    assert len(chain) == 64
    blob = L.route_table_of([(k, i, 0) for i, k in enumerate(chain)], 128)
    for i, k in enumerate(chain):
        r = L.RouteResult.from_buffer_copy(host_lookup(blob, k))
        assert (r.status, r.room, r.route) == (L.RT_MATCHED, i, i)


def test_request_handler_get_room_and_table_helper():
    blob = L.route_table(exact={b"/chat": 4}, prefix={b"/rooms": 9})
    h = W.websocket_request_handler(policy=0)
    import accept_cases as AC
    assert h.parse(AC.RFC) == len(AC.RFC) and h.get_room(blob) == 4
    assert h.parse(AC.browser(path=b"/rooms/lobby?t=1")) > 0 and h.get_room(blob) == 9
    assert h.parse(AC.browser(path=b"/nope")) > 0 and h.get_room(blob) is None
    with pytest.raises(L.XywsError):
        L.route_table(exact={b"/a": 1}, prefix={b"/a/": 2})


SHIM_PROG = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "xyws/websocket.hpp"
static_assert(sizeof(xyws_route) == 24 && sizeof(xyws_route_conn) == 8 && sizeof(xyws_route_result) == 32);

int main(int argc, char** argv) {
  const xyws_route routes[] = {{"/chat", 5, 4, 0, 0}, {"/rooms/", 7, 9, XYWS_ROUTE_PREFIX, 0}};
  const std::vector<std::byte> blob = xyws::route_table(routes);
  for (int i = 1; i < argc; i++) {
    xyws_route_result r;
    if (xyws_route_lookup(blob.data(), blob.size(), argv[i], std::strlen(argv[i]), &r) != XYWS_OK) return 1;
    std::printf("%u %u %u %u\n", r.status, r.room, r.route, r.key_len);
  }
  try {
    const xyws_route twice[] = {{"/a", 2, 0, 0, 0}, {"/a/", 3, 1, 0, 0}};
    xyws::route_table(twice);
    return 2;
  } catch (const xyws::error& e) {
    std::printf("refused %d\n", e.code());
  }
  std::printf("smallest %zu chosen %zu\n", xyws::route_table(routes, 4).size(), blob.size());
  if (argc > 9) {  // (named, never run: the device call of the same shim)
    xyws::context ctx(0);
    xyws::route_streams(ctx, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, 0);
    xyws::route_streams(ctx, nullptr, nullptr, nullptr, 0, blob.data(), blob.size(), nullptr, 0, nullptr, 3,
                        XYWS_RT_MISS_404, nullptr);
  }
  return 0;
}
"""


def test_shim_builds_the_table(tmp_path):
    import os
    src = tmp_path / "shim.cpp"
    src.write_text(SHIM_PROG)
    exe = tmp_path / "shim"
    libdir = os.path.dirname(L.lib_path())
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    r = subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", inc, str(src), "-o", str(exe), "-L",
                        libdir, "-lxyws", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), "/chat?x", "/rooms/b/", "/nope"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    want = ["%d 4 0 5" % L.RT_MATCHED, "%d 9 1 8" % (L.RT_MATCHED | L.RT_BY_PREFIX),
            "%d %d %d 5" % (L.RT_MISS, L.ROOM_NONE, 0xFFFFFFFF), "refused -1"]
    lines = r.stdout.splitlines()
    assert lines[:4] == want
    smallest, chosen = (int(x) for x in lines[4].split()[1::2])
    assert smallest == 32 + 24 * 4 + 5 + 6 and chosen >= smallest

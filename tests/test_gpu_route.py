"""xyws_route_streams on the GPU against tests/route_model.py, bit-exact: the
route rows, the accept rows (rewritten for a 404, untouched otherwise), the
room words of the roster rows and every other byte of those rows, and every
byte of the send slab, guard bytes around the ranges included. The accept rows
and the 101s are the accept model's, as xyws_accept_streams leaves them; the
graph test and the connection_group test run the real chain."""
import ctypes as C

import numpy as np
import pytest

import accept_cases as AC
import accept_model as AM
import route_cases as RC
import route_model as M
from xynet_amd import _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
GUARD = 0xA5
POLICIES = [0, M.MISS_404]
DEFAULT_ROOM = 77
_ACCEPTED = {}


@pytest.fixture(scope="module")
def ws():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from xynet_amd import websocket
    return websocket


@pytest.fixture()
def ctx(ws):
    """A context of the test's own; the device error word must read 0 at the end."""
    c = ws.Context(0)
    yield c
    assert c.last_device_error() == 0
    c.close()


def geometry():
    out = (C.c_uint64 * 4)()
    assert _lib.load().xyws_debug_route_geometry(out) == 0
    return list(out)


def request(target):
    return AC.req(line=b"GET " + target + b" HTTP/1.1")


def accepted(req, out_cap):
    """The accept model's row and response for a whole request (cached: the reference is computed once)."""
    if (req, out_cap) not in _ACCEPTED:
        _ACCEPTED[req, out_cap] = AM.accept(req, 0, AM.MAX_REQUEST, out_cap)
    res, resp = _ACCEPTED[req, out_cap]
    return dict(res), resp


class Entry:
    """One connection of a launch: it sent req[:length] (the bytes behind are
    in the buffer and must not matter); ares: its accept row (default: the
    accept model's for req[:length]); its out range has out_cap bytes and holds
    what the accept wrote; rconn: the roster row it names."""

    def __init__(self, target=None, req=None, length=None, ares=None, out_cap=129, bmis=0, omis=0, abut=False, out=True,
                 rconn=None):
        self.req = request(target) if req is None else bytes(req)
        self.length = len(self.req) if length is None else length
        self.out_cap, self.bmis, self.omis, self.abut, self.out, self.rconn = out_cap, bmis, omis, abut, out, rconn
        res, self.resp = accepted(self.req[:self.length], out_cap)
        self.ares = res if ares is None else ares
        assert out or not out_cap


class Launch:
    """The tables and buffers of one xyws_route_streams call and the model's answer to every entry."""

    def __init__(self, entries, routes, policy=0, slots=0, default_room=DEFAULT_ROOM, results=True, n_rconns=None,
                 blob=None, bad_table=False, table_mis=0):
        self.entries, self.policy, self.default_room = entries, policy, default_room
        n = self.n = len(entries)
        self.n_rconns = n if n_rconns is None else n_rconns
        for k, e in enumerate(entries):
            if e.rconn is None:
                e.rconn = n - 1 - k  # (reversed: route row k names roster row n - 1 - k)
        tab = M.table(routes)
        blob = _lib.route_table_of(routes, slots) if blob is None else blob
        self.blob_image = np.concatenate([np.full(16 + table_mis, GUARD, np.uint8), np.frombuffer(blob, np.uint8),
                                          np.full(16, GUARD, np.uint8)])
        self.blob_t, self.blob_off, self.blob_len = torch.from_numpy(self.blob_image.copy()).cuda(), 16 + table_mis, len(blob)
        self.exp = [M.route(tab, e.req, e.length, e.ares, e.out_cap, e.rconn, self.n_rconns, default_room, policy,
                            bad_table) for e in entries]
        pos, self.boffs = 64, []
        for e in entries:
            pos = (pos + 15) // 16 * 16 + 32 + e.bmis
            self.boffs.append(pos)
            pos += len(e.req)
        self.in_image = np.full(pos + 64, GUARD, np.uint8)
        for e, o in zip(entries, self.boffs):
            self.in_image[o:o + len(e.req)] = np.frombuffer(e.req, np.uint8)
        pos, self.ooffs = 64, []
        for e in entries:
            if not e.abut:
                pos = (pos + 15) // 16 * 16 + 32 + e.omis
            self.ooffs.append(pos)
            pos += e.out_cap
        before = np.full(pos + 64, GUARD, np.uint8)
        for e, o in zip(entries, self.ooffs):  # what the accept left there
            before[o:o + len(e.resp)] = np.frombuffer(e.resp, np.uint8)
        self.out_image = before.copy()
        for (_, _, out, _), o in zip(self.exp, self.ooffs):
            if out is not None:
                self.out_image[o:o + len(out)] = np.frombuffer(out, np.uint8)
        self.in_t = torch.from_numpy(self.in_image.copy()).cuda()
        self.out_t = torch.from_numpy(before).cuda()
        atab = np.zeros((max(n, 1), 4), np.uint64)
        for k, e in enumerate(entries):
            atab[k] = (self.in_t.data_ptr() + self.boffs[k], e.length,
                       self.out_t.data_ptr() + self.ooffs[k] if e.out else 0, e.out_cap)
        self.atab_image, self.atab_t = atab, torch.from_numpy(atab.view(np.int64)).cuda()
        ares = b"".join(AM.pack_result(e.ares) for e in entries) + bytes([GUARD]) * 32
        self.ares_t = torch.from_numpy(np.frombuffer(ares, np.uint8).copy()).cuda()
        self.ares_image = np.frombuffer(b"".join(AM.pack_result(a) for _, a, _, _ in self.exp) + bytes([GUARD]) * 32,
                                        np.uint8)
        rt = np.zeros((max(n, 1), 2), np.uint32)
        rt[:n, 0] = [e.rconn for e in entries]
        rt[:n, 1] = 0x5A5A5A5A  # (reserved: never looked at)
        self.rt_image, self.rt_t = rt, torch.from_numpy(rt.view(np.int32)).cuda()
        rng = np.random.default_rng(n)
        rc = rng.integers(0, 256, 64 * (self.n_rconns + 1), dtype=np.uint8)  # the roster rows: whatever the host put there
        self.rc_t = torch.from_numpy(rc.copy()).cuda()
        self.rc_image = rc.copy()
        for e, (_, _, _, stored) in zip(entries, self.exp):
            if stored is not None:
                self.rc_image[64 * e.rconn + 56:64 * e.rconn + 60] = np.frombuffer(stored.to_bytes(4, "little"), np.uint8)
        self.res_t = torch.full((32 * (n + 1),), GUARD, dtype=torch.uint8, device="cuda") if results else None

    def run(self, ctx, stream=None, null_table=False):
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        rc = ctx.L.xyws_route_streams(
            ctx.h, C.c_void_p(self.atab_t.data_ptr()), C.c_void_p(self.ares_t.data_ptr()), C.c_void_p(self.rt_t.data_ptr()),
            self.n, None if null_table else C.c_void_p(self.blob_t.data_ptr() + self.blob_off),
            0 if null_table else self.blob_len, C.c_void_p(self.rc_t.data_ptr()), self.n_rconns, self.default_room,
            self.policy, C.c_void_p(self.res_t.data_ptr()) if self.res_t is not None else None, C.c_void_p(s))
        assert rc == 0
        return self

    def check(self, what=""):
        out = self.out_t.cpu().numpy()
        bad = np.flatnonzero(out != self.out_image)
        if bad.size:
            k = max(i for i, o in enumerate(self.ooffs) if o <= bad[0] + 16) if self.ooffs else -1
            raise AssertionError((what, "out byte", int(bad[0]), "near entry", k, self.exp[k][0] if k >= 0 else None))
        if self.res_t is not None:
            rows = self.res_t.cpu().numpy().tobytes()
            for k, (row, _, _, _) in enumerate(self.exp):
                got = rows[32 * k:32 * k + 32]
                assert got == M.pack_result(row), (what, k, self.entries[k].req[:60], row,
                                                   np.frombuffer(got, np.uint32)[:5].tolist())
            assert rows[32 * self.n:] == bytes([GUARD]) * 32, what  # the row behind n
        got = self.ares_t.cpu().numpy()
        for k in range(self.n + 1):
            assert got[32 * k:32 * k + 32].tobytes() == self.ares_image[32 * k:32 * k + 32].tobytes(), (what, "accept row", k)
        got = self.rc_t.cpu().numpy()
        bad = np.flatnonzero(got != self.rc_image)
        assert not bad.size, (what, "roster row", int(bad[0]) // 64, "byte", int(bad[0]) % 64)
        # every input unchanged
        assert np.array_equal(self.in_t.cpu().numpy(), self.in_image), what
        assert np.array_equal(self.blob_t.cpu().numpy(), self.blob_image), what
        assert np.array_equal(self.atab_t.cpu().numpy().view(np.uint64), self.atab_image), what
        assert np.array_equal(self.rt_t.cpu().numpy().view(np.uint32), self.rt_image), what
        return self

    def statuses(self):
        return [row["status"] for row, _, _, _ in self.exp]


# --------------------------------------------------------------------------- 1. every case, both policies, both sizes
@pytest.mark.parametrize("smallest", [False, True])
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", list(RC.TABLES))
def test_every_case(ctx, name, policy, smallest):
    routes = RC.TABLES[name]
    entries = [Entry(t, bmis=k % 16, omis=(5 * k) % 16) for k, (_, t) in enumerate(RC.TARGETS)]
    la = Launch(entries, routes, policy, RC.smallest_slots(len(routes)) if smallest else 0).run(ctx).check(name)
    seen = set(la.statuses())
    if name == "root":
        assert seen == {M.MATCHED, M.MATCHED | M.BY_PREFIX, M.MISS | (M.NOT_FOUND if policy else 0)}
    if name == "none":
        assert seen == {M.MISS | (M.NOT_FOUND if policy else 0)}


# --------------------------------------------------------------------------- 2. n and the grid stride
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_connection_counts(ctx, n):
    targets = [t for _, t in RC.TARGETS]
    entries = [Entry(targets[(7 * i) % len(targets)], bmis=i % 16, abut=True) for i in range(n)]
    Launch(entries, RC.TABLES["noroot"], M.MISS_404).run(ctx).check()


def test_past_the_grid_cap(ctx):
    """grid cap + 1 connections: the last one is the first workgroup's second connection."""
    cap = geometry()[3]
    targets = [b"/a", b"/nope", b"/rooms/b/c?x", b"/", b"chat", b"/exact/"]
    entries = [Entry(targets[k % len(targets)], out_cap=(129, 64, 63)[k % 3], bmis=k % 16, abut=True) for k in range(cap + 1)]
    for k in range(0, cap + 1, 5):  # rows that are not accepted among them
        entries[k].ares = dict(entries[k].ares, status=(0, AM.REJECTED)[k % 2])
    la = Launch(entries, RC.TABLES["noroot"], M.MISS_404).run(ctx).check()
    assert la.n == cap + 1 and len(set(la.statuses())) == 4


# --------------------------------------------------------------------------- 3. alignments, key lengths, the end of buf
def test_every_alignment_and_key_length(ctx):
    """Key lengths 1, 15, 16, 17, 255, 256, 257 and those around a lane's four
    bytes and a staged line, at every alignment of the request buffer (the
    target begins four bytes into it); with the `?` that ends the key, with a
    slash to drop, and with a byte more (a miss or a shorter match)."""
    targets = [b"/", RC.K255, RC.K256, RC.K256 + b"m"] + [RC.edge_key(n) for n in RC.EDGE_LENGTHS]
    step = geometry()[1]
    assert {step - 1, step, step + 1, 15, 16, 17} <= set(RC.EDGE_LENGTHS)
    entries = [Entry(t + tail, bmis=mis, omis=mis, out_cap=64 + mis)
               for mis in range(16) for t in targets for tail in (b"", b"?q=1", b"/", b"x")]
    for policy in POLICIES:
        la = Launch(entries, RC.TABLES["root"], policy).run(ctx).check()
        assert {row["key_len"] for row, _, _, _ in la.exp} >= {1, 15, 16, 17, 255, 256, 257}
    Launch(entries, RC.TABLES["noroot"], M.MISS_404, RC.smallest_slots(len(RC.TABLES["noroot"]))).run(ctx).check()


def test_a_key_that_ends_with_buf(ctx):
    """The key's last byte is the last byte of buf: the bytes behind it (which
    would make it another key) are never read into the result."""
    entries = []
    for mis in range(16):
        for target, behind in ((b"/a", b"/b HTTP"), (b"/rooms/b", b"/deep"), (b"/exact", b"?"), (RC.K256, b"/x"),
                               (RC.K255, b"x"), (b"/a/", b"/")):
            req = b"GET " + target
            ares = dict(status=AM.ACCEPTED, http_status=101, reason=0, consumed=len(req), resp_len=129, path_off=4,
                        path_len=len(target), key_off=AM.NO_KEY)
            entries.append(Entry(req=req + behind, length=len(req), ares=ares, bmis=mis))
    for policy in POLICIES:
        la = Launch(entries, RC.TABLES["noroot"], policy).run(ctx).check()
        assert set(la.statuses()) == {M.MATCHED}


# --------------------------------------------------------------------------- 4. chains, small tables, no table
def test_64_routes_in_one_chain(ctx):
    lib = _lib.load()
    chain = [k for k in RC.random_keys(20000, seed=7) if lib.xyws_debug_route_home(k, len(k), 128) == 5][:64]
    routes = [(k, 1000 + i, M.PREFIX if i % 2 else 0) for i, k in enumerate(chain)]
    entries = [Entry(k, bmis=i % 16) for i, k in enumerate(chain)] + \
              [Entry(k + b"/below", bmis=i % 16) for i, k in enumerate(chain)] + [Entry(chain[0] + b"x")]
    la = Launch(entries, routes, M.MISS_404, slots=128).run(ctx).check()
    assert [row["route"] for row, _, _, _ in la.exp[:64]] == list(range(64))
    assert [row["status"] for row, _, _, _ in la.exp[64:128]] == [M.MISS | M.NOT_FOUND, M.MATCHED | M.BY_PREFIX] * 32


@pytest.mark.parametrize("policy", POLICIES)
def test_no_table_and_tables_that_are_none(ctx, policy):
    entries = [Entry(t, bmis=k % 16, abut=True) for k, (_, t) in enumerate(RC.TARGETS[:24])]
    routes = RC.TABLES["noroot"]
    la = Launch(entries, [], policy).run(ctx, null_table=True).check("table_len 0")
    assert set(la.statuses()) == {M.MISS | (M.NOT_FOUND if policy else 0)}
    blob = _lib.route_table_of(routes)
    wrong_version = blob[:4] + b"\x02" + blob[5:]
    for what, bad in (("version", wrong_version), ("magic", b"YXRT" + blob[4:]), ("size", blob[:-1]), ("short", blob[:20])):
        la = Launch(entries, routes, policy, blob=bad, bad_table=True).run(ctx).check(what)
        assert set(la.statuses()) == {M.MISS | M.BAD_TABLE | (M.NOT_FOUND if policy else 0)}
    Launch(entries, routes, policy, blob=blob, bad_table=True, table_mis=2).run(ctx).check("misaligned")
    Launch(entries, routes, policy, blob=blob, table_mis=4).run(ctx).check("aligned to 4")


# --------------------------------------------------------------------------- 5. the 404 in a shared slab
def test_404_capacities_in_one_slab(ctx):
    """out_cap 0, 63, 64, 65 (and a null out) for the 404, the ranges packed one
    behind the other at every alignment, so neighbours share 16-byte lines;
    matched connections between them keep their 101."""
    caps = [0, 63, 64, 65, 1, 15, 16, 17, 129]
    entries = []
    for k in range(96):
        cap = caps[k % len(caps)]
        entries.append(Entry((b"/nope%d" % k, b"/a")[k % 4 == 3], out_cap=cap, abut=k % 16 != 0, omis=k % 16, bmis=k % 16))
    entries.append(Entry(b"/nope", out_cap=0, out=False))
    la = Launch(entries, RC.TABLES["noroot"], M.MISS_404).run(ctx).check()
    assert {a["status"] for _, a, _, _ in la.exp} == {AM.ACCEPTED, AM.ACCEPTED | AM.TRUNCATED, AM.REJECTED,
                                                     AM.REJECTED | AM.TRUNCATED}
    Launch(entries, RC.TABLES["noroot"], 0).run(ctx).check()  # policy 0 writes no byte of out and no accept row


# --------------------------------------------------------------------------- 6. roster rows
def test_roster_rows(ctx):
    """rconn in range (in reversed order), XYWS_ROUTE_NO_ROW and out of range;
    every byte of the roster table but the room words stays as it was."""
    targets = [t for _, t in RC.TARGETS[:40]]
    for policy in POLICIES:
        entries = [Entry(t, bmis=k % 16) for k, t in enumerate(targets)]
        n = len(entries)
        for k in range(0, n, 4):
            entries[k].rconn = M.NO_ROW
        for k in range(1, n, 8):
            entries[k].rconn = (n + 3, n + 2, 0xFFFFFFFE, 0x80000000)[(k // 8) % 4]
        la = Launch(entries, RC.TABLES["noroot"], policy, n_rconns=n + 2).run(ctx).check()
        assert any(s & M.BAD_ROW for s in la.statuses()) and any(st is None for _, _, _, st in la.exp)
        # no roster table at all
        for e in entries:
            e.rconn = M.NO_ROW if e.rconn == M.NO_ROW else 5
        la = Launch(entries, RC.TABLES["noroot"], policy, n_rconns=0)
        rc = ctx.L.xyws_route_streams(ctx.h, C.c_void_p(la.atab_t.data_ptr()), C.c_void_p(la.ares_t.data_ptr()),
                                      C.c_void_p(la.rt_t.data_ptr()), la.n, C.c_void_p(la.blob_t.data_ptr() + la.blob_off),
                                      la.blob_len, None, 0, DEFAULT_ROOM, policy, C.c_void_p(la.res_t.data_ptr()),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        la.check("no roster table")


# --------------------------------------------------------------------------- 7. rows that are not accepted, rows that lie
@pytest.mark.parametrize("policy", POLICIES)
def test_rows_not_accepted_and_rows_that_lie(ctx, policy):
    """Incomplete and rejected accept rows, and accepted ones whose path lies
    behind len or behind XYWS_ACCEPT_MAX_REQUEST: nothing is written but the
    route row (that nothing is read of such a request is the kernel's code to
    show: a test cannot see a read)."""
    good = request(b"/a")
    acc = accepted(good, 129)[0]
    entries = [Entry(b"/a"),
               Entry(req=good[:20]),                                     # incomplete
               Entry(req=AC.BY_NAME["post"]),                            # rejected
               Entry(req=good, ares=dict(acc, status=0)),
               Entry(req=good, ares=dict(acc, status=AM.REJECTED | AM.TRUNCATED)),
               Entry(req=good, ares=dict(acc, path_len=len(good) - 3)),   # ends one byte behind len
               Entry(req=good, ares=dict(acc, path_off=len(good), path_len=1)),
               Entry(req=good, ares=dict(acc, path_off=0xFFFFFFFF, path_len=0xFFFFFFFF)),
               Entry(req=good, ares=dict(acc, path_off=0xFFFFFFF0, path_len=0x20)),
               Entry(req=good, length=6, ares=dict(acc, path_len=3)),     # the accept saw more than len says
               Entry(req=good, ares=dict(acc, path_off=len(good), path_len=0)),  # an empty target at the very end: a miss
               Entry(b"/nope")]
    la = Launch(entries, RC.TABLES["noroot"], policy).run(ctx).check()
    assert [s & (M.NOT_ACCEPTED | M.BAD_ROW) for s in la.statuses()] == \
        [0, M.NOT_ACCEPTED, M.NOT_ACCEPTED, M.NOT_ACCEPTED, M.NOT_ACCEPTED, M.BAD_ROW, M.BAD_ROW, M.BAD_ROW, M.BAD_ROW,
         M.BAD_ROW, 0, 0]
    # a target that ends behind XYWS_ACCEPT_MAX_REQUEST though inside len
    big = request(b"/a" + b"?" + b"q" * 8200)
    ares = dict(acc, path_off=4, path_len=AM.MAX_REQUEST - 3, consumed=len(big))
    la = Launch([Entry(req=big, ares=ares), Entry(req=big, ares=dict(ares, path_len=AM.MAX_REQUEST - 4))],
                RC.TABLES["noroot"], policy).run(ctx).check()
    assert [s & M.BAD_ROW for s in la.statuses()] == [M.BAD_ROW, 0] and la.statuses()[1] & M.MATCHED


# --------------------------------------------------------------------------- 8. no result rows
@pytest.mark.parametrize("policy", POLICIES)
def test_null_results(ctx, policy):
    entries = [Entry(t, bmis=k % 16, abut=True, out_cap=70) for k, (_, t) in enumerate(RC.TARGETS[:40])]
    Launch(entries, RC.TABLES["noroot"], policy, results=False).run(ctx).check()


def test_streams_do_not_touch_the_error_word_and_n_0(ctx):
    la = Launch([Entry(b"/a")], RC.TABLES["noroot"], 0)
    la.n = 0
    la.exp, la.ares_image = [], np.frombuffer(la.ares_t.cpu().numpy().tobytes(), np.uint8)
    la.rc_image, la.out_image = la.rc_t.cpu().numpy().copy(), la.out_t.cpu().numpy().copy()
    la.run(ctx)
    torch.cuda.synchronize()
    assert bool((la.res_t == GUARD).all()) and np.array_equal(la.rc_t.cpu().numpy(), la.rc_image)


# --------------------------------------------------------------------------- 9. accept, route and roster in one graph
def room_tables(n, nr, member_cap, outs, accept_rows_t, want_join):
    """Resident tables of a room set of nr empty rooms for n connections, as
    _lib row tables on the device; every connection in want_join joins on
    accept whatever room its roster row names."""
    T = _lib.Table
    dev = torch.device("cuda")
    t = dict(members=torch.zeros(nr * member_cap, dtype=torch.int32, device=dev),
             notes=[torch.zeros(4096, dtype=torch.uint8, device=dev) for _ in range(nr)],
             seen_members=torch.zeros(nr * member_cap, dtype=torch.int32, device=dev))
    rooms, seen, rrooms, bconns, rconns = T(_lib.Room, nr), T(_lib.Room, nr), T(_lib.RosterRoom, nr), \
        T(_lib.BcastConn, n), T(_lib.RosterConn, n)
    t["seen"] = torch.zeros(32 * nr, dtype=torch.uint8, device=dev)
    for r in range(nr):
        rooms[r].members = t["members"].data_ptr() + 4 * member_cap * r
        seen[r].members = t["seen_members"].data_ptr() + 4 * member_cap * r
        rrooms[r].member_cap, rrooms[r].notes, rrooms[r].notes_cap = member_cap, t["notes"][r].data_ptr(), 4096
        rrooms[r].seen = t["seen"].data_ptr() + 32 * r
    for i in range(n):
        bconns[i].room = _lib.ROOM_NONE
        rconns[i].out, rconns[i].out_cap = outs[i].data_ptr(), outs[i].numel()
        rconns[i].room = _lib.ROOM_NONE
        if i in want_join:
            rconns[i].accept, rconns[i].flags = accept_rows_t.data_ptr() + 32 * i, _lib.RS_JOIN_ON_ACCEPT
    t["seen"].copy_(seen.upload(dev))
    t.update(rooms=rooms.upload(dev), rrooms=rrooms.upload(dev), bconns=bconns.upload(dev), rconns=rconns.upload(dev),
             room_results=torch.zeros(32 * nr, dtype=torch.uint8, device=dev),
             want=torch.zeros(n, dtype=torch.int32, device=dev), results=torch.zeros(32 * n, dtype=torch.uint8, device=dev))
    t["rooms0"], t["bconns0"] = t["rooms"].clone(), t["bconns"].clone()
    return t


def test_accept_route_roster_in_one_graph(ctx):
    """The three calls captured into one graph and replayed three times with
    other requests copied into the same buffers: each time the members' lists
    follow the paths, the 404s are out and nothing ran on the host in between."""
    n, nr, cap = 12, 3, 16
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    paths = [[(b"/rooms/%s" % b"abc"[(i + s) % 3:(i + s) % 3 + 1]) + (b"?t=%d" % i, b"/", b"")[i % 3] if (i + s) % 5 else
              b"/nope/%d" % i for i in range(n)] for s in range(3)]
    width = max(len(request(p)) for ps in paths for p in ps)
    reqs = [[request(p).ljust(width, b"\0") for p in ps] for ps in paths]  # (the bytes behind the blank line are not looked at)
    bufs = [torch.zeros(width, dtype=torch.uint8, device="cuda") for _ in range(n)]
    outs = [torch.zeros(512, dtype=torch.uint8, device="cuda") for _ in range(n)]
    atab = _lib.Table(_lib.AcceptConn, n)
    rtab = _lib.Table(_lib.RouteConn, n)
    for i in range(n):
        atab[i].buf, atab[i].len, atab[i].out, atab[i].out_cap = bufs[i].data_ptr(), width, outs[i].data_ptr(), 512
        rtab[i].rconn = i
    atab_t, rtab_t = atab.upload(torch.device("cuda")), rtab.upload(torch.device("cuda"))
    ares_t = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    rres_t = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    routes = {b"/rooms/a": 0, b"/rooms/b": 1, b"/rooms/c": 2}
    blob = _lib.route_table(exact=routes)
    blob_t = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()
    t = room_tables(n, nr, cap, outs, ares_t, set(range(n)))

    def calls(stream):
        s = C.c_void_p(stream)
        assert ctx.L.xyws_accept_streams(ctx.h, vp(atab_t), n, 1024, 0, vp(ares_t), s) == 0
        assert ctx.L.xyws_route_streams(ctx.h, vp(atab_t), vp(ares_t), vp(rtab_t), n, vp(blob_t), len(blob), vp(t["rconns"]),
                                        n, _lib.ROOM_NONE, _lib.RT_MISS_404, vp(rres_t), s) == 0
        assert ctx.L.xyws_roster_streams(ctx.h, vp(t["bconns"]), vp(t["rconns"]), n, vp(t["rooms"]), vp(t["rrooms"]),
                                         vp(t["room_results"]), nr, None, 0x11, None, vp(t["want"]), vp(t["results"]),
                                         s) == 0

    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        calls(s.cuda_stream)
    torch.cuda.synchronize()
    assert not bool(ares_t.any()) and not bool(rres_t.any())  # (capture ran nothing)
    tab = M.table([(k, r, 0) for k, r in routes.items()])
    for sweep in range(3):
        with torch.cuda.stream(s):
            for i in range(n):
                bufs[i].copy_(torch.from_numpy(np.frombuffer(reqs[sweep][i], np.uint8).copy()), non_blocking=False)
                outs[i].zero_()
            t["rooms"].copy_(t["rooms0"])     # everyone is new each time: empty rooms
            t["bconns"].copy_(t["bconns0"])
            g.replay()
        torch.cuda.synchronize()
        want = [[] for _ in range(nr)]
        for i, p in enumerate(paths[sweep]):
            row = M.lookup(tab, p)
            got = _lib.read_rows(_lib.RouteResult, rres_t, 1, i)[0]
            acc = _lib.read_rows(_lib.AcceptResult, ares_t, 1, i)[0]
            sent = outs[i].cpu().numpy().tobytes()
            if row["status"] & M.MATCHED:
                want[row["room"]].append(i)
                assert (got.status, got.room, got.key_len) == (M.MATCHED, row["room"], row["key_len"]), (sweep, i)
                assert acc.status == AM.ACCEPTED and sent[:12] == b"HTTP/1.1 101" and sent[129] == 0x81
            else:
                assert got.status == M.MISS | M.NOT_FOUND and got.room == _lib.ROOM_NONE
                assert (acc.status, acc.http_status, acc.reason, acc.resp_len) == (AM.REJECTED, 404, 11, 64)
                assert sent[:64] == M.RESP_404 and sent[64:129] == AM.response_101(AC.RFC_KEY)[64:] and not any(sent[129:])
        assert any(p.startswith(b"/nope") for p in paths[sweep]) and sum(len(w) for w in want) < n
        for r in range(nr):
            count = _lib.read_rows(_lib.Room, t["rooms"], 1, r)[0].n_members
            members = t["members"][cap * r:cap * r + count].cpu().numpy().tolist()
            assert members == want[r], (sweep, r, members, want[r])


# --------------------------------------------------------------------------- 10. the Python layer
def test_connection_group_route(ws, ctx):
    """Three rooms; connections that send /rooms/b?x=1, /rooms/b/, /nope and a
    partial request in one sweep: the first two are listed in room b and hold
    101 | welcome, the third holds the 404 and is in no list, the fourth is
    untouched; with miss_404=False and a default room the third is listed
    there."""
    reqs = [AC.browser(path=b"/rooms/b?x=1"), AC.browser(path=b"/rooms/b/"), AC.browser(path=b"/nope"), AC.RFC[:100]]
    names = [b"10.0.0.%d:5000" % k for k in range(4)]
    for miss_404 in (True, False):
        grp = ws.connection_group(4, cap=4, ctx=ctx)
        rs = grp.rooms(3, member_cap=8)
        table = grp.routes(exact={b"/rooms/a": 0, b"/rooms/b": 1, b"/rooms/c": 2})
        assert table.nbytes == len(table.host) and table.host[:4] == b"XYRT"
        bufs = [torch.from_numpy(np.frombuffer(r, np.uint8).copy()).cuda() for r in reqs]
        outs = [torch.full((512,), GUARD, dtype=torch.uint8, device="cuda") for _ in reqs]
        name_ts = [torch.from_numpy(np.frombuffer(nm, np.uint8).copy()).cuda() for nm in names]
        acc = grp.accept(list(enumerate(bufs)), outs)
        rt = grp.route(acc, table, default_room=_lib.ROOM_NONE if miss_404 else 2, miss_404=miss_404)
        empty = [torch.zeros(0, dtype=torch.uint8, device="cuda") for _ in reqs]
        dec = grp.decode(list(enumerate(empty)))
        msgs = grp.reassemble(dec, [torch.zeros(16, dtype=torch.uint8, device="cuda") for _ in reqs])
        bc = grp.broadcast(msgs, rs, outs)
        ro = grp.roster(bc, rs, names=name_ts, on_accept=[0, 1, 2, 3], route=rt)
        assert (rt.result(0).status, rt.result(0).room, rt.result(0).key_len) == (_lib.RT_MATCHED, 1, 8)
        assert (rt.result(1).status, rt.result(1).room, rt.result(1).key_len) == (_lib.RT_MATCHED, 1, 8)
        assert rt.result(3).status == _lib.RT_NOT_ACCEPTED
        assert ro.members(1) == [0, 1] and ro.members(0) == []
        sent = [o.cpu().numpy().tobytes() for o in outs]
        for k in (0, 1):
            res = ro.result(k)
            welcome = sent[k][129:res.send_len]
            assert sent[k][:129] == AM.accept(reqs[k], 0, 1024)[1] and res.status & _lib.RSC_JOINED
            assert names[k] in welcome and sent[k][res.send_len:] == bytes([GUARD]) * (512 - res.send_len)
        assert names[1] in sent[0][129:ro.result(0).send_len]  # the first hears the second's welcome too
        assert sent[3] == bytes([GUARD]) * 512 and ro.result(3).send_len == 0
        if miss_404:
            assert rt.result(2).status == _lib.RT_MISS | _lib.RT_NOT_FOUND
            assert sent[2][:64] == M.RESP_404 and sent[2][64:129] == AM.accept(reqs[2], 0, 1024)[1][64:]
            assert sent[2][129:] == bytes([GUARD]) * (512 - 129)
            assert ro.result(2).send_len == 64 and ro.result(2).status & _lib.RSC_NOT_RECEIVER
            assert (acc.result(2).status, acc.result(2).http_status, acc.result(2).reason) == (_lib.ACC_REJECTED, 404, 11)
            assert ro.members(2) == []
        else:
            assert (rt.result(2).status, rt.result(2).room) == (_lib.RT_MISS, 2)
            assert ro.members(2) == [2] and names[2] in sent[2][129:ro.result(2).send_len]
            assert acc.result(2).status == _lib.ACC_ACCEPTED
        # everything roster() took before keeps working: rooms given on the host, no route
        table.update(prefix={b"/": 0})
        assert table.nbytes == len(table.host)
    with pytest.raises(_lib.XywsError):
        grp.roster(bc, rs, on_accept=[0], accept=acc)  # a plain collection needs the route() result

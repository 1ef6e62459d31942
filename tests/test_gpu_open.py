"""xyws_open_streams on the GPU against a plain dict, exactly: route rows, roster table, guard row, inputs, the
copied-back directory, the error word (ctx). Route rows are hand-made; the graph and group tests run the real chain."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_route import ctx, request, room_tables, ws  # noqa: F401 (ctx, ws: the route tests' fixtures)
from xynet_amd import _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
GUARD, FROM, BASE, NO_ROW, ROOM_WORD = 0xA5, 7, 100, 0xFFFFFFFF, _lib.RosterConn.room.offset
MISS, MATCHED, BY_PREFIX, NOT_FOUND, NOT_ACCEPTED, BAD_ROW, BAD_TABLE = 4, 1, 2, 8, 0x10, 0x20, 0x40
DIRECTORY, OPENED, DIR_FULL = _lib.RT_DIRECTORY, _lib.RT_OPENED, _lib.RT_DIR_FULL


def row(key, status=MISS, room=FROM, rconn=None, mis=0, cut=0):  # cut: bytes by which len ends before the key does
    return dict(key=key, status=status, room=room, rconn=rconn, mis=mis, cut=cut)


class Dir:
    """A directory on the device between guard bytes, and the dict that says what it must hold."""

    def __init__(self, room_cap, slots=0, keys_cap=None, mis=0, damage=None):
        blob = bytearray(_lib.directory_blob(BASE, room_cap, slots, keys_cap))
        self.bad = bool(mis % 16) or damage is not None
        if damage is not None:
            blob = damage(blob)
        self.off, self.len = 32 + mis, len(blob)
        self.image = np.concatenate([np.full(self.off, GUARD, np.uint8), np.frombuffer(bytes(blob), np.uint8),
                                     np.full(32, GUARD, np.uint8)])
        self.t = torch.from_numpy(self.image.copy()).cuda()
        self.room_cap, self.keys_cap = room_cap, _lib.ROUTE_KEY_MAX * room_cap if keys_cap is None else keys_cap
        self.names, self.n_open, self.keys_used, self.dead = {}, 0, 0, 0
        self.slots = 0 if self.bad else _lib.directory_info(bytes(blob)).slots

    def answer(self, rows, n_rconns):
        """The reference: the rows in index order; [(status, room, stored room or None)] and the new state."""
        closed = self.n_open >= self.room_cap or self.keys_used >= self.keys_cap or self.dead > 0 or \
            len(rows) > self.slots - self.n_open - self.dead  # (a free slot for every row, or nothing is claimed)
        new, used, out = {}, self.keys_used, []
        for r in rows:
            st, key = r["status"], r["key"]
            by = st & MISS or st & (MATCHED | BY_PREFIX) == MATCHED | BY_PREFIX
            if r["room"] != FROM or not by or st & (NOT_FOUND | NOT_ACCEPTED | BAD_ROW) or not 1 <= len(key) <= 256:
                out.append((st, r["room"], None))
                continue
            if r["cut"]:
                out.append((st | BAD_ROW, r["room"], None))
                continue
            if self.bad:
                st, room = st | BAD_TABLE | DIR_FULL, FROM
            elif key in self.names:
                st, room = st | DIRECTORY, self.names[key]
            else:
                if key not in new and not closed:
                    used += len(key)
                    ok = self.n_open + len(new) < self.room_cap and used <= self.keys_cap
                    new[key] = BASE + self.n_open + len(new) if ok else None
                room = new.get(key)
                st, room = (st | OPENED, room) if room is not None else (st | DIR_FULL, FROM)
            stored = room if r["rconn"] < n_rconns else None
            out.append((st | (BAD_ROW if n_rconns <= r["rconn"] != NO_ROW else 0), room, stored))
        opened = {k: v for k, v in new.items() if v is not None}
        self.names.update(opened)
        self.n_open += len(opened)
        self.keys_used += sum(len(k) for k in opened)
        self.dead += len(new) - len(opened)
        return out

    def check(self, what=""):
        got = self.t.cpu().numpy()
        if self.bad:
            assert np.array_equal(got, self.image), (what, "a blob that is no directory was written")
            return
        assert (got[:self.off] == GUARD).all() and (got[-32:] == GUARD).all(), what
        blob = bytes(got[self.off:self.off + self.len])
        info = _lib.directory_info(blob)
        assert (info.n_open, info.keys_used, info.dead) == (self.n_open, self.keys_used, self.dead), what
        assert {k: _lib.directory_lookup(blob, k) for k in self.names} == self.names == _lib.directory_names(blob), what


class Launch:
    """The tables and buffers of one xyws_open_streams call over `rows` and the reference's answer to each."""

    def __init__(self, rows, d, n_rconns=None):
        self.rows, self.d, n = rows, d, len(rows)
        self.n, self.n_rconns = n, n if n_rconns is None else n_rconns
        for k, r in enumerate(rows):
            if r["rconn"] is None:
                r["rconn"] = n - 1 - k  # (reversed: route row k names roster row n - 1 - k)
        pos, offs = 64, []
        for r in rows:
            pos = (pos + 15) // 16 * 16 + 16 + r["mis"]
            offs.append(pos)
            pos += 4 + len(r["key"]) + 3
        self.in_image = np.full(pos + 64, GUARD, np.uint8)
        for r, o in zip(rows, offs):
            self.in_image[o:o + 4 + len(r["key"]) + 3] = np.frombuffer(b"GET " + r["key"] + b" HT", np.uint8)
        self.in_t = torch.from_numpy(self.in_image.copy()).cuda()
        atab = np.zeros((max(n, 1), 4), np.uint64)
        rt = np.full((max(n, 1), 2), 0x5A5A5A5A, np.uint32)
        res = np.full((n + 1, 8), 0x5A5A5A5A, np.uint32)  # (route and the reserved words: never looked at)
        res[n] = np.frombuffer(bytes([GUARD]) * 32, np.uint32)
        for k, (r, o) in enumerate(zip(rows, offs)):
            atab[k] = (self.in_t.data_ptr() + o, 4 + len(r["key"]) + 3 - (r["cut"] + 3 if r["cut"] else 0), 0, 0)
            rt[k, 0] = r["rconn"]
            res[k, [0, 1, 3, 4]] = (r["status"], r["room"], 4, len(r["key"]))
        self.atab_image, self.atab_t = atab, torch.from_numpy(atab.view(np.int64)).cuda()
        self.rt_image, self.rt_t = rt, torch.from_numpy(rt.view(np.int32)).cuda()
        self.res_image, self.res_t = res.copy(), torch.from_numpy(res.view(np.int32)).cuda()
        size = C.sizeof(_lib.RosterConn)
        rc = np.random.default_rng(n).integers(0, 256, size * (self.n_rconns + 1), dtype=np.uint8)
        self.rc_image, self.rc_t = rc.copy(), torch.from_numpy(rc).cuda()
        self.exp = d.answer(rows, self.n_rconns)
        for k, (r, (status, room, stored)) in enumerate(zip(rows, self.exp)):
            self.res_image[k, :2] = (status, room)
            if stored is not None:
                at = size * r["rconn"] + ROOM_WORD
                self.rc_image[at:at + 4] = np.frombuffer(stored.to_bytes(4, "little"), np.uint8)
        self.work_t = torch.full((_lib.OPEN_WORK_WORDS * n + 4,), 0x33333333, dtype=torch.int32, device="cuda")

    def run(self, ctx):
        vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
        s = torch.cuda.current_stream().cuda_stream
        assert ctx.L.xyws_open_streams(ctx.h, vp(self.atab_t), vp(self.rt_t), self.n, vp(self.d.t, self.d.off), self.d.len,
                                       vp(self.rc_t), self.n_rconns, FROM, vp(self.res_t), vp(self.work_t),
                                       C.c_void_p(s)) == 0
        return self

    def check(self, what=""):
        assert np.array_equal(self.res_t.cpu().numpy().view(np.uint32).reshape(-1, 8), self.res_image), (what, "route rows")
        assert np.array_equal(self.rc_t.cpu().numpy(), self.rc_image), (what, "the roster table")
        for t, image in ((self.in_t, self.in_image), (self.atab_t, self.atab_image), (self.rt_t, self.rt_image)):
            assert np.array_equal(t.cpu().numpy().view(image.dtype), image), (what, "an input changed")
        self.d.check(what)
        return self

    def statuses(self):
        return [s & (DIRECTORY | OPENED | DIR_FULL | BAD_ROW | BAD_TABLE) for s, _, _ in self.exp]


@pytest.mark.parametrize("n", [1, 2, 65])
def test_one_new_key_named_by_every_row(ctx, n):
    d = Dir(4, slots=128)
    la = Launch([row(b"/rooms/new", mis=k % 16) for k in range(n)], d).run(ctx).check("first")
    assert la.statuses() == [OPENED] * n and {room for _, room, _ in la.exp} == {BASE} and d.n_open == 1
    la = Launch([row(b"/rooms/new", MATCHED | BY_PREFIX, mis=(k + 3) % 16) for k in range(n)], d).run(ctx).check("again")
    assert la.statuses() == [DIRECTORY] * n and {room for _, room, _ in la.exp} == {BASE} and d.n_open == 1


@pytest.mark.parametrize("which", ["round - 1", "round", "round + 1", "grid cap + 1"])
def test_order(ctx, which):
    g = (C.c_uint64 * 4)()  # lanes per row, key bytes per lane, rows per numbering round, grid cap
    width, cap = (_lib.load().xyws_debug_open_geometry(g), g[2], g[3])[1:]
    n = {"round - 1": width - 1, "round": width, "round + 1": width + 1, "grid cap + 1": cap + 1}[which]
    keys = n // 3 + 1
    rows = [row(b"/r/%d" % ((k * 37) % keys), mis=k % 16) if k % 5 else row(b"/r/other%d" % k, room=FROM + 1)
            for k in range(n)]
    d = Dir(n)
    Launch(rows, d).run(ctx).check("first")
    assert d.n_open == len({r["key"] for r in rows if r["room"] == FROM})
    rows = [row(b"/r/%d" % ((k * 41) % (keys + 9)), MATCHED | BY_PREFIX, mis=(k + 1) % 16) for k in range(n)]
    assert set(Launch(rows, d).run(ctx).check("again").statuses()) == {OPENED, DIRECTORY}


def test_one_chain(ctx):
    lib, slots = _lib.load(), 32
    home = lambda k: lib.xyws_debug_directory_home(k, len(k), slots)  # noqa: E731
    cand = [b"/c/%d" % i for i in range(40000)]
    pre = next(k for k in cand if home(k) == 5 and home(k + b"/z") == 5)
    last = next(k for k in cand if home(k + b"A") == 5 and home(k + b"x") == 5)
    keys = [pre, pre + b"/z", last + b"A", last + b"x"] + [k for k in cand if home(k) == 5 and k != pre][:6]
    assert len(set(keys)) == 10 and {home(k) for k in keys} == {5}
    d = Dir(16, slots)
    la = Launch([row(k, mis=i % 16) for i, k in enumerate(keys + keys[::-1] + keys + keys[:2])], d).run(ctx).check("insert")
    assert [room for _, room, _ in la.exp[:10]] == list(range(BASE, BASE + 10)) and la.n == slots  # (a free slot for each row)
    la = Launch([row(k, mis=(5 * i) % 16) for i, k in enumerate(keys[::-1] + [pre + b"y"])], d).run(ctx).check("find")
    assert la.statuses() == [DIRECTORY] * 10 + [OPENED]


def test_key_lengths_and_alignments(ctx):
    rows = [row(bytes((i * 7 + mis + length) % 251 + 1 for i in range(length)), mis=mis) for mis in range(16)
            for length in (1, 15, 16, 17, 255, 256, 257)]
    d = Dir(128)
    for r in Launch(rows, d).run(ctx).check("insert").rows:
        r["mis"] = (r["mis"] + 9) % 16
    assert Launch(rows, d).run(ctx).check("find").statuses() == ([DIRECTORY] * 6 + [0]) * 16 and (d.n_open, d.dead) == (96, 0)


@pytest.mark.parametrize("limit", ["rooms", "keys", "slots"])
def test_running_out(ctx, limit):
    """Crossed inside one launch: a prefix of the order is admitted (slots: none is); the next launch claims nothing."""
    d, counts = {"rooms": (Dir(5, 64), (5, 7)), "keys": (Dir(16, 64, keys_cap=8 * 5 + 3), (5, 7)), "slots": (Dir(16, 32), (0, 0))}[limit]
    rows = [row(b"/full/%02d" % ((k * 5) % 12), mis=k % 16) for k in range(40)]  # twelve keys of 8 bytes
    la = Launch(rows, d).run(ctx).check("crossing")
    want = [(s & ~OPENED | DIRECTORY if s & OPENED else s, room) for s, room, _ in la.exp]
    la = Launch([dict(r, rconn=None) for r in rows] + [row(b"/full/late")], d).run(ctx).check("closed")
    assert [(s, room) for s, room, _ in la.exp] == want + [(MISS | DIR_FULL, FROM)] and (d.n_open, d.dead) == counts


@pytest.mark.parametrize("what", ["magic", "version", "size", "misaligned"])
def test_bytes_that_are_no_directory(ctx, what):
    damage = {"magic": lambda b: b"YXRD" + b[4:], "version": lambda b: b[:4] + b"\2" + b[5:], "size": lambda b: b[:-1],
              "misaligned": None}[what]
    d = Dir(8, mis=8 if what == "misaligned" else 0, damage=damage)
    la = Launch([row(b"/a"), row(b"/b", room=FROM + 1), row(b"/a", cut=1), row(b"/c", rconn=NO_ROW)], d).run(ctx).check(what)
    assert la.statuses()[0] == BAD_TABLE | DIR_FULL


def test_rows_that_are_no_candidates_or_lie(ctx):
    rows = [row(b"/a"),
            row(b"/a", room=FROM + 1), row(b"/a", MISS | NOT_ACCEPTED), row(b"/a", NOT_ACCEPTED, room=NO_ROW),
            row(b"/a", MISS | NOT_FOUND), row(b"/a", MATCHED), row(b"/a", MISS | BAD_ROW), row(b"", MISS),
            row(b"/b", MATCHED | BY_PREFIX, rconn=NO_ROW), row(b"/c", rconn=40), row(b"/d", rconn=0xFFFFFFFE),
            row(b"/e", cut=1), row(b"/a", cut=2, rconn=NO_ROW), row(b"/b")]
    d = Dir(8)
    Launch(rows, d, n_rconns=len(rows) + 2).run(ctx).check()
    assert d.names == {b"/a": BASE, b"/b": BASE + 1, b"/c": BASE + 2, b"/d": BASE + 3}
    Launch([], d).run(ctx).check("n == 0")  # launches nothing


def test_accept_route_open_roster_in_one_graph(ctx):
    n, nr, cap, lobby = 12, 9, 16, 0
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    paths = [[b"/rooms/%s" % (b"abc", b"bcd", b"cde")[s][i % 3:i % 3 + 1] + (b"?t=1", b"/", b"")[i % 3] if i % 4 else b"/lobby"
              for i in range(n)] for s in range(3)]
    width = max(len(request(p)) for ps in paths for p in ps)
    bufs = [torch.zeros(width, dtype=torch.uint8, device="cuda") for _ in range(n)]
    outs = [torch.zeros(512, dtype=torch.uint8, device="cuda") for _ in range(n)]
    atab, rtab = _lib.Table(_lib.AcceptConn, n), _lib.Table(_lib.RouteConn, n)
    for i in range(n):
        atab[i].buf, atab[i].len, atab[i].out, atab[i].out_cap = bufs[i].data_ptr(), width, outs[i].data_ptr(), 512
        rtab[i].rconn = i
    atab_t, rtab_t = atab.upload(torch.device("cuda")), rtab.upload(torch.device("cuda"))
    ares_t, rres_t = (torch.zeros(32 * n, dtype=torch.uint8, device="cuda") for _ in range(2))
    work_t = torch.zeros(_lib.OPEN_WORK_WORDS * n, dtype=torch.int32, device="cuda")
    blob = _lib.route_table(exact={b"/lobby": lobby}, prefix={b"/rooms": 1})
    blob_t = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()
    dblob = _lib.directory_blob(2, nr - 2)
    dir_t = torch.from_numpy(np.frombuffer(dblob, np.uint8).copy()).cuda()
    t = room_tables(n, nr, cap, outs, ares_t, set(range(n)))

    st, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=st):
        s = C.c_void_p(st.cuda_stream)
        assert ctx.L.xyws_accept_streams(ctx.h, vp(atab_t), n, 1024, 0, vp(ares_t), s) == 0
        assert ctx.L.xyws_route_streams(ctx.h, vp(atab_t), vp(ares_t), vp(rtab_t), n, vp(blob_t), len(blob), vp(t["rconns"]),
                                        n, _lib.ROOM_NONE, 0, vp(rres_t), s) == 0
        assert ctx.L.xyws_open_streams(ctx.h, vp(atab_t), vp(rtab_t), n, vp(dir_t), len(dblob), vp(t["rconns"]), n, 1,
                                       vp(rres_t), vp(work_t), s) == 0
        assert ctx.L.xyws_roster_streams(ctx.h, vp(t["bconns"]), vp(t["rconns"]), n, vp(t["rooms"]), vp(t["rrooms"]),
                                         vp(t["room_results"]), nr, None, 0x11, None, vp(t["want"]), vp(t["results"]),
                                         s) == 0
    names = {}
    for sweep in range(3):
        with torch.cuda.stream(st):
            for i in range(n):
                bufs[i].copy_(torch.from_numpy(np.frombuffer(request(paths[sweep][i]).ljust(width, b"\0"), np.uint8).copy()))
            t["rooms"].copy_(t["rooms0"])  # everyone is new each time: empty rooms
            t["bconns"].copy_(t["bconns0"])
            g.replay()
        torch.cuda.synchronize()
        want, before = [[] for _ in range(nr)], set(names)
        for i, p in enumerate(paths[sweep]):
            got = _lib.read_rows(_lib.RouteResult, rres_t, 1, i)[0]
            key = p.split(b"?")[0].rstrip(b"/")
            exp = (MATCHED, lobby) if key == b"/lobby" else \
                (MATCHED | BY_PREFIX | (DIRECTORY if key in before else OPENED), names.setdefault(key, 2 + len(names)))
            assert (got.status, got.room) == exp, (sweep, i, p)
            want[got.room].append(i)
        assert _lib.directory_names(bytes(dir_t.cpu().numpy())) == names and len(names) == (3, 4, 5)[sweep]
        for r in range(nr):
            count = _lib.read_rows(_lib.Room, t["rooms"], 1, r)[0].n_members
            assert t["members"][cap * r:cap * r + count].cpu().numpy().tolist() == want[r], (sweep, r)


def test_connection_group_open(ws, ctx):
    import accept_cases as AC
    reqs = [AC.browser(path=b"/rooms/blue?x=1"), AC.browser(path=b"/rooms/red"), AC.browser(path=b"/rooms/blue/")]
    grp = ws.connection_group(3, cap=4, ctx=ctx)
    rs, table, rooms = grp.rooms(5, member_cap=8), grp.routes(prefix={b"/rooms": 0}), grp.directory(1, 4)
    bufs = [torch.from_numpy(np.frombuffer(r, np.uint8).copy()).cuda() for r in reqs]
    outs = [torch.full((512,), GUARD, dtype=torch.uint8, device="cuda") for _ in reqs]
    names = [torch.from_numpy(np.frombuffer(b"10.0.0.%d:5000" % k, np.uint8).copy()).cuda() for k in range(3)]
    acc = grp.accept(list(enumerate(bufs)), outs)
    rt = grp.open(grp.route(acc, table), rooms, from_room=0)
    empty, small = ([torch.zeros(k, dtype=torch.uint8, device="cuda") for _ in reqs] for k in (0, 16))
    msgs = grp.reassemble(grp.decode(list(enumerate(empty))), small)
    ro = grp.roster(grp.broadcast(msgs, rs, outs), rs, names=names, on_accept=[0, 1, 2], route=rt)
    assert [(rt.result(k).status, rt.result(k).room) for k in range(3)] == [(MATCHED | BY_PREFIX | OPENED, r) for r in (1, 2, 1)]
    assert rooms.names() == {b"/rooms/blue": 1, b"/rooms/red": 2} and rooms.info().n_open == 2
    assert ro.members(1) == [0, 2] and ro.members(2) == [1] and ro.members(0) == []

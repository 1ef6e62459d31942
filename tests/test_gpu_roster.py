"""xyws_roster_streams on the device: every room's member list updated from
the sweep's rows, the welcome and farewell notices framed into the room's
notice wire and delivered behind every participant's send bytes, through the
C-ABI. Expected values: the model (tests/roster_model.py), which
tests/test_roster_model.py holds to the reference's room, over the same cases.
Bar: bit-exact notice wires, member arrays, send ranges and result rows; not a
guard byte changed around a notice buffer, between abutting member arrays, in
the send slab, in row n + 1 of either result table or in dev_want[n]; of the
bconns, jconns and rooms rows only the words the rules name are rewritten; the
names, dev_rconns, dev_rrooms and the sweep's rows unchanged.

Tile, scan step, copy step and grid sizes come from xyws_debug_roster_geometry."""
import ctypes as C
import hashlib
import base64

import numpy as np
import pytest

import roster_model as M
import room_model as R
from test_gpu_room import Bcast, Slab, vp
from test_gpu_streams import GUARD, as_array, download, ptr, upload
from xynet_amd import _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
GUARD32 = GUARD * 0x01010101
JUNK = 0x5A5A5A5A5A5A5A5A  # in every word of an input row that the call has no business with


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
    assert _lib.load().xyws_debug_roster_geometry(out) == 0
    return list(out)


def diff(what, got, want, offs):
    if got.tobytes() != want.tobytes():
        bad = int(np.flatnonzero(got != want)[0])
        k = max([j for j in range(len(offs)) if offs[j] <= bad], default=-1)
        raise AssertionError((what, "entry", k, "at", bad - offs[max(k, 0)], "got", int(got[bad]), "want",
                              int(want[bad])))


def u8(table):
    return table.reshape(-1).view(np.uint8)


def pack_reply(r):
    return R.pack_reply_result(R.reply_row(r["reply_len"], status=r["status"]))


def pack_accept(a):
    return (a["status"].to_bytes(4, "little") + (101).to_bytes(2, "little") + (0).to_bytes(2, "little") +
            (0x5A5A5A5A).to_bytes(4, "little") + a["resp_len"].to_bytes(4, "little") + bytes([0x5A]) * 16)


def pack_bcast(b):
    return b["send_len"].to_bytes(8, "little") + JUNK.to_bytes(8, "little") + b["status"].to_bytes(4, "little") + bytes(12)


def text_struct(t):
    s = _lib.RosterText(head_len=len(t.head), joined_len=len(t.joined), left_len=len(t.left))
    for field, data in (("head", t.head), ("joined", t.joined), ("left", t.left)):
        for k, b in enumerate(data):
            getattr(s, field)[k] = b
    return s


class Dev:
    """The resident tables of a room set on the device (member arrays that
    abut, the rooms table, the bconns table) and one xyws_roster_streams call
    after another on them. ext: dict(sends=Slab, bcast=, reply= device addresses
    of 32-byte row tables) when an earlier call on the device wrote the send
    buffers and the rows."""

    def __init__(self, conns, rooms):
        self.n, self.nr = n, nr = len(conns), len(rooms)
        self.alloc = [max(rm.member_cap, len(rm.members)) for rm in rooms]
        self.moffs = [sum(self.alloc[:r]) for r in range(nr)]
        img = np.full(sum(self.alloc) + 4, GUARD32, np.uint32)
        for r, rm in enumerate(rooms):
            img[self.moffs[r]:self.moffs[r] + len(rm.members)] = rm.members
        self.members_image, self.members_t = img, upload(img)
        rtab = np.full((max(nr, 1), 4), JUNK, np.uint64)
        for r, rm in enumerate(rooms):
            rtab[r, :2] = [0 if rm.members_null else ptr(self.members_t) + 4 * self.moffs[r], len(rm.members)]
        self.rooms_image, self.rooms_t = rtab, upload(u8(rtab))
        # the `seen` rows: member arrays of their own, abutting like the rooms' (a row without members: a null array)
        self.seen_image = np.full(sum(self.alloc) + 4, GUARD32, np.uint32)
        self.seen_t = upload(self.seen_image)
        stab = np.full((max(nr, 1), 4), JUNK, np.uint64)
        for r, rm in enumerate(rooms):
            stab[r, 0] = 0 if rm.members_null else ptr(self.seen_t) + 4 * self.moffs[r]
        self.srooms_image, self.srooms_t = stab, upload(u8(stab))
        btab = np.full((max(n, 1), 8), JUNK, np.uint64)
        for i, c in enumerate(conns):
            btab[i, 5] = c.cur | (0x5A5A5A5A << 32)
        self.bconns_image, self.bconns_t = btab, upload(u8(btab))

    def call(self, ctx, conns, rooms, text=M.REF, flags=M.FIN | M.TEXT, nmis=None, smis=None, wmis=None, jconns=True,
             ext=None, what="", stream=None):
        n, nr = self.n, self.nr
        res = M.roster(conns, rooms, text, flags)
        names = Slab()
        for i, c in enumerate(conns):
            names.add(0 if c.name is None else len(c.name), None if nmis is None else nmis[i], c.name or b"")
        names.place()
        if ext is None:
            sends = Slab()
            for i, c in enumerate(conns):
                sends.add(c.send_cap, None if smis is None else (smis[i] - c.base) % 16, c.prefix[:c.send_cap])
            sends.place()
        else:
            sends = ext["sends"]
            sends.image = download(sends.t).copy()
        notes, ncaps = Slab(), []
        for r, rm in enumerate(rooms):
            ncaps.append(0 if rm.notes_null else len(res.rooms[r][0]) if rm.notes_cap is None else rm.notes_cap)
            notes.add(ncaps[r], None if wmis is None else wmis[r])
        notes.place()
        rows = np.full((3, max(n, 1), 32), GUARD, np.uint8)  # bcast, reply, accept rows
        for i, c in enumerate(conns):
            if ext is None and c.bcast is not None:
                rows[0, i] = as_array(pack_bcast(c.bcast))
            if ext is None and c.reply is not None:
                rows[1, i] = as_array(pack_reply(c.reply))
            if c.accept is not None:
                rows[2, i] = as_array(pack_accept(c.accept))
        rows_t = upload(rows.reshape(-1))
        bp = ptr(rows_t) if ext is None else ext["bcast"]
        pp = ptr(rows_t) + 32 * max(n, 1) if ext is None else ext["reply"]
        ap = ptr(rows_t) + 64 * max(n, 1)
        rc = np.zeros((max(n, 1), 8), np.uint64)
        for i, c in enumerate(conns):
            rc[i] = [0 if c.name is None else ptr(names.t) + names.offs[i], c.name_len,
                     0 if c.out_null else ptr(sends.t) + sends.offs[i], 77 if c.out_null else c.send_cap,
                     bp + 32 * i if c.bcast is not None else 0, pp + 32 * i if c.reply is not None else 0,
                     ap + 32 * i if c.accept is not None else 0, c.room | (c.flags << 32)]
        rconns_t = upload(u8(rc))
        rr = np.zeros((max(nr, 1), 4), np.uint64)
        for r, rm in enumerate(rooms):
            rr[r] = [rm.member_cap, 0 if rm.notes_null else ptr(notes.t) + notes.offs[r],
                     77 if rm.notes_null else ncaps[r], ptr(self.srooms_t) + 32 * r if rm.seen else 0]
        rrooms_t = upload(u8(rr))
        jimage = np.full((max(n, 1), 8), JUNK, np.uint64)
        jt = upload(u8(jimage)) if jconns else None
        rres_t = upload(np.full(32 * (nr + 1), GUARD, np.uint8))
        res_t = upload(np.full(32 * (n + 1), GUARD, np.uint8))
        want_t = upload(np.full(n + 1, GUARD32, np.uint32))
        ts = text_struct(text) if text is not M.REF else None
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream)
        rcode = ctx.L.xyws_roster_streams(ctx.h, vp(self.bconns_t), vp(rconns_t), n, vp(self.rooms_t), vp(rrooms_t),
                                          vp(rres_t), nr, C.byref(ts) if ts is not None else None, flags, vp(jt),
                                          vp(want_t), vp(res_t), s)
        assert rcode == 0
        # the notice wires: every byte of the slab
        want = notes.image.copy()
        for r in range(nr):
            w = res.rooms[r][0]
            assert len(w) == min(res.rooms[r][1]["notes_len"], ncaps[r])
            want[notes.offs[r]:notes.offs[r] + len(w)] = as_array(w)
        diff((what, "notes"), download(notes.t), want, notes.offs)
        # the member arrays, the lists' tails and the words between them
        want = self.members_image.copy()
        for r, rm in enumerate(rooms):
            if not rm.members_null:
                m = res.rooms[r][2]
                assert len(m) <= max(rm.member_cap, len(rm.members))
                want[self.moffs[r]:self.moffs[r] + len(m)] = m
        got = download(self.members_t)
        for r, rm in enumerate(rooms):  # (the entries between the new count and the old one are dead: not compared)
            new, old = len(res.rooms[r][2]), len(rm.members)
            if not rm.members_null and new < old:
                want[self.moffs[r] + new:self.moffs[r] + old] = got[self.moffs[r] + new:self.moffs[r] + old]
        diff((what, "members"), got, want, self.moffs)
        self.members_image = want
        # the `seen` lists: the lists as the call found them, nothing around them, only the count of their rows
        for r, rm in enumerate(rooms):
            if res.seen[r] is not None:
                self.seen_image[self.moffs[r]:self.moffs[r] + len(res.seen[r])] = res.seen[r]
                self.srooms_image[r, 1] = len(res.seen[r])
        diff((what, "seen members"), download(self.seen_t), self.seen_image, self.moffs)
        assert download(self.srooms_t).tobytes() == u8(self.srooms_image).tobytes(), (what, "seen rows")
        rows_got = download(rres_t)
        for r in range(nr):
            assert rows_got[32 * r:32 * r + 32].tobytes() == M.pack_room_result(res.rooms[r][1]), (
                what, "room result", r, res.rooms[r][1], rows_got[32 * r:32 * r + 32].view(np.uint32))
        assert (rows_got[32 * nr:] == GUARD).all(), (what, "room result guard")
        # the send ranges
        want = sends.image.copy()
        got_res = download(res_t)
        for i, (lo, data, row) in enumerate(res.conns):
            if not conns[i].out_null:
                o = sends.offs[i]
                want[o + lo:o + lo + len(data)] = as_array(data)
            assert got_res[32 * i:32 * i + 32].tobytes() == M.pack_result(row), (
                what, "result", i, row, got_res[32 * i:32 * i + 32].view(np.uint32))
        assert (got_res[32 * n:] == GUARD).all(), (what, "result guard")
        diff((what, "send bytes"), download(sends.t), want, sends.offs)
        assert int(download(want_t)[n]) == GUARD32, (what, "dev_want guard")
        # the rows the call rewrites a word of
        self.bconns_image[:n, 5] = [cur | (0x5A5A5A5A << 32) for cur in res.cur]
        assert download(self.bconns_t).tobytes() == u8(self.bconns_image).tobytes(), (what, "bconns")
        self.rooms_image[:nr, 1] = [row["n_members"] for _, row, _ in res.rooms]
        assert download(self.rooms_t).tobytes() == u8(self.rooms_image).tobytes(), (what, "rooms")
        if jconns:
            jimage[:n, 4] = [room | (fl << 32) for room, fl in res.jconns]
            assert download(jt).tobytes() == u8(jimage).tobytes(), (what, "jconns")
        # the inputs
        assert download(names.t).tobytes() == names.image.tobytes(), (what, "a name changed")
        assert download(rconns_t).tobytes() == u8(rc).tobytes() and download(rrooms_t).tobytes() == u8(rr).tobytes()
        assert download(rows_t).tobytes() == rows.tobytes(), (what, "a row of the sweep changed")
        self.last = dict(names=names, sends=sends, notes=notes, res_t=res_t, rres_t=rres_t, jt=jt)
        return res


def run(ctx, case):
    d = Dev(case.conns, case.rooms)
    res = d.call(ctx, case.conns, case.rooms, case.text, case.flags, case.nmis, case.smis, case.wmis, case.jconns,
                 what=case.name)
    return d, res


# --------------------------------------------------------------------------- 1. member counts
def test_member_counts_and_tile_seams(ctx):
    T = geometry()[0]
    case = M.member_counts(T)
    _, res = run(ctx, case)
    assert [len(rm.members) for rm in case.rooms[:6]] == [0, 1, T - 1, T, T + 1, 2 * T + 1]
    assert [row["left"] for _, row, _ in res.rooms[:6]] == [0, 1, 2, 2, 3, 5]
    assert res.rooms[6][1]["left"] == T + 3 and res.rooms[6][1]["n_members"] == 0         # all leave
    assert res.rooms[7][1]["joined"] == T + 1 and res.rooms[7][2] == sorted(res.rooms[7][2])  # all join an empty room
    assert res.rooms[8][1]["status"] == M.RS_BAD_MEMBER and len(res.rooms[8][2]) == 2
    # a kept member of the second tile moves into the first one
    lo = case.rooms[5].members[0]
    assert res.rooms[5][2][T - 2] == lo + T + 1


# --------------------------------------------------------------------------- 2. the joiner scan
def test_joiner_scan_steps(ctx):
    S = geometry()[1]
    for n in (1, S - 1, S, S + 1, 2 * S + 1):
        case = M.joiner_scan(n, S)
        _, res = run(ctx, case)
        joined = res.rooms[0][1]["joined"] + res.rooms[1][1]["joined"]
        assert joined == sum(1 for c in case.conns if c.flags) >= 1
        assert res.conns[0][2]["status"] & M.RSC_JOINED and res.conns[n - 1][2]["status"] & M.RSC_JOINED
        if n > S:  # the two rooms' joiners interleave across the seam
            assert res.conns[S - 1][2]["room"] != res.conns[S][2]["room"]


# --------------------------------------------------------------------------- 3. member_cap
def test_member_cap_reached_and_exceeded(ctx):
    case = M.member_caps()
    _, res = run(ctx, case)
    assert [row["status"] for _, row, _ in res.rooms] == [0, M.RS_FULL, M.RS_FULL, 0, M.RS_FULL]
    assert [row["joined"] for _, row, _ in res.rooms] == [3, 3, 3, 0, 0]
    assert sum(bool(r["status"] & M.RSC_FULL) for _, _, r in res.conns) == 1 + 9 + 2
    assert all(row["n_members"] == rm.member_cap for (_, row, _), rm in zip(res.rooms[:3], case.rooms))


# --------------------------------------------------------------------------- 4. names
def test_name_lengths_and_every_alignment(ctx):
    case = M.name_lengths()
    d, res = run(ctx, case)
    lens = {c.name_len for c in case.conns if c.name is not None}
    assert set(M.NAME_LENGTHS) | {80, 81, 82, 83} <= lens
    assert sum(bool(r["status"] & M.RSC_BAD_NAME) for _, _, r in res.conns) == 2 * 16
    sizes = {row["welcome_off"] for _, row, _ in res.rooms}
    assert {2 + 24 + 82 + 19, 4 + 24 + 83 + 19, 4 + 24 + 256 + 19, 2 + 24 + 19} <= sizes
    last = d.last
    assert {(ptr(last["names"].t) + o) % 16 for o in last["names"].offs} == set(range(16))
    assert {(ptr(last["notes"].t) + o) % 16 for o in last["notes"].offs} == set(range(16))
    assert {(ptr(last["sends"].t) + o + c.base) % 16 for o, c in zip(last["sends"].offs, case.conns)} == set(range(16))


# --------------------------------------------------------------------------- 5. caps
def test_notes_cap_and_out_cap_at_every_byte(ctx):
    case = M.notes_caps()
    _, res = run(ctx, case)
    full = res.rooms[-1][1]["notes_len"]
    assert all(row["notes_len"] == full and row["joined"] == 2 and row["left"] == 1 for _, row, _ in res.rooms)
    assert sorted({len(w) for w, _, _ in res.rooms}) == list(range(full + 1))
    cut = [(len(d), r["status"]) for k, (_, d, r) in enumerate(res.conns) if k >= 4 * (full + 3) and k % 4 == 0]
    assert sorted({n for n, _ in cut}) == list(range(full + 1)) and cut[0][1] & M.RSC_TRUNCATED


# --------------------------------------------------------------------------- 6. bases and receivers
def test_bases_and_receivers(ctx):
    case = M.bases()
    _, res = run(ctx, case)
    assert {c.base for c in case.conns} == {0, 129, 66, 9, 40, 4, 11}
    st = [r["status"] for _, _, r in res.conns]
    for bit in (M.RSC_NOT_RECEIVER, M.RSC_NO_ROOM, M.RSC_MEMBER, M.RSC_JOINED, M.RSC_LEFT, M.RSC_ALREADY, M.RSC_TRUNCATED):
        assert any(s & bit for s in st), bit


def test_custom_text_and_no_jconns(ctx):
    _, res = run(ctx, M.custom_text())
    assert res.rooms[0][0][:4] == bytes([0x02, 126, 0, 99 + 32]) and res.rooms[0][1]["joined"] == 1
    assert res.rooms[0][0][res.rooms[0][1]["welcome_off"]:][:2] == bytes([0x02, 61 + 32])


def test_more_rooms_than_the_grid(ctx):
    G = geometry()[3]
    case = M.over_grid(G)
    _, res = run(ctx, case)
    assert len(res.rooms) == G + 3 and all(row["joined"] == 1 and row["left"] == 1 for _, row, _ in res.rooms)


def test_nothing_to_do(ctx):
    """n == 0 with rooms, rooms == 0 with connections, and a sweep without an event."""
    rooms = [M.Room([], member_cap=2)]
    Dev([], rooms).call(ctx, [], rooms, what="n0")
    conns = [M.Conn(b"a", M.JOIN, room=0, send_cap=9)]
    res = Dev(conns, []).call(ctx, conns, [], what="nr0")
    assert res.conns[0][2]["status"] == M.RSC_NO_ROOM
    conns, rooms = [M.Conn(b"a", cur=0, send_cap=4), M.Conn(b"b", send_cap=4)], [M.Room([0], member_cap=2)]
    res = Dev(conns, rooms).call(ctx, conns, rooms, what="idle")
    assert res.rooms[0][1] == dict(notes_len=0, welcome_off=0, joined=0, left=0, n_members=1, status=0)


# --------------------------------------------------------------------------- 7. three sweeps on one room set
def test_three_sweeps_on_one_room_set(ctx):
    """join; talk and join; close and leave: the broadcast of sweep k + 1 reads
    the lists and the bconns rooms the roster of sweep k wrote on the device."""
    n, names, sweeps = M.three_sweeps()
    talk = [{}, {1: [5], 2: [7, 3]}, {2: [9], 3: [4]}]
    mconns = [M.Conn(names[i]) for i in range(n)]
    mrooms = [M.Room([], member_cap=4), M.Room([], member_cap=4)]
    d = Dev(mconns, mrooms)
    for s, ev in enumerate(sweeps):
        # the broadcast, over the resident lists
        bconns = []
        for i in range(n):
            e = ev.get(i, {})
            rp = R.reply_row(e["reply"]["reply_len"], status=e["reply"]["status"],
                             code=1000 if e["reply"]["status"] & M.RPL_CLOSED else 0) if "reply" in e else None
            bconns.append(R.speaker(talk[s].get(i, []), head=R.HEAD24[:i] or None, room=mconns[i].cur, reply=rp))
        brooms = [R.Room(list(rm.members)) for rm in mrooms]
        R.size_sends(bconns, brooms, slack=200)
        b = Bcast(bconns, brooms)
        own = download(b.bconns_t).view(np.uint64).reshape(-1, 8).copy()
        assert [int(x) & 0xFFFFFFFF for x in own[:n, 5]] == [c.cur for c in mconns]
        # the caller's columns of the resident rows are copied on the device; the room word, the lists and the
        # counts stay as the roster of the sweep before left them there: nothing of them is uploaded again
        own[:n, 5] = d.bconns_image[:n, 5]
        d.bconns_image = own
        d.bconns_t.view(torch.int64).view(-1, 8)[:, :5].copy_(b.bconns_t.view(torch.int64).view(-1, 8)[:, :5])
        d.bconns_t.view(torch.int64).view(-1, 8)[:, 6:].copy_(b.bconns_t.view(torch.int64).view(-1, 8)[:, 6:])
        rt = download(b.rooms_t).view(np.uint64).reshape(-1, 4).copy()
        rt[:, :2] = d.rooms_image[:, :2]
        d.rooms_image = rt
        d.rooms_t.view(torch.int64).view(-1, 4)[:, 2:].copy_(b.rooms_t.view(torch.int64).view(-1, 4)[:, 2:])
        b.bconns_t, b.rooms_t = d.bconns_t, d.rooms_t
        b.inputs = [x for x in b.inputs if x[0] is not b.members_t]
        b.launch(ctx).check(("sweep", s, "broadcast"))
        # the roster, behind it
        for i, c in enumerate(mconns):
            e = ev.get(i, {})
            c.flags, c.room, c.accept = e.get("flags", 0), e.get("room", M.NONE), e.get("accept")
            c.bcast = dict(b.model.conns[i][2]) if "accept" not in e else None
            c.reply = bconns[i].reply if "accept" not in e else None
            c.send_cap = bconns[i].send_cap
        res = d.call(ctx, mconns, mrooms, ext=dict(sends=b.sends, bcast=ptr(b.res_t), reply=ptr(b.rpl_t)),
                     what=("sweep", s))
        M.apply(mconns, mrooms, res)
    assert [rm.members for rm in mrooms] == [[2, 3], []]
    assert res.conns[2][1] == M.notice(0x11, M.REF, names[1], M.REF.left) and res.conns[2][0] > 0


# --------------------------------------------------------------------------- 8. the eight-call chain
def request(key):
    return (b"GET /chat HTTP/1.1\r\nHost: h\r\nUpgrade: websocket\r\nConnection: Upgrade\r\n"
            b"Sec-WebSocket-Key: " + key + b"\r\nSec-WebSocket-Version: 13\r\n\r\n")


def response(key):
    acc = base64.b64encode(hashlib.sha1(key + b"258EAFA5-E914-47DA-95CA-C5AB0DC85B11").digest())
    return (b"HTTP/1.1 101 Switching Protocols\r\nUpgrade: websocket\r\nConnection: Upgrade\r\n"
            b"Sec-WebSocket-Accept: " + acc + b"\r\n\r\n")


def masked(payload, op=0x81, key=b"\x11\x22\x33\x44"):
    assert len(payload) < 126
    return bytes([op, 0x80 | len(payload)]) + key + bytes(b ^ key[k % 4] for k, b in enumerate(payload))


class Recorder:
    """The library with every *_streams call written down as it is made."""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        f = getattr(self.lib, name)
        if not name.endswith("_streams"):
            return f

        def call(*a):
            self.calls.append((name, f, a))
            return f(*a)
        return call


def test_eight_call_chain_direct_and_captured(ws, ctx):
    """accept -> decode -> reassemble -> hold -> reply -> broadcast -> roster ->
    backlog on 8 slot-stable connections through connection_group: connection
    6's handshake completes in the sweep and it is sent 101 | its welcome | the
    room's backlog; a member is sent its reply, the room's wire and the notices.
    Then the same eight calls, as they were made, captured into one graph on the
    restored state and replayed twice: the same bytes."""
    n, SEND, HOLD = 8, 1024, 256
    grp = ws.connection_group(n, cap=4, ctx=ctx)
    rs = grp.rooms(2, member_cap=4, wire_cap=512, notes_cap=512)
    names = [M.name_of(i) for i in range(n)]
    names_t = [upload(as_array(nm)) for nm in names]
    heads = [upload(as_array(R.HEAD24)) for _ in range(n)]
    areas = [torch.full((HOLD + 128,), GUARD, dtype=torch.uint8, device="cuda") for _ in range(n)]
    outs = [a[HOLD:] for a in areas]
    sends = [torch.full((SEND,), GUARD, dtype=torch.uint8, device="cuda") for _ in range(n)]
    key = b"dGhlIHNhbXBsZSBub25jZQ=="
    req_t = upload(as_array(request(key)))

    def sweep(pieces, joins=(), leaves=(), accept_conn=None):
        recv = [upload(as_array(p)) if p else torch.zeros(0, dtype=torch.uint8, device="cuda") for p in pieces]
        for t in sends:
            t.fill_(GUARD)
        acc = grp.accept([(accept_conn, req_t)], [sends[accept_conn]]) if accept_conn is not None else None
        dec = grp.decode(list(enumerate(recv)))
        msgs = grp.reassemble(dec, outs)
        held = grp.hold(msgs, HOLD)
        rep = grp.reply(dec, sends, 1 << 20, policy=_lib.POL_FRAGMENTS, flags=0, enc_opts=_lib.ENC_FRAME_OPCODE,
                        action_mask=1 << _lib.ACT_PING)
        got = grp.broadcast(held, rs, sends, heads=heads, reply=rep)
        ro = grp.roster(got, rs, names=names_t, joins=joins, leaves=leaves, accept=acc,
                        on_accept={accept_conn: 0} if accept_conn is not None else None)
        bl = grp.backlog(ro, keep=10, log_cap=2048)
        return recv, ro, bl, (acc, dec, msgs, held, rep, got)

    frame = lambda i, m: R.header(0x11, 24 + len(m)) + R.HEAD24 + m
    # sweep 1: 0, 1, 2 join room 0 and 4 joins room 1; nobody is listed yet, so nobody is heard
    alive = []
    _, ro, _, keep = sweep([b""] * n, joins=[(0, 0), (1, 0), (2, 0), (4, 1)])
    alive.append(keep)
    assert ro.members(0) == [0, 1, 2] and ro.members(1) == [4]
    # sweep 2: 0 and 2 talk, 1 pings
    _, ro, bl, keep = sweep([masked(b"hello room"), masked(b"p", 0x89), masked(b"two") + masked(b"more"), b"", b"", b"", b"", b""])
    alive.append(keep)
    assert bl.room_result(0).count == 3
    # sweep 3: 1 talks, 2 closes, 6 completes its handshake and joins room 0
    stateful = grp.state_tensors() + rs.state_tensors() + areas
    state = [t.clone() for t in stateful]
    pieces = [b"", masked(b"third"), masked(b"\x03\xe8", 0x88), b"", b"", b"", b"", b""]
    rec = Recorder(ctx.L)
    ctx.L = rec
    try:
        recv, ro, bl, keep = sweep(pieces, accept_conn=6)
    finally:
        ctx.L = rec.lib
    assert [c[0] for c in rec.calls] == ["xyws_accept_streams", "xyws_decode_streams", "xyws_reassemble_streams",
                                         "xyws_hold_streams", "xyws_reply_streams", "xyws_broadcast_streams",
                                         "xyws_roster_streams", "xyws_backlog_streams"]
    torch.cuda.synchronize()
    wire = frame(1, b"third")
    bye = M.notice(0x11, M.REF, names[2], M.REF.left)
    hi = M.notice(0x11, M.REF, names[6], M.REF.joined)
    log = frame(0, b"hello room") + frame(2, b"two") + frame(2, b"more") + wire
    want = {6: response(key) + hi + log, 0: wire + bye + hi, 1: wire + bye + hi}
    direct = [t.cpu().numpy().copy() for t in sends]
    for i, data in want.items():
        assert direct[i][:len(data)].tobytes() == data and (direct[i][len(data):] == GUARD).all(), i
        assert bl.result(i).send_len == len(data), i
    closed = ro.result(2)   # nothing behind the close frame
    assert closed.note_len == 0 and 0 < closed.send_len < 16 and (direct[2][closed.send_len:] == GUARD).all()
    assert ro.members(0) == [0, 1, 6] and ro.members(1) == [4]
    assert ro.result(6).status == _lib.RSC_JOINED and ro.result(2).status & _lib.RSC_LEFT
    assert ro.room_result(0).joined == 1 and ro.room_result(0).left == 1
    assert ro.notes(0).cpu().numpy().tobytes() == bye + hi
    after = [t.clone() for t in stateful]
    alive.append(keep)

    # the same eight calls in one graph, on the state the sweep began with
    def restore():
        for t, s in zip(stateful, state):
            t.copy_(s)
        for t, p in zip(recv, pieces):
            if p:
                t.copy_(upload(as_array(p)))     # (the decode unmasked them in place)
        for t in sends:
            t.fill_(GUARD)

    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    restore()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        for name, f, a in rec.calls:
            assert f(*a[:-1], C.c_void_p(s.cuda_stream)) == 0, name
    torch.cuda.synchronize()
    assert all(bool((t == GUARD).all()) for t in sends)  # (capture ran nothing)
    for _ in range(2):
        restore()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize()
        for i, t in enumerate(sends):
            assert t.cpu().numpy().tobytes() == direct[i].tobytes(), ("replay", i)
        for t, a in zip(stateful, after):
            assert bool((t == a).all()), "replay: a carry, a list or a log differs"


def test_talk_then_close_and_a_joiner_that_spoke_keep_the_backlog(ws, ctx):
    """A member says something and closes in the same sweep (its text is in
    the wire, LEAVE_ON_CLOSE takes it off the list) and a connection that joins
    by flag has a message of its own in the sweep's tables: the backlog's fold
    walks the list the broadcast read (the room set's `seen` rows), so the room
    keeps its history, the joiner is sent it, and the next sweep folds on."""
    n, SEND, HOLD = 6, 1024, 256
    grp = ws.connection_group(n, cap=4, ctx=ctx)
    rs = grp.rooms(1, member_cap=5, wire_cap=512, notes_cap=512)
    names = [M.name_of(i) for i in range(n)]
    names_t = [upload(as_array(nm)) for nm in names]
    heads = [upload(as_array(R.HEAD24)) for _ in range(n)]
    areas = [torch.full((HOLD + 128,), GUARD, dtype=torch.uint8, device="cuda") for _ in range(n)]
    outs = [a[HOLD:] for a in areas]
    sends = [torch.full((SEND,), GUARD, dtype=torch.uint8, device="cuda") for _ in range(n)]
    empty = torch.zeros(0, dtype=torch.uint8, device="cuda")

    def sweep(pieces, joins=()):
        for t in sends:
            t.fill_(GUARD)
        dec = grp.decode([(i, upload(as_array(p)) if p else empty) for i, p in enumerate(pieces)])
        msgs = grp.reassemble(dec, outs)
        held = grp.hold(msgs, HOLD)
        rep = grp.reply(dec, sends, 1 << 20, policy=_lib.POL_FRAGMENTS, flags=0, enc_opts=_lib.ENC_FRAME_OPCODE,
                        action_mask=1 << _lib.ACT_PING)
        got = grp.broadcast(held, rs, sends, heads=heads, reply=rep)
        ro = grp.roster(got, rs, names=names_t, joins=joins)
        return rep, got, ro, grp.backlog(ro, keep=10, log_cap=2048)

    frame = lambda m: R.header(0x11, 24 + len(m)) + R.HEAD24 + m
    sweep([b""] * n, joins=[(0, 0), (1, 0), (2, 0)])
    rep, got, ro, bl = sweep([masked(b"one"), b"", masked(b"two") + masked(b"\x03\xe8", 0x88), b"", masked(b"mine"), b""],
                             joins=[(4, 0)])
    wire = frame(b"one") + frame(b"two")
    assert rep.result(2).status & _lib.RPL_CLOSED and got.wire(0).cpu().numpy().tobytes() == wire
    assert got.room_result(0).nmsgs == 2
    assert ro.members(0) == [0, 1, 4] and ro.result(2).status & _lib.RSC_LEFT and ro.result(4).status == _lib.RSC_JOINED
    assert rs.seen_members_t[:3].cpu().tolist() == [0, 1, 2]
    rr, car = bl.room_result(0), grp.backlog_carry(0)
    assert (rr.status, rr.count, rr.folded, rr.dropped, rr.len) == (0, 2, 2, 0, len(wire))
    assert (car.count, car.len, car.gaps, car.total) == (2, len(wire), 0, 2)
    assert list(car.flen[:3]) == [len(frame(b"one")), len(frame(b"two")), 0]
    assert grp.backlog_bytes(0).cpu().numpy().tobytes() == wire
    bye = M.notice(0x11, M.REF, names[2], M.REF.left)
    hi = M.notice(0x11, M.REF, names[4], M.REF.joined)
    for i, data in ((0, wire + bye + hi), (1, wire + bye + hi), (4, hi + wire)):
        got_bytes = sends[i].cpu().numpy()
        assert got_bytes[:len(data)].tobytes() == data and (got_bytes[len(data):] == GUARD).all(), i
        assert bl.result(i).send_len == len(data), i
    assert bl.result(4).status == _lib.BLC_JOINED and bl.result(4).backlog_len == len(wire)
    # the next sweep folds on: the newcomer is heard as a member, the history is whole
    rep, got, ro, bl = sweep([b"", b"", b"", b"", masked(b"later"), b""])
    assert got.wire(0).cpu().numpy().tobytes() == frame(b"later") and ro.members(0) == [0, 1, 4]
    rr, car = bl.room_result(0), grp.backlog_carry(0)
    assert (rr.status, rr.count, rr.folded) == (0, 3, 1) and (car.gaps, car.total) == (0, 3)
    assert grp.backlog_bytes(0).cpu().numpy().tobytes() == wire + frame(b"later")


def test_connection_group_roster_refusals(ws, ctx):
    n = 3
    grp = ws.connection_group(n, cap=2, ctx=ctx)
    rs = grp.rooms(1, member_cap=2)
    sends = [torch.zeros(256, dtype=torch.uint8, device="cuda") for _ in range(n)]
    outs = [torch.zeros(64, dtype=torch.uint8, device="cuda") for _ in range(n)]
    empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
    dec = grp.decode([(0, empty), (2, empty)])
    msgs = grp.reassemble(dec, outs[:2])
    with pytest.raises(_lib.XywsError):
        grp.broadcast(msgs, rs, sends[:2])      # (item 1 is connection 2: not slot-stable)
    dec = grp.decode([(i, empty) for i in range(n)])
    msgs = grp.reassemble(dec, outs)
    got = grp.broadcast(msgs, rs, sends)
    with pytest.raises(_lib.XywsError):
        grp.roster(got, rs, joins=[(0, 1)])     # (no such room)
    with pytest.raises(_lib.XywsError):
        grp.roster(got, rs, joins=[(3, 0)])     # (no such connection)
    with pytest.raises(_lib.XywsError):
        grp.roster(grp.broadcast(msgs, [[0]], sends), rs)  # (a broadcast over lists has no resident tables)
    ro = grp.roster(got, rs, joins=[(0, 0), (1, 0), (2, 0)])
    assert ro.members(0) == [0, 1] and ro.result(2).status == _lib.RSC_FULL | _lib.RSC_NO_ROOM
    assert ro.room_result(0).status == _lib.RS_FULL
    with pytest.raises(_lib.XywsError):
        grp.backlog(ro, joiners=[(2, 0)])       # (the roster names the joiners)

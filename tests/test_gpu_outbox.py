"""xyws_outbox_streams on the device, through the C-ABI: a sweep's result rows
and scattered send ranges turned into a dense pack, an ordered send list and a
summary. Expected values: the model (tests/outbox_model.py), which
tests/test_outbox_model.py holds to hand-computed answers. Bar: bit-exact
entries up to n_entries with guard bytes (0xA5) behind them, the summary, and
every byte of the pack with guards around it and in slots that were not packed;
the conn table, the rows and the send slab unchanged; the device error word 0.

Tile, copy step and grid sizes come from xyws_debug_outbox_geometry."""
import ctypes as C
import itertools
import os
import select

import numpy as np
import pytest

import outbox_model as M
from test_gpu_room import Slab, vp
from test_gpu_streams import GUARD, as_array, download, ptr, upload
from xynet_amd import _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
JUNK = 0x5A5A5A5A5A5A5A5A  # in every field of an input row that the call has no business with
PAD = 64                   # guard bytes in front of and behind every output


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
    assert _lib.load().xyws_debug_outbox_geometry(out) == 0
    return list(out)


def payload(k, n):
    """n nonzero bytes that are not the guard and differ from connection to connection."""
    v = (np.arange(n, dtype=np.uint32) * 7 + 13 * k + 1) % 251 + 1
    v[v == GUARD] = 3
    return v.astype(np.uint8).tobytes()


def conn(k, cap, mis=None, null=False, **rows):
    """A model connection whose send range holds `cap` payload bytes (null: no range)."""
    return dict(out=None if null else payload(k, cap), mis=mis, **rows)


def pack_row(kind, r):
    if kind in ("backlog", "bcast"):
        return bytes(_lib.BacklogResult(send_len=r["send_len"], backlog_len=JUNK, status=r.get("status", 0x5A5A5A5A),
                                        reserved0=0x5A5A5A5A, reserved=JUNK))
    if kind == "reply":
        return bytes(_lib.ReplyResult(reply_len=r["reply_len"], first_close=JUNK, answered=0x5A5A5A5A, close_code=0x5A5A,
                                      status=r["status"], reserved=JUNK))
    return bytes(_lib.AcceptResult(status=r["status"], http_status=0x5A5A, reason=0x5A5A, consumed=0x5A5A5A5A,
                                   resp_len=r["resp_len"], path_off=0x5A5A5A5A, path_len=0x5A5A5A5A, key_off=0x5A5A5A5A,
                                   reserved=0x5A5A5A5A))


class Box:
    """The inputs of one call on the device (the send slab, the row tables, the
    conn table) and one xyws_outbox_streams call after another over them."""

    def __init__(self, conns):
        self.conns, self.n = conns, len(conns)
        sends = Slab()
        for c in conns:
            if c["out"] is not None:
                sends.add(len(c["out"]), c.get("mis"), c["out"])
        self.sends = sends.place()
        rows, where = bytearray(), {}
        for i, c in enumerate(conns):
            for kind in ("backlog", "bcast", "reply", "accept"):
                if c.get(kind) is not None:
                    where[i, kind] = len(rows)
                    rows += pack_row(kind, c[kind])
        self.rows_image = as_array(bytes(rows) + bytes([GUARD]) * 32)
        self.rows_t = upload(self.rows_image)
        tab = np.zeros((max(self.n, 1), 8), np.uint64)
        k = 0
        for i, c in enumerate(conns):
            if c["out"] is not None:
                tab[i, :2] = [ptr(self.sends.t) + self.sends.offs[k], c.get("out_cap", len(c["out"]))]
                k += 1
            else:
                tab[i, 1] = JUNK  # (counts as 0 for a null out)
            for col, kind in enumerate(("backlog", "bcast", "reply", "accept")):
                if (i, kind) in where:
                    tab[i, 2 + col] = ptr(self.rows_t) + where[i, kind]
        self.tab_image = tab.reshape(-1).view(np.uint8)
        self.tab_t = upload(self.tab_image)
        self.need = _lib.load().xyws_outbox_scratch_bytes(self.n)
        self.scratch_t = torch.full((self.need + PAD,), GUARD, dtype=torch.uint8, device="cuda")

    def outputs(self, room, host=False):
        """Guard-filled pack (room bytes), entries (n + 1) and summary, with PAD bytes around each."""
        sizes = (PAD + room + PAD, 32 * (self.n + 1), 64 + PAD)
        if host:
            ts = [torch.full((s,), GUARD, dtype=torch.uint8).pin_memory() for s in sizes]
            lib, ps = _lib.load(), []
            for t in ts:
                d = C.c_void_p()
                if lib.xyws_outbox_map(C.c_void_p(t.data_ptr()), C.byref(d)) != 0:
                    pytest.skip("xyws_outbox_map refuses torch's pinned memory: it is not mapped for the device")
                ps.append(d.value)
            return ts, ps
        ts = [torch.full((s,), GUARD, dtype=torch.uint8, device="cuda") for s in sizes]
        return ts, [ptr(t) for t in ts]

    def launch(self, ctx, ps, pack_cap, null_pack=False, stream=None):
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream)
        return ctx.L.xyws_outbox_streams(ctx.h, vp(self.tab_t), self.n, None if null_pack else C.c_void_p(ps[0] + PAD),
                                         pack_cap, C.c_void_p(ps[1]), C.c_void_p(ps[2]), vp(self.scratch_t), self.need, s)

    def expected(self, room, pack_cap, null_pack=False):
        entries, summary, writes = M.outbox(self.conns, None if null_pack else pack_cap)
        pack = M.apply({PAD + o: b for o, b in writes.items()}, bytearray([GUARD]) * (PAD + room + PAD))
        ent = bytearray([GUARD]) * (32 * (self.n + 1))
        for k, e in enumerate(entries):
            ent[32 * k:32 * k + 32] = bytes(_lib.OutboxEntry(**e))
        summ = bytes(_lib.OutboxSummary(**summary)) + bytes([GUARD]) * PAD
        return as_array(bytes(pack)), as_array(bytes(ent)), as_array(summ), (entries, summary)

    def check(self, ts, room, pack_cap, null_pack=False, what=""):
        torch.cuda.synchronize()
        want = self.expected(room, pack_cap, null_pack)
        for name, t, w in zip(("pack", "entries", "summary"), ts, want):
            got = t.numpy() if t.device.type == "cpu" else download(t)
            if got.tobytes() != w.tobytes():
                bad = int(np.flatnonzero(got != w)[0])
                raise AssertionError((what, name, "byte", bad, "got", int(got[bad]), "want", int(w[bad]),
                                      "entry" if name == "entries" else "", bad // 32))
        assert download(self.tab_t).tobytes() == self.tab_image.tobytes(), (what, "the conn table changed")
        assert download(self.rows_t).tobytes() == self.rows_image.tobytes(), (what, "a row changed")
        assert download(self.sends.t).tobytes() == self.sends.image.tobytes(), (what, "the send slab changed")
        assert bool((self.scratch_t[self.need:] == GUARD).all()), (what, "a byte behind the scratch changed")
        return want[3]

    def run(self, ctx, pack_cap=None, null_pack=False, host=False, what=""):
        """One call over fresh outputs, held to the model. pack_cap None: what always suffices."""
        full = sum(M.align16(len(c["out"])) for c in self.conns if c["out"] is not None)
        cap = full if pack_cap is None else pack_cap
        room = max(cap, 16)
        ts, ps = self.outputs(room, host)
        assert self.launch(ctx, ps, cap, null_pack) == 0, what
        return self.check(ts, room, cap, null_pack, what), ts


# --------------------------------------------------------------------------- 1. tile seams
def seam_conns(n):
    """Every third connection silent, so entry and table indices differ; a few closes without bytes."""
    conns = []
    for i in range(n):
        if i % 3 == 1:
            conns.append(conn(i, 8, bcast=dict(send_len=0), reply=dict(reply_len=0, status=0)))
        elif i % 7 == 3:
            conns.append(conn(i, 8, reply=dict(reply_len=0, status=M.RPL_CLOSED)))
        else:
            conns.append(conn(i, 1 + (5 * i) % 40, bcast=dict(send_len=1 + (3 * i) % 40)))
    return conns


def test_tile_seams(ctx):
    T, S, GX, GY = geometry()
    for n in (1, T - 1, T, T + 1, 2 * T + 1, GX + 1):
        (entries, summary), _ = Box(seam_conns(n)).run(ctx, what=("n", n))
        assert summary["n_entries"] == len(entries) and (n < 3 or summary["n_entries"] < n)
        assert summary["n_deferred"] == 0 and summary["packed_len"] == summary["pack_len"]


def test_more_tiles_than_the_scan_has_threads(ctx):
    """The scan pass loops over the tile sums; the slot that is cut lies in a tile of a later step."""
    T = geometry()[0]
    n = 256 * T + 3 * T + 1
    quiet = dict(out=None)
    conns = [quiet] * n
    talk = list(range(5, n, 997)) + [n - 1]
    for i in talk:
        conns[i] = conn(i, 48, bcast=dict(send_len=20 + i % 29))
    box = Box(conns)
    (entries, summary), _ = box.run(ctx, what="all packed")
    assert [e["conn"] for e in entries] == talk
    cut = entries[-2]["off"] + 16   # the last two do not fit; the cut lies behind the scan's first step
    assert entries[-2]["conn"] >= 256 * T
    (entries, summary), _ = box.run(ctx, pack_cap=cut, what="cut in a late tile")
    assert summary["n_deferred"] == 2 and summary["packed_len"] == entries[-2]["off"]


# --------------------------------------------------------------------------- 2. lengths and alignments
@pytest.mark.parametrize("abut", [False, True])
def test_lengths_and_every_alignment(ctx, abut):
    """Every length around a line and around a copy step at each of the 16
    source alignments. Abutting: a range's successor begins at its last byte,
    so a pad byte that leaks source data holds a neighbour's byte, never zero."""
    S = geometry()[1]
    lens = (0, 1, 15, 16, 17, 31, 32, 33, S - 1, S, S + 1, 2 * S + 5)
    conns = []
    for k, (n, a) in enumerate(itertools.product(lens, range(16))):
        mis = a if not abut or k == 0 else None
        if abut and n == 0:
            n = a  # (a range of 0 .. 15 bytes moves the alignment of everything behind it)
        conns.append(conn(k, n + (0 if abut else 3), mis=mis, bcast=dict(send_len=n)))
    (entries, summary), _ = Box(conns).run(ctx, what=("abut", abut))
    assert summary["n_truncated"] == 0 and summary["send_bytes"] == sum(c["bcast"]["send_len"] for c in conns)


# --------------------------------------------------------------------------- 3. every row combination
def test_every_row_combination(ctx):
    backlogs = (None, dict(send_len=40))
    bcasts = (None, dict(send_len=30), dict(send_len=31, status=0x3F))  # (the last: a roster row's status bits)
    replies = (None, dict(reply_len=20, status=0), dict(reply_len=6, status=M.RPL_CLOSED),
               dict(reply_len=0, status=M.RPL_CLOSED), dict(reply_len=0, status=M.RPL_OVERFLOW | 1))
    accepts = (None, dict(status=0, resp_len=0), dict(status=M.ACC_ACCEPTED, resp_len=129),
               dict(status=M.ACC_REJECTED, resp_len=64), dict(status=M.ACC_REJECTED | 4, resp_len=64))
    conns = []
    for k, (b, c, r, a) in enumerate(itertools.product(backlogs, bcasts, replies, accepts)):
        conns.append(conn(k, 160, backlog=b, bcast=c, reply=r, accept=a))
    k = len(conns)
    for cap in (37, 64):  # full_len = out_cap - 1, out_cap, out_cap + 1 through each row of the chain
        for d in (-1, 0, 1):
            conns.append(conn(k, cap, backlog=dict(send_len=cap + d)))
            conns.append(conn(k + 1, cap, bcast=dict(send_len=cap + d)))
            conns.append(conn(k + 2, cap, reply=dict(reply_len=cap + d, status=0)))
            conns.append(conn(k + 3, cap, accept=dict(status=M.ACC_ACCEPTED, resp_len=cap + d)))
            k += 4
    # no send range: everything it was to send is lost, its flags are still listed
    conns.append(conn(k, 0, null=True, bcast=dict(send_len=5)))
    conns.append(conn(k, 0, null=True, reply=dict(reply_len=0, status=M.RPL_CLOSED)))
    conns.append(conn(k, 0, null=True, bcast=dict(send_len=0)))
    conns.append(conn(k, 0, null=True))
    # out_cap below the range that follows: only out_cap bytes are the connection's
    conns.append(dict(conn(k, 50, bcast=dict(send_len=45)), out_cap=33))
    (entries, summary), _ = Box(conns).run(ctx)
    flags = {e["conn"]: e["flags"] for e in entries}
    assert summary["n_truncated"] == 8 + 1 + 1 and summary["status"] == M.S_TRUNCATED
    assert flags[len(conns) - 5] == M.TRUNCATED and flags[len(conns) - 4] == M.CLOSE
    assert len(conns) - 3 not in flags and len(conns) - 2 not in flags and 0 not in flags
    assert {0, M.CLOSE, M.OVERFLOW, M.CLOSE | M.OVERFLOW, M.TRUNCATED} <= set(flags.values())


# --------------------------------------------------------------------------- 4. capacity
def test_every_capacity(ctx):
    """About twenty slots spread over three tiles; the capacity at every multiple
    of 16 up to the whole pack and one beyond, two that are no multiple, and a
    null pack: offsets and sizes exact every time, no byte of a deferred slot written."""
    T = geometry()[0]
    n = 2 * T + 10
    conns = [conn(i, 4, reply=dict(reply_len=0, status=0)) for i in range(n)]
    for j, i in enumerate(range(3, n, n // 20)):
        conns[i] = conn(i, 80, bcast=dict(send_len=1 + (17 * j) % 70), reply=dict(reply_len=0, status=M.RPL_CLOSED * (j % 5 == 0)))
    conns[T - 1] = conn(T - 1, 4, reply=dict(reply_len=0, status=M.RPL_CLOSED))  # listed without bytes, at a tile's end
    box = Box(conns)
    pack_len = M.outbox(conns, 1 << 30)[1]["pack_len"]
    seen = set()
    for cap in list(range(0, pack_len + 32, 16)) + [pack_len // 2 + 7, pack_len - 1]:
        (entries, summary), _ = box.run(ctx, pack_cap=cap, what=("cap", cap))
        assert summary["pack_len"] == pack_len and summary["packed_len"] <= cap
        seen.add(summary["n_deferred"])
    assert seen == set(range(len([c for c in conns if c.get("bcast")]) + 1))
    (entries, summary), _ = box.run(ctx, pack_cap=pack_len, null_pack=True, what="null pack")
    assert summary["packed_len"] == 0 and summary["n_deferred"] == max(seen) and summary["pack_len"] == pack_len


# --------------------------------------------------------------------------- 5. nothing to do, the same call twice
def test_nothing_to_do_and_n_zero(ctx):
    T = geometry()[0]
    conns = [conn(i, 16, bcast=dict(send_len=0), reply=dict(reply_len=0, status=0), accept=dict(status=0, resp_len=0))
             for i in range(T + 5)]
    (entries, summary), _ = Box(conns).run(ctx)
    assert entries == [] and summary == dict(n_entries=0, pack_len=0, packed_len=0, send_bytes=0, n_close=0,
                                             n_truncated=0, n_deferred=0, status=0)
    # n == 0: nothing is launched and the summary is left alone
    t = torch.full((64,), GUARD, dtype=torch.uint8, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert ctx.L.xyws_outbox_streams(ctx.h, None, 0, None, 0, None, vp(t), None, 0, s) == 0
    torch.cuda.synchronize()
    assert bool((t == GUARD).all())


def test_the_same_call_twice(ctx):
    box = Box(seam_conns(geometry()[0] + 9))
    full = sum(M.align16(len(c["out"])) for c in box.conns)
    for cap in (full, 256):
        ts, ps = box.outputs(full)
        assert box.launch(ctx, ps, cap) == 0
        box.check(ts, full, cap, what="first")
        first = [download(t).copy() for t in ts]
        assert box.launch(ctx, ps, cap) == 0
        box.check(ts, full, cap, what="second")
        assert all(download(t).tobytes() == f.tobytes() for t, f in zip(ts, first))


def test_two_streams_at_once(ctx):
    """Two calls over different tables on two streams: each has its own scratch, neither disturbs the other."""
    T = geometry()[0]
    boxes = [Box(seam_conns(2 * T + 1)), Box(seam_conns(T + 1)[::-1])]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    torch.cuda.synchronize()
    for box, s in zip(boxes, streams):
        room = sum(M.align16(len(c["out"])) for c in box.conns)
        ts, ps = box.outputs(room)
        outs.append((ts, room))
    torch.cuda.synchronize()
    for _ in range(2):
        for box, s, (ts, room) in zip(boxes, streams, outs):
            ps = [ptr(t) for t in ts]
            assert box.launch(ctx, ps, room, stream=s.cuda_stream) == 0
    for box, (ts, room) in zip(boxes, outs):
        box.check(ts, room, room)


# --------------------------------------------------------------------------- 6. pinned destination
def test_pinned_destination_equals_device_destination(ctx):
    S = geometry()[1]
    conns = seam_conns(300) + [conn(900, 2 * S + 40, mis=9, bcast=dict(send_len=2 * S + 21))]
    box = Box(conns)
    full = sum(M.align16(len(c["out"])) for c in conns)
    for cap in (full, full // 2):
        _, dev = box.run(ctx, pack_cap=cap, what="device")
        _, pin = box.run(ctx, pack_cap=cap, host=True, what="pinned")
        for d, p in zip(dev, pin):
            assert download(d).tobytes() == p.numpy().tobytes()


def test_map_refuses_what_is_not_pinned(ctx):
    d = C.c_void_p(0x1234)
    buf = C.create_string_buffer(256)
    assert ctx.L.xyws_outbox_map(C.cast(buf, C.c_void_p), C.byref(d)) == -1 and d.value is None
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")   # a later HIP call still works: no error was left behind
    assert int(t.sum()) == 0


# --------------------------------------------------------------------------- 7. the real chain
def model_conns_of(sends, rows):
    """Model connections from a sweep's send tensors and the rows read back: rows[i] = dict of the row dicts."""
    return [dict(out=t.cpu().numpy().tobytes(), **rows[i]) for i, t in enumerate(sends)]


def test_the_real_chain_direct_and_captured(ws, ctx):
    """accept -> decode -> reassemble -> hold -> reply -> broadcast -> roster ->
    backlog -> outbox on 8 slot-stable connections through connection_group
    (the sweep of tests/test_gpu_roster.py's eight-call test): a member talks, a
    member closes, a connection completes its handshake and joins. Then the nine
    calls, as they were made, captured into one graph and replayed over two
    further sweeps' inputs: every packed slot is the send range of its connection."""
    import roster_model as RM
    import room_model as R
    from test_gpu_roster import Recorder, masked, request
    n, SEND, HOLD = 8, 1024, 256
    grp = ws.connection_group(n, cap=4, ctx=ctx)
    rs = grp.rooms(2, member_cap=4, wire_cap=512, notes_cap=512)
    names_t = [upload(as_array(RM.name_of(i))) for i in range(n)]
    heads = [upload(as_array(R.HEAD24)) for _ in range(n)]
    areas = [torch.full((HOLD + 128,), GUARD, dtype=torch.uint8, device="cuda") for _ in range(n)]
    outs = [a[HOLD:] for a in areas]
    slab = torch.full((n * SEND + 64,), GUARD, dtype=torch.uint8, device="cuda")
    sends = [slab[5 + SEND * i:5 + SEND * (i + 1)] for i in range(n)]   # (abutting, at an odd address)
    req_t = upload(as_array(request(b"dGhlIHNhbXBsZSBub25jZQ==")))

    def sweep(pieces, joins=(), accept_conn=None, pack_cap=None):
        recv = [upload(as_array(p)) if p else torch.zeros(0, dtype=torch.uint8, device="cuda") for p in pieces]
        slab.fill_(GUARD)
        acc = grp.accept([(accept_conn, req_t)], [sends[accept_conn]]) if accept_conn is not None else None
        dec = grp.decode(list(enumerate(recv)))
        msgs = grp.reassemble(dec, outs)
        held = grp.hold(msgs, HOLD)
        rep = grp.reply(dec, sends, 1 << 20, policy=_lib.POL_FRAGMENTS, flags=0, enc_opts=_lib.ENC_FRAME_OPCODE,
                        action_mask=1 << _lib.ACT_PING)
        got = grp.broadcast(held, rs, sends, heads=heads, reply=rep)
        ro = grp.roster(got, rs, names=names_t, joins=joins, accept=acc,
                        on_accept={accept_conn: 0} if accept_conn is not None else None)
        bl = grp.backlog(ro, keep=10, log_cap=2048)
        ob = grp.outbox(bl, accept=acc, pack_cap=pack_cap)
        return recv, (acc, dec, msgs, held, rep, got, ro, bl), ob

    def held_to_the_model(ob, keep, what):
        acc, rep, bl = keep[0], keep[4], keep[7]
        torch.cuda.synchronize()
        rows = []
        for i in range(n):
            r = dict(backlog=dict(send_len=bl.result(i).send_len), bcast=dict(send_len=keep[6].result(i).send_len))
            if acc is not None and i in acc.ids:
                a = acc.result(acc.ids.index(i))
                r["accept"] = dict(status=a.status, resp_len=a.resp_len)
            else:
                p = _lib.read_rows(_lib.ReplyResult, grp.results_t, 1, i)[0]
                r["reply"] = dict(reply_len=p.reply_len, status=p.status)
            rows.append(r)
        entries, summary, writes = M.outbox(model_conns_of(sends, rows), ob.pack_cap)
        s = ob._tensors["summary"].cpu().numpy().tobytes()
        assert s == bytes(_lib.OutboxSummary(**summary)), what
        e = ob._tensors["entries"].cpu().numpy().tobytes()
        assert e[:32 * len(entries)] == b"".join(bytes(_lib.OutboxEntry(**x)) for x in entries), what
        pack = ob._tensors["pack"].cpu().numpy().tobytes()
        for x in entries:
            if x["len"] and not x["flags"] & M.DEFERRED:
                assert pack[x["off"]:x["off"] + x["len"]] == sends[x["conn"]][:x["len"]].cpu().numpy().tobytes(), what
                assert pack[x["off"]:x["off"] + M.align16(x["len"])] == writes[x["off"]], what
        return entries, summary

    keepalive = []
    _, keep, ob = sweep([b""] * n, joins=[(0, 0), (1, 0), (2, 0), (4, 1)])
    keepalive.append(keep)
    entries, summary = held_to_the_model(ob, keep, "sweep 1")
    assert entries and {e["conn"] for e in entries} <= {0, 1, 2, 4}   # the welcomes
    _, keep, ob = sweep([masked(b"hello room"), masked(b"p", 0x89), masked(b"two") + masked(b"more"), b"", b"", b"", b"", b""])
    keepalive.append(keep)
    held_to_the_model(ob, keep, "sweep 2")
    # sweep 3, written down call by call: 1 talks, 2 closes, 6 completes its handshake and joins room 0
    stateful = grp.state_tensors() + rs.state_tensors() + areas
    state = [t.clone() for t in stateful]
    pieces = [b"", masked(b"third"), masked(b"\x03\xe8", 0x88), b"", b"", b"", b"", b""]
    rec = Recorder(ctx.L)
    ctx.L = rec
    try:
        recv, keep, ob = sweep(pieces, accept_conn=6)
    finally:
        ctx.L = rec.lib
    assert [c[0] for c in rec.calls][-2:] == ["xyws_backlog_streams", "xyws_outbox_streams"] and len(rec.calls) == 9
    entries, summary = held_to_the_model(ob, keep, "sweep 3")
    assert [e["conn"] for e in entries] == [0, 1, 2, 6] and entries[2]["flags"] == M.CLOSE and summary["n_close"] == 1
    assert ob.summary().n_entries == 4 and [e.conn for e in ob.entries()] == [0, 1, 2, 6]
    for k, e in enumerate(entries):
        assert ob.bytes(k) == sends[e["conn"]][:e["len"]].cpu().numpy().tobytes()
    direct = (slab.cpu().numpy().copy(), [ob._tensors[k].cpu().numpy().copy() for k in ("pack", "entries", "summary")])

    # the nine calls in one graph; each replay begins on the state the sweep began with, over other bytes
    def restore(texts):
        for t, s in zip(stateful, state):
            t.copy_(s)
        for t, p in zip(recv, texts):
            if p:
                t.copy_(upload(as_array(p)))     # (the decode unmasks in place)
        slab.fill_(GUARD)
        for k in ("pack", "entries", "summary"):
            ob._tensors[k].fill_(GUARD)

    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    restore(pieces)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        for name, f, a in rec.calls:
            assert f(*a[:-1], C.c_void_p(s.cuda_stream)) == 0, name
    torch.cuda.synchronize()
    assert bool((slab == GUARD).all()) and bool((ob._tensors["summary"] == GUARD).all())  # (capture ran nothing)
    for word in (b"third", b"fifth", b"sixth"):
        texts = list(pieces)
        texts[1] = masked(word)
        restore(texts)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize()
        for res in keep:
            if res is not None and hasattr(res, "_rows"):
                res._rows._raw = None   # (host copies of the rows: read again)
        entries, summary = held_to_the_model(ob, keep, ("replay", word))
        assert [e["conn"] for e in entries] == [0, 1, 2, 6]
        assert word in ob._tensors["pack"].cpu().numpy().tobytes()
        if word == b"third":   # the same inputs: the same bytes as the direct run
            assert slab.cpu().numpy().tobytes() == direct[0].tobytes()
            n_e = 32 * summary["n_entries"]
            assert ob._tensors["entries"].cpu().numpy()[:n_e].tobytes() == direct[1][1][:n_e].tobytes()
            assert ob._tensors["summary"].cpu().numpy().tobytes() == direct[1][2].tobytes()
            p_l = summary["packed_len"]
            assert ob._tensors["pack"].cpu().numpy()[:p_l].tobytes() == direct[1][0][:p_l].tobytes()


# --------------------------------------------------------------------------- 8. connection_group.outbox
def test_connection_group_outbox_and_its_refusals(ws, ctx):
    from test_gpu_roster import masked, request
    n = 4
    grp, other = ws.connection_group(n, cap=4, ctx=ctx), ws.connection_group(n, cap=4, ctx=ctx)
    sends = [torch.full((256,), GUARD, dtype=torch.uint8, device="cuda") for _ in range(n + 1)]
    empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
    pieces = [masked(b"ping me", 0x89), b"", masked(b"\x03\xe8", 0x88), masked(b"q", 0x89)]
    dec = grp.decode([(i, upload(as_array(p)) if p else empty) for i, p in enumerate(pieces)])
    rep = grp.reply(dec, sends[:n], 1 << 20, policy=_lib.POL_FRAGMENTS, flags=0, enc_opts=_lib.ENC_FRAME_OPCODE,
                    action_mask=1 << _lib.ACT_PING)
    req = upload(as_array(request(b"dGhlIHNhbXBsZSBub25jZQ==")[:-6] + b"12\r\n\r\n"))  # (a version it refuses)
    acc = other.accept([(0, req)], [sends[n]])
    with pytest.raises(_lib.XywsError):
        grp.outbox(dec)                      # (a decode result is no last call of a sweep)
    with pytest.raises(_lib.XywsError):
        grp.outbox(None)
    with pytest.raises(_lib.XywsError):
        other.outbox(rep)                    # (another group's result)
    with pytest.raises(_lib.XywsError):
        grp.outbox(rep, accept=acc)          # (another group's accept)
    with pytest.raises(ValueError):
        grp.outbox(rep, pack_cap=-1)
    for host in (False, True):
        try:
            ob = grp.outbox(rep, host=host)
        except _lib.XywsError as e:
            if host and "xyws_outbox_map" in str(e):
                continue                     # (this memory is not mapped for the device: the pinned test says so)
            raise
        s = ob.summary()
        lens = [rep.result(i).reply_len for i in range(n)]
        assert [e.conn for e in ob.entries()] == [0, 2, 3] and s.n_entries == 3 and s.n_close == 1
        assert [e.len for e in ob.entries()] == [lens[0], lens[2], lens[3]] and s.send_bytes == sum(lens)
        assert ob.entries()[1].flags == _lib.OB_CLOSE and s.n_deferred == 0 and s.packed_len == s.pack_len
        for k, e in enumerate(ob.entries()):
            assert ob.bytes(k) == sends[e.conn][:e.len].cpu().numpy().tobytes() and len(ob.bytes(k)) == e.len > 0
    ob = grp.outbox(rep, pack_cap=16)        # only the first slot fits; the others are read from their send tensors
    assert [bool(e.flags & _lib.OB_DEFERRED) for e in ob.entries()] == [False, True, True]
    assert ob.summary().status == _lib.OBS_DEFERRED and ob.summary().packed_len == 16
    for k, e in enumerate(ob.entries()):
        assert ob.bytes(k) == sends[e.conn][:e.len].cpu().numpy().tobytes()
    ob = grp.outbox(rep, pack_cap=0)         # a plan-only call
    assert ob.summary().n_deferred == 3 and ob.summary().pack_len == s.pack_len and ob.pack() == b""
    # handshakes alone: the refusal is sent and the connection closed; it is a row of its own behind the sweep's items
    ob = other.outbox(None, accept=acc)
    a = acc.result(0)
    assert a.status & _lib.ACC_REJECTED and ob.conn_ids == [0]
    assert [(e.conn, e.flags, e.len) for e in ob.entries()] == [(0, _lib.OB_CLOSE, a.resp_len)]
    assert ob.bytes(0) == acc.response(0)


# --------------------------------------------------------------------------- 9. the eventfd behind the call
def test_notifier_enqueue_behind_the_outbox(ctx):
    """After the outbox call and xyws_notifier_enqueue on its stream the eventfd
    becomes readable, and the notifier has completed seq + 1 once the stream is passed."""
    lib = ctx.L
    fd = os.eventfd(0, os.EFD_NONBLOCK)
    note = C.c_void_p()
    assert lib.xyws_notifier_create(fd, C.byref(note)) == 0
    try:
        box = Box(seam_conns(40))
        ts, ps = box.outputs(4096)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        assert lib.xyws_notifier_completed(note) == 0
        assert box.launch(ctx, ps, 4096, stream=s.cuda_stream) == 0
        assert lib.xyws_notifier_enqueue(note, 41, C.c_void_p(s.cuda_stream)) == 0
        assert select.select([fd], [], [], 30.0)[0] == [fd]
        s.synchronize()
        assert lib.xyws_notifier_completed(note) == 42 and os.eventfd_read(fd) == 1
        box.check(ts, 4096, 4096)
        for seq in (42, 43):   # one after another on the same stream: in order
            assert lib.xyws_notifier_enqueue(note, seq, C.c_void_p(s.cuda_stream)) == 0
        s.synchronize()
        assert lib.xyws_notifier_completed(note) == 44 and os.eventfd_read(fd) == 2
    finally:
        torch.cuda.synchronize()
        assert lib.xyws_notifier_destroy(note) == 0
        os.close(fd)

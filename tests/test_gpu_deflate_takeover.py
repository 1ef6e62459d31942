"""xyws_deflate_windows_streams on the device. Reference: zlib on the host: a record's payload + 00 00 ff ff must inflate,
in a zlib.decompressobj(-15, zdict=the last 32768 bytes in front of it), to exactly head + message; the history is a plain
concatenation in wire order (Call.check, which also holds carry, text and guards). The tables are test_gpu_deflate's Sweep."""
import ctypes as C
import zlib

import numpy as np
import pytest

from test_gpu_deflate import COMPLETE, CONTINUED, GUARD, VM, Sweep, bound, dev, frames_of, grp, ptr, text  # noqa: F401
from xynet_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
GEO = (C.c_uint64 * 6)()
assert _lib.load().xyws_debug_deflate_windows_geometry(GEO) == 0
STAGE, HIST, WINDOW = GEO[0], GEO[1], GEO[5]
END = b"\x00\x00\xff\xff"


class Room:
    """One room's text area, carry and model history across calls. takeover "text" or "carry": a row with that pointer
    alone (None: neither), which takes nothing over; both areas are then poisoned and must stay as they are."""

    def __init__(self, text_cap=WINDOW + 60000, takeover=True):
        self.text = torch.full((text_cap + 16,), 0 if takeover is True else GUARD, dtype=torch.uint8, device="cuda")
        self.carry = torch.full((32,), 0 if takeover is True else GUARD, dtype=torch.uint8, device="cuda")
        self.text_cap, self.takeover, self.on, self.hist = text_cap, takeover, takeover is True, b""

    def preset(self, hist):  # a history the room never compressed: carry and text as a call would have left them
        self.hist = hist
        self.text[:len(hist)].copy_(dev(hist)[:len(hist)])
        self.carry.copy_(dev(bytes(_lib.DeflateRoomCarry(hist_len=len(hist), n_sweeps=1))))
        return self


class Call:
    """One call's tables over conns (Sweep's form; room r's members name it, in order); joined: rooms the last roster admitted to."""

    def __init__(self, conns, rooms, joined=None, sweep=None, **kw):
        self.s, self.rooms, cuda, nr = sweep or Sweep(conns, **kw), rooms, torch.device("cuda"), len(rooms)
        order = [k for r in range(nr) for k, c in enumerate(conns) if c[1] == r]
        self.members = torch.tensor(order + [0], dtype=torch.int32, device="cuda")
        rt, dt, at = _lib.Table(_lib.Room, nr), _lib.Table(_lib.DeflateRoom, nr), 0
        for r, room in enumerate(rooms):
            count = sum(1 for c in conns if c[1] == r)
            rt.rows[r].members, rt.rows[r].n_members = self.members.data_ptr() + 4 * at, count
            at += count
            if room.takeover in (True, "text"):
                dt.rows[r].text, dt.rows[r].text_cap = room.text.data_ptr(), room.text_cap
            if room.takeover in (True, "carry"):
                dt.rows[r].carry = room.carry.data_ptr()
        ro = _lib.Table(_lib.RosterRoomResult, nr)
        for r in joined or ():
            ro.rows[r].joined = 1
        self.rt, self.dt, self.bconns = rt.upload(cuda), dt.upload(cuda), self.s.bt.upload(cuda)
        self.roster = ro.upload(cuda) if joined is not None else None
        self.rres = torch.zeros(32 * (nr + 1), dtype=torch.uint8, device="cuda")

    def run(self, g, stream=None):
        s = self.s
        assert g.ctx.L.xyws_deflate_windows_streams(
            g.ctx.h, ptr(s.rt), ptr(s.rres), ptr(self.bconns), ptr(s.dt), s.n, ptr(self.rt), ptr(self.dt),
            ptr(self.roster) if self.roster is not None else None, len(self.rooms), 0, ptr(s.view), ptr(s.vres), ptr(s.vbc),
            ptr(s.res), ptr(self.rres), stream) == 0
        return self

    def check(self, g, reset=(), cut=None):
        """Records, room rows, carries, guards. reset: rooms that begin empty; cut: {room: records that fit its text}. Returns the room rows."""
        torch.cuda.synchronize()
        assert g.ctx.last_device_error() == 0
        s = self.s
        host, rows = s.slab.cpu().numpy(), _lib.read_rows(_lib.DeflateRoomResult, self.rres, len(self.rooms))
        free, self.z = np.ones(host.size, bool), {k: [] for k in range(s.n)}  # z[k]: connection k's payloads as written
        for r, room in enumerate(self.rooms):
            hist, sweep_text, n_rec, bad = b"" if r in reset else room.hist, b"", 0, False
            for k, (h, rm, recs) in enumerate(s.conns):
                if rm != r:
                    continue
                want = [m for m, st, _ in recs if st == COMPLETE]
                vrecs = _lib.read_rows(_lib.Message, s.vmsgs, min(len(want), s.vmsg_cap), (VM + 1) * k)
                for j, m in enumerate(want):
                    behind = cut is not None and n_rec >= cut[r]
                    zdict = b"" if behind or not room.on else (hist + sweep_text)[-WINDOW:]
                    if j < len(vrecs) and not vrecs[j].status & _lib.MSG_TRUNCATED:
                        lo = s.offs[k] + vrecs[j].out_off
                        z = host[lo:lo + vrecs[j].length].tobytes()
                        free[lo:lo + len(z)] = False
                        self.z[k].append(z)
                        d = zlib.decompressobj(-15, zdict=zdict) if zdict else zlib.decompressobj(-15)
                        assert d.decompress(z + END) == h + m and not d.unused_data, (r, k, j)
                        assert len(z) <= bound(len(h) + len(m)) and lo + len(z) <= s.offs[k] + s.caps[k]
                    else:
                        bad |= not behind
                    sweep_text, n_rec = sweep_text + h + m, n_rec + 1
            if not room.on:
                assert bytes(rows[r]) == bytes(32) and (room.text == GUARD).all() and (room.carry == GUARD).all()
                continue
            capped = cut is not None and cut[r] < n_rec
            status = (_lib.DFR_RESET if r in reset else 0) | (_lib.DFR_TEXT_CAP if capped else 0) | (_lib.DFR_DESYNC if bad else 0)
            assert (rows[r].text_len, rows[r].n_records, rows[r].status, rows[r].reserved0, rows[r].reserved) == \
                (len(sweep_text), n_rec, status, 0, 0), r
            if n_rec or r in reset:
                room.hist = b"" if capped or bad else (hist + sweep_text)[-WINDOW:]
            c = _lib.read_rows(_lib.DeflateRoomCarry, room.carry, 1)[0]
            assert c.hist_len == len(room.hist) and room.text[:c.hist_len].cpu().numpy().tobytes() == room.hist, r
        for k in (k for k, c in enumerate(s.conns) if c[1] >= len(self.rooms)):
            free[s.offs[k]:s.offs[k] + s.caps[k]] = False  # (connections without a room: the sibling's tests)
        assert (host[free] == GUARD).all()
        return rows


def plain(g, c, conns, **kw):
    """xyws_deflate_streams over the same connections: no record of the call c is longer than it makes it. Returns its Sweep."""
    p = Sweep(conns, **kw)
    p.deflate(g, c.bconns, None)
    torch.cuda.synchronize()
    lens = lambda s: [r.length for r in _lib.read_rows(_lib.Message, s.vmsgs, (VM + 1) * s.n)]  # noqa: E731
    assert all(a <= b for a, b in zip(lens(c.s), lens(p)))
    return p


LENGTHS = [0, 1, 3, 4, STAGE - 1, STAGE, STAGE + 1, 2 * STAGE + 5]
HISTORIES = [0, 1, 3, 4, HIST - 1, HIST, HIST + 1, WINDOW - 1, WINDOW]
BODY = text(2 * STAGE + 5, 41)


@pytest.mark.parametrize("hist_len", HISTORIES)
def test_shapes(grp, hist_len):
    """The sample: every history value is the history in front of a call's first record, and every call has all eight
    record lengths, rotated so that the length of index (case number mod 8) comes first; record k is one text from byte
    3k on, so it repeats what is in front of it. Heads of 0 and 7 bytes; a filler record that is not deliverable puts the
    messages at offsets 0, 10 and 15 of a line, the records behind the short ones at 1, 4 and 8; the second out range lies
    at offset 0, 1 or 15 (Sweep: 8 + caps[0] into the slab). Totals from 40973 to 73741 bytes: the slide runs with and
    without overlap; a second sweep then reads the history the slide left."""
    i = HISTORIES.index(hist_len)
    order = LENGTHS[i % 8:] + LENGTHS[:i % 8]
    recs = [(BODY[3 * k:3 * k + n], COMPLETE, 1) for k, n in enumerate(order)]
    fill = lambda n: [(b"f" * n, CONTINUED, 1)] if n else []  # noqa: E731
    conns = [(b"", 0, recs[:3]), (b"alice: ", 0, fill(10) + recs[3:6]), (b"", 0, fill(15) + recs[6:])]
    caps = [sum(bound(len(h) + len(m)) for m, st, _ in rs if st == COMPLETE) for h, _, rs in conns]
    caps[0] += ((0, 1, 15)[i % 3] - 8 - caps[0]) % 16
    room = Room().preset(text(hist_len, 43 + i))
    c = Call(conns, [room], out_caps=caps).run(grp)
    plain(grp, c, conns, out_caps=caps)
    assert c.check(grp)[0].n_history >= 1 and (c.s.slab.data_ptr() + c.s.offs[1]) % 16 == (0, 1, 15)[i % 3]
    again = [(b"", 0, [(room.hist[-400:-200], COMPLETE, 1), (room.hist[-50:-46], COMPLETE, 1)])]
    assert Call(again, [room]).run(grp).check(grp)[0].n_history >= 1


CHAT = [b'{"user":"u%d","text":"' % k + text(170, 60 + k) + b'"}' for k in range(4)]
said = lambda conns: [h + m for h, _, ((m, _, _),) in conns]  # noqa: E731


def chat(sweep):
    """Three members; little repeats inside a message, every member quotes the one before it."""
    return [(b"m%d: " % k, 0, [(CHAT[(k + sweep) % 4] + CHAT[(k + sweep + 1) % 4][:60], COMPLETE, 1)]) for k in range(3)]


def test_the_history_is_used_and_pays(grp):
    raw = lambda co, m: len(co.compress(m) + co.flush(zlib.Z_SYNC_FLUSH))  # noqa: E731
    flat, one, fresh = said(chat(0)) + said(chat(1)), zlib.compressobj(6, zlib.DEFLATED, -15), lambda: zlib.compressobj(6, zlib.DEFLATED, -15)
    assert sum(raw(one, m) for m in flat) < 0.7 * sum(raw(fresh(), m) for m in flat)  # (zlib's own gain from the history)
    room, taken, total = Room(), 0, 0
    for sw in (0, 1):
        c = Call(chat(sw), [room]).run(grp)
        assert c.check(grp)[0].n_history >= 2 + sw
        taken += sum(_lib.read_rows(_lib.DeflateResult, c.s.res, 1, k)[0].out_len for k in range(3))
        p = plain(grp, c, chat(sw))
        total += sum(_lib.read_rows(_lib.DeflateResult, p.res, 1, k)[0].out_len for k in range(3))
    assert taken < total


@pytest.mark.parametrize("reset", [True, False])
def test_a_joiner_starts_from_an_empty_window(grp, reset):
    """Sweep 2 repeats sweep 1: after a reset a fresh inflater follows it; without one it points into sweep 1."""
    room, old, new = Room(), zlib.decompressobj(-15), zlib.decompressobj(-15)
    for sw in (0, 1):
        c = Call(chat(0), [room], joined=[0] if reset and sw else None).run(grp)
        c.check(grp, reset=(0,) if reset and sw else ())
        zs = [z for k in range(3) for z in c.z[k]]
        assert [old.decompress(z + END) for z in zs] == said(chat(0))
    if reset:
        assert [new.decompress(z + END) for z in zs] == said(chat(0))
    else:
        with pytest.raises(zlib.error, match="distance too far back"):
            [new.decompress(z + END) for z in zs]


@pytest.mark.parametrize("short", ["text_cap", "out_cap"])
def test_degradation(grp, short):
    room = Room().preset(BODY[:500])
    if short == "text_cap":
        room.text_cap = 500 + len(said(chat(0))[0]) + 10  # the history and one record
        Call(chat(0), [room]).run(grp).check(grp, cut={0: 1})
    else:
        assert Call(chat(0), [room], out_caps=[400, 20, 400]).run(grp).check(grp)[0].status == _lib.DFR_DESYNC
    assert room.hist == b""
    room.text_cap = WINDOW
    Call(chat(1), [room]).run(grp).check(grp)  # the next sweep starts from nothing and builds a history again
    assert room.hist == b"".join(said(chat(1)))


@pytest.mark.parametrize("has", ["text", "carry", None])
def test_rooms_that_do_not_take_over(grp, has):
    """A room with a text alone, a carry alone or neither, and a roomless connection, beside two takeover rooms (same
    messages: each sees its own text only). check() holds the room's row to zero and its poisoned areas to the poison."""
    conns = [(h, r, recs) for r in (0, 1, 2) for h, _, recs in chat(0)] + [(b"n: ", _lib.ROOM_NONE, [(CHAT[0], COMPLETE, 1)])]
    c = Call(conns, [Room(), Room(takeover=has), Room()]).run(grp)
    c.check(grp)
    s, p = c.s, plain(grp, c, conns)
    for k in (3, 4, 5, 9):
        for a, b, lo, hi in ((s.slab, p.slab, s.offs[k], s.offs[k] + s.caps[k]), (s.vres, p.vres, 32 * k, 32 * k + 32),
                             (s.res, p.res, 32 * k, 32 * k + 32), (s.vbc, p.vbc, 64 * k, 64 * k + 64)):
            assert bytes(a[lo:hi].cpu().numpy()) == bytes(b[lo:hi].cpu().numpy()), k
    assert c.z[0] == c.z[6] and c.z[1] != c.z[4]


def test_captured_and_replayed(grp):
    """The call captured once and replayed for two sweeps equals two eager sweeps: out ranges, room rows, history."""
    eager, graphed, want = Room(), Room(), []
    for sw in (0, 1):
        c = Call(chat(sw), [eager]).run(grp)
        c.check(grp)
        want.append((bytes(c.s.slab.cpu().numpy()), bytes(c.rres.cpu().numpy())))
    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    s = Sweep(chat(0))
    Call(chat(0), [Room()], sweep=s).run(grp)  # (eager once, as the sibling's test does)
    c = Call(chat(0), [graphed], sweep=s)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        c.run(grp, C.c_void_p(stream.cuda_stream))
    for sw in (0, 1):
        s.load(chat(sw))
        s.slab.fill_(GUARD)
        graph.replay()
        torch.cuda.synchronize()
        assert (bytes(s.slab.cpu().numpy()), bytes(c.rres.cpu().numpy())) == want[sw]
    assert all(bytes(a.cpu().numpy()) == bytes(b.cpu().numpy()) for a, b in ((graphed.text, eager.text), (graphed.carry, eager.carry)))


def test_a_client_with_a_persistent_inflater(grp):
    """connection_group over a room set: deflate(takeover=rs, last_roster=ro), broadcast(deflated=...), roster(). Members 0-2
    say the same in three sweeps; the first one's roster admits 3, so the second begins empty and the third does not.
    Member 1's z wire of all three goes into one inflater, 3's from the second on into a fresh one."""
    import streams
    from xynet_amd import websocket as ws
    g, key, heads = ws.connection_group(4, cap=8), b"\x37\xfa\x21\x3d", [b"%d: " % k for k in range(4)]
    rs, old, new, msgs_in = g.rooms(1, member_cap=4), zlib.decompressobj(-15), zlib.decompressobj(-15), [m for _, _, ((m, _, _),) in chat(0)]
    want, ro = [(0xC1, h + m) for h, m in zip(heads, msgs_in)], None
    for sw, joins in enumerate(([(0, 0), (1, 0), (2, 0)], [(3, 0)], [], [])):  # (sweep 0: nobody is a member yet)
        bufs = [dev(streams.header(0x81, len(m), key) + streams.masked(m, key)) if sw else dev(b"")[:0] for m in msgs_in] + [dev(b"")[:0]]
        msgs = g.reassemble(g.decode(list(enumerate(bufs))), [torch.zeros(600, dtype=torch.uint8, device="cuda") for _ in range(4)])
        sends = [torch.zeros(2000, dtype=torch.uint8, device="cuda") for _ in range(4)]
        dfl = g.deflate(msgs, [0, 1, 2, 3], 400, takeover=rs, last_roster=ro)
        bc = g.broadcast(msgs, rs, sends, heads=[dev(h) for h in heads], deflated=dfl)
        ro = g.roster(bc, rs, joins=joins)
        for k, client in ((1, old), (3, new)) if sw else ():
            sent = frames_of(sends[k][:bc.result(k).send_len].cpu().numpy().tobytes())
            assert [(b0, client.decompress(pay + END)) for b0, pay in sent] == (want if sw > 1 or k == 1 else [])
        assert not sw or (dfl.room_result(0).n_history >= 2, dfl.room_result(0).status) == (True, 0 if sw == 3 else _lib.DFR_RESET)
    assert g.deflate_carry(0).n_sweeps == 2 and g.deflate_history(0).cpu().numpy().tobytes() == 2 * b"".join(p for _, p in want)

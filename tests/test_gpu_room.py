"""xyws_broadcast_streams on the device: every room's messages of a sweep
framed once into the room's wire and the wire copied behind every member's
reply, through the C-ABI. Expected values: the model (tests/room_model.py),
which tests/test_room_model.py holds to the reference's room, over the same
scenarios. Bar: bit-exact wires, out ranges and result rows; not a guard byte
changed outside the written ranges, in row n + 1 of either result table or in
a wire past min(wire_len, wire_cap); the inputs unchanged.

Plumbing as in tests/test_gpu_reasm_streams.py: one guard-filled device buffer
per kind (message buffers, heads, wires, send ranges; misalignments 0..15 or
send ranges packed back to back); tile, step and grid sizes come from
xyws_debug_broadcast_geometry."""
import ctypes as C

import numpy as np
import pytest

import reasm_model as M
import reasm_streams_model as SM
import reply_model as RM
import room_model as R
from test_gpu_streams import GUARD, as_array, download, ptr, upload, zeros
from xynet_amd import _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


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
    assert _lib.load().xyws_debug_broadcast_geometry(out) == 0
    return list(out)


def vp(t, off=0):
    return C.c_void_p(ptr(t) + off) if t is not None else None


class Slab:
    """Byte ranges in one guard-filled device buffer."""

    def __init__(self):
        self.pos, self.offs, self.parts = 32, [], []

    def add(self, size, mis=None, data=b""):
        """mis: the misalignment of the range's first byte, None: directly after its predecessor."""
        if mis is not None:
            self.pos = (self.pos + 15) // 16 * 16 + 32 + mis % 16
        self.offs.append(self.pos)
        self.parts.append((self.pos, bytes(data)))
        self.pos += size
        return self.offs[-1]

    def place(self):
        self.image = np.full(self.pos + 64, GUARD, np.uint8)
        for o, d in self.parts:
            self.image[o:o + len(d)] = as_array(d)
        self.t = upload(self.image)
        return self


class Bcast:
    """One xyws_broadcast_streams call over the model's conns and rooms.
    ext: dict(reasm=, rres=, replies=) device addresses of tables an earlier
    call on the device wrote (the real sweep); the send ranges then hold guard
    bytes for the reply call to fill. results = False: a null dev_results."""

    def __init__(self, conns, rooms, flags=R.FIN | R.TEXT, enc_opts=0, packed=False, results=True, ext=None,
                 n_rooms=None):
        self.conns, self.rooms, self.flags, self.enc_opts = conns, rooms, flags, enc_opts
        n, nr = self.n, self.nr = len(conns), len(rooms) if n_rooms is None else n_rooms
        self.model = R.broadcast(conns, rooms[:nr], flags, enc_opts)
        self.inputs = []
        heads = Slab()
        for k, c in enumerate(conns):
            heads.add(len(c.head or b""), getattr(c, "hmis", (5 * k) % 16), c.head or b"")
        self.heads = heads.place()
        if ext is None:
            bufs = Slab()
            for k, c in enumerate(conns):
                bufs.add(len(c.buf), getattr(c, "bmis", k % 16), c.buf)
            self.bufs = bufs.place()
            rows, tot = [], 0
            for c in conns:
                rows.append(tot)
                tot += len(c.recs)
            recs = b"".join(SM.pack_records(c.recs) for c in conns)
            self.recs_image = np.concatenate([as_array(recs), np.full(40, GUARD, np.uint8)])
            self.recs_t = upload(self.recs_image)
            tab = np.zeros((max(n, 1), 8), np.uint64)
            rres = np.zeros((max(n, 1), 4), np.uint64)
            rpl = np.full(32 * max(n, 1), GUARD, np.uint8)
            for k, c in enumerate(conns):
                tab[k, :5] = [0 if c.out_null else ptr(self.bufs.t) + bufs.offs[k], len(c.buf), 0,
                              0 if c.msgs_null else ptr(self.recs_t) + 40 * rows[k], 7 if c.msgs_null else c.msg_cap]
                rres[k] = [sum(r[3] for r in c.recs), c.nmsgs, c.rsm_status << 32, 0]
                if c.reply is not None:
                    rpl[32 * k:32 * k + 32] = as_array(R.pack_reply_result(c.reply))
            self.reasm_t, self.rres_t = upload(tab.reshape(-1).view(np.uint8)), upload(rres.reshape(-1).view(np.uint8))
            self.rpl_image, self.rpl_t = rpl, upload(rpl)
            reasm_p, rres_p, rpl_p = ptr(self.reasm_t), ptr(self.rres_t), ptr(self.rpl_t)
            self.inputs = [(self.bufs.t, self.bufs.image), (self.recs_t, self.recs_image), (self.rpl_t, rpl)]
        else:
            reasm_p, rres_p, rpl_p = ext["reasm"], ext["rres"], ext["replies"]
        self.reasm_p, self.rres_p = reasm_p, rres_p
        self.inputs.append((self.heads.t, self.heads.image))
        sends = Slab()
        for k, c in enumerate(conns):
            mis = None if packed else (getattr(c, "smis", k % 16) - c.base) % 16
            sends.add(c.send_cap, mis, c.prefix[:c.send_cap] if ext is None else b"")
        self.sends = sends.place()
        wires, self.wcaps = Slab(), []
        for r, rm in enumerate(rooms):
            cap = 0 if rm.wire_null else (len(R.room_wire(conns, rm.members, flags, enc_opts)[0])
                                          if rm.wire_cap is None else rm.wire_cap)
            self.wcaps.append(cap)
            wires.add(cap, getattr(rm, "wmis", (3 * r) % 16))
        self.wires = wires.place()
        flat = [i for rm in rooms for i in rm.members] + [0]
        self.members_image = np.asarray(flat, np.uint32)
        self.members_t = upload(self.members_image)
        self.inputs.append((self.members_t, self.members_image))
        rtab = np.zeros((max(len(rooms), 1), 4), np.uint64)
        pos = 0
        for r, rm in enumerate(rooms):
            rtab[r] = [ptr(self.members_t) + 4 * pos, len(rm.members),
                       0 if rm.wire_null else ptr(self.wires.t) + wires.offs[r], 77 if rm.wire_null else self.wcaps[r]]
            pos += len(rm.members)
        self.rooms_t = upload(rtab.reshape(-1).view(np.uint8))
        btab = np.zeros((max(n, 1), 8), np.uint64)
        for k, c in enumerate(conns):
            hl = len(c.head or b"")
            btab[k, :6] = [ptr(self.heads.t) + heads.offs[k] if c.head is not None else 0, hl,
                           ptr(self.sends.t) + sends.offs[k], c.send_cap,
                           rpl_p + 32 * k if c.reply is not None else 0, c.room]
        self.bconns_t = upload(btab.reshape(-1).view(np.uint8))
        self.rr_t = upload(np.full(32 * (len(rooms) + 1), GUARD, np.uint8))
        self.res_t = upload(np.full(32 * (n + 1), GUARD, np.uint8)) if results else None

    def launch(self, ctx, stream=None):
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream)
        rc = ctx.L.xyws_broadcast_streams(ctx.h, C.c_void_p(self.reasm_p), C.c_void_p(self.rres_p), vp(self.bconns_t),
                                          self.n, vp(self.rooms_t) if self.nr else None,
                                          vp(self.rr_t) if self.nr else None, self.nr, self.flags, self.enc_opts,
                                          vp(self.res_t), s)
        assert rc == 0
        return self

    def check(self, what="", prefixes=True):
        m = self.model
        got = download(self.wires.t)
        want = self.wires.image.copy()
        for r in range(self.nr):
            w = m.rooms[r][0]
            assert len(w) == min(m.rooms[r][2]["wire_len"], self.wcaps[r])
            want[self.wires.offs[r]:self.wires.offs[r] + len(w)] = as_array(w)
        if got.tobytes() != want.tobytes():
            bad = int(np.flatnonzero(got != want)[0])
            r = max([j for j in range(len(self.rooms)) if self.wires.offs[j] <= bad], default=-1)
            raise AssertionError((what, "wire", "room", r, "at", bad - self.wires.offs[max(r, 0)], "wire_len",
                                  m.rooms[r][2]["wire_len"] if 0 <= r < self.nr else None, "cap", self.wcaps[max(r, 0)],
                                  "got", int(got[bad]), "want", int(want[bad])))
        got = download(self.sends.t)
        want = self.sends.image.copy()
        for k, c in enumerate(self.conns):
            o = self.sends.offs[k]
            if prefixes:
                want[o:o + min(len(c.prefix), c.send_cap)] = as_array(c.prefix[:c.send_cap])
            lo, data, _ = m.conns[k]
            want[o + lo:o + lo + len(data)] = as_array(data)
        if got.tobytes() != want.tobytes():
            bad = int(np.flatnonzero(got != want)[0])
            k = max([j for j in range(self.n) if self.sends.offs[j] <= bad], default=-1)
            raise AssertionError((what, "send bytes", "connection", k, "at", bad - self.sends.offs[max(k, 0)],
                                  m.conns[max(k, 0)][2], "cap", self.conns[max(k, 0)].send_cap, "got", int(got[bad]),
                                  "want", int(want[bad])))
        rr = download(self.rr_t)
        for r in range(self.nr):
            assert rr[32 * r:32 * r + 32].tobytes() == R.pack_room_result(m.rooms[r][2]), (
                what, "room result", r, m.rooms[r][2], rr[32 * r:32 * r + 32].view(np.uint32))
        assert (rr[32 * self.nr:] == GUARD).all(), (what, "room result guard")
        if self.res_t is not None:
            res = download(self.res_t)
            for k in range(self.n):
                assert res[32 * k:32 * k + 32].tobytes() == R.pack_bcast_result(m.conns[k][2]), (
                    what, "result", k, m.conns[k][2], res[32 * k:32 * k + 32].view(np.uint64))
            assert (res[32 * self.n:] == GUARD).all(), (what, "result guard")
        for t, image in self.inputs:
            assert download(t).tobytes() == image.tobytes(), (what, "an input changed")
        return self


def run(ctx, conns, rooms, kw, what="", **more):
    return Bcast(conns, rooms, **kw, **more).launch(ctx).check(what)


# --------------------------------------------------------------------------- 1. header forms
def test_header_forms(ctx):
    b = run(ctx, *R.header_forms())
    assert sorted({len(h) for _, _, h, _ in b.model.rooms[0][1]}) == [2, 4, 10]
    assert sorted(len(p) for _, _, _, p in b.model.rooms[0][1]) == [0, 1, 125, 125, 126, 126, 127, 127, 65535, 65535,
                                                                    65536, 65536]


# --------------------------------------------------------------------------- 2. the alignment matrix
@pytest.mark.parametrize("packed", [False, True], ids=["misaligned", "packed"])
def test_alignment_matrix(ctx, packed):
    S = geometry()[1]
    for length in (1, 15, 16, 17, 31, 33, S - 1, S, S + 1, 2 * S + 5):
        b = run(ctx, *R.alignment_matrix(S, length, packed), what=length)
        assert all(r[2]["status"] == R.ROOM_TRUNCATED and r[2]["wire_len"] > length for r in b.model.rooms)
        assert all(c[2]["bcast_len"] == length for c in b.model.conns)
        if not packed:
            seen = {((ptr(b.wires.t) + b.wires.offs[c.room]) % 16, (ptr(b.sends.t) + b.sends.offs[k] + c.base) % 16)
                    for k, c in enumerate(b.conns)}
            assert len(seen) == 256


# --------------------------------------------------------------------------- 3. tiles, the grid
def test_member_tiles(ctx):
    T = geometry()[0]
    b = run(ctx, *R.tiles(T))
    assert [len(rm.members) for rm in b.rooms] == [0, 1, T - 1, T, T + 1, 2 * T + 3]
    assert sorted({len(c.recs) for c in b.conns}) == [0, 1, 3, 5]
    assert b.model.rooms[4][2]["status"] & R.ROOM_MSG_CAP and not b.model.rooms[3][2]["status"]
    cov = R.Coverage().add(b.conns, b.rooms, b.model)
    cov.require("continued", "open", "interrupted", "utf8_bad", "truncated", "empty_room", "msg_cap")


def test_more_rooms_and_connections_than_the_grid(ctx):
    G = geometry()[2]
    b = run(ctx, *R.over_grid(G))
    assert b.n == b.nr == G + 3 and all(r[2]["nmsgs"] == 1 for r in b.model.rooms)


# --------------------------------------------------------------------------- 4. caps
def test_wire_cap_at_every_byte_of_a_frame(ctx):
    conns, rooms, kw = R.wire_caps()
    b = run(ctx, conns, rooms, kw)
    free = b.model.rooms[-1][2]
    assert free["status"] == 0 and free["wire_len"] == 35
    for (w, _, rr, _), rm in zip(b.model.rooms, rooms):  # exact whatever the cap
        assert (rr["wire_len"], rr["nmsgs"], rr["skipped"], rr["receivers"]) == (35, 1, 0, 2)
        assert len(w) == (0 if rm.wire_null else 35 if rm.wire_cap is None else min(rm.wire_cap, 35))
    assert sorted({len(r[0]) for r in b.model.rooms}) == list(range(36))


def test_out_cap_at_every_byte_of_a_frame(ctx):
    conns, rooms, kw = R.out_caps()
    b = run(ctx, conns, rooms, kw)
    for c, (lo, data, cr) in zip(conns, b.model.conns):  # exact whatever the cap
        assert cr["send_len"] == c.base + 35 and cr["bcast_len"] == 35
        assert len(data) == max(0, min(c.send_cap, c.base + 35) - min(c.base, c.send_cap))
    assert b.model.conns[-2][2]["status"] == R.BC_TRUNCATED and not b.model.conns[-2][1]  # base > out_cap
    assert not b.model.conns[-3][1]                                                       # base == out_cap


# --------------------------------------------------------------------------- 5. nulls and trivia
def test_nulls_and_trivia(ctx):
    conns, rooms, kw = R.nulls_and_trivia()
    b = run(ctx, conns, rooms, kw)
    assert b.model.rooms[0][2]["status"] == R.ROOM_BAD_MEMBER and len(conns) in rooms[0].members
    assert b.model.conns[7][2]["status"] == R.BC_NO_ROOM
    # a null dev_results
    run(ctx, conns, rooms, kw, results=False)
    # reply NULL for all connections
    for c in conns:
        c.reply = None
    conns, rooms = R.size_sends(conns, rooms)
    b = run(ctx, conns, rooms, kw)
    assert all(c[2]["send_len"] == c[2]["bcast_len"] for c in b.model.conns)
    # n_rooms == 0 with n > 0: every row NO_ROOM, the outs untouched
    b = run(ctx, conns, rooms, kw, n_rooms=0)
    assert all(c[2] == dict(send_len=0, bcast_len=0, status=R.BC_NO_ROOM) for c in b.model.conns)
    # n == 0 launches nothing
    Bcast([], rooms[2:], n_rooms=0).launch(ctx).check("n == 0")


# --------------------------------------------------------------------------- 6. the real sweep
class DeviceSweep:
    """decode -> reassemble -> reply -> broadcast of one sweep through the C-ABI."""

    def __init__(self, oracle, st, gst, pieces, caps, members, room_of, enc_opts):
        import test_gpu_reasm_streams as GS
        self.sw = GS.Sweep(oracle, gst, pieces, caps=caps)
        self.exp, self.replies, conns, rooms, _ = R.model_real_sweep(oracle, st, pieces, caps, members, room_of,
                                                                     enc_opts=enc_opts, exp=self.sw.exp)
        self.rres_t = upload(np.full(32 * (len(pieces) + 1), GUARD, np.uint8))
        self.b = Bcast(conns, rooms, enc_opts=enc_opts, ext=dict(reasm=ptr(self.sw.rtab_t), rres=ptr(self.sw.res_t),
                                                                 replies=ptr(self.rres_t)))
        rtab = np.zeros((len(pieces), 4), np.uint64)
        for k, c in enumerate(conns):
            rtab[k] = [ptr(self.b.sends.t) + self.b.sends.offs[k], c.send_cap, ptr(st.rcarry_t) + 32 * k, 0]
        self.rtab_t = upload(rtab.reshape(-1).view(np.uint8))

    def launch(self, ctx):
        self.sw.launch(ctx)
        call, m = self.sw.call, R.REPLY_MODE
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert ctx.L.xyws_reply_streams(ctx.h, vp(call.table_t), vp(call.counts_t), vp(self.rtab_t), call.n, 1 << 20,
                                        m["policy"], m["flags"], m["enc_opts"], m["action_mask"], vp(self.rres_t),
                                        s) == 0
        self.b.launch(ctx)
        return self

    def check(self, what):
        self.sw.check(what)
        rows = download(self.rres_t)
        for k, (_, res, _) in enumerate(self.replies):
            assert rows[32 * k:32 * k + 32].tobytes() == R.pack_reply_result(res), (what, "reply result", k)
        self.b.check(what)
        return self


@pytest.mark.parametrize("enc_opts", [0, R.ENC_FRAME_OPCODE], ids=["text", "frame_opcode"])
def test_the_real_sweep(ctx, oracle, enc_opts):
    import test_gpu_reasm_streams as GS
    sweeps, caps, members, room_of = R.sweep_streams()
    gst = GS.State(len(caps))
    st = R.SweepState()
    st.sm, st.rcarry_t = gst, zeros(32 * len(caps))
    cov = R.Coverage()
    for r, pieces in enumerate(sweeps):
        d = DeviceSweep(oracle, st, gst, pieces, caps, members, room_of, enc_opts).launch(ctx).check(("sweep", r))
        cov.add(d.b.conns, d.b.rooms, d.b.model)
        assert any(c.base > 0 for c in d.b.conns) or r
    cov.require("continued", "open", "interrupted", "utf8_bad", "rsm_overflow", "rpl_overflow", "before_close",
                "after_close", "closed_earlier", "hdr2", "hdr4", "no_room")
    got = download(st.rcarry_t)
    for k in range(len(caps)):
        assert got[32 * k:32 * k + 32].tobytes() == st.rc[k].pack(), ("reply carry", k)


# --------------------------------------------------------------------------- 7. capture
def test_four_calls_captured_and_replayed(ctx, oracle):
    """Decode, reassemble, reply and broadcast captured once on one stream (a
    linear chain, no reserve), replayed for two sweeps with new bytes uploaded
    into the same buffers in between; each replay against the model."""
    sweeps, caps, members, room_of = R.sweep_streams()
    n, cap = len(caps), 8
    caps = [cap if c == 8 else c for c in caps]
    size, W = max(len(p) for s in sweeps for p in s), 1024
    SEND = size + 13 + W
    st = R.SweepState()
    runs = [R.model_real_sweep(oracle, st, pieces, caps, members, room_of, send_cap=SEND, wire_cap=W,
                               out_caps=[size] * n, msg_caps=[cap + 1] * n) for pieces in sweeps]
    recv = torch.full((n * size + 64,), GUARD, dtype=torch.uint8, device="cuda")
    outs = torch.full((n * size + 64,), GUARD, dtype=torch.uint8, device="cuda")
    sends = torch.full((n * SEND + 64,), GUARD, dtype=torch.uint8, device="cuda")
    wires = torch.full((len(members) * W + 64,), GUARD, dtype=torch.uint8, device="cuda")
    heads = upload(as_array(R.HEAD24))
    frames = torch.zeros(n * cap * 32, dtype=torch.uint8, device="cuda")
    msgs = torch.zeros(n * (cap + 1) * 40, dtype=torch.uint8, device="cuda")
    dcar, mcar, rcar = zeros(64 * n), zeros(64 * n), zeros(32 * n)
    counts = torch.zeros(n, dtype=torch.int64, device="cuda")
    mres, rres, bres, rrres = (torch.zeros(32 * n, dtype=torch.uint8, device="cuda") for _ in range(4))
    tabs, stage = [], []
    for pieces in sweeps:
        tab = np.zeros((n, 8), np.uint64)
        img = np.full(n * size, GUARD, np.uint8)
        for i in range(n):
            tab[i, :5] = [ptr(recv) + size * i, len(pieces[i]), ptr(dcar) + 64 * i, ptr(frames) + 32 * cap * i,
                          caps[i]]
            img[size * i:size * i + len(pieces[i])] = as_array(pieces[i])
        tabs.append(upload(tab.reshape(-1).view(np.uint8)))
        stage.append(upload(img))
    ctab = torch.zeros_like(tabs[0])
    mtab, rtab, btab = np.zeros((n, 8), np.uint64), np.zeros((n, 4), np.uint64), np.zeros((n, 8), np.uint64)
    for i in range(n):
        mtab[i, :5] = [ptr(outs) + size * i, size, ptr(mcar) + 64 * i, ptr(msgs) + 40 * (cap + 1) * i, cap + 1]
        rtab[i] = [ptr(sends) + SEND * i, SEND, ptr(rcar) + 32 * i, 0]
        btab[i, :6] = [ptr(heads) if i else 0, 3 * i, ptr(sends) + SEND * i, SEND, ptr(rres) + 32 * i, room_of[i]]
    flat = np.asarray([i for m in members for i in m], np.uint32)
    members_t = upload(flat)
    roomtab, pos = np.zeros((len(members), 4), np.uint64), 0
    for r, m in enumerate(members):
        roomtab[r] = [ptr(members_t) + 4 * pos, len(m), ptr(wires) + W * r, W]
        pos += len(m)
    mtab_t, rtab_t, btab_t, roomtab_t = (upload(t.reshape(-1).view(np.uint8)) for t in (mtab, rtab, btab, roomtab))
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    mode = R.REPLY_MODE
    with torch.cuda.graph(g, stream=s):
        sp = C.c_void_p(s.cuda_stream)
        assert ctx.L.xyws_decode_streams(ctx.h, vp(ctab), n, vp(counts), 0, sp) == 0
        assert ctx.L.xyws_reassemble_streams(ctx.h, vp(ctab), vp(counts), vp(mtab_t), n, M.REASM_UTF8, vp(mres), sp) == 0
        assert ctx.L.xyws_reply_streams(ctx.h, vp(ctab), vp(counts), vp(rtab_t), n, 1 << 20, mode["policy"],
                                        mode["flags"], mode["enc_opts"], mode["action_mask"], vp(rres), sp) == 0
        assert ctx.L.xyws_broadcast_streams(ctx.h, vp(mtab_t), vp(mres), vp(btab_t), n, vp(roomtab_t), vp(rrres),
                                            len(members), 0x11, 0, vp(bres), sp) == 0
    torch.cuda.synchronize()
    assert bool((sends == GUARD).all()) and bool((wires == GUARD).all())  # (capture ran nothing)
    kept = []
    for r in range(len(sweeps)):
        recv[:n * size].copy_(stage[r])
        ctab.copy_(tabs[r])
        sends.fill_(GUARD)
        wires.fill_(GUARD)
        g.replay()
        kept.append((sends.clone(), wires.clone(), bres.clone(), rrres.clone()))  # (device copies)
    torch.cuda.synchronize()
    for r, (sd, wr, br, rr) in enumerate(kept):
        sd, wr, br, rr = download(sd), download(wr), download(br), download(rr)
        exp, replies, conns, rooms, res = runs[r]
        for j in range(len(members)):
            w = res.rooms[j][0]
            assert rr[32 * j:32 * j + 32].tobytes() == R.pack_room_result(res.rooms[j][2]), (r, j)
            assert wr[W * j:W * j + len(w)].tobytes() == w and (wr[W * j + len(w):W * (j + 1)] == GUARD).all(), (r, j)
        for i, c in enumerate(conns):
            lo, data, cr = res.conns[i]
            assert br[32 * i:32 * i + 32].tobytes() == R.pack_bcast_result(cr), (r, i)
            want = np.full(SEND, GUARD, np.uint8)
            want[:len(c.prefix)] = as_array(c.prefix)
            want[lo:lo + len(data)] = as_array(data)
            assert sd[SEND * i:SEND * (i + 1)].tobytes() == want.tobytes(), (r, i)
    assert sum(res.rooms[j][2]["nmsgs"] for _, _, _, _, res in runs for j in range(len(members))) >= 8


# --------------------------------------------------------------------------- 8. the Python layer
def test_connection_group_broadcast(ws, ctx, oracle):
    from test_gpu_parity import dev_bytes
    sweeps, caps, members, room_of = R.sweep_streams()
    n = len(caps)
    grp = ws.connection_group(n + 1, cap=8, ctx=ctx)
    st = R.SweepState()
    heads = [None] + [upload(as_array(R.HEAD24[:3 * k])) for k in range(1, n)]
    for r, pieces in enumerate(sweeps):
        exp, replies, conns, rooms, res = R.model_real_sweep(oracle, st, pieces, [8] * n, members, room_of,
                                                             msg_caps=[9] * n)
        items = [(i + 1, dev_bytes(p, 1 + i)[0]) for i, p in enumerate(pieces)]
        outs = [torch.full((t.numel() + 3,), GUARD, dtype=torch.uint8, device=t.device) for _, t in items]
        sends = [torch.full((c.send_cap,), GUARD, dtype=torch.uint8, device="cuda") for c in conns]
        dec = grp.decode(items)
        msgs = grp.reassemble(dec, outs)
        rep = grp.reply(dec, sends, 1 << 20, policy=_lib.POL_FRAGMENTS, flags=0, enc_opts=_lib.ENC_FRAME_OPCODE,
                        action_mask=1 << _lib.ACT_PING)
        got = grp.broadcast(msgs, [[i + 1 for i in m] for m in members], sends, heads=heads, reply=rep)
        for j in range(len(members)):
            rr, want = got.room_result(j), res.rooms[j][2]
            assert (rr.wire_len, rr.nmsgs, rr.skipped, rr.receivers, rr.status) == \
                (want["wire_len"], want["nmsgs"], want["skipped"], want["receivers"], want["status"]), (r, j)
            assert got.wire(j).cpu().numpy().tobytes() == res.rooms[j][3], (r, j)
        for k, c in enumerate(conns):
            br, (lo, data, want) = got.result(k), res.conns[k]
            assert (br.send_len, br.bcast_len, br.status) == (want["send_len"], want["bcast_len"], want["status"]), (r, k)
            image = np.full(c.send_cap, GUARD, np.uint8)
            image[:len(c.prefix)] = as_array(c.prefix)
            image[lo:lo + len(data)] = as_array(data)
            assert sends[k].cpu().numpy().tobytes() == image.tobytes(), (r, k)
    with pytest.raises(_lib.XywsError):
        grp.broadcast(msgs, [[1, 1]], sends)
    with pytest.raises(_lib.XywsError):
        grp.broadcast(msgs, [[0]], sends)  # (connection 0 is no item of the sweep)

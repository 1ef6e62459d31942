"""xyws_backlog_streams on the device: a sweep's newest frames folded into
every room's log and the log copied behind every joiner's send bytes, through
the C-ABI. Expected values: the model (tests/backlog_model.py), which
tests/test_backlog_model.py holds to the reference's room, over the same
cases. Bar: bit-exact logs, carries, send ranges and result rows; not a guard
byte changed around a log's halves, between abutting logs, in a send slab or in
row n + 1 of either result table; the wires and every input unchanged.

Plumbing: each case's broadcast runs on the device first (tests/test_gpu_room.py's
Bcast, checked against its own model), so the wires and room rows the backlog
reads are the ones the device wrote; tile, step and grid sizes come from
xyws_debug_backlog_geometry."""
import ctypes as C

import numpy as np
import pytest

import backlog_model as B
import room_model as R
from test_gpu_room import Bcast, Slab, vp
from test_gpu_streams import GUARD, as_array, download, ptr, upload
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
    assert _lib.load().xyws_debug_backlog_geometry(out) == 0
    return list(out)


def diff(what, got, want, offs):
    if got.tobytes() != want.tobytes():
        bad = int(np.flatnonzero(got != want)[0])
        k = max([j for j in range(len(offs)) if offs[j] <= bad], default=-1)
        raise AssertionError((what, "entry", k, "at", bad - offs[max(k, 0)], "got", int(got[bad]), "want",
                              int(want[bad])))


class Dev:
    """A case's logs and carries on the device; its calls run one after another on them."""

    def __init__(self, case):
        self.case, self.nr = case, len(case.brooms)
        logs = Slab()
        for r, br in enumerate(case.brooms):
            logs.add(br.log_cap, case.lmis[r] if case.lmis else None, bytes(br.log))
        self.logs = logs.place()
        car = b"".join(br.carry.pack() for br in case.brooms)
        self.car_t = upload(np.concatenate([as_array(car), np.full(192, GUARD, np.uint8)]))
        tab = np.zeros((self.nr, 4), np.uint64)
        for r, br in enumerate(case.brooms):
            tab[r] = [0 if br.log_null else ptr(self.logs.t) + logs.offs[r], br.log_cap,
                      0 if br.bc_null else ptr(self.car_t) + 192 * r, br.keep]
        self.brooms_image = tab.reshape(-1).view(np.uint8)
        self.brooms_t = upload(self.brooms_image)

    def call(self, ctx, call, what=""):
        case = self.case
        b = Bcast(call.conns, call.rooms, **call.kw).launch(ctx).check((case.name, what, "broadcast"))
        assert b.nr == self.nr
        n = b.n
        rr_t = b.rr_t
        if call.rows is not None:
            img = download(b.rr_t).copy()
            for r, row in enumerate(call.rows):
                if row is not None:
                    img[32 * r:32 * r + 32] = as_array(R.pack_room_result(row))
            rr_t = upload(img)
        rr_image, wires_image, sends_image = download(rr_t).copy(), download(b.wires.t).copy(), download(b.sends.t).copy()
        jt = None
        if call.jconns is not None:
            B.resolve(call, b.model)
            tab = np.zeros((n, 8), np.uint64)
            for k, (j, c) in enumerate(zip(call.jconns, call.conns)):
                tab[k, :5] = [0 if j.out_null else ptr(b.sends.t) + b.sends.offs[k], j.send_cap,
                              ptr(b.res_t) + 32 * k if j.use_bcast else 0,
                              ptr(b.rpl_t) + 32 * k if j.use_reply and c.reply is not None else 0,
                              j.room | ((B.BL_JOIN if j.join else 0) << 32)]
            jt = upload(tab.reshape(-1).view(np.uint8))
            res_t = upload(np.full(32 * (n + 1), GUARD, np.uint8))
        brr_t = upload(np.full(32 * (self.nr + 1), GUARD, np.uint8))
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = ctx.L.xyws_backlog_streams(ctx.h, C.c_void_p(b.reasm_p), C.c_void_p(b.rres_p), vp(b.bconns_t), n,
                                        vp(b.rooms_t), vp(rr_t), vp(self.brooms_t), vp(brr_t), self.nr,
                                        vp(jt), vp(res_t) if jt is not None else None, s)
        assert rc == 0
        _, rres, whys, dl = B.run_call(case, call)
        # the logs: every byte of the slab
        want = self.logs.image.copy()
        for r, br in enumerate(case.brooms):
            want[self.logs.offs[r]:self.logs.offs[r] + br.log_cap] = as_array(bytes(br.log))
        diff((case.name, what, "log"), download(self.logs.t), want, self.logs.offs)
        self.logs.image = want
        car = download(self.car_t)
        for r, br in enumerate(case.brooms):
            assert car[192 * r:192 * r + 192].tobytes() == br.carry.pack(), (
                case.name, what, "carry", r, whys[r], car[192 * r:192 * r + 192].view(np.uint64), vars(br.carry))
        assert (car[192 * self.nr:] == GUARD).all(), (case.name, what, "carry guard")
        rows = download(brr_t)
        for r in range(self.nr):
            assert rows[32 * r:32 * r + 32].tobytes() == B.pack_room_result(rres[r]), (
                case.name, what, "room result", r, whys[r], rres[r], rows[32 * r:32 * r + 32].view(np.uint32))
        assert (rows[32 * self.nr:] == GUARD).all(), (case.name, what, "room result guard")
        # the send ranges: what the broadcast left, plus the backlogs
        want = sends_image.copy()
        if dl is not None:
            res = download(res_t)
            for k, (lo, data, r) in enumerate(dl):
                o = b.sends.offs[k]
                want[o + lo:o + lo + len(data)] = as_array(data)
                assert res[32 * k:32 * k + 32].tobytes() == B.pack_result(r), (
                    case.name, what, "result", k, r, res[32 * k:32 * k + 32].view(np.uint64))
            assert (res[32 * n:] == GUARD).all(), (case.name, what, "result guard")
        diff((case.name, what, "send bytes"), download(b.sends.t), want, b.sends.offs)
        # the inputs
        assert download(b.wires.t).tobytes() == wires_image.tobytes(), (case.name, what, "a wire changed")
        assert download(rr_t).tobytes() == rr_image.tobytes(), (case.name, what, "a room row changed")
        assert download(self.brooms_t).tobytes() == self.brooms_image.tobytes()
        for t, image in b.inputs:
            assert download(t).tobytes() == image.tobytes(), (case.name, what, "an input changed")
        return b, rres, whys, dl


def run(ctx, case):
    d = Dev(case)
    return d, [d.call(ctx, call, s) for s, call in enumerate(case.calls)]


# --------------------------------------------------------------------------- 1. fold seams
def test_fold_seams(ctx):
    case = B.fold_seams()
    d, ((b, rres, whys, _),) = run(ctx, case)
    seen = set()
    for r, br in enumerate(case.brooms):  # (log, the new suffix's first byte in the wire) mod 16
        b_new = sum(br.carry.flen[br.carry.count - rres[r]["folded"]:br.carry.count])
        seen.add(((ptr(d.logs.t) + d.logs.offs[r]) % 16,
                  (ptr(b.wires.t) + b.wires.offs[r] + b.model.rooms[r][2]["wire_len"] - b_new) % 16))
    assert len(seen) == 256
    assert all(w == "kept" and r["folded"] == (3 if r["count"] == 4 else 2) for w, r in zip(whys, rres))
    assert sorted({r["count"] - r["folded"] for r in rres}) == [0, 1]
    assert sorted({br.carry.flen[0] for br in case.brooms if br.carry.count == 4}) == [1, 15, 16, 17, 33]


# --------------------------------------------------------------------------- 2. frame sizes
def test_frame_sizes(ctx):
    case = B.frame_sizes()
    _, ((b, rres, whys, _),) = run(ctx, case)
    assert all(r == B.room_result(r["len"], 2, 2, 1, 0) for r in rres)
    assert sorted({br.carry.flen[1] - t for br, t in zip(case.brooms, (125, 125, 126, 126, 65535, 65535, 65536,
                                                                       65536))}) == [2, 4, 10]


# --------------------------------------------------------------------------- 3. members and tiles
def test_members_and_tiles(ctx):
    T = geometry()[0]
    case = B.member_tiles(T)
    _, ((b, rres, whys, _),) = run(ctx, case)
    assert [len(rm.members) for rm in b.rooms[:4]] == [T - 1, T, T + 1, 2 * T + 3]
    assert all(r["count"] == 10 and r["folded"] == 10 and r["dropped"] == 2 for r in rres[:4])
    assert b.model.rooms[4][2]["status"] & R.ROOM_BAD_MEMBER and rres[4]["folded"] == 10
    assert rres[5] == B.room_result(rres[5]["len"], 3, 3, 0, 0)
    # the last keep messages of the room of T + 1 members come from both tiles
    owners = [i for i, _, _, _ in b.model.rooms[2][1]][-10:]
    lo = b.rooms[2].members[0]
    assert min(owners) - lo < T <= max(owners) - lo


# --------------------------------------------------------------------------- 4. rules
def test_rules_over_four_chained_calls(ctx):
    case = B.rules()
    d = Dev(case)
    runs, starts = [], []
    for s, call in enumerate(case.calls):
        runs.append(d.call(ctx, call, s))
        starts.append([br.carry.start for br in case.brooms])
    st = [[r["status"] for r in rres] for _, rres, _, _ in runs]
    assert all(s[4:8] == [B.BL_PASSTHROUGH] * 4 for s in st)
    assert [s[8] for s in st] == [0, B.BL_EVICTED, B.BL_EVICTED, B.BL_EVICTED | B.BL_TOO_LONG]
    assert [w[9] for _, _, w, _ in runs] == ["kept", "n0", "kept", "n0"]
    assert st[0][10] == st[0][14] == st[0][15] == st[0][16] == B.BL_BAD_CARRY
    assert st[1][11] == st[2][12] == B.BL_MISMATCH | B.BL_GAP and st[1][13] == B.BL_GAP
    assert [case.brooms[r].carry.gaps for r in (11, 12, 13)] == [1, 1, 1]
    for r in (0, 1, 2, 3):  # the halves alternate
        H = case.brooms[r].H
        assert [s[r] for s in starts] == [0, H, 0, H], r
    assert [case.brooms[r].carry.count for r in range(4)] == [1, 10, 16, 16]


# --------------------------------------------------------------------------- 5. grid stride
def test_more_rooms_and_connections_than_the_grid(ctx):
    G = geometry()[2]
    case = B.over_grid(G)
    _, ((b, rres, whys, dl),) = run(ctx, case)
    assert b.n == b.nr == G + 3 and all(r["folded"] == 1 for r in rres)
    assert sum(bool(r["status"] & B.BLC_JOINED) for _, _, r in dl) == (G + 3 + 2) // 3


# --------------------------------------------------------------------------- 6. delivery
def test_delivery_alignment_matrix(ctx):
    case = B.delivery_matrix()
    d, ((b, rres, whys, dl),) = run(ctx, case)
    assert set(whys) == {"n0"}
    seen = {((ptr(d.logs.t) + d.logs.offs[j.room] + case.brooms[j.room].carry.start) % 16,
             (ptr(b.sends.t) + b.sends.offs[k] + j.base) % 16) for k, j in enumerate(case.calls[0].jconns)}
    assert len(seen) == 256
    assert sorted({r["backlog_len"] for _, _, r in dl}) == list(B.LENGTHS)
    assert B.LENGTHS[-1] > geometry()[1] + 16


def test_delivery_rules(ctx):
    case = B.delivery_rules()
    _, ((b, rres, whys, dl), (_, rres2, whys2, dl2)) = run(ctx, case)
    cov = B.Coverage().add_delivery(case.calls[0].jconns, dl)
    cov.require("joined", "join_truncated", "join_no_room", "join_not_receiver", "non_joiner", "empty_join")
    assert rres[0]["folded"] == 1 and rres[0]["len"] == 12 + 35 and dl2 is None
    assert rres2[0] == B.room_result(35, 1, 1, 2, B.BL_EVICTED)  # (the second call, fold only: the frame again)


# --------------------------------------------------------------------------- 7. the real six-call sweep
LOG_CAP = B.cap_for(400)
KEEPS = (10, 2)


def real_rooms():
    brooms = [B.BRoom(LOG_CAP, keep=k) for k in KEEPS]
    for br in brooms:
        br.log = bytearray([GUARD]) * LOG_CAP
    return brooms


class SixCalls:
    """decode -> reassemble -> hold -> reply -> broadcast -> backlog over fixed
    buffers (tests/test_gpu_hold.py's Pipeline and one call more), the rooms'
    member lists, the connections' rooms and the joiners copied into the fixed
    tables before each sweep."""

    def __init__(self, oracle):
        import hold_model as HM
        import test_gpu_hold as GH
        sweeps, caps, memberships, room_ofs, joiners = B.sweep_streams()
        self.p = p = GH.Pipeline(oracle, sweeps, caps, memberships[-1], room_ofs[-1])
        self.nsweeps, n = len(sweeps), p.n
        st, hst = R.SweepState(), HM.State()
        hst.hold = {i: bytes([GUARD]) * GH.HOLD_CAP for i in range(n)}
        p.runs = [HM.real_sweep(oracle, st, hst, pieces, p.caps, memberships[r], room_ofs[r], GH.HOLD_CAP,
                                send_cap=p.SEND, wire_cap=p.W, out_caps=[p.size] * n, msg_caps=[p.cap + 1] * n)
                  for r, pieces in enumerate(sweeps)]
        # the model of the sixth call, sweep after sweep
        brooms, self.want = real_rooms(), []
        for r in range(self.nsweeps):
            vconns, rooms, res = p.runs[r][3], p.runs[r][4], p.runs[r][6]
            jc = B.real_jconns(vconns, res, joiners[r])
            rres, whys, dl = B.backlog(vconns, rooms, res, brooms, jc)
            self.want.append((rres, dl, [bytes(br.log) for br in brooms], [br.carry.pack() for br in brooms]))
        dev = dict(device="cuda", dtype=torch.uint8)
        nr = len(KEEPS)
        self.logs = torch.full((64 + nr * LOG_CAP + 64,), GUARD, **dev)
        self.car = torch.zeros(192 * nr, **dev)
        self.blrr, self.blres = torch.zeros(32 * nr, **dev), torch.zeros(32 * n, **dev)
        tab = np.zeros((nr, 4), np.uint64)
        for r in range(nr):
            tab[r] = [ptr(self.logs) + 64 + LOG_CAP * r, LOG_CAP, ptr(self.car) + 192 * r, KEEPS[r]]
        self.brooms_t = upload(tab.reshape(-1).view(np.uint8))
        # per sweep: members, rooms, bconns (the room column), jconns
        base_b = download(p.btab_t).view(np.uint64).reshape(n, 8)
        self.stage = []
        for r in range(self.nsweeps):
            flat = [i for m in memberships[r] for i in m]
            flat += [0] * (p.members_t.numel() - len(flat))
            roomtab, pos = np.zeros((nr, 4), np.uint64), 0
            for j, m in enumerate(memberships[r]):
                roomtab[j] = [ptr(p.members_t) + 4 * pos, len(m), ptr(p.wires) + p.W * j, p.W]
                pos += len(m)
            bt = base_b.copy()
            bt[:, 5] = room_ofs[r]
            jt = np.zeros((n, 8), np.uint64)
            for i in range(n):
                room = dict(joiners[r]).get(i)
                jt[i, :5] = [ptr(p.sends) + p.SEND * i, p.SEND, ptr(p.bres) + 32 * i, ptr(p.rres) + 32 * i,
                             R.NONE if room is None else room | (B.BL_JOIN << 32)]
            self.stage.append((upload(np.asarray(flat, np.uint32)), upload(roomtab.reshape(-1).view(np.uint8)),
                               upload(bt.reshape(-1).view(np.uint8)), upload(jt.reshape(-1).view(np.uint8))))
        self.jtab_t = torch.zeros_like(self.stage[0][3])

    def calls(self, ctx, stream):
        p = self.p
        p.calls(ctx, stream)
        assert ctx.L.xyws_backlog_streams(ctx.h, vp(p.view), vp(p.vres), vp(p.btab_t), p.n, vp(p.roomtab_t), vp(p.rrres),
                                          vp(self.brooms_t), vp(self.blrr), len(KEEPS), vp(self.jtab_t),
                                          vp(self.blres), C.c_void_p(stream)) == 0

    def load(self, r):
        p = self.p
        p.load(r)
        for dst, src in zip((p.members_t, p.roomtab_t, p.btab_t, self.jtab_t), self.stage[r]):
            dst.copy_(src)

    def keep(self):
        return self.p.keep(), tuple(t.clone() for t in (self.logs, self.car, self.blrr, self.blres))

    def check(self, r, kept):
        p, (five, (logs, car, blrr, blres)) = self.p, kept
        rres, dl, want_logs, want_car = self.want[r]
        sd = download(five[0]).copy()
        res = download(blres)
        for i, (lo, data, row) in enumerate(dl):  # the backlog bytes, then the five-call checks on the rest
            a = p.SEND * i + lo
            assert sd[a:a + len(data)].tobytes() == data, (r, "backlog bytes", i)
            sd[a:a + len(data)] = GUARD
            assert res[32 * i:32 * i + 32].tobytes() == B.pack_result(row), (r, "backlog result", i, row)
        p.check(r, (torch.from_numpy(sd),) + tuple(five[1:]))
        lg, cr, rr = download(logs), download(car), download(blrr)
        for j in range(len(KEEPS)):
            a = 64 + LOG_CAP * j
            assert lg[a:a + LOG_CAP].tobytes() == want_logs[j], (r, "log", j)
            assert cr[192 * j:192 * j + 192].tobytes() == want_car[j], (r, "carry", j)
            assert rr[32 * j:32 * j + 32].tobytes() == B.pack_room_result(rres[j]), (r, "room result", j, rres[j])
        assert (lg[:64] == GUARD).all() and (lg[64 + len(KEEPS) * LOG_CAP:] == GUARD).all(), (r, "log guards")
        return dl


def joiner_saw_the_room(six, dls):
    """Connection 8 is sent room 0's talk of sweeps 1 and 2 when it joins, the
    message that spanned them included, and sweep 3's as a member."""
    cut = R.header(R.FIN | R.TEXT, 12 + 17) + R.HEAD24[:12] + b"cut in two sweeps"
    lo, data, row = dls[1][8]
    assert row["status"] == B.BLC_JOINED and cut in data and b"hello room" in data and row["backlog_len"] == len(data)
    assert all(not d for i, (_, d, _) in enumerate(dls[1]) if i != 8) and not any(d for dl in (dls[0], dls[2])
                                                                                  for _, d, _ in dl)
    assert b"the newcomer speaks" in six.p.runs[2][6].conns[8][1]
    assert six.want[2][0][0]["folded"] >= 3 and six.want[1][0][1]["count"] == 2


def test_the_real_six_call_sweep(ctx, oracle):
    six = SixCalls(oracle)
    stream = torch.cuda.current_stream().cuda_stream
    kept = []
    for r in range(six.nsweeps):
        six.load(r)
        six.calls(ctx, stream)
        kept.append(six.keep())
    torch.cuda.synchronize()
    joiner_saw_the_room(six, [six.check(r, k) for r, k in enumerate(kept)])


def test_six_calls_captured_and_replayed(ctx, oracle):
    """The six calls captured once on one stream, replayed for the three sweeps
    with new bytes and tables copied into the same buffers in between; each
    replay against the model."""
    six = SixCalls(oracle)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        six.calls(ctx, s.cuda_stream)
    torch.cuda.synchronize()
    assert bool((six.logs == GUARD).all()) and not bool(six.car.any())  # (capture ran nothing)
    kept = []
    with torch.cuda.stream(s):
        for r in range(six.nsweeps):
            six.load(r)
            g.replay()
            kept.append(six.keep())
    torch.cuda.synchronize()
    joiner_saw_the_room(six, [six.check(r, k) for r, k in enumerate(kept)])


# --------------------------------------------------------------------------- 8. the Python layer
def test_connection_group_backlog(ws, ctx, oracle):
    import hold_model as HM
    from test_gpu_hold import HOLD_CAP
    from test_gpu_parity import dev_bytes
    sweeps, caps, memberships, room_ofs, joiners = B.sweep_streams()
    n, SEND = len(caps), 2048
    size = max(len(p) for s in sweeps for p in s) + 3
    grp = ws.connection_group(n + 1, cap=8, ctx=ctx)
    st, hst = R.SweepState(), HM.State()
    hst.hold = {i: bytes([GUARD]) * HOLD_CAP for i in range(n)}
    heads = [None] + [upload(as_array(R.HEAD24[:3 * k])) for k in range(1, n)]
    areas = [torch.full((HOLD_CAP + size,), GUARD, dtype=torch.uint8, device="cuda") for _ in range(n)]
    brooms = [B.BRoom(LOG_CAP, keep=10) for _ in KEEPS]
    for r, pieces in enumerate(sweeps):
        exp, replies, conns, vconns, rooms, plain, res, houts = HM.real_sweep(
            oracle, st, hst, pieces, [8] * n, memberships[r], room_ofs[r], HOLD_CAP, msg_caps=[9] * n,
            out_caps=[len(p) + 3 for p in pieces], send_cap=SEND)
        rres, _, dl = B.backlog(vconns, rooms, res, brooms, B.real_jconns(vconns, res, joiners[r]))
        items = [(i + 1, dev_bytes(p, 1 + i)[0]) for i, p in enumerate(pieces)]
        outs = [areas[i][HOLD_CAP:HOLD_CAP + len(p) + 3] for i, p in enumerate(pieces)]
        sends = [torch.full((SEND,), GUARD, dtype=torch.uint8, device="cuda") for _ in vconns]
        dec = grp.decode(items)
        msgs = grp.reassemble(dec, outs)
        rep = grp.reply(dec, sends, 1 << 20, policy=_lib.POL_FRAGMENTS, flags=0, enc_opts=_lib.ENC_FRAME_OPCODE,
                        action_mask=1 << _lib.ACT_PING)
        held = grp.hold(msgs, HOLD_CAP)
        got = grp.broadcast(held, [[i + 1 for i in m] for m in memberships[r]], sends, heads=heads, reply=rep)
        bl = grp.backlog(got, joiners=[(i + 1, room) for i, room in joiners[r]], keep=10, log_cap=LOG_CAP)
        for j, br in enumerate(brooms):
            rr, want = bl.room_result(j), rres[j]
            assert (rr.len, rr.count, rr.folded, rr.dropped, rr.status) == \
                (want["len"], want["count"], want["folded"], want["dropped"], want["status"]), (r, j)
            assert bytes(grp.backlog_carry(j)) == br.carry.pack(), (r, j)
            assert grp.backlog_bytes(j).cpu().numpy().tobytes() == br.held(), (r, j)
        for k, c in enumerate(vconns):
            row, (lo, data, want) = bl.result(k), dl[k]
            assert (row.send_len, row.backlog_len, row.status) == (want["send_len"], want["backlog_len"],
                                                                   want["status"]), (r, k)
            blo, bdata, _ = res.conns[k]
            image = np.full(SEND, GUARD, np.uint8)
            image[:len(c.prefix)] = as_array(c.prefix)
            image[blo:blo + len(bdata)] = as_array(bdata)
            image[lo:lo + len(data)] = as_array(data)
            assert sends[k].cpu().numpy().tobytes() == image.tobytes(), (r, k)
        if r == 1:
            assert dl[8][2]["status"] == B.BLC_JOINED and b"cut in two sweeps" in dl[8][1]
    with pytest.raises(_lib.XywsError):
        grp.backlog(got, joiners=[(0, 0)])   # (connection 0 is no item of the sweep)
    with pytest.raises(_lib.XywsError):
        grp.backlog(got, joiners=[(1, 7)])   # (no such room)
    with pytest.raises(_lib.XywsError):
        grp.backlog(msgs)


def test_connection_group_backlog_joiner_that_closed_or_overflowed(ws, ctx):
    """A joiner is not yet a member, so its broadcast row says NO_ROOM: only
    its reply row can say that it closed or overflowed in the sweep in which
    it joins. With broadcast() given the sweep's reply such a joiner is sent
    nothing; without it the layer has no reply row to name."""
    from test_gpu_parity import dev_bytes
    rng = R.streams.SplitMix(0x701E)
    pieces = [R._f(rng, 0x81, b"hello"), R._f(rng, 0x81, b"room") + R._f(rng, 0x81, b"zero"),
              R._f(rng, 0x88, b"\x03\xe8"),                                               # 2 joins and closes
              R._f(rng, 0x81, b"a") + R._f(rng, 0x81, b"b") + R._f(rng, 0x81, b"c"),      # 3 joins, more frames than cap
              b""]                                                                        # 4 joins
    n, SEND = len(pieces), 256
    wire = b"".join(R.header(R.FIN | R.TEXT, len(m)) + m for m in (b"hello", b"room", b"zero"))
    for with_reply in (True, False):
        grp = ws.connection_group(n, cap=2, ctx=ctx)
        items = [(i, dev_bytes(p, 1 + i)[0]) for i, p in enumerate(pieces)]
        outs = [torch.full((t.numel() + 3,), GUARD, dtype=torch.uint8, device="cuda") for _, t in items]
        sends = [torch.full((SEND,), GUARD, dtype=torch.uint8, device="cuda") for _ in items]
        dec = grp.decode(items)
        msgs = grp.reassemble(dec, outs)
        rep = grp.reply(dec, sends, 1 << 20, policy=_lib.POL_FRAGMENTS, flags=0, enc_opts=_lib.ENC_FRAME_OPCODE,
                        action_mask=1 << _lib.ACT_PING)
        assert rep.result(2).status & _lib.RPL_CLOSED and rep.result(3).status & _lib.RPL_OVERFLOW
        assert not rep.result(4).status
        before = [t.clone() for t in sends]
        got = grp.broadcast(msgs, [[0, 1]], sends, reply=rep if with_reply else None)
        assert got.wire(0).cpu().numpy().tobytes() == wire
        assert all(got.result(k).status == _lib.BC_NO_ROOM for k in (2, 3, 4))
        bl = grp.backlog(got, joiners=[(2, 0), (3, 0), (4, 0)], keep=10, log_cap=LOG_CAP)
        rr = bl.room_result(0)
        assert (rr.len, rr.count, rr.folded, rr.status) == (len(wire), 3, 3, 0)
        base = [rep.result(k).reply_len if with_reply else 0 for k in range(n)]
        for k in (2, 3):
            row = bl.result(k)
            if with_reply:  # closed, overflowed: nothing behind the close frame
                assert (row.send_len, row.backlog_len, row.status) == (base[k], 0, _lib.BLC_NOT_RECEIVER), k
                assert sends[k].cpu().numpy().tobytes() == before[k].cpu().numpy().tobytes(), k
            else:
                assert (row.send_len, row.backlog_len, row.status) == (len(wire), len(wire), _lib.BLC_JOINED), k
        row = bl.result(4)
        assert (row.send_len, row.backlog_len, row.status) == (base[4] + len(wire), len(wire), _lib.BLC_JOINED)
        image = before[4].cpu().numpy().copy()
        image[base[4]:base[4] + len(wire)] = as_array(wire)
        assert sends[4].cpu().numpy().tobytes() == image.tobytes()
        assert rep.result(2).reply_len > 0  # (the close frame the backlog must not follow)
        with pytest.raises(_lib.XywsError):
            grp.backlog(got, keep=10, log_cap=LOG_CAP + 16)  # (a room's log keeps its log_cap)
        with pytest.raises(IndexError):
            bl.result(n)
        with pytest.raises(IndexError):
            bl.room_result(1)

"""xyws_hold_streams on the device: the parts of a message a recv boundary
cut kept in the connection's hold, the whole message handed to
xyws_broadcast_streams through the view, through the C-ABI. Expected values:
the model (tests/hold_model.py), which tests/test_hold_model.py holds to the
reference's reassembly of the unsplit stream, over the same scenarios. Bar:
bit-exact hold bytes, view table, view rows, view records, carries and result
rows; not a guard byte changed in front of a hold, between areas, in a view
record past min(s, vmsg_cap) or in row n + 1 of a table; the inputs unchanged.

Plumbing as in tests/test_gpu_room.py: every connection's area (its hold, then
its reassembly range) lies in ONE guard-filled device buffer, out
misalignments 0..15, or the areas packed back to back; lanes, line, step and
grid sizes come from xyws_debug_hold_geometry."""
import ctypes as C

import numpy as np
import pytest

import hold_model as HM
import reasm_model as M
import reasm_streams_model as SM
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
    assert _lib.load().xyws_debug_hold_geometry(out) == 0
    return list(out)


def vp(t, off=0):
    return C.c_void_p(ptr(t) + off) if t is not None else None


def pad_for(ins, caps, omis, start=64):
    """Areas packed back to back with out of connection k at misalignment
    omis[k]: the reassembly range before it grows by up to 15 unnamed bytes.
    Returns the first area's offset."""
    pos = start + (omis[0] - (start + caps[0])) % 16
    first = pos
    for k, inp in enumerate(ins):
        pos += caps[k] + inp.out_cap
        if k + 1 < len(ins):
            pad = (omis[k + 1] - (pos + caps[k + 1])) % 16
            inp.buf += bytes([HM.FILL]) * pad
            pos += pad
    return first


class HoldCall:
    """One xyws_hold_streams call over the model's Outs (HM.State.sweep ran
    already: each Out carries its inputs). packed: areas back to back from
    `start`; else out of connection k at misalignment k % 16, guard bytes
    between areas. results = False: a null dev_results."""

    def __init__(self, outs, packed=False, start=64, results=True):
        n = self.n = len(outs)
        self.outs = outs
        pos, self.aoffs = start, []
        for k, o in enumerate(outs):
            if not packed:
                pos = (pos + 15) // 16 * 16 + 48
                pos += (k % 16 - (pos + o.hold_cap)) % 16
            self.aoffs.append(pos)
            pos += o.hold_cap + o.inp.out_cap
        self.image = np.full(pos + 64, GUARD, np.uint8)
        self.want = self.image.copy()
        for k, o in enumerate(outs):
            a = self.aoffs[k]
            before, after = o.hold_in + o.inp.buf, o.hold + o.inp.buf
            self.image[a:a + len(before)] = as_array(before)
            self.want[a:a + len(after)] = as_array(after)
        self.areas_t = upload(self.image)
        base = ptr(self.areas_t)
        # record rows: the stored records and a guard record; the view's rows: guards
        self.moffs, self.voffs, mt, vt = [], [], 0, 0
        for o in outs:
            self.moffs.append(mt)
            self.voffs.append(vt)
            mt += len(o.inp.recs) + 1
            vt += o.vmsg_cap + 1
        self.msgs_image = np.full(40 * mt, GUARD, np.uint8)
        for k, o in enumerate(outs):
            self.msgs_image[40 * self.moffs[k]:40 * (self.moffs[k] + len(o.inp.recs))] = \
                as_array(SM.pack_records(o.inp.recs))
        self.msgs_t = upload(self.msgs_image)
        self.vmsgs_t = upload(np.full(40 * vt, GUARD, np.uint8))
        self.hc_image = np.concatenate([as_array(o.carry_in.pack()) for o in outs] + [np.full(32, GUARD, np.uint8)])
        self.hc_t = upload(self.hc_image)
        tab, htab = np.zeros((n, 8), np.uint64), np.zeros((n, 4), np.uint64)
        rres = np.zeros(32 * n, np.uint8)
        for k, o in enumerate(outs):
            inp = o.inp
            tab[k, :5] = [0 if inp.out_null else base + self.aoffs[k] + o.hold_cap, inp.out_cap, 0x1000 + 64 * k,
                          0 if inp.msgs_null else ptr(self.msgs_t) + 40 * self.moffs[k],
                          7 if inp.msgs_null else inp.msg_cap]
            htab[k] = [o.hold_cap, 0 if o.hc_null else ptr(self.hc_t) + 32 * k,
                       0 if o.vmsgs_null else ptr(self.vmsgs_t) + 40 * self.voffs[k], o.vmsg_cap]
            rres[32 * k:32 * k + 32] = as_array(SM.pack_result(inp.row))
        self.tab, self.htab, self.rres = tab, htab, rres
        self.tab_t, self.htab_t, self.rres_t = (upload(t.reshape(-1).view(np.uint8)) for t in (tab, htab, rres))
        self.view_t = upload(np.full(64 * (n + 1), GUARD, np.uint8))
        self.vres_t = upload(np.full(32 * (n + 1), GUARD, np.uint8))
        self.res_t = upload(np.full(32 * (n + 1), GUARD, np.uint8)) if results else None

    def launch(self, ctx, stream=None):
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream)
        assert ctx.L.xyws_hold_streams(ctx.h, vp(self.tab_t), vp(self.rres_t), vp(self.htab_t), self.n, vp(self.view_t),
                                       vp(self.vres_t), vp(self.res_t), s) == 0
        return self

    def check(self, what=""):
        n = self.n
        got = download(self.areas_t)
        if got.tobytes() != self.want.tobytes():
            bad = int(np.flatnonzero(got != self.want)[0])
            k = max([j for j in range(n) if self.aoffs[j] <= bad], default=-1)
            o = self.outs[max(k, 0)]
            raise AssertionError((what, "area bytes", "connection", k, "at", bad - self.aoffs[max(k, 0)], "hold_cap",
                                  o.hold_cap, "copies", o.copies, "got", int(got[bad]), "want", int(self.want[bad])))
        view, vres = download(self.view_t), download(self.vres_t)
        vm = download(self.vmsgs_t)
        vwant = np.full(vm.size, GUARD, np.uint8)
        hc = download(self.hc_t)
        for k, o in enumerate(self.outs):
            row = self.tab[k].copy()
            if not o.passthrough:
                row[:] = [int(self.tab[k, 0]) - o.hold_cap, o.hold_cap + o.inp.out_cap, int(self.tab[k, 2]),
                          int(self.htab[k, 2]), o.view_msg_cap, 0, 0, 0]
                vwant[40 * self.voffs[k]:40 * (self.voffs[k] + len(o.view_recs))] = \
                    as_array(SM.pack_records(o.view_recs))
            assert view[64 * k:64 * k + 64].tobytes() == row.tobytes(), (
                what, "view entry", k, view[64 * k:64 * k + 64].view(np.uint64), row)
            assert vres[32 * k:32 * k + 32].tobytes() == SM.pack_result(o.view_row), (
                what, "view row", k, o.view_row, vres[32 * k:32 * k + 32].view(np.uint32))
            want = o.carry_in if o.passthrough else o.carry
            assert hc[32 * k:32 * k + 32].tobytes() == want.pack(), (
                what, "carry", k, hc[32 * k:32 * k + 32].view(np.uint64), want, o.events)
        assert (view[64 * n:] == GUARD).all() and (vres[32 * n:] == GUARD).all() and (hc[32 * n:] == GUARD).all(), \
            (what, "row n + 1")
        if vm.tobytes() != vwant.tobytes():
            bad = int(np.flatnonzero(vm != vwant)[0]) // 40
            k = max(j for j in range(n) if self.voffs[j] <= bad)
            raise AssertionError((what, "view record", "connection", k, "index", bad - self.voffs[k], "got",
                                  vm[40 * bad:40 * bad + 40].view(np.uint64), "want", self.outs[k].view_recs))
        if self.res_t is not None:
            res = download(self.res_t)
            for k, o in enumerate(self.outs):
                assert res[32 * k:32 * k + 32].tobytes() == HM.pack_result(o.result), (
                    what, "result", k, o.result, o.events, res[32 * k:32 * k + 32].view(np.uint64))
            assert (res[32 * n:] == GUARD).all(), (what, "result guard")
        for t, image in ((self.msgs_t, self.msgs_image), (self.tab_t, self.tab), (self.htab_t, self.htab),
                         (self.rres_t, self.rres)):
            assert download(t).tobytes() == image.tobytes(), (what, "an input changed")
        return self


def sweep_with(ins, carries, caps, vmsg_caps=None, **kw):
    hst = HM.State()
    hst.hc = dict(enumerate(carries))
    return hst.sweep(ins, caps, vmsg_caps=vmsg_caps, **kw)


# --------------------------------------------------------------------------- 1. copy seams
@pytest.mark.parametrize("kind", HM.SEAM_KINDS)
def test_copy_seams(ctx, kind):
    lanes, line, step, _ = geometry()
    ins, carries, caps, omis = HM.seam_call(step, kind)
    start = pad_for(ins, caps, omis)
    outs = sweep_with(ins, carries, caps)
    call = HoldCall(outs, packed=True, start=start).launch(ctx).check(kind)
    assert all(("append" if kind.startswith("append") else kind) in o.events for o in outs)
    kind = HM.SEAM_KINDS.index(kind)
    lengths = {c[2] for o in outs for c in o.copies}
    assert {0, 1, 15, 16, 17, step - 1, step, step + 1, 2 * step + 1} <= lengths
    # every out misalignment with every source misalignment, every hold_cap tail with every out misalignment
    base = ptr(call.areas_t)
    assert base % 16 == 0
    seen = {((base + call.aoffs[k] + o.hold_cap) % 16, (base + call.aoffs[k] + o.hold_cap + o.copies[-1][1]) % 16)
            for k, o in enumerate(outs)}
    assert len(seen) == 256
    assert len({((base + call.aoffs[k] + o.hold_cap) % 16, o.hold_cap % 32) for k, o in enumerate(outs)}) == 64
    if kind >= 2:
        assert {o.carry_in.held for o in outs} == {1, 15, 16, 17}
        assert {o.carry_in.start for o in outs} == ({0} if kind == 2 else {HM.half(caps[0])})


# --------------------------------------------------------------------------- 2. record rows
def test_record_rows(ctx):
    ins, carries, vcaps = HM.row_calls()
    outs = sweep_with(ins, carries, 158, vmsg_caps=vcaps)
    HoldCall(outs).launch(ctx).check("rows")
    assert sorted({len(o.inp.recs) for o in outs}) == [0, 1, 2, 63, 64, 65, 129]
    assert {(len(o.inp.recs), o.vmsg_cap) for o in outs} >= {(129, 0), (129, 1), (129, 128), (129, 129), (65, 64)}
    assert any(o.delivered is not None and o.view_recs and o.view_recs[0][0] == 0 for o in outs)
    assert any(o.delivered is not None and not o.view_recs for o in outs)  # (vmsg_cap 0: the carry is exact)
    # a null dev_results
    HoldCall(sweep_with(ins, carries, 158, vmsg_caps=vcaps), results=False).launch(ctx).check("null results")


# --------------------------------------------------------------------------- 3. more connections than the grid
def test_more_connections_than_the_grid(ctx):
    G = geometry()[3]
    ins, carries = HM.over_grid(G)
    outs = sweep_with(ins, carries, 64)
    HoldCall(outs, packed=True).launch(ctx).check("grid")
    assert len(outs) == G + 3 and sum(1 for o in outs if o.delivered is not None) == (G + 3 + 2) // 3
    assert {o.carry.start for o in outs if o.carry.status & HM.ACTIVE} == {0, 32}


# --------------------------------------------------------------------------- 4. loss and pass-through
def test_every_loss_path_and_pass_through(ctx):
    sweeps, kws = HM.loss_and_passthrough(64)
    hst, cov = HM.State(), HM.Coverage()
    for r, (ins, kw) in enumerate(zip(sweeps, kws)):
        outs = hst.sweep(ins, **kw)
        cov.add(outs)
        HoldCall(outs).launch(ctx).check(("loss", r))
        if r == 0:
            HM.bad_carry_for(hst)
    cov.require("too_long_begin", "too_long_append", "append_fills_half", "begin_fills_half", "truncated_begin",
                "truncated_append", "rec0_unstored", "last_unstored", "vmsg_cap0", "vmsg_cap_short", "mid_join",
                "interrupted", "utf8_bad_delivered", "overflow", "lost_cleared", "bad_carry", "pt_out_null",
                "pt_hc_null", "pt_h0", "begin_half1")


def test_n_zero_launches_nothing(ctx):
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert ctx.L.xyws_hold_streams(ctx.h, None, None, None, 0, None, None, None, s) == 0


# --------------------------------------------------------------------------- 5. the real sweep
HOLD_CAP = 2 * 64 + 30


class Pipeline:
    """decode -> reassemble -> hold -> reply -> broadcast over fixed buffers,
    the device tables chained: no host read between the calls. Connection i's
    area (hold, then reassembly range) is fixed across sweeps; areas are packed
    back to back."""

    def __init__(self, oracle, sweeps, caps, members, room_of, W=1024):
        n, cap = len(caps), 8
        self.n, self.cap, self.W, self.members = n, cap, W, members
        self.caps = caps = [cap if c == 8 else c for c in caps]
        size = self.size = max(len(p) for s in sweeps for p in s)
        SEND = self.SEND = size + 13 + W
        AREA = self.AREA = HOLD_CAP + size
        st, hst = R.SweepState(), HM.State()
        hst.hold = {i: bytes([GUARD]) * HOLD_CAP for i in range(n)}
        self.runs = [HM.real_sweep(oracle, st, hst, pieces, caps, members, room_of, HOLD_CAP, send_cap=SEND, wire_cap=W,
                                   out_caps=[size] * n, msg_caps=[cap + 1] * n) for pieces in sweeps]
        dev = dict(device="cuda", dtype=torch.uint8)
        self.recv = torch.full((n * size + 64,), GUARD, **dev)
        self.areas = torch.full((64 + n * AREA + 64,), GUARD, **dev)
        self.sends = torch.full((n * SEND + 64,), GUARD, **dev)
        self.wires = torch.full((len(members) * W + 64,), GUARD, **dev)
        self.heads = upload(as_array(R.HEAD24))
        self.frames = torch.zeros(n * cap * 32, **dev)
        self.msgs = torch.zeros(n * (cap + 1) * 40, **dev)
        self.vmsgs = torch.full((n * (cap + 1) * 40,), GUARD, **dev)
        self.dcar, self.mcar, self.rcar, self.hcar = zeros(64 * n), zeros(64 * n), zeros(32 * n), zeros(32 * n)
        self.counts = torch.zeros(n, dtype=torch.int64, device="cuda")
        self.mres, self.rres, self.bres, self.rrres, self.hres, self.vres = (torch.zeros(32 * max(n, len(members)), **dev)
                                                                             for _ in range(6))
        self.view = torch.zeros(64 * n, **dev)
        self.tabs, self.stage = [], []
        for pieces in sweeps:
            tab = np.zeros((n, 8), np.uint64)
            img = np.full(n * size, GUARD, np.uint8)
            for i in range(n):
                tab[i, :5] = [ptr(self.recv) + size * i, len(pieces[i]), ptr(self.dcar) + 64 * i,
                              ptr(self.frames) + 32 * cap * i, caps[i]]
                img[size * i:size * i + len(pieces[i])] = as_array(pieces[i])
            self.tabs.append(upload(tab.reshape(-1).view(np.uint8)))
            self.stage.append(upload(img))
        self.ctab = torch.zeros_like(self.tabs[0])
        mtab, rtab, btab = np.zeros((n, 8), np.uint64), np.zeros((n, 4), np.uint64), np.zeros((n, 8), np.uint64)
        htab = np.zeros((n, 4), np.uint64)
        for i in range(n):
            mtab[i, :5] = [self.out_ptr(i), size, ptr(self.mcar) + 64 * i, ptr(self.msgs) + 40 * (cap + 1) * i, cap + 1]
            htab[i] = [HOLD_CAP, ptr(self.hcar) + 32 * i, ptr(self.vmsgs) + 40 * (cap + 1) * i, cap + 1]
            rtab[i] = [ptr(self.sends) + SEND * i, SEND, ptr(self.rcar) + 32 * i, 0]
            btab[i, :6] = [ptr(self.heads) if i else 0, 3 * i, ptr(self.sends) + SEND * i, SEND,
                           ptr(self.rres) + 32 * i, room_of[i]]
        self.mtab = mtab
        flat = np.asarray([i for m in members for i in m], np.uint32)
        self.members_t = upload(flat)
        roomtab, pos = np.zeros((len(members), 4), np.uint64), 0
        for r, m in enumerate(members):
            roomtab[r] = [ptr(self.members_t) + 4 * pos, len(m), ptr(self.wires) + W * r, W]
            pos += len(m)
        self.mtab_t, self.rtab_t, self.btab_t, self.htab_t, self.roomtab_t = (
            upload(t.reshape(-1).view(np.uint8)) for t in (mtab, rtab, btab, htab, roomtab))

    def out_ptr(self, i):
        return ptr(self.areas) + 64 + self.AREA * i + HOLD_CAP

    def calls(self, ctx, stream):
        """The five calls of a sweep, in order, on one stream."""
        n, L, mode, sp = self.n, ctx.L, R.REPLY_MODE, C.c_void_p(stream)
        assert L.xyws_decode_streams(ctx.h, vp(self.ctab), n, vp(self.counts), 0, sp) == 0
        assert L.xyws_reassemble_streams(ctx.h, vp(self.ctab), vp(self.counts), vp(self.mtab_t), n, M.REASM_UTF8,
                                         vp(self.mres), sp) == 0
        assert L.xyws_hold_streams(ctx.h, vp(self.mtab_t), vp(self.mres), vp(self.htab_t), n, vp(self.view),
                                   vp(self.vres), vp(self.hres), sp) == 0
        assert L.xyws_reply_streams(ctx.h, vp(self.ctab), vp(self.counts), vp(self.rtab_t), n, 1 << 20, mode["policy"],
                                    mode["flags"], mode["enc_opts"], mode["action_mask"], vp(self.rres), sp) == 0
        assert L.xyws_broadcast_streams(ctx.h, vp(self.view), vp(self.vres), vp(self.btab_t), n, vp(self.roomtab_t),
                                        vp(self.rrres), len(self.members), 0x11, 0, vp(self.bres), sp) == 0

    def load(self, r):
        """Sweep r's bytes and table into the fixed buffers (device copies)."""
        self.recv[:self.n * self.size].copy_(self.stage[r])
        self.ctab.copy_(self.tabs[r])
        self.sends.fill_(GUARD)
        self.wires.fill_(GUARD)

    def keep(self):
        return tuple(t.clone() for t in (self.sends, self.wires, self.bres, self.rrres, self.hres, self.vres, self.view,
                                         self.vmsgs, self.hcar, self.areas))

    def check(self, r, kept):
        sd, wr, br, rr, hr, vr, vw, vm, hc, ar = (download(t) for t in kept)
        n, W, SEND, cap = self.n, self.W, self.SEND, self.cap
        exp, replies, conns, vconns, rooms, plain, res, outs = self.runs[r]
        for j in range(len(self.members)):
            w = res.rooms[j][0]
            assert rr[32 * j:32 * j + 32].tobytes() == R.pack_room_result(res.rooms[j][2]), (r, "room result", j)
            assert wr[W * j:W * j + len(w)].tobytes() == w and (wr[W * j + len(w):W * (j + 1)] == GUARD).all(), (r, j)
        for i, (c, o) in enumerate(zip(vconns, outs)):
            lo, data, cr = res.conns[i]
            assert br[32 * i:32 * i + 32].tobytes() == R.pack_bcast_result(cr), (r, "bcast result", i)
            want = np.full(SEND, GUARD, np.uint8)
            want[:len(c.prefix)] = as_array(c.prefix)
            want[lo:lo + len(data)] = as_array(data)
            assert sd[SEND * i:SEND * (i + 1)].tobytes() == want.tobytes(), (r, "send range", i)
            assert hr[32 * i:32 * i + 32].tobytes() == HM.pack_result(o.result), (r, "hold result", i, o.result)
            assert hc[32 * i:32 * i + 32].tobytes() == o.carry.pack(), (r, "hold carry", i, o.carry)
            assert vr[32 * i:32 * i + 32].tobytes() == SM.pack_result(o.view_row), (r, "view row", i)
            entry = np.asarray([self.out_ptr(i) - HOLD_CAP, HOLD_CAP + self.size, int(self.mtab[i, 2]),
                                ptr(self.vmsgs) + 40 * (cap + 1) * i, cap + 1, 0, 0, 0], np.uint64)
            assert vw[64 * i:64 * i + 64].tobytes() == entry.tobytes(), (r, "view entry", i)
            row = 40 * (cap + 1) * i
            assert vm[row:row + 40 * len(o.view_recs)].tobytes() == SM.pack_records(o.view_recs), (r, "view records", i)
            a = 64 + self.AREA * i
            assert ar[a:a + HOLD_CAP].tobytes() == o.hold, (r, "hold bytes", i, o.copies)
        assert (ar[:64] == GUARD).all() and (ar[64 + n * self.AREA:] == GUARD).all(), (r, "area guards")
        return res


def reaches_room_0(p, res):
    """Connection 4's message, cut by the recv boundary, in every receiver of room 0."""
    frame = R.header(R.FIN | R.TEXT, 12 + 17) + R.HEAD24[:12] + b"cut in two sweeps"
    receivers = [i for i in p.members[0] if not res.conns[i][2]["status"] & R.BC_NOT_RECEIVER]
    assert len(receivers) >= 2 and 4 in receivers
    return all(frame in res.conns[i][1] for i in receivers) and frame in res.rooms[0][0]


def test_the_real_sweep(ctx, oracle):
    sweeps, caps, members, room_of = R.sweep_streams()
    p = Pipeline(oracle, sweeps, caps, members, room_of)
    stream = torch.cuda.current_stream().cuda_stream
    kept = []
    for r in range(len(sweeps)):
        p.load(r)
        p.calls(ctx, stream)
        kept.append(p.keep())
    torch.cuda.synchronize()
    results = [p.check(r, k) for r, k in enumerate(kept)]
    assert not reaches_room_0(p, results[0]) and reaches_room_0(p, results[1])
    plain2, res2 = p.runs[1][5], p.runs[1][6]
    assert res2.rooms[0][2]["skipped"] == plain2.rooms[0][2]["skipped"] - 1
    assert p.runs[1][7][4].result == dict(held=0, delivered_len=17, status=HM.DELIVERED)


# --------------------------------------------------------------------------- 6. capture
def test_five_calls_captured_and_replayed(ctx, oracle):
    """The five calls captured once on one stream (a linear chain, no reserve),
    replayed for both sweeps with new bytes copied into the same buffers in
    between; each replay against the model, and equal to the eager run."""
    sweeps, caps, members, room_of = R.sweep_streams()
    eager = Pipeline(oracle, sweeps, caps, members, room_of)
    kept_eager = []
    for r in range(len(sweeps)):
        eager.load(r)
        eager.calls(ctx, torch.cuda.current_stream().cuda_stream)
        kept_eager.append(eager.keep())
    p = Pipeline(oracle, sweeps, caps, members, room_of)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        p.calls(ctx, s.cuda_stream)
    torch.cuda.synchronize()
    assert bool((p.sends == GUARD).all()) and bool((p.areas == GUARD).all()) and not bool(p.hcar.any())  # (capture ran nothing)
    kept = []
    for r in range(len(sweeps)):
        p.load(r)
        g.replay()
        kept.append(p.keep())
    torch.cuda.synchronize()
    results = [p.check(r, k) for r, k in enumerate(kept)]
    assert reaches_room_0(p, results[1])
    for r in range(len(sweeps)):  # sends, wires, results, hold results, view rows, carries, holds: the eager run's
        for j in (0, 1, 2, 3, 4, 5, 8):
            assert download(kept[r][j]).tobytes() == download(kept_eager[r][j]).tobytes(), (r, j)
        a, b = download(kept[r][9]), download(kept_eager[r][9])
        for i in range(p.n):
            lo = 64 + p.AREA * i
            assert a[lo:lo + HOLD_CAP].tobytes() == b[lo:lo + HOLD_CAP].tobytes(), (r, "hold", i)


# --------------------------------------------------------------------------- 7. the Python layer
def test_connection_group_hold(ws, ctx, oracle):
    from test_gpu_parity import dev_bytes
    sweeps, caps, members, room_of = R.sweep_streams()
    n = len(caps)
    size = max(len(p) for s in sweeps for p in s) + 3
    grp = ws.connection_group(n + 1, cap=8, ctx=ctx)
    st, hst = R.SweepState(), HM.State()
    hst.hold = {i: bytes([GUARD]) * HOLD_CAP for i in range(n)}
    heads = [None] + [upload(as_array(R.HEAD24[:3 * k])) for k in range(1, n)]
    areas = [torch.full((HOLD_CAP + size,), GUARD, dtype=torch.uint8, device="cuda") for _ in range(n)]
    for r, pieces in enumerate(sweeps):
        exp, replies, conns, vconns, rooms, plain, res, houts = HM.real_sweep(
            oracle, st, hst, pieces, [8] * n, members, room_of, HOLD_CAP, msg_caps=[9] * n,
            out_caps=[len(p) + 3 for p in pieces])
        items = [(i + 1, dev_bytes(p, 1 + i)[0]) for i, p in enumerate(pieces)]
        outs = [areas[i][HOLD_CAP:HOLD_CAP + len(p) + 3] for i, p in enumerate(pieces)]
        sends = [torch.full((c.send_cap,), GUARD, dtype=torch.uint8, device="cuda") for c in vconns]
        dec = grp.decode(items)
        msgs = grp.reassemble(dec, outs)
        rep = grp.reply(dec, sends, 1 << 20, policy=_lib.POL_FRAGMENTS, flags=0, enc_opts=_lib.ENC_FRAME_OPCODE,
                        action_mask=1 << _lib.ACT_PING)
        held = grp.hold(msgs, HOLD_CAP)
        got = grp.broadcast(held, [[i + 1 for i in m] for m in members], sends, heads=heads, reply=rep)
        for j in range(len(members)):
            rr, want = got.room_result(j), res.rooms[j][2]
            assert (rr.wire_len, rr.nmsgs, rr.skipped, rr.receivers, rr.status) == \
                (want["wire_len"], want["nmsgs"], want["skipped"], want["receivers"], want["status"]), (r, j)
            assert got.wire(j).cpu().numpy().tobytes() == res.rooms[j][3], (r, j)
        for k, (c, o) in enumerate(zip(vconns, houts)):
            hr = held.result(k)
            assert (hr.held, hr.delivered_len, hr.status) == (o.result["held"], o.result["delivered_len"],
                                                              o.result["status"]), (r, k)
            assert [(m.first_frame, m.nframes, m.out_off, m.length, m.status, m.opcode)
                    for m in held.messages(k)] == o.view_recs, (r, k)
            assert bytes(grp.hold_carry(k + 1)) == o.carry.pack(), (r, k)
            br, (lo, data, want) = got.result(k), res.conns[k]
            assert (br.send_len, br.bcast_len, br.status) == (want["send_len"], want["bcast_len"], want["status"]), (r, k)
            image = np.full(c.send_cap, GUARD, np.uint8)
            image[:len(c.prefix)] = as_array(c.prefix)
            image[lo:lo + len(data)] = as_array(data)
            assert sends[k].cpu().numpy().tobytes() == image.tobytes(), (r, k)
        if r == 0:
            assert any(bytes(grp.hold_carry(i + 1)) != bytes(32) for i in range(n))
    assert b"cut in two sweeps" in got.wire(0).cpu().numpy().tobytes()
    # an out tensor without hold_cap bytes of its storage in front of it
    with pytest.raises(ValueError):
        grp.hold(msgs, HOLD_CAP + 1)
    flat = [torch.full((len(p) + 3,), GUARD, dtype=torch.uint8, device="cuda") for p in sweeps[1]]
    dec = grp.decode([(i + 1, dev_bytes(b"", 1 + i)[0]) for i in range(n)])
    with pytest.raises(ValueError):
        grp.hold(grp.reassemble(dec, flat), HOLD_CAP)
    grp.reset([5])
    assert bytes(grp.hold_carry(5)) == bytes(32)
    grp.reset()
    assert all(bytes(grp.hold_carry(i)) == bytes(32) for i in range(n + 1))

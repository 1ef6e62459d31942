"""xyws_reassemble_streams on the device: every connection's messages gathered
and validated by one launch, a message, frame or UTF-8 sequence cut by a recv
boundary continued through the message carry. Every sweep here is
xyws_decode_streams on the wire bytes, then xyws_reassemble_streams on its
table and counts, through the C-ABI. Expected values: the model
(tests/reasm_streams_model.py) on the oracle's decode of the same bytes, over
the scenarios tests/test_reasm_streams_model.py holds to the unsplit stream.
Bar: bit-exact out bytes, stored records, result rows and all 64 carry bytes;
not a guard byte changed outside [out, out + min(out_len, out_cap)), past the
stored records or in the n+1-th result row.

Plumbing as in tests/test_gpu_reply.py: a call's out ranges lie in ONE
guard-filled device buffer (misalignments 0..15, or packed back to back);
record rows and result rows are guard-filled too. Tile, step and grid sizes
come from xyws_debug_reasm_streams_geometry."""
import ctypes as C

import numpy as np
import pytest

import reasm_model as M
import reasm_streams_model as SM
from test_gpu_streams import GUARD, Call, as_array, download, ptr, upload, zeros
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
    assert _lib.load().xyws_debug_reasm_streams_geometry(out) == 0
    return list(out)


class State(SM.State):
    """n connections across sweeps: the device carries (decode and message) and the model's."""

    def __init__(self, n):
        super().__init__()
        self.n = n
        self.dcarry_t = zeros(64 * max(n, 1))
        self.mcarry_t = zeros(64 * max(n, 1))

    def check(self, what=""):
        got = download(self.mcarry_t)
        for i in range(self.n):
            want = self.mc[i].pack() if i in self.mc else bytes(64)
            assert got[64 * i:64 * i + 64].tobytes() == want, (
                what, "carry", i, M.Carry.unpack(got[64 * i:64 * i + 64].tobytes()), self.mc.get(i))


class Sweep:
    """One decode + reassemble of some connections: the model's answer
    (SM.model_sweep), the device buffers, the launch and the comparison.
    mis / omis: misalignments of the recv and out ranges (default k % 16), or
    packed. results = False: a null dev_results."""

    def __init__(self, oracle, st, pieces, ids=None, mis=None, omis=None, packed=False, results=True, **kw):
        n = self.n = len(pieces)
        self.st, self.opts = st, kw.get("opts", M.REASM_UTF8)
        self.ids = list(range(n)) if ids is None else list(ids)
        self.use_mc = kw.get("use_mc", True)
        self.exp = SM.model_sweep(oracle, st, pieces, ids=self.ids, **kw)
        self.call = Call(pieces, mis=mis, packed=packed, caps=[e.cap for e in self.exp], carries=st.dcarry_t,
                         ids=self.ids)
        pos, self.ooffs = 32, []
        for k, e in enumerate(self.exp):
            if not packed:
                pos = (pos + 15) // 16 * 16 + 32 + (k % 16 if omis is None else omis[k])
            self.ooffs.append(pos)
            pos += e.out_cap
        self.oimage = np.full(pos + 64, GUARD, np.uint8)
        self.out_t = upload(self.oimage)
        self.moffs, tot = [], 0
        for e in self.exp:
            self.moffs.append(tot)
            tot += e.msg_cap + 1  # (a guard record after each row)
        self.msgs_t = upload(np.full(40 * max(tot, 1), GUARD, np.uint8))
        self.res_t = upload(np.full(32 * (n + 1), GUARD, np.uint8)) if results else None
        tab = np.zeros((max(n, 1), 8), np.uint64)
        for k, e in enumerate(self.exp):
            tab[k, 0] = 0 if e.out_null else ptr(self.out_t) + self.ooffs[k]
            tab[k, 1] = e.out_cap
            tab[k, 2] = ptr(st.mcarry_t) + 64 * e.id if self.use_mc else 0
            tab[k, 3] = 0 if e.msgs_null else ptr(self.msgs_t) + 40 * self.moffs[k]
            tab[k, 4] = e.msg_cap
        self.rtab_t = upload(tab.reshape(-1).view(np.uint8))

    def reasm_launch(self, ctx, stream=None):
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream)
        return ctx.L.xyws_reassemble_streams(ctx.h, C.c_void_p(ptr(self.call.table_t)),
                                             C.c_void_p(ptr(self.call.counts_t)), C.c_void_p(ptr(self.rtab_t)), self.n,
                                             self.opts, C.c_void_p(ptr(self.res_t)) if self.res_t is not None else None,
                                             s)

    def launch(self, ctx, stream=None):
        self.call.run(ctx, stream=stream)
        assert self.reasm_launch(ctx, stream) == 0
        return self

    def check(self, what=""):
        out = download(self.out_t)
        want = self.oimage.copy()
        for k, e in enumerate(self.exp):
            assert len(e.out) == (0 if e.out_null else min(e.res["out_len"], e.out_cap))
            want[self.ooffs[k]:self.ooffs[k] + len(e.out)] = as_array(e.out)
        if out.tobytes() != want.tobytes():
            bad = int(np.flatnonzero(out != want)[0])
            k = max(j for j in range(self.n) if self.ooffs[j] <= bad) if bad >= self.ooffs[0] else -1
            raise AssertionError((what, "out bytes", "connection", k, "at", bad - self.ooffs[max(k, 0)], "out_len",
                                  self.exp[max(k, 0)].res["out_len"], "cap", self.exp[max(k, 0)].out_cap))
        mgot = download(self.msgs_t)
        mwant = np.full(mgot.size, GUARD, np.uint8)
        for k, e in enumerate(self.exp):
            if not e.msgs_null:
                mwant[40 * self.moffs[k]:40 * (self.moffs[k] + len(e.recs))] = as_array(SM.pack_records(e.recs))
        if mgot.tobytes() != mwant.tobytes():
            bad = int(np.flatnonzero(mgot != mwant)[0]) // 40
            k = max(j for j in range(self.n) if self.moffs[j] <= bad)
            j = bad - self.moffs[k]
            raw = mgot[40 * bad:40 * bad + 40].tobytes()
            got = tuple(int.from_bytes(raw[8 * i:8 * i + 8], "little") for i in range(4)) + \
                (int.from_bytes(raw[32:36], "little"), raw[36])
            raise AssertionError((what, "record", "connection", k, "index", j, "got", got, "want",
                                  self.exp[k].recs[j] if j < len(self.exp[k].recs) else "guard"))
        if self.res_t is not None:
            rgot = download(self.res_t)
            for k, e in enumerate(self.exp):
                assert rgot[32 * k:32 * k + 32].tobytes() == SM.pack_result(e.res), (
                    what, "result", k, e.res, rgot[32 * k:32 * k + 32].view(np.uint64)[:3])
            assert (rgot[32 * self.n:] == GUARD).all(), (what, "result guard")
        if self.use_mc:
            self.st.check(what)
        # the decode's output is not written: the recv bytes are the decoded ones
        self.call.fetch()
        for k, e in enumerate(self.exp):
            assert self.call.bytes_of(k).tobytes() == e.host.tobytes(), (what, "recv bytes", k)
        assert self.call.guards_intact(), what
        return self


def run_sweeps(ctx, oracle, sweeps, n, cov=None, what=""):
    st = State(n)
    done = []
    for r, (pieces, kw) in enumerate(sweeps):
        sw = Sweep(oracle, st, pieces, **kw).launch(ctx).check((what, "sweep", r))
        if cov is not None:
            cov.add(sw.exp)
        done.append(sw)
    return done


# --------------------------------------------------------------------------- 1. every cut of the short stream
@pytest.mark.parametrize("middle", [False, True], ids=["two_sweeps", "one_byte_middle"])
def test_short_stream_every_cut(ctx, oracle, middle):
    sweeps, wires, conns = SM.short_every_cut(middle)
    cov = SM.Coverage()
    run_sweeps(ctx, oracle, sweeps, len(conns), cov)
    cov.require("continued", "closing", "orphans_carried", "tail1", "tail2", "interrupted")


# --------------------------------------------------------------------------- 2. generator streams
def test_generator_streams(ctx, oracle):
    sweeps, wires, conns = SM.generator(oracle)
    cov = SM.Coverage()
    run_sweeps(ctx, oracle, sweeps, len(conns), cov)
    cov.require("continued", "orphans_carried", "interrupted")


# --------------------------------------------------------------------------- 3. frame-tile seams
def test_frame_tile_seams(ctx, oracle):
    T = geometry()[0]
    sweeps, kinds, conns = SM.tile_seams(T)
    cov = SM.Coverage()
    done = run_sweeps(ctx, oracle, sweeps, len(conns), cov)
    assert sorted({e.cnt for e in done[0].exp if len(conns[e.id]) == 1}) == [T - 1, T, T + 1, 2 * T + 1]
    cov.require("continued", "closing", "orphans_carried")


# --------------------------------------------------------------------------- 4. copy-step and lane-line seams
def test_copy_seams(ctx, oracle):
    step = geometry()[1]
    (pieces, kw), = SM.copy_seams(step)
    sw, = run_sweeps(ctx, oracle, [(pieces, kw)], len(pieces))
    bad = sum(1 for e in sw.exp for r in e.recs if r[4] & M.UTF8_BAD)
    assert 0 < bad < 2 * len(pieces)


# --------------------------------------------------------------------------- 5. UTF-8 across fragments and sweeps
def test_utf8_across_fragments_and_sweeps(ctx, oracle):
    sweeps, conns = SM.utf8_fragments()
    cov = SM.Coverage()
    run_sweeps(ctx, oracle, sweeps, len(conns), cov)
    cov.require("tail1", "tail2", "tail3", "bad_after_cut", "continued")


# --------------------------------------------------------------------------- 6. a slab, more connections than the grid
def test_slab_over_the_grid_cap(ctx, oracle):
    G = geometry()[2]
    sweeps, conns = SM.slab(G)
    cov = SM.Coverage()
    done = run_sweeps(ctx, oracle, sweeps, len(conns), cov)
    assert len(done) == 2 and done[0].n == G + 3
    cov.require("continued", "tail1")


# --------------------------------------------------------------------------- 7. caps and nulls
def test_caps_and_nulls(ctx, oracle):
    sweeps, noutf8, nomc = SM.caps_and_nulls()
    done = run_sweeps(ctx, oracle, sweeps, 7, what="caps")
    first = done[0].exp
    assert first[1].res["status"] & SM.RSM_TRUNCATED and first[2].res["status"] & SM.RSM_MSG_CAP
    for sw in done:  # the structural carry is the uncapped run's
        free = sw.exp[0].carry
        for e in sw.exp[1:]:
            c = e.carry
            assert (c.opcode, c.length, c.nframes, c.first_frame, c.frame_remaining, c.frame_member, c.frames_seen) == \
                (free.opcode, free.length, free.nframes, free.first_frame, free.frame_remaining, free.frame_member,
                 free.frames_seen)
    assert all(done[2].exp[k].recs[0][4] & M.UNCHECKED for k in (1, 2, 3, 4, 5))
    # a call without XYWS_REASM_UTF8 in the middle of a stream: UNCHECKED sticks
    d2 = run_sweeps(ctx, oracle, noutf8, 2, what="no utf8")
    assert d2[2].exp[0].recs[0][4] & M.UNCHECKED
    # null message carries; a null dev_results
    st = State(2)
    for r, (pieces, kw) in enumerate(nomc):
        Sweep(oracle, st, pieces, **kw).launch(ctx).check(("null mc", r))
    assert not bool(st.mcarry_t.any())
    st = State(7)
    for r, (pieces, kw) in enumerate(sweeps):
        Sweep(oracle, st, pieces, results=False, **kw).launch(ctx).check(("null results", r))
    # n == 0 launches nothing
    assert Sweep(oracle, State(0), []).reasm_launch(ctx) == 0


# --------------------------------------------------------------------------- 8. overflow
def test_overflow_is_sticky_and_local(ctx, oracle):
    done = run_sweeps(ctx, oracle, SM.overflow_sweeps(), 4)
    for sw in done:
        assert [e.res["status"] & SM.RSM_OVERFLOW for e in sw.exp] == [4, 0, 4, 0]
    assert done[1].exp[1].carry.frames_seen == 10 and done[0].exp[1].res["completed"] == 4
    assert done[1].exp[0].carry.status == SM.MSG_OVERFLOW


# --------------------------------------------------------------------------- 9. no slot, no history
def test_no_slot_and_no_history(ws, ctx, oracle):
    import history
    from test_gpu_parity import dev_bytes
    sweeps, wires, conns = SM.generator(oracle)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pol = (C.c_uint64 * _lib.POL_WORDS)()
    st = State(len(conns))
    Sweep(oracle, st, sweeps[0][0]).launch(ctx)
    torch.cuda.synchronize()
    assert ctx.L.xyws_debug_policy(ctx.h, stream, pol) == -1  # no slot bound: neither call took one
    primer = history.primers()["equal_264_lat"]
    dec = ws.frame_decoder(ctx=ctx, opts=primer.opts)
    for src, fresh in primer.calls:
        if fresh:
            dec.reset()
        dec.decode(dev_bytes(src)[0], cap=0, count=False)
        torch.cuda.synchronize()
    assert ctx.L.xyws_debug_policy(ctx.h, stream, pol) == 0
    before = list(pol)
    assert tuple(before[1:5]) == primer.words
    Sweep(oracle, st, sweeps[1][0]).launch(ctx).check("after the primer")
    assert ctx.L.xyws_debug_policy(ctx.h, stream, pol) == 0
    assert list(pol) == before


# --------------------------------------------------------------------------- 10. capture, streams
def test_decode_reassemble_reply_captured_and_replayed(ctx, oracle):
    """Decode, reassemble and reply captured on one stream into one graph
    without any reserve, replayed over 4 successive sweeps copied into the
    fixed buffers; nothing is read back in between."""
    import msg_streams
    import reasm_cases as RC
    wires = [msg_streams.message_stream(s, nmsg=24)[0] for s in (5, 6, 7)]
    B = 4
    conns = [[w[k * (len(w) // B):(k + 1) * (len(w) // B) if k < B - 1 else len(w)] for k in range(B)] for w in wires]
    size = max(len(p) for c in conns for p in c)
    n = len(conns)
    cap = size // 2 + 2
    st = SM.State()
    exps = [SM.model_sweep(oracle, st, [c[r] for c in conns], caps=[cap] * n, out_caps=[size] * n,
                           msg_caps=[cap + 1] * n) for r in range(B)]
    # fixed buffers: recv slots of `size`, tables that take the lengths from a device vector
    recv = torch.full((n * size + 64,), GUARD, dtype=torch.uint8, device="cuda")
    outs = torch.full((n * size + 64,), GUARD, dtype=torch.uint8, device="cuda")
    sends = torch.full((n * (size + 13) + 64,), GUARD, dtype=torch.uint8, device="cuda")
    frames = torch.zeros(n * cap * 32, dtype=torch.uint8, device="cuda")
    msgs = torch.zeros(n * (cap + 1) * 40, dtype=torch.uint8, device="cuda")
    dcar, mcar, rcar = zeros(64 * n), zeros(64 * n), zeros(32 * n)
    counts = torch.zeros(n, dtype=torch.int64, device="cuda")
    res = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    rres = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    tabs, stage = [], []
    for r in range(B):
        tab = np.zeros((n, 8), np.uint64)
        for i in range(n):
            tab[i, :5] = [ptr(recv) + size * i, len(conns[i][r]), ptr(dcar) + 64 * i, ptr(frames) + 32 * cap * i, cap]
        tabs.append(upload(tab.reshape(-1).view(np.uint8)))
        img = np.full(n * size, GUARD, np.uint8)
        for i in range(n):
            img[size * i:size * i + len(conns[i][r])] = as_array(conns[i][r])
        stage.append(upload(img))
    ctab = torch.zeros_like(tabs[0])
    mtab = np.zeros((n, 8), np.uint64)
    rtab = np.zeros((n, 4), np.uint64)
    for i in range(n):
        mtab[i, :5] = [ptr(outs) + size * i, size, ptr(mcar) + 64 * i, ptr(msgs) + 40 * (cap + 1) * i, cap + 1]
        rtab[i] = [ptr(sends) + (size + 13) * i, size + 13, ptr(rcar) + 32 * i, 0]
    mtab_t, rtab_t = upload(mtab.reshape(-1).view(np.uint8)), upload(rtab.reshape(-1).view(np.uint8))
    s = torch.cuda.Stream()  # (new to the context; no call was made on it, nothing reserved)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        sp = C.c_void_p(s.cuda_stream)
        assert ctx.L.xyws_decode_streams(ctx.h, C.c_void_p(ptr(ctab)), n, C.c_void_p(ptr(counts)), 0, sp) == 0
        assert ctx.L.xyws_reassemble_streams(ctx.h, C.c_void_p(ptr(ctab)), C.c_void_p(ptr(counts)),
                                             C.c_void_p(ptr(mtab_t)), n, M.REASM_UTF8, C.c_void_p(ptr(res)), sp) == 0
        assert ctx.L.xyws_reply_streams(ctx.h, C.c_void_p(ptr(ctab)), C.c_void_p(ptr(counts)), C.c_void_p(ptr(rtab_t)),
                                        n, 1 << 20, 0x1, 0x11, 0x1, 0x3, C.c_void_p(ptr(rres)), sp) == 0
    torch.cuda.synchronize()
    assert not bool(mcar.any()) and bool((outs == GUARD).all())  # (capture ran nothing)
    kept = []
    for r in range(B):
        recv[:n * size].copy_(stage[r])
        ctab.copy_(tabs[r])
        outs.fill_(GUARD)
        g.replay()
        kept.append((outs.clone(), msgs.clone(), res.clone(), mcar.clone()))  # (device copies)
    torch.cuda.synchronize()
    for r, (o, m, rs, mc) in enumerate(kept):
        o, m, rs, mc = download(o), download(m), download(rs), download(mc)
        for i, e in enumerate(exps[r]):
            assert rs[32 * i:32 * i + 32].tobytes() == SM.pack_result(e.res), (r, i)
            assert o[size * i:size * i + len(e.out)].tobytes() == e.out, (r, i)
            assert (o[size * i + len(e.out):size * (i + 1)] == GUARD).all(), (r, i)
            row = 40 * (cap + 1) * i
            assert m[row:row + 40 * len(e.recs)].tobytes() == SM.pack_records(e.recs), (r, i)
            assert mc[64 * i:64 * i + 64].tobytes() == e.carry.pack(), (r, i)
    assert sum(e.res["completed"] for ex in exps for e in ex) > 30
    assert bool((download(rres).reshape(n, 32)[:, 0:8].view(np.uint64) > 0).all())  # (the replies were written too)


def test_two_streams_concurrently(ctx, oracle):
    sa, _, ca = SM.short_every_cut()
    sb, _, cb = SM.generator(oracle)
    sta, stb = State(len(ca)), State(len(cb))
    swa, swb = Sweep(oracle, sta, sa[0][0]), Sweep(oracle, stb, sb[0][0], packed=True)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    swa.launch(ctx, stream=s1.cuda_stream)
    swb.launch(ctx, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    swa.check("stream 1")
    swb.check("stream 2")


# --------------------------------------------------------------------------- 11. the Python layer
@pytest.mark.parametrize("order", ["before_reply", "after_reply"])
def test_connection_group_reassemble(ws, ctx, oracle, order):
    from test_gpu_parity import dev_bytes
    wires = SM.group_wires()
    grp = ws.connection_group(4, cap=64, ctx=ctx)
    st = SM.State()
    for r, (lo, hi) in enumerate(((0, 150), (150, 151), (151, 600))):
        pieces = [w[lo:hi] for w in wires]
        exp = SM.model_sweep(oracle, st, pieces, ids=[1, 2, 3], caps=[64] * 3, msg_caps=[65] * 3)
        items = [(i + 1, dev_bytes(p, 1 + i)[0]) for i, p in enumerate(pieces)]
        outs = [torch.full((t.numel() + 3,), GUARD, dtype=torch.uint8, device=t.device) for _, t in items]
        sends = [torch.empty(t.numel() + 13, dtype=torch.uint8, device=t.device) for _, t in items]
        dec = grp.decode(items)
        if order == "after_reply":
            grp.reply(dec, sends, 1 << 20, policy=_lib.POL_FRAGMENTS, enc_opts=_lib.ENC_FRAME_OPCODE, action_mask=3)
        got = grp.reassemble(dec, outs)
        if order == "before_reply":
            grp.reply(dec, sends, 1 << 20, policy=_lib.POL_FRAGMENTS, enc_opts=_lib.ENC_FRAME_OPCODE, action_mask=3)
        for k, e in enumerate(exp):
            res = got.result(k)
            assert (res.out_len, res.nmsgs, res.completed, res.status) == \
                (e.res["out_len"], e.res["nmsgs"], e.res["completed"], e.res["status"]), (r, k)
            o = outs[k].cpu().numpy()
            assert o[:res.out_len].tobytes() == e.out and (o[res.out_len:] == GUARD).all(), (r, k)
            assert [(m.first_frame, m.nframes, m.out_off, m.length, m.status, m.opcode)
                    for m in got.messages(k)] == e.recs, (r, k)
            assert bytes(grp.msg_carry(k + 1)) == e.carry.pack(), (r, k)
    assert bytes(grp.msg_carry(0)) == bytes(64) and any(bytes(grp.msg_carry(i)) != bytes(64) for i in (1, 2, 3))
    with pytest.raises(_lib.XywsError):
        ws.connection_group(2, cap=0, ctx=ctx).reassemble(dec, outs)
    with pytest.raises(_lib.XywsError):
        grp.reassemble(dec, outs, msg_cap=66)
    grp.reset([1])
    assert bytes(grp.msg_carry(1)) == bytes(64) and bytes(grp.msg_carry(2)) == st.mc[2].pack()
    grp.reset()
    assert bytes(grp.msg_carry(2)) == bytes(64)

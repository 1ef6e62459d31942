"""xyws_reply_streams on the device: every connection of a sweep classified,
answered and closed by one launch, a frame cut by a recv boundary continued
through the reply carry. Every sweep here is the pair an echo service runs:
xyws_decode_streams on the wire bytes, then xyws_reply_streams on its table
and counts. Expected values: the Python model (tests/reply_model.py) on the
oracle's decode of the same bytes. Bar: bit-exact reply bytes, results,
verdicts and carries; not a guard byte changed outside
[out, out + min(reply_len, out_cap)).

Plumbing as in tests/test_gpu_streams.py: a call's out ranges lie in ONE
guard-filled device buffer (misalignments 0..15, or packed back to back);
verdict rows and result rows are guard-filled too. Tile and grid sizes come
from xyws_debug_reply_geometry."""
import ctypes as C

import numpy as np
import pytest

import msg_streams
import reply_cases as RC
import reply_model as M
import streams
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
    assert _lib.load().xyws_debug_reply_geometry(out) == 0
    return list(out)


RFC, REF = M.MODES["rfc"], M.MODES["reference"]


class State:
    """n connections across sweeps: the device carries (decode and reply) and
    the model's."""

    def __init__(self, n):
        self.n = n
        self.dcarry_t = zeros(64 * max(n, 1))
        self.rcarry_t = zeros(32 * max(n, 1))
        self.dc, self.rc = {}, {}

    def check(self, what=""):
        got = download(self.rcarry_t)
        for i, rc in self.rc.items():
            assert got[32 * i:32 * i + 32].tobytes() == rc.pack(), (what, i, rc.as_tuple())
        for i in range(self.n):
            if i not in self.rc:
                assert not got[32 * i:32 * i + 32].any(), (what, i)


def pack_result(r):
    return (r["reply_len"].to_bytes(8, "little") + r["first_close"].to_bytes(8, "little") +
            r["answered"].to_bytes(4, "little") + r["close_code"].to_bytes(2, "little") +
            r["status"].to_bytes(2, "little") + bytes(8))


def pack_verdicts(vd):
    return b"".join(v.close_code.to_bytes(2, "little") + v.peer_code.to_bytes(2, "little") + bytes([v.action, 0, 0, 0])
                    for v in vd)


class Sweep:
    """One decode + reply of some connections. pieces[k]: the wire bytes
    connection ids[k] received. caps[k]: its descriptor capacity (default: its
    count + 1; None: a null frames pointer). out_caps[k]: default len + 13.
    omis[k]: misalignment of its out range (default k % 16), or packed.
    rows / results / use_rc = False: null verdict rows, a null dev_results,
    null reply carries."""

    def __init__(self, oracle, st, pieces, mode, ids=None, caps=None, out_caps=None, omis=None, packed=False,
                 rows=True, results=True, use_rc=True, max_payload=RC.MAX_PAYLOAD):
        n = self.n = len(pieces)
        self.st, self.mode, self.max_payload, self.use_rc = st, mode, max_payload, use_rc
        self.ids = list(range(n)) if ids is None else list(ids)
        self.exp, dcaps, self.ocaps = [], [], []
        for k, i in enumerate(self.ids):
            buf = as_array(pieces[k])
            fr, dc, cnt = oracle.decode_stream(buf, carry_in=st.dc.get(i))
            assert cnt == len(fr)
            st.dc[i] = dc
            cap = caps[k] if caps is not None else cnt + 1
            ocap = out_caps[k] if out_caps is not None else buf.size + 13
            w, res, vd, rc = M.reply(oracle, buf, fr, st.rc.get(i, M.Carry()) if use_rc else None, ocap, max_payload,
                                     nframes=cnt, cap=cap or 0, frames_null=cap is None, **mode)
            if use_rc:
                st.rc[i] = rc
            self.exp.append((w, res, vd, cnt))
            dcaps.append(cap)
            self.ocaps.append(ocap)
        self.call = Call(pieces, caps=dcaps, carries=st.dcarry_t, ids=self.ids)
        # the out ranges, in one guarded buffer
        pos, self.ooffs = 32, []
        for k in range(n):
            if not packed:
                pos = (pos + 15) // 16 * 16 + 32 + (k % 16 if omis is None else omis[k])
            self.ooffs.append(pos)
            pos += self.ocaps[k]
        self.oimage = np.full(pos + 64, GUARD, np.uint8)
        self.out_t = upload(self.oimage)
        # verdict rows (count + 1 entries each) and result rows (n + 1)
        self.voffs, tot = [], 0
        for e in self.exp:
            self.voffs.append(tot)
            tot += e[3] + 1
        self.rows = rows
        self.verd_t = upload(np.full(8 * max(tot, 1), GUARD, np.uint8))
        self.res_t = upload(np.full(32 * (n + 1), GUARD, np.uint8)) if results else None
        tab = np.zeros((max(n, 1), 4), np.uint64)
        for k, i in enumerate(self.ids):
            tab[k, 0] = ptr(self.out_t) + self.ooffs[k]
            tab[k, 1] = self.ocaps[k]
            tab[k, 2] = ptr(st.rcarry_t) + 32 * i if use_rc else 0
            tab[k, 3] = ptr(self.verd_t) + 8 * self.voffs[k] if rows else 0
        self.rtab_t = upload(tab.reshape(-1).view(np.uint8))

    def reply_launch(self, ctx, stream=None):
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream)
        m = self.mode
        return ctx.L.xyws_reply_streams(ctx.h, C.c_void_p(ptr(self.call.table_t)), C.c_void_p(ptr(self.call.counts_t)),
                                        C.c_void_p(ptr(self.rtab_t)), self.n, self.max_payload, m["policy"],
                                        m["flags"], m["enc_opts"], m["action_mask"],
                                        C.c_void_p(ptr(self.res_t)) if self.res_t is not None else None, s)

    def launch(self, ctx, stream=None):
        self.call.run(ctx, stream=stream)
        assert self.reply_launch(ctx, stream) == 0
        return self

    def check(self, what=""):
        out = download(self.out_t)
        want = self.oimage.copy()
        for k, (w, res, vd, cnt) in enumerate(self.exp):
            assert len(w) == min(res["reply_len"], self.ocaps[k])
            want[self.ooffs[k]:self.ooffs[k] + len(w)] = as_array(w)
        if out.tobytes() != want.tobytes():
            bad = int(np.flatnonzero(out != want)[0])
            k = max(j for j in range(self.n) if self.ooffs[j] <= bad) if bad >= self.ooffs[0] else -1
            raise AssertionError((what, "reply bytes", "connection", k, "at", bad - self.ooffs[max(k, 0)],
                                  "reply_len", self.exp[max(k, 0)][1]["reply_len"], "cap", self.ocaps[max(k, 0)]))
        vgot = download(self.verd_t)
        vwant = np.full(vgot.size, GUARD, np.uint8)
        if self.rows:
            for k, (w, res, vd, cnt) in enumerate(self.exp):
                if vd is not None:
                    vwant[8 * self.voffs[k]:8 * (self.voffs[k] + len(vd))] = as_array(pack_verdicts(vd))
        assert vgot.tobytes() == vwant.tobytes(), (what, "verdicts")
        if self.res_t is not None:
            rgot = download(self.res_t)
            for k, (w, res, vd, cnt) in enumerate(self.exp):
                assert rgot[32 * k:32 * k + 32].tobytes() == pack_result(res), (what, "result", k, res)
            assert (rgot[32 * self.n:] == GUARD).all(), (what, "result guard")
        self.st.check(what)
        return self

    def written(self, k):
        return self.exp[k][0]


def run_rounds(ctx, oracle, conns, mode, packed=False):
    """conns: a list of piece lists. Round r sweeps piece r of every connection
    that has one, all in one call; returns every connection's concatenated
    reply (the model's, which check() held the device to)."""
    st = State(len(conns))
    got = [bytearray() for _ in conns]
    for r in range(max(len(c) for c in conns)):
        live = [i for i, c in enumerate(conns) if r < len(c)]
        sw = Sweep(oracle, st, [conns[i][r] for i in live], mode, ids=live, packed=packed).launch(ctx).check(("round", r))
        for k, i in enumerate(live):
            got[i] += sw.written(k)
    return [bytes(g) for g in got]


def pieces_of(wire, cuts):
    out, prev = [], 0
    for c in list(cuts) + [len(wire)]:
        out.append(wire[prev:c])
        prev = c
    return out


# --------------------------------------------------------------------------- 1. table sizes
def sized_stream(rng, nframes, unmasked=False, forms=False):
    sizes = (0, 1, 125, 126, 127)
    out = b""
    for j in range(nframes):
        b0 = 0x89 if j % 11 == 7 else (0x81 if j & 1 else 0x82)
        n = sizes[j % 5] if b0 != 0x89 else j % 126
        form = None
        if forms and b0 != 0x89:
            form = (16, 64, None)[j % 3] if n < 126 else (64, None)[j % 2]
        out += streams.frame(rng, b0, n, masked_frame=not (unmasked and j % 3 == 0), form=form)
    return out


@pytest.mark.parametrize("mode", ["rfc", "reference"])
def test_table_sizes(ctx, oracle, mode):
    T = geometry()[0]
    rng = streams.SplitMix(0x7AB1)
    m = dict(M.MODES[mode], policy=M.MODES[mode]["policy"] | M.POL_UNMASKED)
    pieces = [sized_stream(rng, n) for n in (0, 1, T - 1, T, T + 1, 2 * T, 2 * T + 1)]
    pieces.append(sized_stream(rng, T + 3, unmasked=True))
    pieces.append(sized_stream(rng, T + 2, forms=True))
    pieces.append(streams.frame(rng, 0x82, 5) + streams.frame(rng, 0x82, 65536) + streams.frame(rng, 0x81, 9))
    st = State(len(pieces))
    sw = Sweep(oracle, st, pieces, m).launch(ctx).check(mode)
    counts = [e[3] for e in sw.exp]
    assert counts[:7] == [0, 1, T - 1, T, T + 1, 2 * T, 2 * T + 1]
    if mode == "rfc":  # every frame answered, pings as pongs, all three header forms
        assert [e[1]["answered"] for e in sw.exp] == counts
        assert sw.exp[9][1]["reply_len"] == 2 + 5 + 10 + 65536 + 2 + 9
        assert sw.written(3)[:2] == bytes([0x82, 0])
        assert not any(e[1]["status"] for e in sw.exp)
    else:  # the reference's test closes 1000 on the first ping (index 7)
        assert [e[1]["first_close"] for e in sw.exp[2:7]] == [7] * 5 and sw.exp[4][1]["answered"] == 7
    # packed out ranges: neighbours share lines
    st = State(len(pieces))
    Sweep(oracle, st, pieces, m, packed=True).launch(ctx).check((mode, "packed"))


# --------------------------------------------------------------------------- 2. close placement
CLOSERS = {1000: lambda rng: msg_streams.close_frame(rng, 1001, b"x"),
           1002: lambda rng: streams.frame(rng, 0xC2, 7),            # RSV1 under XYWS_POL_STRICT
           1003: lambda rng: streams.frame(rng, 0x02, 7),            # FIN = 0
           1008: lambda rng: streams.frame(rng, 0x82, 7, masked_frame=False),
           1009: lambda rng: streams.frame(rng, 0x82, 2000)}         # max_payload 1000


def test_close_placement(ctx, oracle):
    T = geometry()[0]
    rng = streams.SplitMix(0xC105)
    m = dict(RFC, policy=M.POL_STRICT)
    total = 2 * T + 2
    pieces, where = [], []
    for code, make in CLOSERS.items():
        for at in (0, T - 1, T, total - 1):
            pieces.append(b"".join(make(rng) if j == at else streams.frame(rng, 0x81, j % 9) for j in range(total)))
            where.append((code, at))
    # 1009 on a header whose payload is cut by the batch end
    pieces.append(streams.frame(rng, 0x81, 3) + streams.frame(rng, 0x82, 2000)[:8 + 10])
    where.append((1009, 1))
    st = State(len(pieces))
    sw = Sweep(oracle, st, pieces, m, max_payload=1000).launch(ctx).check("close")
    for k, (code, at) in enumerate(where):
        w, res, vd, cnt = sw.exp[k]
        assert (res["first_close"], res["close_code"], res["status"], res["answered"]) == (at, code, M.CLOSED, at), k
        assert w[-4:] == bytes([0x88, 2, code >> 8, code & 0xFF]) and len(vd) == cnt  # (verdicts past the close too)
    # the next call on a closed connection writes nothing
    more = [streams.frame(rng, 0x81, 5) for _ in pieces]
    sw = Sweep(oracle, st, more, m, max_payload=1000).launch(ctx).check("closed")
    for k, (code, at) in enumerate(where):
        assert sw.exp[k][:3] == (b"", M.result(close_code=code, status=M.CLOSED), None)


# --------------------------------------------------------------------------- 3. split invariance
def short_stream():
    rng = streams.SplitMix(0x5407)
    return (streams.frame(rng, 0x81, 5) + streams.frame(rng, 0x89, 3) + streams.frame(rng, 0x82, 4, form=16) +
            streams.frame(rng, 0x82, 0) + msg_streams.close_frame(rng, 1000))


@pytest.mark.parametrize("mode", ["reference", "rfc"])
def test_split_invariance(ctx, oracle, mode):
    rng = streams.SplitMix(0x1417)
    conns, wires = [], []

    def add(wire, cuts):
        conns.append(pieces_of(wire, cuts))
        wires.append(wire)

    named = RC.named_streams()
    named["echo"] = RC.echo_stream(0xEC40, 40)
    named["echo_big"] = RC.echo_stream(0xB16, 12, big=True)
    for name, wire in named.items():
        for _ in range(3):
            add(wire, RC.random_cuts(rng, len(wire), 1 + rng.below(6)))
        if len(wire) < 8192:
            for cuts in RC.header_cuts(wire, RC.frame_starts(oracle, wire)[:3]):
                add(wire, cuts)
    short = short_stream()
    for p in range(1, len(short)):
        add(short, [p])
    add(short, list(range(1, len(short))))  # a byte at a time
    got = run_rounds(ctx, oracle, conns, M.MODES[mode])
    memo = {}
    for i, wire in enumerate(wires):
        if wire not in memo:
            memo[wire] = M.unsplit(oracle, wire, mode, RC.MAX_PAYLOAD)
        assert got[i] == memo[wire], (mode, i)
    assert any(memo[w][-4:-2] == bytes([0x88, 2]) for w in memo)


# --------------------------------------------------------------------------- 4. out_cap
def test_out_cap(ctx, oracle):
    rng = streams.SplitMix(0xCA9)
    wire = streams.frame(rng, 0x81, 200) + streams.frame(rng, 0x89, 30) + streams.frame(rng, 0x82, 300)
    cut = len(wire) - 120
    full = M.run_split(oracle, wire, [cut], "rfc", RC.MAX_PAYLOAD)
    header, lens = 4, [c[4]["reply_len"] for c in full]
    assert lens[0] == 4 + 200 + 2 + 30 + 4 + 180 and lens[1] == 120
    for packed in (False, True):
        caps0 = [0, 1, header - 1, header, lens[0] - 1, lens[0], lens[0] + 1]
        caps1 = [0, 1, 1, 2, lens[1] - 1, lens[1], lens[1] + 1]
        st = State(len(caps0))
        for r, caps in enumerate((caps0, caps1)):
            piece = wire[:cut] if r == 0 else wire[cut:]
            sw = Sweep(oracle, st, [piece] * len(caps), RFC, out_caps=caps, packed=packed,
                       omis=[15 - k for k in range(len(caps))]).launch(ctx).check(("cap", packed, r))
            for k, cap in enumerate(caps):
                w, res, vd, cnt = sw.exp[k]
                assert res["reply_len"] == lens[r] and res["status"] == (M.TRUNCATED if lens[r] > cap else 0)
                assert w == full[r][3][:cap]
        # the carries are exact whatever the capacity
        assert len({st.rc[i].as_tuple() for i in range(len(caps0))}) == 1


# --------------------------------------------------------------------------- 5. overflow
def test_overflow_is_sticky_and_local(ctx, oracle):
    rng = streams.SplitMix(0x0F10)
    piece = b"".join(streams.frame(rng, 0x81, 3 + j) for j in range(5))
    st = State(4)
    sw = Sweep(oracle, st, [piece] * 4, RFC, caps=[4, 6, None, 5]).launch(ctx).check("overflow")
    assert [e[1]["status"] for e in sw.exp] == [M.OVERFLOW, 0, M.OVERFLOW, 0]
    assert sw.exp[1][1]["answered"] == 5 and sw.exp[0][2] is None
    sw = Sweep(oracle, st, [piece] * 4, RFC, caps=[9, 9, 9, 9]).launch(ctx).check("sticky")
    assert [e[1]["status"] for e in sw.exp] == [M.OVERFLOW, 0, M.OVERFLOW, 0]
    assert st.rc[0].status == M.OVERFLOW and st.rc[1].replies_total == 10


# --------------------------------------------------------------------------- 6. nulls, empties, the grid stride
def test_nulls_and_empties(ctx, oracle):
    rng = streams.SplitMix(0x2E20)
    wire = streams.frame(rng, 0x81, 50) + streams.frame(rng, 0x82, 400) + msg_streams.close_frame(rng, 1000)
    # null reply carries, null verdict rows, a null dev_results: each alone and all together
    for kw in (dict(use_rc=False), dict(rows=False), dict(results=False), dict(use_rc=False, rows=False, results=False)):
        st = State(3)
        Sweep(oracle, st, [wire, wire[:100], b""], RFC, **kw).launch(ctx).check(tuple(kw))
    # len == 0 with a carry in mid-frame: nothing moves, the frame goes on in the next call
    st = State(2)
    parts = [wire[:70], b"", wire[70:]]
    got = bytearray()
    for r, p in enumerate(parts):
        sw = Sweep(oracle, st, [p, p], RFC).launch(ctx).check(("empty", r))
        got += sw.written(0)
        if r == 1:
            assert sw.exp[0][1] == M.result() and st.rc[0].frame_remaining == 400 - (70 - 56 - 8)
    assert bytes(got) == M.unsplit(oracle, wire, "rfc", RC.MAX_PAYLOAD)
    # n == 0 launches nothing
    sw = Sweep(oracle, State(0), [], RFC)
    assert sw.reply_launch(ctx) == 0


def test_grid_stride(ctx, oracle):
    n = geometry()[2] + 1
    rng = streams.SplitMix(0x6A1D)
    pieces = [streams.frame(rng, 0x81, 1 + i % 5) for i in range(n)]
    st = State(n)
    sw = Sweep(oracle, st, pieces, RFC, packed=True).launch(ctx).check("grid")
    assert all(e[1]["answered"] == 1 for e in sw.exp)


# --------------------------------------------------------------------------- 7. capture, streams
def test_captured_at_once_and_replayed(ctx, oracle):
    wire = RC.echo_stream(0x6EA9, 70)
    pieces = [wire, wire[:len(wire) // 2], short_stream(), RC.named_streams()["messages"]]
    st = State(len(pieces))
    sw = Sweep(oracle, st, pieces, RFC)
    orig = sw.call.view.clone()
    s = torch.cuda.Stream()  # (new to the context; no call was made on it, nothing reserved)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        sw.launch(ctx, stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert not bool(st.rcarry_t.any()) and bool((sw.out_t == GUARD).all())  # (capture ran nothing)
    for rep in range(2):
        sw.call.view.copy_(orig)
        st.dcarry_t.zero_()
        st.rcarry_t.zero_()
        sw.out_t.fill_(GUARD)
        sw.verd_t.fill_(GUARD)
        sw.res_t.fill_(GUARD)
        g.replay()
        torch.cuda.synchronize()
        sw.check(("replay", rep))


def test_two_streams_concurrently(ctx, oracle):
    a = [RC.echo_stream(0xA0 + i, 30) for i in range(8)]
    b = [RC.echo_stream(0xB0 + i, 30, big=True) for i in range(8)]
    sta, stb = State(8), State(8)
    swa, swb = Sweep(oracle, sta, a, RFC), Sweep(oracle, stb, b, REF, packed=True)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    swa.launch(ctx, stream=s1.cuda_stream)
    swb.launch(ctx, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    swa.check("stream 1")
    swb.check("stream 2")


# --------------------------------------------------------------------------- 8. the Python layer
def test_connection_group_reply(ws, ctx, oracle):
    from test_gpu_parity import dev_bytes
    wires = [RC.echo_stream(0x90 + i, 12) for i in range(3)]
    grp = ws.connection_group(4, cap=64, ctx=ctx)
    got = [bytearray() for _ in wires]
    for r, (lo, hi) in enumerate(((0, 150), (150, 151), (151, 1 << 30))):
        items = [(i + 1, dev_bytes(w[lo:hi], 1 + i)[0]) for i, w in enumerate(wires)]
        outs = [torch.full((t.numel() + 13,), GUARD, dtype=torch.uint8, device=t.device) for _, t in items]
        dec = grp.decode(items)
        rep = grp.reply(dec, outs, RC.MAX_PAYLOAD, policy=RFC["policy"], flags=RFC["flags"], enc_opts=RFC["enc_opts"],
                        action_mask=RFC["action_mask"])
        for k, o in enumerate(outs):
            res = rep.result(k)
            assert not res.status & (_lib.RPL_TRUNCATED | _lib.RPL_OVERFLOW)
            got[k] += o[:res.reply_len].cpu().numpy().tobytes()
            assert bool((o[res.reply_len:] == GUARD).all())
            if res.first_close != _lib.NPOS or not res.status & _lib.RPL_CLOSED:  # (not closed by an earlier call)
                assert len(rep.verdicts(k)) == dec.nframes(k)
    for k, w in enumerate(wires):
        assert bytes(got[k]) == M.unsplit(oracle, w, "rfc", RC.MAX_PAYLOAD), k
        assert grp.reply_carry(k + 1).close_code != 0
    assert bytes(grp.reply_carry(0)) == bytes(32)
    with pytest.raises(_lib.XywsError):
        ws.connection_group(2, cap=0, ctx=ctx).reply(dec, outs, 1)
    grp.reset()
    assert bytes(grp.reply_carry(1)) == bytes(32)

"""xyws_inflate_windows_streams on the device: client context takeover, a window per connection. Reference: one
persistent zlib.decompressobj(-15) per connection, fed each message + 00 00 ff ff (hand-assembled messages state
their bytes). Bar: byte-exact messages, exact result rows, n_history, win_len, the window equal to the history's last
bytes and no byte changed outside it, around it or around an out range. Frames and tables as in test_gpu_inflate."""
import ctypes as C
import zlib

import numpy as np
import pytest

from xynet_amd import _lib
from test_gpu_inflate import COMPLETE, GUARD, TRUNC, deflate, frames, rnd, text, torch, ws  # noqa: F401

pytestmark = pytest.mark.gpu
TAIL, WIN, GAP = b"\x00\x00\xff\xff", 32768, 48
NEG, KEEP = _lib.INFC_NEGOTIATED, _lib.INFC_NEGOTIATED | _lib.INFC_TAKEOVER
ptr = lambda t: C.c_void_p(t.data_ptr())


class Client:
    """What a client that keeps its context sends: zlib level 6, raw, Z_SYNC_FLUSH, the tail stripped."""

    def __init__(self):
        self.c = zlib.compressobj(6, zlib.DEFLATED, -15)

    def __call__(self, data):
        return self.c.compress(data) + self.c.flush(zlib.Z_SYNC_FLUSH)[:-4]


class Fixed:
    """One fixed-Huffman block, bit by bit (RFC 1951 3.2.6), then the empty stored block's header that a sync flush
    leaves in front of the stripped tail."""
    LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]

    def __init__(self, bfinal=0):
        self.v, self.n = 0, 0
        self.put(bfinal | 2, 3)

    def put(self, val, nbits):
        self.v |= val << self.n
        self.n += nbits

    def code(self, val, nbits):  # a Huffman code: first bit highest
        self.put(int(format(val, f"0{nbits}b")[::-1], 2), nbits)

    def sym(self, s):
        self.code(*((0x30 + s, 8) if s < 144 else (0x190 + s - 144, 9) if s < 256 else (s - 256, 7) if s < 280 else (0xC0 + s - 280, 8)))

    def lits(self, data):
        for b in data:
            self.sym(b)
        return self

    def match(self, length, dist):
        i = max(k for k, b in enumerate(self.LBASE) if b <= length)
        self.sym(257 + i)
        self.put(length - self.LBASE[i], 0 if i < 8 or i == 28 else (i - 4) // 4)
        j = max(k for k, b in enumerate(self.DBASE) if b <= dist)
        self.code(j, 5)
        self.put(dist - self.DBASE[j], 0 if j < 4 else j // 2 - 1)
        return self

    def done(self):
        self.sym(256)
        self.put(0, 3)
        return self.v.to_bytes((self.n + 7) // 8, "little")


class Conns:
    """n connections over several calls: decode and reassemble through a connection_group, then one inflate call over
    tables of the test. Out ranges and windows lie in guard-filled slabs; window k is 16-byte aligned."""

    def __init__(self, ws, flags, out_cap, fn="xyws_inflate_windows_streams"):
        self.n, self.flags, self.cap, self.fn = len(flags), flags, out_cap, fn
        self.grp = ws.connection_group(self.n, cap=8)
        self.areas = [torch.zeros(out_cap + 4096, dtype=torch.uint8, device="cuda") for _ in flags]
        self.ic = torch.zeros(32 * self.n, dtype=torch.uint8, device="cuda")
        self.win = torch.full((GAP + (WIN + GAP) * self.n,), GUARD, dtype=torch.uint8, device="cuda")
        assert self.win.data_ptr() % 16 == 0
        self.hist, self.alive, self.wfree = [b""] * self.n, [f == KEEP and fn.endswith("windows_streams") for f in flags], None

    def call(self, sent, off=3):
        """One sweep: sent[k] is connection k's messages as (payload, rsv1); its out range begins `off` bytes into a line."""
        g, n, VM = self.grp, self.n, 9
        self.sent, wires = sent, [b"".join(frames(p, rsv1=r, op=2) for p, r in msgs) for msgs in sent]
        self.slab = torch.tensor(list(b"".join(wires)), dtype=torch.uint8, device="cuda")
        ends = np.cumsum([len(w) for w in wires])
        self.dec = g.decode([(k, self.slab[e - len(w):e]) for k, (w, e) in enumerate(zip(wires, ends))])
        self.src = g.reassemble(self.dec, self.areas)
        self.stride = (self.cap + 16 + GAP) & ~15
        self.out = torch.full((self.stride * n + 64,), GUARD, dtype=torch.uint8, device="cuda")
        self.vmsgs = torch.full((40 * (VM + 1) * n,), GUARD, dtype=torch.uint8, device="cuda")
        tab = _lib.Table(_lib.InflateConn, n)
        for k, row in enumerate(tab.rows):
            row.out, row.out_cap = self.out.data_ptr() + self.stride * k + off, self.cap
            row.vmsgs, row.vmsg_cap = self.vmsgs.data_ptr() + 40 * (VM + 1) * k, VM
            row.ic, row.flags, row.window = self.ic.data_ptr() + 32 * k, self.flags[k], self.win.data_ptr() + GAP + (WIN + GAP) * k
        self.it = tab.upload(torch.device("cuda"))
        self.view, self.vres, self.res = (torch.zeros(s * n, dtype=torch.uint8, device="cuda") for s in (64, 32, 32))
        self.launch(C.c_void_p(torch.cuda.current_stream().cuda_stream))
        return self.read(off)

    def launch(self, stream):
        tin, tres = self.src.tables()
        assert getattr(self.grp.ctx.L, self.fn)(self.grp.ctx.h, ptr(self.dec.conns_t), ptr(tin), ptr(tres), None, ptr(self.it),
                                                self.n, _lib.INF_UTF8, ptr(self.view), ptr(self.vres), ptr(self.res), stream) == 0

    def read(self, off):
        torch.cuda.synchronize()
        assert self.grp.ctx.last_device_error() == 0
        out, win, got, free = self.out.cpu().numpy(), self.win.cpu().numpy(), [], np.ones(self.out.numel(), bool)
        wfree = np.ones(win.size, bool)
        for k in range(self.n):
            r = _lib.read_rows(_lib.InflateResult, self.res, 1, k)[0]
            c = _lib.read_rows(_lib.InflateCarry, self.ic, 1, k)[0]
            recs = _lib.read_rows(_lib.Message, self.vmsgs, min(_lib.read_rows(_lib.ReasmResult, self.vres, 1, k)[0].nmsgs, 9), 10 * k)
            at = self.stride * k + off
            free[at:at + min(r.out_len, self.cap)] = False
            msgs = [out[at + m.out_off:at + min(m.out_off + m.length, self.cap)].tobytes() for m in recs]
            if self.alive[k]:  # the history: the compressed messages inflated whole, while nothing failed
                self.alive[k] = not r.status & (_lib.INF_BAD_DATA | _lib.INF_TOO_LONG)
                whole = b"".join(b for b, m, (_, rsv1) in zip(msgs, recs, self.sent[k]) if rsv1 and m.status == COMPLETE)
                self.hist[k] = (self.hist[k] + whole)[-WIN:] if self.alive[k] else b""
            h, w0 = self.hist[k], GAP + (WIN + GAP) * k
            assert c.win_len == len(h) and (not h or c.win_pos < WIN)
            ring = (c.win_pos - len(h) + np.arange(len(h))) % WIN
            assert win[w0 + ring].tobytes() == h, k  # the window: the ring's image, the history in front of win_pos
            if self.alive[k]:
                wfree[w0 + ring] = False
            got.append(dict(res=(r.out_len, r.n_inflated, r.n_bad, r.status, r.n_history), msgs=msgs, win_len=c.win_len,
                            status=[m.status for m in recs]))
        self.wfree = wfree if self.wfree is None else self.wfree & wfree  # (bytes an earlier history held may stay)
        assert (out[free] == GUARD).all() and (win[self.wfree] == GUARD).all()
        return got


A, B = text(300, 11), text(100, 12)
BIG = rnd(20000, 13) + text(20000, 14)
OLD = rnd(WIN, 15)  # a full window


def zipped(plain):
    c = Client()
    return [c(m) for m in plain]


ZA = zipped([A, A])
SEQUENCES = {  # name: (payloads, rsv1 of each, what each is afterwards (None: bad data), messages per call, out_cap)
    "twice_two_calls": (ZA, "11", [A, A], [1, 1], 512),
    "twice_one_call": (ZA, "11", [A, A], [2], 1024),
    "three_phases": (zipped([A, B + A, A[::-1] + B]), "111", [A, B + A, A[::-1] + B], [1, 1, 1], 1024),
    "ring_wraps": (zipped([BIG, B, BIG[-50:] + B]), "111", [BIG, B, BIG[-50:] + B], [1, 1, 1], 40960),
    "plain_between": ([ZA[0], B, ZA[1]], "101", [A, B, A], [1, 1, 1], 512),
    "distance_win_len": ([Fixed().lits(b"abcdefgh").done(), Fixed().match(8, 8).done()], "11", [b"abcdefgh"] * 2, [1, 1], 64),
    "distance_win_len_plus_1": ([Fixed().lits(b"abcdefgh").done(), Fixed().match(8, 9).done(), Fixed().lits(b"xy").match(3, 2).done()],
                                "111", [b"abcdefgh", None, b"xyxyx"], [1, 2], 64),
    "distance_32768_full_window": ([deflate(OLD, 0), Fixed().match(8, WIN).done()], "11", [OLD, OLD[:8]], [1, 1], WIN + 8),
    "periodic_from_history": ([Fixed().lits(b"abc").done(), Fixed().match(10, 2).done()], "11", [b"abc", b"bcbcbcbcbc"], [1, 1], 64),
    "across_bfinal": ([Fixed(1).lits(b"abcdefgh").done(), Fixed().lits(b"Z").match(8, 9).done()], "11", [b"abcdefgh", b"Zabcdefgh"],
                      [1, 1], 64),
}


def alone(z):
    """Whether the message inflates from an empty window: it does not when a match reaches in front of its first byte."""
    try:
        zlib.decompressobj(-15).decompress(z + TAIL)
        return True
    except zlib.error:
        return False


@pytest.mark.parametrize("name", SEQUENCES)
def test_sequences(ws, name):
    """One connection's messages over one or more calls, the out range at another phase in each."""
    z, rsv1, want, calls, cap = SEQUENCES[name]
    ref, s, i = zlib.decompressobj(-15), Conns(ws, [KEEP], cap), 0
    for c, n in enumerate(calls):
        js = range(i, i + n)
        got = s.call([[(z[j], rsv1[j] == "1") for j in js]], (1, 7, 14)[c])[0]
        for j in js:
            if rsv1[j] == "1" and ref is not None and not ref.eof:  # the reference, as long as its own stream goes on
                try:
                    assert ref.decompress(z[j] + TAIL) == want[j]
                except zlib.error:
                    assert want[j] is None
                    ref = None
            assert got["msgs"][j - i] == (want[j] or b""), (name, j)
            assert got["status"][j - i] == (COMPLETE if want[j] is not None else COMPLETE | TRUNC)
        bad = sum(want[j] is None for j in js)
        assert got["res"] == (sum(len(want[j] or b"") for j in js), sum(rsv1[j] == "1" for j in js) - bad, bad,
                              _lib.INF_BAD_DATA if bad else 0, 0 if bad else sum(rsv1[j] == "1" and not alone(z[j]) for j in js))
        i += n
    assert i == len(z) and s.hist[0] == (b"" if None in want else b"".join(w for w, r in zip(want, rsv1) if r == "1")[-WIN:])


def test_a_capped_record_ends_the_context(ws):
    s, z = Conns(ws, [KEEP], 200), zipped([B, A])
    first, second = s.call([[(z[0], True)]])[0], s.call([[(z[1], True)]])[0]
    assert first["win_len"] == 100 and second["win_len"] == 0 and second["res"] == (201, 0, 0, _lib.INF_TOO_LONG, 0)
    assert second["msgs"] == [A[:200]] and second["status"] == [COMPLETE | TRUNC]


def test_takeover_beside_none_in_one_call(ws):
    """The same streams to a connection that keeps its context and to one that does not (window untouched), and through
    xyws_inflate_streams, which ignores the flag."""
    for fn, flags in (("xyws_inflate_windows_streams", [KEEP, NEG]), ("xyws_inflate_streams", [KEEP, KEEP])):
        s = Conns(ws, flags, 512, fn)
        assert [g["msgs"] for g in s.call([[(ZA[0], True)]] * 2)] == [[A], [A]]
        keeps, other = s.call([[(ZA[1], True)]] * 2, off=9)
        assert other["res"] == (0, 0, 1, _lib.INF_BAD_DATA, 0) and other["win_len"] == 0
        assert (keeps["msgs"] == [A] and keeps["res"] == (300, 1, 0, 0, 1)) if s.alive[0] else keeps == other


def test_graph_replays_follow_the_eager_sweeps(ws):
    """decode, reassemble and the inflate captured once, replayed over three sweeps of new input of the same length."""
    c, sweeps = [Client(), Client()], []
    for t in range(3):
        z = [c[k](text(150 + 20 * k, 20 + t) + A[:120]) for k in range(2)]
        sweeps.append([[(x, True), (b"." * (600 - len(frames(x)) - 8), False)] for x in z])
    eager, want = Conns(ws, [KEEP, KEEP], 1024), []
    for w in sweeps:
        want.append((eager.call(w), eager.win.cpu().numpy().tobytes(), eager.ic.cpu().numpy().tobytes()))
    s = Conns(ws, [KEEP, KEEP], 1024)
    s.call(sweeps[0])  # makes the tables; then every carry and the windows as new
    for t in [t for t, _ in s.grp._carries()] + [s.ic]:
        t.zero_()
    s.win.fill_(GUARD)
    s.hist, s.wfree, L, g, h = [b"", b""], None, s.grp.ctx.L, s.grp, s.grp.ctx.h
    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        st = C.c_void_p(stream.cuda_stream)
        rin, rres = s.src.tables()
        assert L.xyws_decode_streams(h, ptr(s.dec.conns_t), 2, ptr(g.counts_t), 0, st) == 0
        assert L.xyws_reassemble_streams(h, ptr(s.dec.conns_t), ptr(g.counts_t), ptr(rin), 2, 1, ptr(rres), st) == 0
        s.launch(st)
    for w, (rows, win, ic) in zip(sweeps, want):
        s.sent = w
        s.slab.copy_(torch.tensor(list(b"".join(frames(p, rsv1=r, op=2) for msgs in w for p, r in msgs)), dtype=torch.uint8, device="cuda"))
        s.out.fill_(GUARD)
        graph.replay()
        assert s.read(3) == rows and s.win.cpu().numpy().tobytes() == win and s.ic.cpu().numpy().tobytes() == ic
    assert want[2][0][0]["res"] == (270 + len(sweeps[2][0][1][0]), 1, 0, 0, 1) and want[2][0][0]["win_len"] == 3 * 270


def test_through_connection_group(ws):
    """grp.inflate(takeover=...) over two sweeps: connection 0 keeps its context, connection 1 negotiated without."""
    g = ws.connection_group(2, cap=8)
    for t in range(2):
        bufs = [torch.tensor(list(frames(ZA[t])), dtype=torch.uint8, device="cuda") for _ in range(2)]
        areas = [torch.zeros(600, dtype=torch.uint8, device="cuda") for _ in range(2)]
        inf = g.inflate(g.reassemble(g.decode(list(enumerate(bufs))), areas), [0, 1], 512, takeover=[0])
        torch.cuda.synchronize()
        (rec,) = inf.messages(0)
        assert inf.outs[0][rec.out_off:rec.out_off + rec.length].cpu().numpy().tobytes() == A
        assert (inf.result(0).status, inf.result(0).n_history, g.inflate_carry(0).win_len) == (0, t, 300 * (t + 1))
        assert inf.result(1).status == (_lib.INF_BAD_DATA if t else 0) and g.inflate_carry(1).win_len == 0

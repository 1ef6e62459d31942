"""xyws_decode_streams on the device: the recv buffers of many connections in
one call, each decoded exactly as xyws_decode_stream decodes it from its own
carry. Expected values: the CPU oracle, per connection, the carry chained
(oracle.decode_stream(buf, carry_in=...)). Bar: bit-exact bytes, descriptors
with status, counts and carries; not a byte outside a connection's range
written.

A call's connections lie in ONE guarded device buffer (dev_bytes of a host
image filled with 0xA5): connection i starts at misalignment mis[i] of a
16-byte line, or directly after its predecessor (`packed`: a receive slab,
neighbours share lines). Window sizes come from xyws_debug_streams_geometry.
"""
import ctypes as C

import numpy as np
import pytest

import history
import streams
from test_gpu_parity import carry_list, dev_bytes, frames_list, host
from xynet_amd import _lib
from xynet_amd._lib import Carry, Frame

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 0xA5


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
    assert _lib.load().xyws_debug_streams_geometry(out) == 0
    return list(out)


# --------------------------------------------------------------------------- device plumbing
# (five functions: everything below reaches the device through them)
def upload(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def place(image):
    """The host image of a call's buffer on the device."""
    return dev_bytes(image.tobytes(), 0, 0)[0]


def download(t):
    return t.cpu().numpy()


def ptr(t):
    return t.data_ptr()


def launch(ctx, table, n, counts, opts, stream=None):
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream)
    return ctx.L.xyws_decode_streams(ctx.h, C.c_void_p(ptr(table)) if table is not None else None, n,
                                     C.c_void_p(ptr(counts)) if counts is not None else None, opts, s)


def zeros(n, dtype=np.uint8):
    return upload(np.zeros(n, dtype))


# --------------------------------------------------------------------------- one call
def as_array(src):
    return np.frombuffer(src, np.uint8).copy() if len(src) else np.zeros(0, np.uint8)


class Call:
    """The connections of one xyws_decode_streams call.

    srcs: each connection's bytes. mis: each one's misalignment (default
    i % 16), or packed=True: back to back. caps: descriptors per connection
    (None: a null frames pointer). carries: a device tensor of 64 bytes per
    connection id, `ids` the ids (default 0..n-1); carries=None: null carry
    pointers. counts=False: a null dev_nframes."""

    def __init__(self, srcs, mis=None, packed=False, caps=None, carries=None, ids=None, counts=True):
        n = self.n = len(srcs)
        self.srcs = srcs
        self.lens = [len(s) for s in srcs]
        self.ids = list(range(n)) if ids is None else list(ids)
        self.caps = [None] * n if caps is None else list(caps)
        self.carries = carries
        pos, self.offs = 32, []
        for i, s in enumerate(srcs):
            if not packed:
                pos = (pos + 15) // 16 * 16 + 32 + (i % 16 if mis is None else mis[i])
            self.offs.append(pos)
            pos += len(s)
        image = np.full(pos + 64, GUARD, np.uint8)
        for o, s in zip(self.offs, srcs):
            image[o:o + len(s)] = as_array(s)
        self.image = image
        self.view = place(image)
        self.foffs, tot = [], 0
        for c in self.caps:
            self.foffs.append(tot)
            tot += (c or 0)
        self.frames_t = upload(np.full(max(tot, 1) * 32, GUARD, np.uint8))
        self.counts_t = upload(np.full(max(n, 1), -7, np.int64)) if counts else None
        tab = np.zeros((max(n, 1), 8), np.uint64)
        for i in range(n):
            tab[i, 0] = ptr(self.view) + self.offs[i]
            tab[i, 1] = self.lens[i]
            tab[i, 2] = ptr(carries) + 64 * self.ids[i] if carries is not None else 0
            tab[i, 3] = ptr(self.frames_t) + 32 * self.foffs[i] if self.caps[i] is not None else 0
            tab[i, 4] = self.caps[i] or 0
        self.table_t = upload(tab.reshape(-1).view(np.uint8))

    def run(self, ctx, opts=0, stream=None):
        assert launch(ctx, self.table_t, self.n, self.counts_t, opts, stream) == 0
        return self

    # ---- results (host copies)
    def fetch(self):
        self.out = download(self.view)
        self.fr = download(self.frames_t)
        self.cnt = download(self.counts_t) if self.counts_t is not None else None
        self.car = download(self.carries) if self.carries is not None else None
        return self

    def bytes_of(self, i):
        return self.out[self.offs[i]:self.offs[i] + self.lens[i]]

    def frames_of(self, i, n):
        raw = self.fr[32 * self.foffs[i]:32 * (self.foffs[i] + n)].tobytes()
        arr = (Frame * max(n, 1)).from_buffer_copy(raw.ljust(32 * max(n, 1), b"\0"))
        return [arr[k] for k in range(n)]

    def carry_of(self, i):
        return Carry.from_buffer_copy(self.car[64 * self.ids[i]:64 * self.ids[i] + 64].tobytes())

    def guards_intact(self):
        """Every byte of the buffer outside the connections' ranges is still
        the guard value, and so is every descriptor past a connection's cap or
        count."""
        m = np.ones(self.out.size, bool)
        for o, ln in zip(self.offs, self.lens):
            m[o:o + ln] = False
        return bool((self.out[m] == GUARD).all())


def expect(oracle, srcs, carries_in=None):
    """The oracle's decode of every connection: (bytes, frames with status,
    carry, count, the Carry itself)."""
    res = []
    for i, s in enumerate(srcs):
        ob = as_array(s)
        cin = carries_in[i] if carries_in is not None else None
        fr, cout, n = oracle.decode_stream(ob, carry_in=cin)
        assert n == len(fr)
        res.append((ob, frames_list(fr, True), carry_list(cout), n, cout))
    return res


def check(call, exp, what=""):
    """A fetched call against the oracle's results."""
    for i, (ob, ofr, ocarry, on, _) in enumerate(exp):
        w = (what, i)
        if call.cnt is not None:
            assert int(call.cnt[i]) == on, w
        assert call.bytes_of(i).tobytes() == ob.tobytes(), w
        cap = call.caps[i]
        if cap is not None:
            k = min(cap, on)
            assert frames_list(call.frames_of(i, k), True) == ofr[:k], w
            rest = call.fr[32 * (call.foffs[i] + k):32 * (call.foffs[i] + cap)]
            assert (rest == GUARD).all(), w  # (no descriptor past the count or the cap)
        if call.car is not None:
            assert carry_list(call.carry_of(i)) == ocarry, w
    assert call.guards_intact(), what


# --------------------------------------------------------------------------- 1. every edge stream, one call
_EDGE = {}


def edge_expected(oracle):
    if not _EDGE:
        srcs = [streams.case_bytes(n) for n in streams.EDGE_CASES]
        _EDGE["srcs"], _EDGE["exp"] = srcs, expect(oracle, srcs)
    return _EDGE["srcs"], _EDGE["exp"]


def edge_caps(exp, capmode):
    return {"all": [e[3] + 2 for e in exp], "none": None, "some": [e[3] * 6 // 10 for e in exp]}[capmode]


@pytest.mark.parametrize("capmode", ["all", "none", "some"])
def test_every_edge_stream_in_one_call(ctx, oracle, capmode):
    srcs, exp = edge_expected(oracle)
    assert len(srcs) == 31 and max(len(s) for s in srcs) > 4 << 20
    carries = zeros(64 * len(srcs))
    call = Call(srcs, caps=edge_caps(exp, capmode), carries=carries).run(ctx).fetch()
    check(call, exp, capmode)


# --------------------------------------------------------------------------- 2. carry across calls
def test_carry_across_calls(ctx, oracle):
    probes = [p for p in history._fixed_probes() if p.kind == "split"]
    assert len(probes) >= 6 * len(history.SPLIT_NAMES) - 6  # (six split points each, where the list has as many)
    carries = zeros(64 * len(probes))
    cin = None
    for k in (0, 1):
        srcs = [p.pieces[k] for p in probes]
        exp = expect(oracle, srcs, cin)
        call = Call(srcs, caps=[e[3] + 1 for e in exp], carries=carries).run(ctx).fetch()
        check(call, exp, ("piece", k))
        cin = [e[4] for e in exp]
    # negative frame_off and a carried payload whose end resets the key are among them
    assert any(f[0] < 0 for e in exp for f in e[1])


# --------------------------------------------------------------------------- 3. dribble
def test_dribble(ctx, oracle):
    names = ["rfc_hello", "rsv_reserved_ops", "bad_control", "trunc_hdr_13"]
    conns = [(streams.case_bytes(nm), step) for nm in names for step in (1, 2, 3, 7)]
    whole = expect(oracle, [s for s, _ in conns])
    carries = zeros(64 * len(conns))
    got = [bytearray() for _ in conns]
    total = [0] * len(conns)
    k = 0
    while True:
        live = [i for i, (s, step) in enumerate(conns) if k * step < len(s)]
        if not live:
            break
        srcs = [conns[i][0][k * conns[i][1]:(k + 1) * conns[i][1]] for i in live]
        call = Call(srcs, carries=carries, ids=live).run(ctx).fetch()
        assert call.guards_intact(), k
        for j, i in enumerate(live):
            got[i] += call.bytes_of(j).tobytes()
            total[i] += int(call.cnt[j])
        k += 1
    car = download(carries)
    for i, (ob, _, ocarry, on, _) in enumerate(whole):
        assert bytes(got[i]) == ob.tobytes(), i
        assert total[i] == on, i
        assert carry_list(Carry.from_buffer_copy(car[64 * i:64 * i + 64].tobytes())) == ocarry, i


# --------------------------------------------------------------------------- 4. window edges
def test_window_edges(ctx, oracle):
    W = geometry()[0]
    rng = streams.SplitMix(0x57EA)
    srcs, mis = [], []

    def add(src, m=0):
        srcs.append(bytes(src))
        mis.append(m)

    # equal frames of W - k bytes (8-byte headers): headers straddle window ends at every offset
    assert 126 + 24 + 8 <= W <= 65535
    for k in range(24):
        add(b"".join(history.quick_frame(rng, 0x82, W - 8 - k) for _ in range(4)), k % 16)
    # a 14-byte header beginning at W - j
    for j in range(1, 14):
        add(history.sized_frame(rng, W - j) + history.quick_frame(rng, 0x82, 65536 + j))
    # a frame ending exactly at W, and exactly at the end of the connection
    add(history.sized_frame(rng, W) + history.quick_frame(rng, 0x81, 5))
    add(history.sized_frame(rng, W))
    # a masked payload spanning three windows
    for m in (0, 1, 15):
        add(history.quick_frame(rng, 0x82, 3 * W + 100) + history.quick_frame(rng, 0x82, 9), m)
    exp = expect(oracle, srcs)
    carries = zeros(64 * len(srcs))
    call = Call(srcs, mis=mis, caps=[e[3] + 1 for e in exp], carries=carries).run(ctx).fetch()
    check(call, exp, "edges")
    # a connection lying wholly inside a carried frame (history's no_frame shape, 3 W of body)
    hdr = streams.header(0x82, 1 << 20, rng.bytes(4))
    body = rng.bytes(3 * W)
    carries = zeros(64 * 3)
    cin = None
    for piece in (hdr, body):
        pieces = [piece] * 3
        exp = expect(oracle, pieces, cin)
        call = Call(pieces, mis=[0, 1, 15], caps=[2] * 3, carries=carries).run(ctx).fetch()
        check(call, exp, "inside")
        cin = [e[4] for e in exp]
    assert exp[0][3] == 0 and exp[0][4].payload_remaining == (1 << 20) - 3 * W


# --------------------------------------------------------------------------- 5. slab
def test_slab_of_tiny_connections(ctx, oracle):
    n = 20000
    assert n > geometry()[3]
    rng = streams.SplitMix(0x51AB)
    srcs = []
    for _ in range(n):
        srcs.append(b"".join(history.quick_frame(rng, 0x82, rng.below(41)) for _ in range(1 + rng.below(3))))
    slab = as_array(b"".join(srcs))
    _, _, total = oracle.decode_stream(slab, cap=1)
    carries = zeros(64 * n)
    call = Call(srcs, packed=True, carries=carries).run(ctx).fetch()
    a = call.offs[0]
    assert call.out[a:a + slab.size].tobytes() == slab.tobytes()
    assert call.guards_intact()
    assert int(call.cnt.sum()) == total
    ft = call.car.reshape(n, 64)[:, 16:24].copy().view(np.uint64).reshape(-1)
    assert (ft == call.cnt.astype(np.uint64)).all()
    # every connection holds whole frames: its frames_total is the frames it was built from
    want = []
    for s in srcs:
        c, p = 0, 0
        while p < len(s):
            p += 6 + (s[p + 1] & 0x7F)
            c += 1
        want.append(c)
    assert (ft == np.array(want, np.uint64)).all()
    rest = call.car.reshape(n, 64)
    assert not rest[:, :16].any() and not rest[:, 24:43].any()  # every carry at a frame boundary


# --------------------------------------------------------------------------- 6. mixed lengths
def test_mixed_lengths(ctx, oracle):
    W = geometry()[0]
    lens = [0, 1, 2, 5, 6, 13, 14, 15, 16, 17, 100, 1000, 4096, W - 1, W, W + 1, 65539]
    rng = streams.SplitMix(0x3117)
    traffic, starts = bytearray(), []
    while len(traffic) < (3 << 20):
        starts.append(len(traffic))
        traffic += history.quick_frame(rng, 0x82 if rng.below(8) else 0x89, rng.below(1001))
    traffic = bytes(traffic)
    n = 1000
    first, second = [], []
    for i in range(n):
        a = 1 << 20 if i == 333 else lens[rng.below(len(lens))]
        b = 1 << 20 if i == 777 else lens[rng.below(len(lens))]
        o = starts[rng.below(len(starts) // 2)]
        first.append(traffic[o:o + a])
        second.append(traffic[o + a:o + a + b])
        assert len(first[-1]) == a and len(second[-1]) == b
    carries = zeros(64 * n)
    cin = None
    for k, srcs in enumerate((first, second)):
        exp = expect(oracle, srcs, cin)
        call = Call(srcs, carries=carries).run(ctx).fetch()
        for i, (ob, _, ocarry, on, _) in enumerate(exp):
            assert int(call.cnt[i]) == on, (k, i)
            assert oracle.digest(np.ascontiguousarray(call.bytes_of(i))) == oracle.digest(ob), (k, i)
            assert carry_list(call.carry_of(i)) == ocarry, (k, i)
        assert call.guards_intact(), k
        cin = [e[4] for e in exp]


# --------------------------------------------------------------------------- 7. options and nulls
def test_options_and_nulls(ws, ctx, oracle):
    srcs, exp = edge_expected(oracle)
    srcs, exp = srcs[:13], exp[:13]
    # parse only: the bytes stay, the descriptors and carries are the same
    carries = zeros(64 * len(srcs))
    call = Call(srcs, caps=[e[3] + 1 for e in exp], carries=carries).run(ctx, _lib.OPT_PARSE_ONLY).fetch()
    for i, (ob, ofr, ocarry, on, _) in enumerate(exp):
        assert call.bytes_of(i).tobytes() == srcs[i]
        assert int(call.cnt[i]) == on and frames_list(call.frames_of(i, on), True) == ofr
        assert carry_list(call.carry_of(i)) == ocarry
    assert call.guards_intact()
    # the hint is accepted and ignored; null carries, null counts
    call = Call(srcs, caps=[e[3] + 1 for e in exp], carries=None, counts=False).run(ctx, _lib.OPT_UNMASKED_HINT).fetch()
    check(call, exp, "nulls")
    # n == 0 launches nothing; n == 1 is frame_decoder.decode on the same bytes
    assert launch(ctx, None, 0, None, 0) == 0
    src = streams.case_bytes("random_frames_40")
    one = Call([src], mis=[3], caps=[100], carries=zeros(64)).run(ctx).fetch()
    dec = ws.frame_decoder(ctx=ctx)
    view, _ = dev_bytes(src, 3)
    r = dec.decode(view, cap=100)
    assert int(one.cnt[0]) == r.nframes > 100  # (more frames than descriptors: the count exceeds the cap)
    assert one.bytes_of(0).tobytes() == host(view)
    assert frames_list(one.frames_of(0, 100), True) == frames_list(r.frames(), True)
    assert carry_list(one.carry_of(0)) == carry_list(dec.carry())
    # refused options: -1, nothing touched
    for bad in (_lib.OPT_SERIAL_SCAN, _lib.OPT_PARSE_ONLY | _lib.OPT_STATS, 0x80000000):
        call = Call(srcs, caps=[e[3] + 1 for e in exp], carries=zeros(64 * len(srcs)))
        assert launch(ctx, call.table_t, call.n, call.counts_t, bad) == -1
        call.fetch()
        assert call.out.tobytes() == call.image.tobytes()
        assert (call.fr == GUARD).all() and not call.car.any() and (call.cnt == -7).all()
    assert launch(ctx, None, 3, None, 0) == -1


# --------------------------------------------------------------------------- 8. no slot, no history
def test_no_slot_and_no_history(ws, ctx, oracle):
    srcs, exp = edge_expected(oracle)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pol = (C.c_uint64 * _lib.POL_WORDS)()
    call = Call(srcs[:8], carries=zeros(64 * 8)).run(ctx)
    torch.cuda.synchronize()
    assert ctx.L.xyws_debug_policy(ctx.h, stream, pol) == -1  # no slot bound: the call took none
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
    call = Call(srcs[:8], carries=zeros(64 * 8)).run(ctx).fetch()
    check(call, exp[:8], "after the primer")
    assert ctx.L.xyws_debug_policy(ctx.h, stream, pol) == 0
    assert list(pol) == before


# --------------------------------------------------------------------------- 9. capture
def test_captured_without_a_reserve(ctx, oracle):
    srcs, exp = edge_expected(oracle)
    carries = zeros(64 * len(srcs))
    call = Call(srcs, caps=[e[3] + 2 for e in exp], carries=carries)
    orig = call.view.clone()
    s = torch.cuda.Stream()  # (new to the context; nothing was reserved)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        call.run(ctx, stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(call.view, orig) and not bool(carries.any())  # (capture ran nothing)
    for rep in range(3):
        call.view.copy_(orig)
        carries.zero_()
        g.replay()
        torch.cuda.synchronize()
        check(call.fetch(), exp, ("replay", rep))


# --------------------------------------------------------------------------- 10. the Python layer
def test_connection_group(ws, ctx, oracle):
    srcs, exp = edge_expected(oracle)
    names = list(streams.EDGE_CASES)
    grp = ws.connection_group(12, cap=800, ctx=ctx)
    state = {}

    def feed(items):
        bufs = [(i, dev_bytes(piece, 1 + i % 7)[0]) for i, piece in items]
        res = grp.decode(bufs)
        for k, ((i, piece), (_, view)) in enumerate(zip(items, bufs)):
            ob = as_array(piece)
            fr, cout, n = oracle.decode_stream(ob, carry_in=state.get(i))
            state[i] = cout
            assert res.nframes(k) == n, (i, k)
            assert frames_list(res.frames(k), True) == frames_list(fr[:800], True), (i, k)
            assert host(view) == ob.tobytes(), (i, k)
            assert carry_list(grp.carry(i)) == carry_list(cout), (i, k)

    a, b = streams.case_bytes("lengths"), streams.case_bytes("tiny_frames")
    feed([(2, a[:70000]), (5, b[:1001]), (9, srcs[names.index("rfc_hello")])])
    feed([(5, b[1001:]), (2, a[70000:]), (11, srcs[names.index("trunc_hdr_9")])])
    for i in range(12):
        if i not in state:
            assert bytes(grp.carry(i)) == bytes(64), i
    with pytest.raises(_lib.XywsError):
        grp.decode([(1, dev_bytes(a)[0]), (1, dev_bytes(b)[0])])  # an id twice
    grp.reset([2])
    assert bytes(grp.carry(2)) == bytes(64) and grp.carry(5).frames_total == state[5].frames_total
    grp.reset()
    assert bytes(grp.carry(5)) == bytes(64)

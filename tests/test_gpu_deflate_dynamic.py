"""xyws_deflate_streams with XYWS_DFO_DYNAMIC over the tables of test_gpu_deflate. Reference: zlib's inflater (Sweep.check:
round trip, bound, exact rows, guard bytes), the same call with opts = 0, for the code builder a plain Huffman (heapq)."""
import ctypes as C
import heapq
import zlib

import pytest

from xynet_amd import _lib
from test_gpu_deflate import CASES, COMPLETE, HEADED, VM, W, Rooms, Sweep, dev, frames_of, grp, ptr, rnd, text, torch  # noqa: F401

pytestmark = pytest.mark.gpu


class Dynamic(Sweep):
    def deflate(self, g, bconns, stream):
        assert g.ctx.L.xyws_deflate_streams(g.ctx.h, ptr(self.rt), ptr(self.rres), ptr(bconns), ptr(self.dt), self.n,
                                            _lib.DFO_DYNAMIC, ptr(self.view), ptr(self.vres), ptr(self.vbc), ptr(self.res),
                                            stream) == 0


def one_call(g, cls, conns, **kw):
    s = cls(conns, **kw)
    bconns = s.bt.upload(torch.device("cuda"))
    s.deflate(g, bconns, None)
    torch.cuda.synchronize()
    assert g.ctx.last_device_error() == 0
    return s.check(bconns)


def de_bruijn():
    """B(4, 4) unrolled to 259 bytes over four values (prefer the largest value that makes a new 4-gram): no 4-gram twice."""
    s, seen = [0] * 4, {(0, 0, 0, 0)}
    while len(s) < 259:
        v = next(v for v in (3, 2, 1, 0) if tuple(s[-3:] + [v]) not in seen)
        seen.add(tuple(s[-3:] + [v]))
        s.append(v)
    return bytes(b"acgt"[v] for v in s)


SHAPES = {  # name: head + message
    "de_bruijn": de_bruijn(), "de_bruijn_run": de_bruijn() + b"q" * 300, "text_300": text(300, 21), "json": CASES["json"],
    "random_300": rnd(300, 4), "L1": b"a", "run_1000": b"x" * 1000, "piece_W+1": CASES["piece_W+1"], "piece_2W+65": CASES["piece_2W+65"],
}


@pytest.fixture(scope="module")
def both(grp):
    conns = [(m[:HEADED.get(k, 0)], 0, [(m[HEADED.get(k, 0):], COMPLETE, 1)]) for k, m in SHAPES.items()]
    return {k: (d, f) for k, d, f in zip(SHAPES, one_call(grp, Dynamic, conns), one_call(grp, Sweep, conns))}


@pytest.mark.parametrize("name", SHAPES)
def test_message_shapes(both, name):
    ((z,), r), ((z0,), r0) = both[name]
    L = len(SHAPES[name])
    assert len(z) <= len(z0) and r.n_deflated + r.n_stored == 1 and r.n_dynamic <= r.n_deflated and r0.n_dynamic == 0
    if name in ("random_300", "L1", "run_1000"):
        assert z == z0 and r.n_dynamic == 0 and r.n_stored == (name == "random_300")
    else:
        assert r.n_dynamic == 1
    if name == "de_bruijn":
        assert len(z) < L // 2
    if name == "text_300":
        assert len(z) < L
    if name in ("json", "piece_2W+65"):
        assert len(z) < len(z0)


@pytest.mark.parametrize("short", ["out_cap", "vmsg_cap"])
def test_the_caps(grp, short):
    recs = [(text(300, 1), COMPLETE, 1), (rnd(200, 2), COMPLETE, 2), (b"tail", COMPLETE, 1)]
    full = one_call(grp, Dynamic, [(b"", 0, recs)] * 2)[0][0]
    caps = [len(full[0]) + len(full[1]) - 1, 500] if short == "out_cap" else None
    got = one_call(grp, Dynamic, [(b"", 0, recs)] * 2, out_caps=caps, vmsg_cap=VM if caps else 2)
    assert got[1][0] == (full if caps else full[:2]) and got[0][0] == (full[:1] if caps else full[:2])
    assert got[0][1].status == (_lib.DFL_TOO_LONG if caps else _lib.DFL_MSG_CAP) and (not caps or got[0][1].out_len > caps[0])
    assert (got[0][1].n_dynamic, got[1][1].n_dynamic) == (1, 1)  # (the prose record, in both connections)


FIB = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181, 6765]
BUILDER = {"fibonacci_20": (FIB, 15), "fibonacci_19_limit_7": (FIB[:19], 7), "equal_286": ([5] * 286, 15),
           "one_heavy": ([1] * 100 + [1 << 20] + [1] * 185, 15), "two_used": ([0, 3, 0, 0, 9, 0], 15),
           "one_used": ([0, 0, 7, 0], 15), "none_used": ([0] * 19, 7)}


def huffman(freq):
    """(cost, depth) of the optimal prefix code, the shallowest of the optimal trees. (The device's merge does not promise
    the shallowest one: a vector with ties whose shallowest optimum just fits the limit does not belong in BUILDER.)"""
    h = [(f, 0) for f in freq if f]
    heapq.heapify(h)
    cost = 0
    while len(h) > 1:
        (a, da), (b, d) = heapq.heappop(h), heapq.heappop(h)
        cost += a + b
        heapq.heappush(h, (a + b, max(da, d) + 1))
    return cost, h[0][1]


@pytest.mark.parametrize("name", BUILDER)
def test_code_builder(grp, name):
    freq, limit = BUILDER[name]
    f, lens = torch.tensor(freq, dtype=torch.int32, device="cuda"), torch.full((len(freq) + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    assert grp.ctx.L.xyws_debug_deflate_code_lengths(grp.ctx.h, ptr(f), len(freq), limit, ptr(lens), None) == 0
    torch.cuda.synchronize()
    got, used = lens.tolist()[:len(freq)], sum(1 for v in freq if v)
    assert lens[len(freq):].tolist() == [0xA5] * 8 and [l == 0 for l in got] == [v == 0 for v in freq] and max(got) <= limit
    assert used != 1 or max(got) == 1
    if used >= 2:
        (best, depth), cost = huffman(freq), sum(v * l for v, l in zip(freq, got))
        assert sum(1 << (limit - l) for l in got if l) == 1 << limit  # Kraft, exactly
        assert (cost == best) if depth <= limit else (best <= cost <= (used - 1).bit_length() * sum(freq))


class DynamicRooms(Rooms):
    # the first message is prose that only the dynamic code shortens; the sweep's call has the bit
    def __init__(self, g, negotiated, seed):
        super().__init__(g, negotiated, seed)
        self.sweep.__class__ = Dynamic

    def messages(self, seed):
        return [(b"m%d: " % k, r, [(text(200 + 9 * k, seed + k), COMPLETE, 1), (rnd(40, seed + k), COMPLETE, 2)])
                for k, r in enumerate(self.ROOM)]


def test_captured_and_replayed_on_a_second_sweep(grp):
    ref, rooms = DynamicRooms(grp, (), 11), DynamicRooms(grp, (2,), 11)
    s, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    rooms.deflated()  # eager once: what the replays are held against
    ref.plain()
    rooms.check(ref.image())
    with torch.cuda.graph(graph, stream=s):
        rooms.deflated(C.c_void_p(s.cuda_stream))
    for seed in (23, 23, 11):
        for r in (ref, rooms):
            r.sweep.load(r.messages(seed))
            for t in (r.sends, r.sweep.slab, *r.wires, *r.zwires):
                t.fill_(0xA5)
        graph.replay()
        ref.plain()
        rooms.check(ref.image())
        assert [row.n_dynamic for row in _lib.read_rows(_lib.DeflateResult, rooms.sweep.res, 5, 0)] == [1] * 5


def test_through_connection_group(grp):
    """grp.deflate(dynamic=True), grp.broadcast(deflated=...): RSV1 frames, what the others get, shorter than dynamic=False."""
    import streams
    from xynet_amd import websocket as ws
    key, said, sent = b"\x37\xfa\x21\x3d", [text(90, k) * 3 for k in range(3)], {}
    for dynamic in (True, False):
        g = ws.connection_group(3, cap=8)
        bufs = [dev(streams.header(0x81, len(m), key) + streams.masked(m, key)) for m in said]  # (alive until the sweep's last call)
        msgs = g.reassemble(g.decode(list(enumerate(bufs))), [torch.zeros(600, dtype=torch.uint8, device="cuda") for _ in range(3)])
        sends = [torch.zeros(2000, dtype=torch.uint8, device="cuda") for _ in range(3)]
        dfl = g.deflate(msgs, [1], 300, dynamic=dynamic)
        bc = g.broadcast(msgs, [[0, 1, 2]], sends, heads=[dev(b"%d: " % k) for k in range(3)], deflated=dfl)
        torch.cuda.synchronize()
        plain = sends[0][:bc.result(0).send_len].cpu().numpy().tobytes()
        sent[dynamic] = sends[1][:bc.result(1).send_len].cpu().numpy().tobytes()
        assert [dfl.result(k).n_dynamic for k in range(3)] == [int(dynamic)] * 3
        for (b0, pay), (p0, body), k in zip(frames_of(sent[dynamic]), frames_of(plain), range(3)):
            d = zlib.decompressobj(-15)
            assert b0 == 0xC1 and p0 == 0x81 and d.decompress(pay + b"\x00\x00\xff\xff") == body == b"%d: " % k + said[k]
            assert not d.unused_data
    assert len(sent[True]) < len(sent[False])

"""xyws_inflate_streams on the device: the permessage-deflate messages of a
sweep inflated between hold and broadcast, through the C-ABI. Reference:
zlib.decompressobj(-15) on the host over payload + 00 00 ff ff; bad inputs are
fixed bytes with fixed expectations. Bar: byte-exact out ranges, exact view
records and result rows, not a guard byte changed around an out range or behind
a record row. The frames are built by tests/golden/streams.py; only RSV1 is
ORed into byte 0 of a message's first frame. Every out range lies in one
guard-filled slab at odd offsets; decode, reassemble and hold run through
connection_group, the inflate call through ctypes over tables of the test."""
import ctypes as C
import random
import zlib

import numpy as np
import pytest

import streams
from xynet_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
GUARD, KEY = 0xA5, b"\x37\xfa\x21\x3d"
COMPLETE, UTF8_BAD, TRUNC = 0x1, 0x2, 0x8


@pytest.fixture(scope="module")
def ws():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from xynet_amd import websocket
    return websocket


def deflate(data, level=9, **kw):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, **kw)
    out = c.compress(data) + c.flush(zlib.Z_SYNC_FLUSH)
    assert out.endswith(b"\x00\x00\xff\xff")
    return out[:-4]


def frames(payload, rsv1=True, op=1, parts=1):
    """One client message of `parts` frames; RSV1 on the first only."""
    cut = [len(payload) * i // parts for i in range(parts + 1)]
    return b"".join(streams.header((0x80 if i == parts - 1 else 0) | (0x40 if rsv1 and i == 0 else 0) | (op if i == 0 else 0),
                                   cut[i + 1] - cut[i], KEY) + streams.masked(payload[cut[i]:cut[i + 1]], KEY)
                    for i in range(parts))


class Sweeps:
    """n connections over several sweeps: decode, reassemble and (hold_cap > 0)
    hold through a connection_group, then one xyws_inflate_streams call."""

    def __init__(self, ws, negotiated, out_caps, hold_cap=0, utf8=True, area=4096):
        self.n, self.hold_cap, self.utf8, self.out_caps = len(out_caps), hold_cap, utf8, out_caps
        self.grp = ws.connection_group(self.n, cap=8)
        self.areas = [torch.zeros(hold_cap + area, dtype=torch.uint8, device="cuda") for _ in range(self.n)]
        self.offs, pos = [], 3
        for k, c in enumerate(out_caps):  # out ranges at odd offsets, 5..11 guard bytes between them
            self.offs.append(pos)
            pos += c + 5 + k % 7
        self.slab_len = pos
        self.ic = torch.zeros(32 * self.n, dtype=torch.uint8, device="cuda")
        self.flags = [1 if g else 0 for g in negotiated]

    def sweep(self, wires):
        g, n, VM = self.grp, self.n, 9
        bufs = [torch.tensor(list(w), dtype=torch.uint8, device="cuda") for w in wires]
        dec = g.decode(list(enumerate(bufs)))
        src = g.reassemble(dec, [a[self.hold_cap:] for a in self.areas])
        if self.hold_cap:
            src = g.hold(src, self.hold_cap)
        slab = torch.full((self.slab_len,), GUARD, dtype=torch.uint8, device="cuda")
        vmsgs = torch.full((40 * (VM + 1) * n,), GUARD, dtype=torch.uint8, device="cuda")
        tab = _lib.Table(_lib.InflateConn, n)
        for k, row in enumerate(tab.rows):
            row.out, row.out_cap = slab.data_ptr() + self.offs[k], self.out_caps[k]
            row.vmsgs, row.vmsg_cap = vmsgs.data_ptr() + 40 * (VM + 1) * k, VM
            row.ic, row.flags = self.ic.data_ptr() + 32 * k, self.flags[k]
        it = tab.upload(torch.device("cuda"))
        view, vres, res = (torch.full((s * (n + 1),), GUARD, dtype=torch.uint8, device="cuda") for s in (64, 32, 32))
        tin, tres = src.tables()
        hres = src._tensors["results"].data_ptr() if self.hold_cap else None
        p = lambda t: C.c_void_p(t.data_ptr())
        rc = g.ctx.L.xyws_inflate_streams(g.ctx.h, p(dec.conns_t), p(tin), p(tres), hres, p(it), n,
                                          _lib.INF_UTF8 if self.utf8 else 0, p(view), p(vres), p(res),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        torch.cuda.synchronize()
        assert g.ctx.last_device_error() == 0
        got, host, vm, free = [], slab.cpu().numpy(), vmsgs.cpu().numpy(), np.ones(self.slab_len, bool)
        for t, s in ((view, 64), (vres, 32), (res, 32)):
            assert (t[s * n:].cpu().numpy() == GUARD).all()  # row n of every table
        for k in range(n):
            r = _lib.read_rows(_lib.InflateResult, res, 1, k)[0]
            v = _lib.read_rows(_lib.ReasmResult, vres, 1, k)[0]
            recs = _lib.read_rows(_lib.Message, vmsgs, min(v.nmsgs, VM), (VM + 1) * k) if not r.status & 1 else src.messages(k)
            if not r.status & 1:
                assert (vm[40 * ((VM + 1) * k + len(recs)):40 * (VM + 1) * (k + 1)] == GUARD).all(), k
                free[self.offs[k]:self.offs[k] + min(r.out_len, self.out_caps[k])] = False  # nothing behind out_len
                assert v.out_len == r.out_len == sum(m.length for m in recs)
            data = host[self.offs[k]:self.offs[k] + self.out_caps[k]].tobytes()
            got.append(dict(res=(r.out_len, r.n_inflated, r.n_bad, r.status), vstatus=v.status, inputs=src.messages(k),
                            recs=[(m.out_off, m.length, m.status, m.opcode) for m in recs],
                            msgs=[data[m.out_off:m.out_off + m.length] for m in recs]))
        assert (host[free] == GUARD).all()
        return got


def text(n, seed):
    r = random.Random(seed)
    return bytes(r.choice(b"eeeeeeeetttttaaaaooiinnsshhrrdlucmfwypvbgkqjxz ,.") for _ in range(n))


def rnd(n, seed):
    return random.Random(seed).randbytes(n)


BLOCK = rnd(300, 5)
GOOD = {  # name: the message's compressed payload
    "empty": bytes.fromhex("00"),
    "rfc_hello_fixed": bytes.fromhex("f248cdc9c90700"),
    "rfc_hello_bfinal": bytes.fromhex("f348cdc9c9070000"),
    "stored": deflate(text(300, 1), 0),
    "rfc_two_blocks": bytes.fromhex("f24805000000ffffcac9c90700"),
    "dynamic_repeat_codes": deflate(text(600, 7) + b"z" * 400),
    "single_distance_code": bytes.fromhex("0de081000000008020b0be3fc487db02"),
    "distance_32768": deflate(BLOCK + rnd(32468, 6) + BLOCK),
    "distance_32769": deflate(BLOCK + rnd(32469, 6) + BLOCK),
    **{f"period_{p}": deflate((rnd(p, p) * 700)[:700]) for p in (1, 2, 3, 63, 64, 65)},
}
BAD = {  # fixed bytes
    "preset_dictionary": bytes.fromhex("cac02e0c650300"),  # zlib: invalid distance too far back
    "block_type_3": bytes.fromhex("06"),
    "len_nlen": bytes.fromhex("000500000068656c6c6f"),
    "oversubscribed_lengths": bytes.fromhex("04e093244992244992000000"),
    "stored_past_the_end": bytes.fromhex("001000efff6162"),
}


def inflated(payload):
    return zlib.decompressobj(-15).decompress(payload + b"\x00\x00\xff\xff")


@pytest.mark.parametrize("name", sorted(GOOD))
def test_block_kinds_and_matches(ws, name):
    want = inflated(GOOD[name])
    got = Sweeps(ws, [True], [len(want) + 3], area=40000).sweep([frames(GOOD[name], op=2)])[0]
    assert got["res"] == (len(want), 1, 0, 0) and got["recs"] == [(0, len(want), COMPLETE, 2)]
    assert got["msgs"][0] == want


@pytest.mark.parametrize("name", sorted(BAD))
def test_bad_data_next_to_a_good_connection(ws, name):
    hello = GOOD["rfc_hello_fixed"]
    got = Sweeps(ws, [True] * 3, [64, 64, 64]).sweep([frames(hello), frames(BAD[name]) + frames(hello), frames(hello)])
    for k in (0, 2):
        assert got[k]["res"] == (5, 1, 0, 0) and got[k]["msgs"] == [b"Hello"]
    assert got[1]["res"] == (5, 1, 1, _lib.INF_BAD_DATA)  # the record after the bad one is still inflated
    assert got[1]["recs"] == [(0, 0, COMPLETE | TRUNC, 1), (0, 5, COMPLETE, 1)] and got[1]["msgs"][1] == b"Hello"


def test_where_the_flag_comes_from(ws):
    msg, plain = text(200, 3), b"not compressed"
    z = deflate(msg)
    wires = [frames(z, parts=3), frames(z) + frames(plain, rsv1=False), frames(z) + frames(plain, rsv1=False)]
    got = Sweeps(ws, [True, True, False], [300, 300, 300]).sweep(wires)
    assert got[0]["msgs"] == [msg] and got[0]["recs"] == [(0, 200, COMPLETE, 1)] and got[0]["inputs"][0].nframes == 3
    assert got[1]["msgs"] == [msg, plain] and got[1]["res"] == (214, 1, 0, 0)
    assert got[2]["res"] == (0, 0, 0, _lib.INF_PASSTHROUGH)  # the reassembly's rows, verbatim
    assert [(m.length, m.status & ~UTF8_BAD) for m in got[2]["inputs"]] == [(len(z), COMPLETE), (len(plain), COMPLETE)]


@pytest.mark.parametrize("cut", ["header_after_1_byte", "mid_payload"])
def test_messages_that_span_sweeps(ws, cut):
    msg = text(500, 4)
    wire = frames(deflate(msg))
    at = 1 if cut == "header_after_1_byte" else len(wire) // 2
    s = Sweeps(ws, [True], [600], hold_cap=2 * 600 + 32)
    first = s.sweep([wire[:at]])[0]
    assert first["res"][1:] == (0, 0, 0) and all(not st & COMPLETE for _, _, st, _ in first["recs"])
    got = s.sweep([wire[at:]])[0]
    assert got["res"] == (500, 1, 0, 0) and got["recs"] == [(0, 500, COMPLETE, 1)] and got["msgs"] == [msg]
    again = s.sweep([frames(b"plain", rsv1=False)])[0]  # the carry's answer ended with the message
    assert again["res"] == (5, 0, 0, 0) and again["msgs"] == [b"plain"]


@pytest.mark.parametrize("over", [0, 1, "bomb"])
def test_the_cap(ws, over):
    msg = b"\0" * (1 << 20) if over == "bomb" else text(333, 8)
    z = deflate(msg)
    cap = 4096 if over == "bomb" else len(msg) - over
    assert over != "bomb" or len(z) > 1000  # a 1 KiB payload, 1 MiB inflated
    got = Sweeps(ws, [True, True], [cap, 64]).sweep([frames(z, op=2), frames(GOOD["rfc_hello_fixed"])])
    if over == 0:
        assert got[0]["res"] == (cap, 1, 0, 0) and got[0]["msgs"] == [msg]
    else:  # no further than the first byte that does not fit; the guards behind the cap are checked by sweep()
        assert got[0]["res"] == (cap + 1, 0, 0, _lib.INF_TOO_LONG) and got[0]["recs"] == [(0, cap + 1, COMPLETE | TRUNC, 2)]
        assert got[0]["msgs"][0][:cap] == msg[:cap] and got[0]["vstatus"] & 0x1
    assert got[1]["msgs"] == [b"Hello"]


@pytest.mark.parametrize("utf8", [True, False])
def test_utf8_is_judged_on_the_inflated_bytes(ws, utf8):
    good, bad = ("Grüße, ünïcödé € 𝄞 日本語 " * 9).encode(), "ab€".encode()[:-1] + b"cd" * 40
    # (the compressed bytes of `good` are no UTF-8: the reassembly marks the record)
    got = Sweeps(ws, [True, True], [400, 400], utf8=utf8).sweep([frames(deflate(good)), frames(deflate(bad))])
    assert got[0]["inputs"][0].status & UTF8_BAD and got[0]["msgs"] == [good] and got[1]["msgs"] == [bad]
    assert got[0]["recs"][0][2] == COMPLETE and got[1]["recs"][0][2] == COMPLETE | (UTF8_BAD if utf8 else 0)
    assert bool(got[1]["vstatus"] & 0x10) == utf8 and not got[0]["vstatus"] & 0x10


@pytest.mark.parametrize("held", [False, True])
def test_a_mixed_room_through_connection_group(ws, held):
    """Negotiated and other connections in one room through grp.inflate and
    grp.broadcast: an item that passes through keeps its input's records,
    bytes and capacity (larger than the inflate range here)."""
    plain = [text(30, 1), text(300, 2), text(40, 3), text(500, 4)]
    HC = 2 * 600 + 32 if held else 0

    def sweep(deflated):
        g = ws.connection_group(4, cap=8)
        wires = [frames(deflate(m) if deflated and k % 2 == 0 else m, rsv1=deflated and k % 2 == 0) for k, m in enumerate(plain)]
        bufs = [torch.tensor(list(w), dtype=torch.uint8, device="cuda") for w in wires]  # (alive until the sweep's last call)
        dec = g.decode(list(enumerate(bufs)))
        areas = [torch.zeros(HC + 600, dtype=torch.uint8, device="cuda") for _ in range(4)]
        msgs = g.reassemble(dec, [a[HC:] for a in areas])
        msgs = g.hold(msgs, HC) if held else msgs
        inf = g.inflate(msgs, [0, 2], 64) if deflated else msgs
        sends = [torch.zeros(2000, dtype=torch.uint8, device="cuda") for _ in range(4)]
        bc = g.broadcast(inf, [[0, 1, 2, 3]], sends)
        torch.cuda.synchronize()
        return inf, bc

    inf, bc = sweep(True)
    want = sweep(False)[1]
    assert bc.room_result(0).nmsgs == 4 and bc.room_result(0).status == 0
    assert bc.wire(0).cpu().numpy().tobytes() == want.wire(0).cpu().numpy().tobytes()
    assert inf.out_caps == [64, 600 + HC, 64, 600 + HC]
    for k, m in enumerate(plain):
        (rec,) = inf.messages(k)
        assert inf.result(k).status == (0 if k % 2 == 0 else _lib.INF_PASSTHROUGH)
        assert (rec.length, rec.status) == (len(m), COMPLETE)
        assert inf.outs[k][rec.out_off:rec.out_off + rec.length].cpu().numpy().tobytes() == m, k


def test_many_connections_eager_and_captured(ws):
    """130 connections, a mix of the above, through connection_group: the
    broadcast's wires equal those of the same messages sent uncompressed, in
    the eager sweep and in three replays of one graph of decode, reassemble,
    hold, inflate and broadcast."""
    n, kinds = 130, sorted(k for k in GOOD if not k.startswith("distance")) + sorted(BAD)
    plan = []  # per connection: (compressed payload or None, what the room gets)
    for k in range(n):
        name = kinds[k % len(kinds)]
        if k % 5 == 4:
            m = text(20 + k, k)
            plan.append([(None, m), (deflate(m), m)])
        elif name in BAD:
            plan.append([(BAD[name], None), (GOOD["rfc_hello_fixed"], b"Hello")])
        else:
            plan.append([(GOOD[name], inflated(GOOD[name]))])
    wires = [b"".join(frames(m if z is None else z, rsv1=z is not None, op=2) for z, m in p) for p in plan]
    twins = [b"".join(frames(m, rsv1=False, op=2) for _, m in p if m is not None) for p in plan]
    rooms, HC = [list(range(r, n, 4)) for r in range(4)], 2 * 1100 + 32

    def sweep(grp, slab, lens, deflated):
        bufs, pos = [], 0
        for ln in lens:
            bufs.append(slab[pos:pos + ln])
            pos += ln
        dec = grp.decode(list(enumerate(bufs)))
        areas = [torch.zeros(HC + 1200, dtype=torch.uint8, device="cuda") for _ in range(n)]
        msgs = grp.hold(grp.reassemble(dec, [a[HC:] for a in areas]), HC)
        inf = grp.inflate(msgs, range(n), 1100) if deflated else None
        sends = [torch.zeros(60000, dtype=torch.uint8, device="cuda") for _ in range(n)]
        bc = grp.broadcast(inf or msgs, rooms, sends, flags=0x12)
        return dec, msgs, inf, bc, sends, areas

    def image(ws_wires):
        return torch.tensor(list(b"".join(ws_wires)), dtype=torch.uint8, device="cuda")

    gt = ws.connection_group(n, cap=8)
    want = sweep(gt, image(twins), [len(w) for w in twins], False)[3]
    want_wires = [want.wire(r).cpu().numpy().tobytes() for r in range(4)]
    g, pristine = ws.connection_group(n, cap=8), image(wires)
    slab = pristine.clone()
    dec, msgs, inf, bc, sends, areas = sweep(g, slab, [len(w) for w in wires], True)
    assert [bc.wire(r).cpu().numpy().tobytes() for r in range(4)] == want_wires and len(want_wires[0]) > 3000
    assert sum(inf.result(k).n_bad for k in range(n)) == sum(1 for p in plan if p[0][1] is None)
    eager_sends = [t.cpu().numpy().tobytes() for t in sends]

    carries, L, h = [t for t, _ in g._carries()], g.ctx.L, g.ctx.h
    zero = [torch.zeros_like(t) for t in carries]
    p = lambda t: C.c_void_p(t.data_ptr())
    hold_t, inf_t = msgs._tensors, inf._tensors
    s, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=s):
        st = C.c_void_p(s.cuda_stream)
        slab.copy_(pristine)
        for t, z in zip(carries, zero):
            t.copy_(z)
        rin, rres = msgs.messages_in.tables()
        assert L.xyws_decode_streams(h, p(dec.conns_t), n, p(g.counts_t), 0, st) == 0
        assert L.xyws_reassemble_streams(h, p(dec.conns_t), p(g.counts_t), p(rin), n, 1, p(rres), st) == 0
        assert L.xyws_hold_streams(h, p(rin), p(rres), p(hold_t["hold"]), n, p(hold_t["view"]), p(hold_t["view_results"]),
                                   p(hold_t["results"]), st) == 0
        assert L.xyws_inflate_streams(h, p(dec.conns_t), p(hold_t["view"]), p(hold_t["view_results"]), p(hold_t["results"]),
                                      p(inf_t["iconns"]), n, 1, p(inf_t["view"]), p(inf_t["view_results"]),
                                      p(inf_t["results"]), st) == 0
        assert L.xyws_broadcast_streams(h, p(inf_t["view"]), p(inf_t["view_results"]), p(bc.bconns_t), n, p(bc.rooms_t),
                                        p(bc.room_results_t), 4, 0x12, 0, p(bc.results_t), st) == 0
    for _ in range(3):
        for t in sends + [inf_t["out"]]:
            t.fill_(0x5A)
        graph.replay()
        torch.cuda.synchronize()
        assert [bc.wire(r).cpu().numpy().tobytes() for r in range(4)] == want_wires
        got = [t.cpu().numpy().tobytes() for t in sends]
        for k in range(n):  # what a member is sent: its room's wire
            ln = len(want_wires[k % 4])
            assert got[k][:ln] == eager_sends[k][:ln] == want_wires[k % 4], k
    assert g.ctx.last_device_error() == 0

"""xyws_encode_frames / xyws_classify_frames / xyws_reassemble across every
size at which xyws_frames.hip changes path, bit-exact against the oracle
(oracle/xyws_oracle.c: a sequential restatement with no scans, tiles or
staging) on frame tables built directly (tests/op_tables.py):

  scans    1 block, exactly 1 full block, 2+, and more than FT blocks (a
           second round of scan_parts, its carry needed by the max scan, the
           reversed min scan and the sums)
  gather   tiles of 1 item, 2..GMAP_ITEMS (binary search), the chunk map up to
           GLDS, and the per-byte path (tiny items; runs of zero-size items)
  UTF-8    tiles of fewer and of more than UMS messages, the probe's edge,
           the streaming pass on long valid text, a misaligned output

The CPU tests state which of these each shape reaches (from the constants in
the kernel source: a changed constant fails them, it does not silently move
the coverage) and pin the oracle at these sizes against the builder's own
message list and Python's UTF-8 decoder."""
import codecs
import functools
import os
import re

import numpy as np
import pytest

import op_tables as T
import xynet_amd._lib as L

U64MAX = (1 << 64) - 1
SRC = open(os.path.join(L.PKG, "csrc", "xyws_frames.hip")).read()


def const(name):
    m = re.search(r"^constexpr uint\d+_t %s = (\d+);" % name, SRC, re.M)
    assert m, f"xyws_frames.hip no longer states {name} as a plain number"
    return int(m.group(1))


FT = const("FT")
SB = int(re.search(r"constexpr uint32_t SB = (\d+) \* FT;", SRC).group(1)) * FT
GTILE, GLDS, GMAP_ITEMS, UT, UMS, UPROBE = (const(k) for k in ("GTILE", "GLDS", "GMAP_ITEMS", "UT", "UMS", "UPROBE"))

# --------------------------------------------------------------------------- shapes

SCAN_N = (0, 1, 1023, 1024, 1025, 2049)
BIG_N = 263169
PERIOD = "aé€\U0001d11e".encode()   # 1 + 2 + 3 + 4 bytes
assert len(PERIOD) == 10
FAULTS = [b"\xff", b"\xc0\xaf", b"\xed\xa0\x80", b"\xf4\x90\x80\x80"]          # invalid in any context
# (the fault list of test_frames.py::test_reassemble_utf8_probe_window)
PROBE_SEQS = [b"\x80", b"\xc0\xaf", b"\xe0\x80\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xff", b"\xe2\x82",
              "é".encode(), "€".encode(), "\U0001d11e".encode()]
LONG = 200 << 10
FAULT_LEN = 70000


def _big():
    # frames 0..1024 (the reversed min scan's blocks 256 and 257) find their FIN
    # in a later block, and the frames of block 256 and 257 their start in an
    # earlier one: both through scan_parts' carry between rounds
    head, tail = T.message(1100, 1), T.message(1300, 3)
    mid = [T.tiny(100, 4), T.orphans(30, 5)]
    fill = BIG_N - head.n - tail.n - sum(s.n for s in mid)
    return T.build([head] + mid + [T.tiny(fill, 2), tail], seed=21)


def _reasm_blocks():
    segs = [T.sized(300, 1, 0, 40), T.uniform(3, 0, T.OP_TEXT), T.uniform(3, 0),
            T.message(2100, 2, 0, 3, ping_every=7), T.interrupted(2100, 3, 0, 3, ping_every=7),
            T.sized(1, 4, 0, 40), T.orphans(1500, 5), T.sized(50, 6, 0, 40)]
    count = sum(s.n for s in segs)
    segs.append(T.sized((1023 - count) % 1024, 7, 0, 40))   # the next frame sits in a block's last slot
    segs += [T.message(2, sizes=[5, 6]), T.message(3, sizes=[0, 0, 0]), T.text(b"split text", [3, 3, 7])]
    count = sum(s.n for s in segs)
    segs += [T.sized(8950 - count, 8, 0, 40), T.uniform(1, 10), T.orphans(40, 9)]
    return T.build(segs, seed=22)


def _devn():
    segs = [T.mixed(1020, 31), T.message(12, 32, 0, 40, ping_every=7)]
    segs.append(T.mixed(3000 - sum(s.n for s in segs), 33))
    return T.build(segs, seed=23)


def _segments():
    return T.build([T.tiny(9000, 41), T.sized(200, 42, 33, 1800), T.uniform(60, 2337), T.sized(40, 43, 2560, 8192),
                    T.uniform(1, 70000)], seed=24)


def _sparse():
    s = T.sized(6000, 51, 0, 40)
    return T.build(T.with_b0(s, [700, 2200, 3700, 5200], T.FIN | T.OP_PING), seed=25)


def _texts_short():
    segs = []
    n = 4000
    ln = T.draws(61, n, 1, 60)
    r = T.draws(62, 3 * n, 0, 1 << 20).reshape(n, 3)
    for k in range(n):
        body = bytearray(T.ascii_text(int(ln[k]), 7000 + k))
        if r[k, 0] % 3 == 0:
            seq = PROBE_SEQS[r[k, 1] % len(PROBE_SEQS)]
            pos = r[k, 2] % ln[k]
            body = (body[:pos] + seq + body[pos:])[: ln[k]]
        cuts = [int(r[k, 2] % (ln[k] + 1))] if r[k, 1] % 5 == 0 else []
        segs.append(T.text(bytes(body), cuts))
    return T.build(segs, seed=26)


def long_text():
    return PERIOD * (LONG // 10)


def _text_long():
    body = long_text()
    c3 = [int(x) for x in np.sort(T.draws(71, 2, 1, LONG - 1))]
    c40 = [int(x) for x in np.sort(T.draws(72, 39, 1, LONG - 1))]
    return T.build([T.uniform(1, 7), T.text(body), T.text(body, c3), T.text(body, c40)], seed=27)


def first_boundary(k, out_shift):
    """Message offset of the first UTF-8 tile boundary inside text k of the
    forty (text k starts at out[] byte k * FAULT_LEN)."""
    return UT - (k * FAULT_LEN + out_shift) % UT


def fault_plan(out_shift):
    """[(position in the message, fault bytes or None, kind)] of the forty
    70 000-byte texts, message k starting at out[] byte k * FAULT_LEN: the
    first UTF-8 tile boundary inside message k lies at message offset
    bnd(k)."""
    plan = []
    k = 0
    for d in (-3, -2, -1, 0, 1, 2):
        for f in FAULTS:
            plan.append((first_boundary(k, out_shift) + d, f, "boundary"))
            k += 1
    for pos in (15, 16, 17):
        for f in FAULTS[:2]:
            plan.append((pos, f, "probe"))
            k += 1
    for _ in range(7):
        plan.append((0, None, "clean"))
    plan += [(FAULT_LEN - 2, b"\xe2\x82", "cut_complete"), (FAULT_LEN - 2, b"\xe2\x82", "cut_incomplete"),
             (FAULT_LEN - 3, "€".encode(), "cut_by_cap")]
    assert len(plan) == 40
    return plan


def _text_faults(out_shift):
    base = PERIOD * (FAULT_LEN // 10 - 1) + b"0123456789"
    segs = []
    for pos, f, kind in fault_plan(out_shift):
        b = bytearray(base)
        if f:
            b[pos:pos + len(f)] = f
        segs.append(T.text(bytes(b), [FAULT_LEN // 2], fin=kind != "cut_incomplete"))
    return T.build(segs, seed=28)


SHAPES = {
    **{f"mixed_{n}": (lambda n=n: T.build(T.mixed(n, 100 + n), seed=n)) for n in SCAN_N},
    "big": _big,
    "closers": lambda: T.tiny(BIG_N, 81),      # (a run: test_first_close turns frames of it into closes)
    "reasm_blocks": _reasm_blocks,
    "devn": _devn,
    "u30": lambda: T.build(T.uniform(3000, 30), seed=30),
    "u31": lambda: T.build(T.uniform(3000, 31), seed=31),
    "segments": _segments,
    "tiny_9000": lambda: T.build(T.tiny(9000, 41), seed=29),
    "sparse": _sparse,
    "texts_short": _texts_short,
    "text_long": _text_long,
    "text_faults_0": lambda: _text_faults(0),
    "text_faults_5": lambda: _text_faults(5),
}


@functools.lru_cache(maxsize=None)
def shape(name):
    return SHAPES[name]()


# the cases of the GPU tests below, by what each hands the kernels
SHIFTS = [(0, 0), (5, 3), (11, 14)]
ENC_MODES = {"echo": (0x11, False), "client": (0x22, True)}
GATHER_SHAPES = ("u30", "u31", "segments")
REASM_SHAPES = ("reasm_blocks", "big", "devn", "segments", "u30", "u31", "tiny_9000", "texts_short", "text_long",
                "text_faults_0", "text_faults_5") + tuple(f"mixed_{n}" for n in SCAN_N)
UTF8_CASES = [(s, sh) for s in ("texts_short", "text_long") for sh in (0, 5)] + [("text_faults_0", 0),
                                                                                  ("text_faults_5", 5)]


def keys_for(t):
    return T.rand_bytes(0xC0FFEE + t.n, 4 * t.n)


def member_offsets(t, ne=None):
    """Per-frame output offsets of a reassembly (n + 1): a message's frames
    hold their payload bytes, every other frame none."""
    ne = t.n if ne is None else ne
    sz = np.where(t.mid[:ne] >= 0, t.plen[:ne], 0)
    return np.concatenate([[0], np.cumsum(sz)]).astype(np.int64)


def gather_tiles(off, out_lo, out_cap):
    """(items, zero-size items) of every gather tile, as k_tile_map and
    k_gather count them: f1 - f0, f0 the item holding the tile's first byte,
    f1 one past the item holding the next tile's first byte."""
    off = np.asarray(off, dtype=np.int64)
    ne = off.size - 1
    lim = min(int(off[-1]), out_cap)
    if not lim or not ne:
        return []
    nt = (out_lo + lim + GTILE - 1) // GTILE
    q = np.maximum(np.arange(nt + 1) * GTILE - out_lo, 0)
    hold = np.searchsorted(off[:-1], q, side="right") - 1     # the last item starting at or before q
    size = np.diff(off)
    res = []
    for t in range(nt):
        f0, f1 = int(hold[t]), (int(hold[t + 1]) + 1 if t + 1 < nt else ne)
        res.append((f1 - f0, int((size[f0:f1] == 0).sum())))
    return res


def utf8_tiles(recs, out_lo, out_cap):
    """Messages per UTF-8 tile, as k_rs_msgs maps them and k_utf8 counts them
    (m1 - m0 + 1, m0 / m1 the messages holding this and the next tile's first
    byte), and the tiles each text message covers."""
    r = recs.reshape(-1, 40)
    if not len(r):
        return [], []
    mo = r[:, 16:24].copy().view(np.uint64).reshape(-1).astype(np.int64)
    ln = r[:, 24:32].copy().view(np.uint64).reshape(-1).astype(np.int64)
    total = min(int(mo[-1] + ln[-1]), out_cap)
    if not total:
        return [], []
    nt = (out_lo + total + UT - 1) // UT
    q = np.maximum(np.arange(nt + 1) * UT - out_lo, 0)
    hold = np.searchsorted(mo, q, side="right") - 1
    per = [(int(hold[t + 1]) if t + 1 < nt else len(r) - 1) - int(hold[t]) + 1 for t in range(nt)]
    text = r[:, 36] == 1
    span = ((np.minimum(mo + ln, total) - 1 + out_lo) // UT - (mo + out_lo) // UT + 1)[text & (ln > 0) & (mo < total)]
    return per, span.tolist()


# --------------------------------------------------------------------------- CPU

def test_shapes_reach_what_they_name(oracle):
    assert SB == 4 * FT and (FT, GTILE, GLDS, GMAP_ITEMS, UT, UMS, UPROBE) == (256, 16384, 512, 8, 65536, 512, 16), \
        "a threshold of xyws_frames.hip moved: re-derive the shapes of this file for it"
    # ---- scans
    blocks = {n: -(-n // SB) for n in SCAN_N + (BIG_N, shape("reasm_blocks").n, 3000)}
    assert 0 in blocks.values()
    assert any(nb == 1 and n < SB for n, nb in blocks.items())
    assert blocks[SB] == 1 and SB in SCAN_N
    assert blocks[SB + 1] == 2 and any(nb > 2 for nb in blocks.values())
    assert blocks[BIG_N] > FT and -(-blocks[BIG_N] // FT) == 2
    big = shape("big")
    op = big.b0 & 0x0F
    # the carry between rounds is needed: the frames of the reversed scan's
    # second round have no FIN among them, those of the forward scan's no start
    r2 = BIG_N - FT * SB
    assert not np.any((big.b0[:r2] & T.FIN) & (op[:r2] <= 2)) and big.mid[r2 - 1] == 0
    assert not np.any((op[FT * SB:] == 1) | (op[FT * SB:] == 2)) and np.all(big.mid[FT * SB:] == big.mid[-1])
    assert np.any((big.mid[:SB * 2] == -1) & (op[:SB * 2] == 0))   # orphans before the later blocks
    # ---- reassembly across blocks
    rb = shape("reasm_blocks")
    assert 8900 <= rb.n <= 9100
    rop = rb.b0 & 0x0F
    start, fin = (rop == 1) | (rop == 2), (rop <= 2) & ((rb.b0 & T.FIN) != 0)
    quiet = [b for b in range(rb.n // SB) if not start[b * SB:(b + 1) * SB].any() and not fin[b * SB:(b + 1) * SB].any()]
    lens = np.bincount(rb.mid[rb.mid >= 0])
    inside = [int(rb.mid[b * SB:(b + 1) * SB].max()) for b in quiet]   # (the block's other frames are pings)
    assert any(m >= 0 and rb.mfin[m] for m in inside), "no block without start or FIN inside a whole message"
    assert any(m >= 0 and not rb.mfin[m] for m in inside), "no such block inside an interrupted message"
    assert sorted(lens)[-2:] == [2100, 2100]
    edge = [i for i in range(SB - 1, rb.n - 1, SB) if start[i] and not fin[i] and fin[i + 1] and rop[i + 1] == 0]
    assert edge, "no start in a block's last slot with its FIN in the next block's first"
    out, recs, nm = oracle.reassemble_raw(rb.src, rb.table, 1)
    r = recs.reshape(-1, 40)
    st = r[:, 32]
    assert np.any((st & 0x10) != 0) and np.any((st & 0x04) != 0) and np.any(r[:, 24:32].view(np.uint64) == 0)
    orph_before = np.flatnonzero((st & 0x10) != 0)[0]
    first = int(r[orph_before, 0:8].copy().view(np.uint64)[0])
    assert np.all(rb.mid[first - 1500:first] == -1) and np.all(rop[first - 1500:first] == 0)
    assert rb.mid[-1] == -1 and rop[-1] == 0                               # trailing orphans: 0x200
    assert member_offsets(rb)[-1] > 2 * GTILE
    # ---- dev_n: 1024 and 1025 cut inside a message
    dv = shape("devn")
    assert dv.n == 3000 and dv.mid[1023] == dv.mid[1024] == dv.mid[1025] >= 0
    # ---- gather tiles
    tiles = []
    for name in GATHER_SHAPES:
        t = shape(name)
        for mode, (flags, with_keys) in ENC_MODES.items():
            _, offs, total = oracle.encode_frames_raw(t.src, t.table, flags, 0, keys_for(t) if with_keys else None)
            for _, osh in SHIFTS:
                tiles += [(name, mode, osh) + x for x in gather_tiles(offs, osh, total)]
        offs = member_offsets(t)
        _, recs, nm = oracle.reassemble_raw(t.src, t.table, 0)
        r = recs.reshape(-1, 40)
        assert np.array_equal(offs[r[:, 0:8].copy().view(np.uint64).reshape(-1).astype(np.int64)],
                              r[:, 16:24].copy().view(np.uint64).reshape(-1).astype(np.int64))
        for _, osh in SHIFTS:
            tiles += [(name, "reasm", osh) + x for x in gather_tiles(offs, osh, int(offs[-1]))]
    # (uniform replies of 32 and 33 bytes: payload 30 and 31 under flags 0x11)
    assert {x[3] for x in tiles if x[:3] == ("u30", "echo", 0)} >= {GLDS + 1}
    assert all(GLDS - 20 <= x[3] <= GLDS for x in tiles if x[:3] == ("u31", "echo", 0) and x[3] > 100)
    sp = shape("sparse")
    verd, _ = oracle.classify_raw(sp.src, sp.table, 1 << 40, L.POL_FRAGMENTS)
    _, offs, total = oracle.encode_frames_raw(sp.src, sp.table, 0, L.ENC_FRAME_OPCODE, None, verd, 1 << L.ACT_PING)
    assert total > 0
    tiles += [("sparse", "pings", 0) + x for x in gather_tiles(offs, 0, total)]
    tiles += [("reasm_blocks", "reasm", 0) + x for x in gather_tiles(member_offsets(rb), 0, 1 << 40)]
    items = [x[3] for x in tiles]
    reached = {
        "1 item": any(i == 1 for i in items),
        "2..GMAP_ITEMS": any(2 <= i < GMAP_ITEMS for i in items),
        "exactly GMAP_ITEMS": GMAP_ITEMS in items,
        "GMAP_ITEMS + 1": GMAP_ITEMS + 1 in items,
        "chunk map": any(GMAP_ITEMS + 1 < i < GLDS - 20 for i in items),
        "just under GLDS": any(GLDS - 20 <= i <= GLDS for i in items),
        "over GLDS": any(i > GLDS for i in items),
        "over GLDS, zero-size": any(i > GLDS and z > 500 for _, _, _, i, z in tiles),
        "over GLDS, zero-size, encode": any(i > GLDS and z > 500 for s, _, _, i, z in tiles if s == "sparse"),
        "over GLDS, zero-size, reassembly": any(i > GLDS and z > 500 for s, _, _, i, z in tiles if s == "reasm_blocks"),
    }
    # neighbouring tiles of the segment stream take different routes
    seg = [x[3] for x in tiles if x[:3] == ("segments", "echo", 0)]
    route = [0 if i == 1 else 1 if i <= GMAP_ITEMS else 2 if i <= GLDS else 3 for i in seg]
    reached["all four routes in one call"] = set(route) == {0, 1, 2, 3}
    # ---- UTF-8 tiles
    per, spans = [], []
    for name, osh in UTF8_CASES:
        t = shape(name)
        _, recs, nm = oracle.reassemble_raw(t.src, t.table, 1)
        p, s = utf8_tiles(recs, osh, 1 << 40)
        per += p
        spans += s
        if name == "text_long":   # a sequence straddles the first tile boundary inside each message
            r = recs.reshape(-1, 40)
            mo = r[:, 16:24].copy().view(np.uint64).reshape(-1).astype(np.int64)
            for m in range(1, 4):
                bnds = range(UT - (int(mo[m]) + osh) % UT, LONG, UT)
                assert len(bnds) >= 3 and any(b % 10 not in (0, 1, 3, 6) for b in bnds), (name, osh, m)
    reached["fewer than UMS messages"] = any(p < UMS for p in per)
    reached["more than UMS messages"] = any(p > UMS for p in per)
    reached["a text over 3 tiles"] = any(s >= 3 for s in spans)
    print(reached)
    assert all(reached.values()), reached
    # ---- the forty faulty texts: the oracle flags exactly the ones with a fault
    for osh in (0, 5):
        t = shape(f"text_faults_{osh}")
        total = int(member_offsets(t)[-1])
        _, recs, nm = oracle.reassemble_raw(t.src, t.table, 1, out_cap=total - 1)
        st = recs.reshape(-1, 40)[:, 32]
        plan = fault_plan(osh)
        assert nm == 40
        for k, (pos, f, kind) in enumerate(plan):
            assert 0 <= pos and pos + len(f or b"") <= FAULT_LEN
            assert bool(st[k] & 2) == (kind in ("boundary", "probe", "cut_complete")), (osh, k, kind, int(st[k]))
            if kind == "boundary":
                assert -3 <= pos - first_boundary(k, osh) <= 2 and 3 <= first_boundary(k, osh) < FAULT_LEN - 8
        assert st[39] & 8 and st[38] & 4 and not st[38] & 1


def _python_says_bad(data, final):
    try:
        codecs.getincrementaldecoder("utf-8")().decode(data, final=final)
        return False
    except UnicodeDecodeError:
        return True


def test_oracle_at_scale_against_python(oracle):
    for name in REASM_SHAPES:
        t = shape(name)
        total = int(member_offsets(t)[-1])
        out, recs, nm = oracle.reassemble_raw(t.src, t.table, 1, out_cap=total)
        r = recs.reshape(-1, 40)
        assert nm == len(r) == t.mop.size, name
        mo = r[:, 16:24].copy().view(np.uint64).reshape(-1).astype(np.int64)
        ln = r[:, 24:32].copy().view(np.uint64).reshape(-1).astype(np.int64)
        gathered, goff = t.gathered()
        assert np.array_equal(out, gathered) and np.array_equal(mo, goff[:-1]) and np.array_equal(ln, np.diff(goff))
        assert np.array_equal((r[:, 32] & 1) != 0, t.mfin) and np.array_equal(r[:, 36], t.mop), name
        if nm <= 10000:
            complete = [(int(x[36]), out[a:a + b].tobytes()) for x, a, b in zip(r, mo, ln) if x[32] & 1]
            assert complete == t.messages(), name
        caps = [total] + ([total - 1] if name.startswith("text") else [])
        for cap in caps:
            out, recs, nm = oracle.reassemble_raw(t.src, t.table, 1, out_cap=cap)
            r = recs.reshape(-1, 40)
            for m in np.flatnonzero(r[:, 36] == 1):
                final = bool(r[m, 32] & 1) and not r[m, 32] & 8
                assert bool(r[m, 32] & 8) == (mo[m] + ln[m] > cap)
                data = out[mo[m]:min(mo[m] + ln[m], cap)].tobytes()
                assert bool(r[m, 32] & 2) == _python_says_bad(data, final), (name, cap, int(m))
    # the long valid text is valid, and the table is what a decode leaves
    assert not _python_says_bad(long_text(), True)
    for name in ("reasm_blocks", "mixed_2049", "segments"):
        t = shape(name)
        wire = t.wire()
        raw, _, n = oracle.decode_stream_raw(wire, t.n + 4)
        assert n == t.n and np.array_equal(raw, t.table) and np.array_equal(wire, t.src), name


# --------------------------------------------------------------------------- GPU

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ws():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from xynet_amd import websocket
    return websocket


def _placed(arr, shift):
    """arr on the device at `shift` bytes past a 16-byte aligned address."""
    base = torch.zeros(arr.size + 32, dtype=torch.uint8, device="cuda")
    v = base[shift:shift + arr.size]
    if arr.size:
        v.copy_(torch.from_numpy(np.ascontiguousarray(arr)))
    return v


class Guarded:
    """size bytes of 0xA5 at `shift` past a 16-byte aligned address, 0xA5
    before and after."""

    def __init__(self, size, shift=0):
        self.base = torch.full((size + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        self.lo, self.size = 16 + shift, size
        self.view = self.base[self.lo:self.lo + size]

    def check(self, written):
        """The first `written` bytes (returned); every other byte still 0xA5."""
        h = self.base.cpu().numpy()
        assert np.all(h[:self.lo] == 0xA5), "bytes before the buffer were written"
        assert np.all(h[self.lo + written:] == 0xA5), f"bytes past the first {written} were written"
        return h[self.lo:self.lo + written]


@functools.lru_cache(maxsize=8)
def _dev_table(name, src_shift):
    t = shape(name)
    return _placed(t.src, src_shift), _placed(t.table, 0)


def _dev_n(v):
    return None if v is None else torch.tensor([v], dtype=torch.int64, device="cuda")


def _err(ws, want):
    got = ws.context().last_device_error()
    assert got == want, f"device error word {got:#x}, expected {want:#x}"


def _orphan_err(t, ne):
    """0x200 when continuations follow the last message's FIN (or there is no
    message at all) in frames [0, ne)."""
    op, b0 = t.b0[:ne] & 0x0F, t.b0[:ne]
    starts = np.flatnonzero((op == 1) | (op == 2))
    cont = np.flatnonzero(op == 0)
    if not cont.size:
        return 0
    if not starts.size:
        return 0x200
    fins = np.flatnonzero((op <= 2) & ((b0 & T.FIN) != 0))
    fins = fins[fins >= starts[-1]]
    return 0x200 if fins.size and cont[-1] > fins[0] else 0


def run_encode(ws, oracle, t, dev, flags, enc_opts=0, with_keys=False, verd=None, amask=0, out_cap=None,
               out_shift=0, src_len=None, dev_n=None, err=0):
    src_d, tab_d = dev
    n = t.n
    ne = n if dev_n is None else min(n, dev_n)
    slen = t.src.size if src_len is None else src_len
    keys = keys_for(t) if with_keys else None
    want, offs, total = oracle.encode_frames_raw(t.src[:slen], t.table[:ne * 32], flags, enc_opts,
                                                 None if keys is None else keys[:4 * ne],
                                                 None if verd is None else verd[:8 * ne], amask, out_cap)
    cap = total if out_cap is None else out_cap
    out = Guarded(cap, out_shift)
    og = Guarded(8 * (n + 1))
    keys_d = None if keys is None else _placed(keys, 0)
    verd_d = None if verd is None else _placed(verd, 0)
    ws.context().last_device_error()
    _, olen = ws.encode_frames(src_d[:slen], tab_d, n, flags, dev_n=_dev_n(dev_n), enc_opts=enc_opts, keys=keys_d,
                               verdicts=verd_d, action_mask=amask, out=out.view, offsets=og.view.view(torch.int64))
    torch.cuda.synchronize()
    assert int(olen.item()) == total
    got = out.check(min(cap, total))
    assert np.array_equal(got, want), f"first difference at byte {np.flatnonzero(got != want)[:1]}"
    goffs = og.check(8 * (n + 1)).view(np.uint64)
    assert np.array_equal(goffs[:ne + 1], offs)
    _err(ws, err)
    return total, offs


def run_classify(ws, oracle, t, dev, max_payload, policy, dev_n=None):
    src_d, tab_d = dev
    n = t.n
    ne = n if dev_n is None else min(n, dev_n)
    want, first = oracle.classify_raw(t.src, t.table[:ne * 32], max_payload, policy)
    vg = Guarded(8 * n)
    ws.context().last_device_error()
    _, f = ws.classify_frames(src_d, tab_d, n, max_payload, policy, dev_n=_dev_n(dev_n), verdicts=vg.view)
    torch.cuda.synchronize()
    assert int(f.item()) & U64MAX == first
    assert np.array_equal(vg.check(8 * ne), want)
    _err(ws, 0)
    return want, first


def run_reassemble(ws, oracle, t, dev, opts=L.REASM_UTF8, out_cap=None, msg_cap=None, dev_n=None, out_shift=0,
                   src_len=None, err=None):
    src_d, tab_d = dev
    n = t.n
    ne = n if dev_n is None else min(n, dev_n)
    slen = t.src.size if src_len is None else src_len
    total = int(member_offsets(t, ne)[-1])
    cap = total if out_cap is None else out_cap
    mcap = n if msg_cap is None else msg_cap
    want, recs, nm = oracle.reassemble_raw(t.src[:slen], t.table[:ne * 32], opts, cap, mcap)
    out = Guarded(cap, out_shift)
    mg = Guarded(40 * mcap)
    ws.context().last_device_error()
    _, _, cnt = ws.reassemble(src_d[:slen], tab_d, n, opts, dev_n=_dev_n(dev_n), out=out.view, out_cap=cap,
                              msgs=mg.view, msg_cap=mcap)
    torch.cuda.synchronize()
    assert int(cnt.item()) == nm
    got = mg.check(40 * min(nm, mcap))
    if not np.array_equal(got, recs):
        bad = np.flatnonzero(np.any(got.reshape(-1, 40) != recs.reshape(-1, 40), axis=1))
        m = int(bad[0])
        raise AssertionError(f"{bad.size} records differ, the first is {m}: got {got.reshape(-1, 40)[m].tolist()}, "
                             f"oracle {recs.reshape(-1, 40)[m].tolist()}")
    gout = out.check(min(cap, total))
    assert np.array_equal(gout, want[:min(cap, total)]), f"first difference at byte {np.flatnonzero(gout != want[:gout.size])[:1]}"
    _err(ws, _orphan_err(t, ne) if err is None else err)
    return nm, total


# ---- scan sizes

@pytest.mark.gpu
@pytest.mark.parametrize("n", SCAN_N + (BIG_N,))
def test_scan_sizes_encode(ws, oracle, n):
    name = "big" if n == BIG_N else f"mixed_{n}"
    t, dev = shape(name), _dev_table(name, 0)
    total, offs = run_encode(ws, oracle, t, dev, 0x20, L.ENC_FRAME_OPCODE, with_keys=True)
    if n == 0:
        assert total == 0 and offs.tolist() == [0]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SCAN_N + (BIG_N,))
def test_scan_sizes_classify(ws, oracle, n):
    name = "big" if n == BIG_N else f"mixed_{n}"
    t, dev = shape(name), _dev_table(name, 0)
    for policy, maxp in ((L.POL_FRAGMENTS, 1 << 40), (0, 20)):
        _, first = run_classify(ws, oracle, t, dev, maxp, policy)
        if n == 0:
            assert first == U64MAX


@pytest.mark.gpu
@pytest.mark.parametrize("n", SCAN_N + (BIG_N,))
def test_scan_sizes_reassemble(ws, oracle, n):
    name = "big" if n == BIG_N else f"mixed_{n}"
    t, dev = shape(name), _dev_table(name, 0)
    nm, total = run_reassemble(ws, oracle, t, dev)
    if n == 0:
        assert nm == 0 and total == 0


# ---- reassembly across blocks

@pytest.mark.gpu
@pytest.mark.parametrize("msg_cap", ["all", "one", "nm-1"])
@pytest.mark.parametrize("out_cap", ["total", "total-1", "gtile", "one"])
def test_reassemble_across_blocks(ws, oracle, msg_cap, out_cap):
    t, dev = shape("reasm_blocks"), _dev_table("reasm_blocks", 0)
    nm, total = t.mop.size, int(member_offsets(t)[-1])
    run_reassemble(ws, oracle, t, dev, out_cap={"total": total, "total-1": total - 1, "gtile": GTILE, "one": 1}[out_cap],
                   msg_cap={"all": None, "one": 1, "nm-1": nm - 1}[msg_cap], err=0x200)


# ---- dev_n

DEV_N = (0, 1, 1024, 1025, 2999, 3000, 3005)


@pytest.mark.gpu
@pytest.mark.parametrize("dev_n", DEV_N)
def test_dev_n(ws, oracle, dev_n):
    t, dev = shape("devn"), _dev_table("devn", 0)
    run_classify(ws, oracle, t, dev, 1 << 40, L.POL_FRAGMENTS, dev_n=dev_n)
    run_encode(ws, oracle, t, dev, 0x11, dev_n=dev_n)
    run_reassemble(ws, oracle, t, dev, dev_n=dev_n)
    if dev_n == 1025:   # (cuts inside a message: its record is there, incomplete)
        _, recs, nm = oracle.reassemble_raw(t.src, t.table[:dev_n * 32], 1)
        assert not recs.reshape(-1, 40)[nm - 1, 32] & 1


# ---- first close

CLOSERS = {"none": [], "last": [BIG_N - 1], "at_1024": [1024], "four_blocks": [70000, 70000 + SB, 150000, 263000]}


@pytest.mark.gpu
@pytest.mark.parametrize("policy", [0, L.POL_STRICT, 0x8])
@pytest.mark.parametrize("case", list(CLOSERS) + ["dev_n_below"])
def test_first_close(ws, oracle, case, policy):
    """atomicMin across blocks. (Policy 0x8, XYWS_POL_REFERENCE, also closes on
    the ping at 5 000 of four_blocks.)"""
    at = CLOSERS["four_blocks" if case == "dev_n_below" else case]
    seg = T.with_b0(shape("closers"), at, T.FIN | T.OP_CLOSE) if at else shape("closers")
    if case == "four_blocks":
        seg = T.with_b0(seg, [5000], T.FIN | T.OP_PING)
    t = T.build(seg, seed=82)
    dev = (_placed(t.src, 0), _placed(t.table, 0))
    dev_n = 69000 if case == "dev_n_below" else None
    _, first = run_classify(ws, oracle, t, dev, 1 << 40, policy, dev_n=dev_n)
    want = {"none": U64MAX, "last": BIG_N - 1, "at_1024": 1024, "four_blocks": 5000 if policy == 0x8 else 70000,
            "dev_n_below": U64MAX}[case]
    assert first == want


# ---- gather classes

@pytest.mark.gpu
@pytest.mark.parametrize("shifts", SHIFTS)
@pytest.mark.parametrize("name", GATHER_SHAPES)
@pytest.mark.parametrize("op", list(ENC_MODES) + ["reasm"])
def test_gather_classes(ws, oracle, op, name, shifts):
    t, dev = shape(name), _dev_table(name, shifts[0])
    if op == "reasm":
        run_reassemble(ws, oracle, t, dev, opts=0, out_shift=shifts[1])
    else:
        flags, with_keys = ENC_MODES[op]
        run_encode(ws, oracle, t, dev, flags, with_keys=with_keys, out_shift=shifts[1])


@pytest.mark.gpu
@pytest.mark.parametrize("cap", ["total", "total-1", "2gtile", "zero", "in_header"])
@pytest.mark.parametrize("op", list(ENC_MODES) + ["reasm"])
def test_gather_output_clipped(ws, oracle, op, cap):
    t, dev = shape("segments"), _dev_table("segments", 0)
    if op == "reasm":
        total = int(member_offsets(t)[-1])
        caps = {"total": total, "total-1": total - 1, "2gtile": 2 * GTILE, "zero": 0,
                "in_header": int(member_offsets(t)[101]) + 1}
        run_reassemble(ws, oracle, t, dev, opts=0, out_cap=caps[cap], out_shift=3)
    else:
        flags, with_keys = ENC_MODES[op]
        _, offs, total = oracle.encode_frames_raw(t.src, t.table, flags, 0, keys_for(t) if with_keys else None, out_cap=0)
        caps = {"total": total, "total-1": total - 1, "2gtile": 2 * GTILE, "zero": 0, "in_header": int(offs[100]) + 1}
        run_encode(ws, oracle, t, dev, flags, with_keys=with_keys, out_cap=caps[cap], out_shift=3)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["segments", "tiny_9000"])
@pytest.mark.parametrize("op", list(ENC_MODES) + ["reasm"])
def test_gather_source_clipped(ws, oracle, op, name):
    """The source ends 40 000 bytes early: those bytes read as zero, 0x100."""
    t, dev = shape(name), _dev_table(name, 5)
    slen = t.src.size - 40000
    assert slen > 0
    if op == "reasm":
        run_reassemble(ws, oracle, t, dev, opts=0, src_len=slen, out_shift=3, err=0x100)
    else:
        flags, with_keys = ENC_MODES[op]
        run_encode(ws, oracle, t, dev, flags, with_keys=with_keys, src_len=slen, out_shift=3, err=0x100)


@pytest.mark.gpu
@pytest.mark.parametrize("mask", ["pings", "nothing"])
def test_gather_sparse_selection(ws, oracle, mask):
    """classify -> encode of the pings only: thousands of zero-size items
    between the replies."""
    t, dev = shape("sparse"), _dev_table("sparse", 0)
    verd, first = run_classify(ws, oracle, t, dev, 1 << 40, L.POL_FRAGMENTS)
    assert first == U64MAX
    amask = {"pings": 1 << L.ACT_PING, "nothing": 1 << L.ACT_CLOSE}[mask]
    total, _ = run_encode(ws, oracle, t, dev, 0x00, L.ENC_FRAME_OPCODE, verd=verd, amask=amask)
    assert (total == 0) == (mask == "nothing")


# ---- UTF-8

@pytest.mark.gpu
@pytest.mark.parametrize("name,out_shift", UTF8_CASES)
def test_utf8_at_scale(ws, oracle, name, out_shift):
    t, dev = shape(name), _dev_table(name, 0)
    total = int(member_offsets(t)[-1])
    cap = total - 1 if name.startswith("text_faults") else total
    run_reassemble(ws, oracle, t, dev, out_cap=cap, out_shift=out_shift)
    if name == "text_long":   # (it must come out valid, whatever the oracle says)
        _, recs, nm = oracle.reassemble_raw(t.src, t.table, 1)
        assert nm == 4 and not np.any(recs.reshape(-1, 40)[:, 32] & 2)


# ---- reused scratch

@pytest.mark.gpu
@pytest.mark.parametrize("op", ["encode", "reassemble"])
def test_small_call_after_large_on_the_same_scratch(ws, oracle, op):
    """The tile maps live in the slot's reused scratch: a call must not read
    what a larger one left there."""
    for name in ("big", "mixed_1025", "segments", "mixed_1"):
        t, dev = shape(name), _dev_table(name, 0)
        if op == "encode":
            run_encode(ws, oracle, t, dev, 0x11)
        else:
            run_reassemble(ws, oracle, t, dev)


# ---- bridge

@pytest.mark.gpu
def test_built_table_is_what_the_decoder_leaves(ws):
    t = shape("reasm_blocks")
    buf = _placed(t.wire(), 0)
    r = ws.frame_decoder().decode(buf, cap=t.n + 4)
    assert r.nframes == t.n
    assert np.array_equal(r.frames_t[: t.n * 32].cpu().numpy(), t.table)
    assert np.array_equal(buf.cpu().numpy(), t.src)

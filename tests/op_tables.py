"""Frame tables for the tests of the callers either side of the decode path
(xyws_encode_frames / xyws_classify_frames / xyws_reassemble) at sizes a
wire stream built frame by frame in Python cannot reach: the table a decode
would leave (xyws_frame records: payload_off ascending, no overlap, a header
before every payload, hdr_len and status as the flags imply), the decoded
source buffer it points into, and what the builder itself knows about the
messages in it. Built with numpy from segments (each a function of counts and
sizes); every random draw is splitmix64 of a counter, vectorised in uint64, so
the layout never depends on a library's RNG.

    t = build([tiny(300, seed=1), message(5, seed=2, lo=0, hi=3, ping_every=2), close(1001)], seed=9)
    t.table   uint8[n * 32]   the xyws_frame records
    t.src     uint8[...]      header bytes as on the wire, payloads unmasked
    t.wire()  uint8[...]      the same bytes with every payload masked by its key
"""
import numpy as np

GAMMA = np.uint64(0x9E3779B97F4A7C15)
M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)

OP_CONT, OP_TEXT, OP_BIN, OP_CLOSE, OP_PING, OP_PONG = 0x0, 0x1, 0x2, 0x8, 0x9, 0xA
FIN = 0x80  # (wire byte 0; the table's flags carry it as 0x10)


def mix(seed, idx):
    """splitmix64's output number idx (from 0) for `seed`, idx a uint64 array."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & ((1 << 64) - 1)) + (np.asarray(idx, dtype=np.uint64) + np.uint64(1)) * GAMMA
        z = (z ^ (z >> np.uint64(30))) * M1
        z = (z ^ (z >> np.uint64(27))) * M2
        return z ^ (z >> np.uint64(31))


def draws(seed, n, lo, hi):
    """n integers in [lo, hi] (int64)."""
    if n == 0:
        return np.zeros(0, np.int64)
    return (mix(seed, np.arange(n, dtype=np.uint64)) % np.uint64(hi - lo + 1)).astype(np.int64) + lo


def rand_bytes(seed, n):
    if n == 0:
        return np.zeros(0, np.uint8)
    return mix(seed, np.arange((n + 7) // 8, dtype=np.uint64)).view(np.uint8)[:n].copy()


class Seg:
    """A run of frames: wire byte 0 and payload length of each, the message
    (numbered within the run) each data frame belongs to (-1: control frames
    and orphan continuations), each message's opcode and whether its FIN frame
    is in the run, and payloads given as bytes ({frame: bytes}; the others
    are random)."""

    def __init__(self, b0, plen, mid=None, mop=(), mfin=(), fixed=None):
        self.b0 = np.asarray(b0, dtype=np.uint8).reshape(-1)
        self.plen = np.asarray(plen, dtype=np.int64).reshape(-1)
        self.mid = np.full(self.b0.size, -1, np.int64) if mid is None else np.asarray(mid, dtype=np.int64)
        self.mop = np.asarray(mop, dtype=np.uint8).reshape(-1)
        self.mfin = np.asarray(mfin, dtype=bool).reshape(-1)
        self.fixed = dict(fixed or {})
        assert self.b0.size == self.plen.size == self.mid.size and self.mop.size == self.mfin.size

    @property
    def n(self):
        return self.b0.size


# ------------------------------------------------------------------ building blocks

def singles(plen, op=OP_BIN):
    """One whole single-frame message per entry of plen."""
    plen = np.asarray(plen, dtype=np.int64).reshape(-1)
    n = plen.size
    ops = np.broadcast_to(np.asarray(op, dtype=np.uint8), (n,))
    return Seg(ops | np.uint8(FIN), plen, np.arange(n), ops, np.ones(n, bool))


def uniform(n, plen, op=OP_BIN):
    """n whole single-frame messages of plen bytes."""
    return singles(np.full(n, plen, np.int64), op)


def sized(n, seed, lo, hi, op=OP_BIN):
    """n whole single-frame messages of lo..hi bytes."""
    return singles(draws(seed, n, lo, hi), op)


def tiny(n, seed, op=OP_BIN):
    """n whole single-frame messages of 0..5 bytes."""
    return sized(n, seed, 0, 5, op)


def message(k, seed=0, lo=0, hi=3, op=OP_BIN, ping_every=0, fin=True, sizes=None):
    """One message of k fragments of lo..hi bytes (or `sizes`), a ping after
    every ping_every-th fragment but the last; fin=False leaves the FIN
    fragment out (k fragments, none with FIN: the next start interrupts it)."""
    sz = draws(seed, k, lo, hi) if sizes is None else np.asarray(sizes, dtype=np.int64)
    assert sz.size == k and k >= 1
    b0 = np.zeros(k, np.uint8)
    b0[0] = op
    if fin:
        b0[k - 1] |= FIN
    if ping_every:
        after = np.arange(ping_every - 1, k - 1, ping_every)   # a ping after these fragments
        slots = np.arange(k) + np.searchsorted(after, np.arange(k), side="left")
        nf = k + after.size
        fb0 = np.full(nf, FIN | OP_PING, np.uint8)
        fpl = draws(seed ^ 0x5555, nf, 0, 7)
        fmid = np.full(nf, -1, np.int64)
        fb0[slots], fpl[slots], fmid[slots] = b0, sz, 0
        return Seg(fb0, fpl, fmid, [op], [fin])
    return Seg(b0, sz, np.zeros(k, np.int64), [op], [fin])


def interrupted(k, seed=0, lo=0, hi=3, op=OP_BIN, ping_every=0):
    """A message whose FIN fragment never comes (follow it with a start)."""
    return message(k, seed, lo, hi, op, ping_every, fin=False)


def orphans(n, seed, lo=0, hi=3):
    """n continuation frames outside any message (place them after a FIN);
    about one in four carries FIN."""
    b0 = np.where(draws(seed ^ 0x0F0F, n, 0, 3) == 0, FIN, 0).astype(np.uint8)
    return Seg(b0, draws(seed, n, lo, hi))


def text(data, cuts=(), fin=True):
    """One text message: `data` cut into fragments at `cuts` (ascending byte
    positions; equal cuts give empty fragments)."""
    data = bytes(data)
    edges = [0] + [int(c) for c in cuts] + [len(data)]
    assert all(a <= b for a, b in zip(edges, edges[1:]))
    parts = [data[a:b] for a, b in zip(edges, edges[1:])]
    k = len(parts)
    b0 = np.zeros(k, np.uint8)
    b0[0] = OP_TEXT
    if fin:
        b0[k - 1] |= FIN
    return Seg(b0, [len(p) for p in parts], np.zeros(k, np.int64), [OP_TEXT], [fin], dict(enumerate(parts)))


def control(op, payload=b""):
    assert len(payload) <= 125
    return Seg([FIN | op], [len(payload)], fixed={0: bytes(payload)})


def close(code=None, reason=b""):
    return control(OP_CLOSE, b"" if code is None else int(code).to_bytes(2, "big") + bytes(reason))


def ping(payload=b""):
    return control(OP_PING, payload)


def pong(payload=b""):
    return control(OP_PONG, payload)


def ascii_text(n, seed):
    """n ASCII bytes (0x20..0x7E)."""
    return (rand_bytes(seed, n) % np.uint8(95) + np.uint8(0x20)).tobytes()


def mixed(n, seed, hi=40):
    """Exactly n small frames (payload 0..hi): whole text and binary messages,
    fragmented ones with pings between the fragments, pings, pongs, closes
    with a status code and a few orphan continuations."""
    segs, left, k = [], n, 0
    while left > 0:
        r = int(mix(seed, np.uint64(k))) % 100
        s = seed * 1000003 + k
        k += 1
        if r < 30:
            sg = sized(1, s, 0, hi)
        elif r < 50:
            sg = text(ascii_text(int(draws(s, 1, 0, hi)[0]), s + 1))
        elif r < 70:
            sg = message(2 + r % 4, s, 0, hi, op=OP_BIN if r & 1 else OP_TEXT, ping_every=2 if r % 3 == 0 else 0)
        elif r < 80:
            sg = ping(rand_bytes(s, r % 9).tobytes())
        elif r < 86:
            sg = pong(rand_bytes(s, r % 5).tobytes())
        elif r < 90:
            sg = close(1000 + r, b"bye"[: r % 4])
        elif r < 94:
            sg = interrupted(2, s, 0, hi)
        else:
            # (after a whole message, so that the continuations are orphans)
            sg = join([sized(1, s, 0, hi), orphans(1 + r % 3, s, 0, hi)])
        if sg.n > left:
            sg = sized(left, s, 0, hi)
        segs.append(sg)
        left -= sg.n
    return join(segs) if segs else Seg([], [])


def join(segs):
    """Several runs as one."""
    segs = [s for s in segs if s.n]
    if not segs:
        return Seg([], [])
    mids, fixed, f0, m0 = [], {}, 0, 0
    for s in segs:
        mids.append(np.where(s.mid >= 0, s.mid + m0, -1))
        for k, v in s.fixed.items():
            fixed[k + f0] = v
        f0 += s.n
        m0 += s.mop.size
    return Seg(np.concatenate([s.b0 for s in segs]), np.concatenate([s.plen for s in segs]), np.concatenate(mids),
               np.concatenate([s.mop for s in segs]), np.concatenate([s.mfin for s in segs]), fixed)


# ------------------------------------------------------------------ layout

class Table:
    """What build() returns (see the module docstring); frame fields as arrays:
    frame_off, payload_off, plen (int64), hdr_len, flags, b0 (uint8), key
    (uint8[n, 4]); mid / mop / mfin as in Seg."""

    def wire(self):
        """The stream a client would have sent: src with every payload byte j
        XORed with key[j % 4] (what a decode turns back into src)."""
        w = self.src.copy()
        total = int(self.plen.sum())
        if total:
            fr = np.repeat(np.arange(self.n), self.plen)
            j = np.arange(total) - np.repeat(np.cumsum(self.plen) - self.plen, self.plen)
            w[np.repeat(self.payload_off, self.plen) + j] ^= self.key[fr, j & 3]
        return w

    def payload(self, i):
        return self.src[self.payload_off[i]:self.payload_off[i] + self.plen[i]].tobytes()

    def gathered(self):
        """(bytes, offsets): the payloads of every message's frames back to
        back in frame order (the builder's own reassembly: by the message
        numbers the segments gave, no walk over the opcodes), and each
        message's offset in them (nm + 1)."""
        mem = self.mid >= 0
        pl, po = self.plen[mem], self.payload_off[mem]
        total = int(pl.sum())
        idx = np.repeat(po, pl) + (np.arange(total) - np.repeat(np.cumsum(pl) - pl, pl))
        per = np.bincount(self.mid[mem], weights=pl, minlength=self.mop.size).astype(np.int64)
        return self.src[idx], np.concatenate([[0], np.cumsum(per)])

    def messages(self):
        """[(opcode, payload)] of every complete message, in order."""
        out, off = self.gathered()
        return [(int(self.mop[m]), out[off[m]:off[m + 1]].tobytes()) for m in range(self.mop.size) if self.mfin[m]]

    def head(self, n):
        """The table of the first n frames (the same source)."""
        return self.table[: n * 32]


def build(segs, seed, src_pad=0):
    """Lay the runs out as one decoded stream. src_pad: zero bytes after the
    last frame (the source is longer than the stream)."""
    s = segs if isinstance(segs, Seg) else join(segs)
    n = s.n
    t = Table()
    t.n, t.b0, t.plen, t.mid, t.mop, t.mfin = n, s.b0, s.plen, s.mid, s.mop, s.mfin
    ext = np.where(s.plen < 126, 0, np.where(s.plen <= 0xFFFF, 2, 8))
    hdr = (2 + ext + 4).astype(np.int64)
    size = hdr + s.plen
    t.frame_off = np.cumsum(size) - size
    t.payload_off = t.frame_off + hdr
    t.hdr_len = hdr.astype(np.uint8)
    total = int(size.sum())
    t.key = mix(seed ^ 0xA5A5A5A5, np.arange(n, dtype=np.uint64)).astype(np.uint32).view(np.uint8).reshape(n, 4) \
        if n else np.zeros((0, 4), np.uint8)
    src = np.concatenate([rand_bytes(seed, total), np.zeros(src_pad, np.uint8)])
    # headers (masked frames, minimal length form)
    fo = t.frame_off
    if n:
        src[fo] = s.b0
        src[fo + 1] = (0x80 | np.where(ext == 0, s.plen, np.where(ext == 2, 126, 127))).astype(np.uint8)
        m2 = ext == 2
        for k in range(2):
            src[fo[m2] + 2 + k] = (s.plen[m2] >> (8 * (1 - k))) & 0xFF
        m8 = ext == 8
        for k in range(8):
            src[fo[m8] + 2 + k] = (s.plen[m8] >> (8 * (7 - k))) & 0xFF
        for k in range(4):
            src[t.payload_off - 4 + k] = t.key[:, k]
    for i, b in s.fixed.items():
        assert len(b) == s.plen[i]
        src[t.payload_off[i]:t.payload_off[i] + len(b)] = np.frombuffer(b, np.uint8)
    t.src = src
    # the records (include/xyws.h: frame_off, payload_off, payload_len, key[4],
    # flags, hdr_len, status, reserved)
    t.flags = ((s.b0 & 0x0F) | ((s.b0 & FIN) >> 3) | 0x20).astype(np.uint8)
    op = s.b0 & 0x0F
    status = np.where((op >= 8) & (((s.b0 & FIN) == 0) | (s.plen > 125)), 0x20, 0).astype(np.uint8)
    status |= np.where(((op >= 3) & (op <= 7)) | (op >= 11), 0x04, 0).astype(np.uint8)
    rec = np.zeros((n, 32), np.uint8)
    rec[:, 0:8] = t.frame_off.astype("<i8").view(np.uint8).reshape(n, 8)
    rec[:, 8:16] = t.payload_off.astype("<i8").view(np.uint8).reshape(n, 8)
    rec[:, 16:24] = s.plen.astype("<u8").view(np.uint8).reshape(n, 8)
    rec[:, 24:28] = t.key
    rec[:, 28], rec[:, 29], rec[:, 30] = t.flags, t.hdr_len, status
    t.table = rec.reshape(-1)
    return t


def with_b0(seg, at, b0):
    """The run with the frames at indices `at` turned into whole control
    frames of wire byte 0 `b0` (their payload lengths kept; they leave their
    messages, so use it on single-frame messages only)."""
    s = Seg(seg.b0.copy(), seg.plen, seg.mid.copy(), seg.mop, seg.mfin.copy(), seg.fixed)
    at = np.asarray(at, dtype=np.int64)
    assert np.all(s.mfin[s.mid[at]]) and np.all(seg.b0[at] & FIN)
    s.mfin[s.mid[at]] = False
    s.mid[at] = -1
    s.b0[at] = b0
    return s

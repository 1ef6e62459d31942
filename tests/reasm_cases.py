"""Streams, cut lists and the model run shared by tests/test_reasm_model.py
(CPU) and tests/test_gpu_reasm_stream.py (device): a wire stream cut into
batches, each decoded by the CPU checker with its carry chained and fed to
the model (tests/reasm_model.py)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import streams  # noqa: E402

import msg_streams
import reasm_model as M


def batches(wire, cuts):
    """wire cut at the ascending positions `cuts` (parts may be empty)."""
    pts = [0] + list(cuts) + [len(wire)]
    return [wire[a:b] for a, b in zip(pts, pts[1:])]


class Call:
    """One batch: decoded bytes, frame list, raw table, and the model's answer."""

    def __init__(self, wire, host, frames, table, out, recs, carry_in, carry, nm):
        self.wire, self.host, self.frames, self.table = wire, host, frames, table
        self.out, self.recs, self.carry_in, self.carry, self.nm = out, recs, carry_in, carry, nm


def run_model(oracle, parts, opts=M.REASM_UTF8, out_caps=None, msg_caps=None, opts_per=None):
    """Every part decoded (carry chained) and fed to the model (carry chained)."""
    calls, dc, mc = [], None, None
    for k, p in enumerate(parts):
        host = np.frombuffer(p, np.uint8).copy() if p else np.zeros(0, np.uint8)
        cap = len(p) // 2 + 2
        table, dc2, n = oracle.decode_stream_raw(host, cap, carry_in=dc)
        host2 = np.frombuffer(p, np.uint8).copy() if p else np.zeros(0, np.uint8)
        frames, dc, n2 = oracle.decode_stream(host2, carry_in=dc, cap=cap)
        assert n == n2 <= cap
        o = opts if opts_per is None else opts_per[k]
        oc = None if out_caps is None else out_caps[k]
        mcap = None if msg_caps is None else msg_caps[k]
        out, recs, mc2, nm = M.feed(host.tobytes(), frames, o, mc, oc, mcap)
        calls.append(Call(p, host, frames, table.copy(), out, recs, mc, mc2, nm))
        mc = mc2
    return calls


def unsplit(oracle, wire, opts=M.REASM_UTF8):
    """xyws_reassemble's answer for the whole stream: (bytes, records as lists
    with out_off dropped, frames)."""
    host = np.frombuffer(wire, np.uint8).copy() if wire else np.zeros(0, np.uint8)
    frames, _, n = oracle.decode_stream(host, cap=len(wire) // 2 + 2)
    out, recs = oracle.reassemble(host, frames, opts)
    total = sum(r.length for r in recs)
    return out[:total].tobytes(), [[r.first_frame, r.nframes, None, r.length, r.status, r.opcode] for r in recs], \
        frames


def check_fold(oracle, wire, calls, opts=M.REASM_UTF8, records=None):
    """The acceptance property: the calls' records folded = the unsplit
    stream's, their outputs concatenated = its output; UTF8_BAD monotone within
    a message. records: per call, instead of the model's (the device's)."""
    want_out, want, frames = unsplit(oracle, wire, opts)
    folded, seen = [], 0
    bad_before = False
    for k, c in enumerate(calls):
        recs = c.recs if records is None else records[k]
        for r in recs:
            if r[4] & M.CONTINUED:
                assert not (bad_before and not r[4] & M.UTF8_BAD), (k, r)
            bad_before = bool(r[4] & M.UTF8_BAD)
        M.fold(folded, recs, seen)
        seen += len(c.frames)
    assert seen == len(frames)
    # the unsplit record of a message still open at the stream's end holds the bytes of a cut last
    # frame that never arrived: none here (every stream ends whole or the caller compares prefixes)
    assert folded == want, (folded, want)
    assert b"".join(c.out for c in calls) == want_out
    return folded


# --------------------------------------------------------------------------- 1. the short stream

def short_stream():
    """(wire, marks): a 3-fragment text message with a ping between fragments,
    an orphan continuation, an interrupted message, a binary message, a text
    message ending in E2 82. marks: name -> (start, end) wire ranges."""
    rng = streams.SplitMix(0x5EA)
    wire, marks = b"", {}

    def add(name, b0, payload):
        nonlocal wire
        fr = msg_streams._frame(rng, b0, payload)
        hdr = len(fr) - len(payload)
        marks[name] = (len(wire), len(wire) + hdr, len(wire) + len(fr))
        wire += fr

    add("t0", 0x01, "héllo ".encode() * 3)
    add("ping", 0x89, b"ping-payload")
    add("t1", 0x00, "wörld € ".encode() * 3)
    add("t2", 0x80, "𝄞 done".encode())
    add("orphan", 0x80, b"orphan continuation bytes")
    add("i0", 0x02, bytes(range(20)))
    add("i1", 0x00, bytes(range(20, 40)))
    add("bin", 0x82, bytes(range(100, 160)))
    add("text_cut", 0x81, b"tail " + b"\xe2\x82")
    return wire, marks


def short_cut_kinds(marks, cut):
    """Which of the required situations a cut position is."""
    kinds = set()
    for name, (a, h, e) in marks.items():
        if a < cut < h:
            kinds.add("header")
        if cut == h and e > h:
            kinds.add("after_header")
        if h < cut < e:
            kinds.add({"ping": "control", "orphan": "orphan"}.get(name, "member"))
    if cut in (marks["t2"][2], marks["bin"][2], marks["orphan"][2]):
        kinds.add("boundary")
    return kinds


# --------------------------------------------------------------------------- 2. generator streams

def random_cuts(seed, length, k):
    rng = streams.SplitMix(seed)
    return sorted(rng.below(length + 1) for _ in range(k - 1))


def orphan_cuts(frames):
    """A cut inside (or right after the header of) every orphan continuation of
    an unsplit frame list: random cuts rarely leave orphans pending."""
    cuts, is_open = [], False
    for f in frames:
        op, fin = f.flags & 0x0F, bool(f.flags & 0x10)
        if op in (1, 2):
            is_open = not fin
        elif op == 0:
            if is_open:
                is_open = not fin
            else:
                cuts.append(f.payload_off + f.payload_len // 2)
    return cuts


def generator_splits(oracle, seed, wire):
    """The cut lists of a generator stream: k-way random splits and the orphan cuts."""
    host = np.frombuffer(wire, np.uint8).copy()
    frames, _, _ = oracle.decode_stream(host, cap=len(wire) // 2 + 2)
    return [random_cuts(seed * 100 + k, len(wire), k) for k in (2, 5, 17)] + [orphan_cuts(frames)]


def whole_frame_prefix(oracle, wire, limit=400):
    """wire up to the first frame boundary at or after `limit` (an unsplit
    reference of it sees only whole frames)."""
    host = np.frombuffer(wire, np.uint8).copy()
    frames, _, _ = oracle.decode_stream(host, cap=len(wire) // 2 + 2)
    return wire[:min(f.payload_off + f.payload_len for f in frames if f.payload_off + f.payload_len >= limit)]


# --------------------------------------------------------------------------- 3. UTF-8 seams

SEAM_SEQS = ["é".encode(), "€".encode(), "𝄞".encode(), b"\xe0\x80\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80",
             b"\xc0\xaf", b"\x80", b"\xf0\x9f\x98"]


def seam_stream(seq, completes):
    """(wire, positions): a text message of two fragments, `seq` at the end of
    the first fragment's bytes; positions = wire offsets after each byte of
    seq. completes: the FIN fragment follows, else the message stays open."""
    rng = streams.SplitMix(len(seq) * 131 + seq[0])
    f0 = msg_streams._frame(rng, 0x01, b"abc " + seq)
    wire = f0 + msg_streams._frame(rng, 0x80 if completes else 0x00, b" xyz")
    if completes:
        wire += msg_streams._frame(rng, 0x81, b"next")
    pos = [len(f0) - len(seq) + j + 1 for j in range(len(seq))]
    return wire, pos


# --------------------------------------------------------------------------- 6. caps

def caps_stream():
    """(wire, cuts): two whole messages, then a text message of three fragments
    (an FF in the second) open across both cuts, then one more message. The
    first batch ends inside the open message, its third record."""
    rng = streams.SplitMix(3)
    wire = msg_streams._frame(rng, 0x82, b"b" * 40) + msg_streams._frame(rng, 0x81, b"t" * 40)
    open_at = len(wire)
    wire += msg_streams._frame(rng, 0x01, "héllo wörld ".encode() * 8) + msg_streams._frame(rng, 0x00, b"more\xff")
    wire += msg_streams._frame(rng, 0x80, b" end") + msg_streams._frame(rng, 0x81, "next €".encode())
    return wire, [open_at + 50, open_at + 110]


# --------------------------------------------------------------------------- 4. tile seams

def tile_stream(corrupt_at=None):
    """One text message of about 200 KiB of valid UTF-8 in frames of 70 000
    payload bytes: (wire, payload, list of (wire offset of payload byte 0,
    payload bytes) per frame)."""
    rng = streams.SplitMix(0x71)
    unit = "€𝄞 日本語 ✓ ".encode()
    text = bytearray(unit * (200 * 1024 // len(unit)))
    if corrupt_at is not None:
        text[corrupt_at] = 0xFF
    text = bytes(text)
    wire, spans, p = b"", [], 0
    while p < len(text):
        part = text[p:p + 70000]
        last = p + 70000 >= len(text)
        fr = msg_streams._frame(rng, (0x01 if p == 0 else 0x00) | (0x80 if last else 0), part)
        spans.append((len(wire) + len(fr) - len(part), len(part)))
        wire += fr
        p += len(part)
    return wire, text, spans


def wire_pos_of_payload(spans, q):
    """Wire offset just before payload byte q (q = total: the stream's end)."""
    for off, ln in spans:
        if q < ln:
            return off + q
        q -= ln
    return spans[-1][0] + spans[-1][1]

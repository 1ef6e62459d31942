"""Plain-Python model of xyws_reassemble_streams (include/xyws.h): per
connection it is xyws_reassemble_stream's model (tests/reasm_model.py, feed),
to which this adds only the overflow rule, the sticky XYWS_MSG_OVERFLOW bit
and the result row. Below it, the inputs shared by the CPU test
(tests/test_reasm_streams_model.py) and the device test
(tests/test_gpu_reasm_streams.py): scenarios of connections cut into sweeps,
and the model run over them with the oracle's decode."""
import numpy as np

import msg_streams
import reasm_cases as RC
import reasm_model as M
import streams

MSG_OVERFLOW = 0x80
RSM_TRUNCATED, RSM_MSG_CAP, RSM_OVERFLOW, RSM_OPEN, RSM_UTF8_BAD = 0x1, 0x2, 0x4, 0x8, 0x10


def pack_result(r):
    return (r["out_len"].to_bytes(8, "little") + r["nmsgs"].to_bytes(8, "little") +
            r["completed"].to_bytes(4, "little") + r["status"].to_bytes(4, "little") + bytes(8))


def pack_records(recs):
    return b"".join(f.to_bytes(8, "little") + n.to_bytes(8, "little") + o.to_bytes(8, "little") +
                    ln.to_bytes(8, "little") + st.to_bytes(4, "little") + bytes([op, 0, 0, 0])
                    for (f, n, o, ln, st, op) in recs)


def copy_carry(mc):
    return M.Carry(**{f: getattr(mc, f) for f in M.Carry.FIELDS})


def feed(src, frames, opts, carry, out_cap, msg_cap, nframes=None, cap=None, frames_null=False):
    """One connection's share of a call. carry: M.Carry or None (a null mc:
    fresh, no state kept). out_cap / msg_cap: the effective ones (0 for a null
    out / msgs). nframes: the count the decode wrote (default len(frames));
    cap: the table's capacity (default: enough). Returns (bytes written,
    stored records, carry out, result)."""
    mc = carry if carry is not None else M.Carry()
    t = len(frames) if nframes is None else nframes
    if (mc.status & MSG_OVERFLOW) or (cap is not None and t > cap) or (frames_null and t):
        co = copy_carry(mc)
        co.status |= MSG_OVERFLOW
        return b"", [], co, dict(out_len=0, nmsgs=0, completed=0, status=RSM_OVERFLOW)
    out, recs, co, nm = M.feed(src, frames, opts, mc, out_cap, msg_cap)
    # out_len: the bytes of all records, whatever the caps
    _, allrecs, _, _ = M.feed(src, frames, opts, mc, len(src), len(frames) + 1)
    out_len = sum(r[3] for r in allrecs)
    st = (RSM_TRUNCATED if out_len > out_cap else 0) | (RSM_MSG_CAP if nm > msg_cap else 0) | \
        (RSM_OPEN if co.opcode else 0) | (RSM_UTF8_BAD if any(r[4] & M.UTF8_BAD for r in recs) else 0)
    res = dict(out_len=out_len, nmsgs=nm, completed=sum(1 for r in recs if r[4] & M.COMPLETE), status=st)
    return out, recs, co, res


# --------------------------------------------------------------------------- sweeps
class Exp:
    """What one connection of one sweep is given and what the model expects."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class State:
    """The connections' decode and message carries across sweeps (model side)."""

    def __init__(self):
        self.dc, self.mc = {}, {}


def model_sweep(oracle, st, pieces, ids=None, opts=M.REASM_UTF8, out_caps=None, msg_caps=None, caps=None,
                out_null=(), msgs_null=(), use_mc=True):
    """The model's answer for one decode + reassemble of pieces[k] received by
    connection ids[k]. caps[k]: descriptor capacity (default count + 1; None: a
    null frames pointer). out_caps / msg_caps default len and count + 1.
    out_null / msgs_null: the k with a null out / msgs pointer."""
    ids = list(range(len(pieces))) if ids is None else list(ids)
    exp = []
    for k, i in enumerate(ids):
        buf = np.frombuffer(pieces[k], np.uint8).copy() if len(pieces[k]) else np.zeros(0, np.uint8)
        fr, dc, cnt = oracle.decode_stream(buf, carry_in=st.dc.get(i))
        assert cnt == len(fr)
        st.dc[i] = dc
        cap = caps[k] if caps is not None else cnt + 1
        ocap = out_caps[k] if out_caps is not None and out_caps[k] is not None else buf.size
        mcap = msg_caps[k] if msg_caps is not None and msg_caps[k] is not None else cnt + 1
        cin = st.mc.get(i, M.Carry()) if use_mc else None
        out, recs, co, res = feed(buf.tobytes(), fr, opts, cin, 0 if k in out_null else ocap,
                                  0 if k in msgs_null else mcap, nframes=cnt, cap=cap or 0, frames_null=cap is None)
        if use_mc:
            st.mc[i] = co
        exp.append(Exp(id=i, piece=pieces[k], host=buf, frames=fr, cnt=cnt, cap=cap, out_cap=ocap, msg_cap=mcap,
                       out_null=k in out_null, msgs_null=k in msgs_null, carry_in=cin, out=out, recs=recs, carry=co,
                       res=res))
    return exp


def rounds(conns):
    """conns: piece lists. Sweep r holds piece r of every connection (len 0
    for those that have no more)."""
    return [[c[r] if r < len(c) else b"" for c in conns] for r in range(max(len(c) for c in conns))]


class Coverage:
    """Counts of the situations the device tests must reach (on the model)."""
    KEYS = ("continued", "closing", "orphans_carried", "tail1", "tail2", "tail3", "interrupted", "bad_after_cut")

    def __init__(self):
        self.n = dict.fromkeys(self.KEYS, 0)

    def add(self, exp):
        for e in exp:
            c = e.carry
            self.n["continued"] += sum(1 for r in e.recs if r[4] & M.CONTINUED)
            self.n["interrupted"] += sum(1 for r in e.recs if r[4] & M.INTERRUPTED)
            if e.res["status"] & RSM_OVERFLOW:
                continue
            self.n["closing"] += bool(c.opcode and c.status & M.COMPLETE)
            self.n["orphans_carried"] += bool(not c.opcode and c.status & M.ORPHANS)
            if c.utf8:
                self.n["tail%d" % len(c.utf8)] += 1
            # UTF8_BAD found only by the call after the cut: a continued record that is bad while the carry was not
            cin = e.carry_in
            if cin is not None and cin.utf8 and e.recs and e.recs[0][4] & M.CONTINUED and e.recs[0][4] & M.UTF8_BAD:
                self.n["bad_after_cut"] += 1
        return self

    def require(self, *keys):
        missing = [k for k in (keys or self.KEYS) if not self.n[k]]
        assert not missing, (missing, self.n)


# --------------------------------------------------------------------------- scenarios
# Each returns a list of sweeps; a sweep is (pieces, kwargs of model_sweep plus
# the placement hints `mis`, `omis`, `packed` the device test uses).

def short_every_cut(middle=False):
    """RC.short_stream() at every cut, one connection per cut."""
    wire, _ = RC.short_stream()
    if middle:
        conns = [RC.batches(wire, [cut, cut + 1]) for cut in range(len(wire))]
    else:
        conns = [RC.batches(wire, [cut]) for cut in range(len(wire) + 1)]
    return [(p, {}) for p in rounds(conns)], [wire] * len(conns), conns


def generator(oracle):
    """msg_streams.message_stream seeds 1-4, each cut by every list of
    RC.generator_splits: a connection per (seed, cut list)."""
    conns, wires = [], []
    for seed in (1, 2, 3, 4):
        wire, _ = msg_streams.message_stream(seed, nmsg=60)
        for cuts in RC.generator_splits(oracle, seed, wire):
            conns.append(RC.batches(wire, cuts))
            wires.append(wire)
    return [(p, {}) for p in rounds(conns)], wires, conns


TILE_PATTERN = ("text", "cont", "ping", "fin", "binary", "orphan")
TILE_TEXT = "wörld € 𝄞 ✓ 日本語 ".encode()


def tile_stream(nframes, phase, seed=0x711E):
    """nframes frames, frame j being TILE_PATTERN[(j + phase) % 6]: a text
    message of three fragments with a ping before the last (the fragments cut
    TILE_TEXT at byte positions that move with j, so inside its sequences), a
    one-frame binary message, an orphan FIN continuation."""
    rng = streams.SplitMix(seed + 131 * nframes + phase)
    wire, kinds = b"", []
    for j in range(nframes):
        kind = TILE_PATTERN[(j + phase) % 6]
        a = (j * 5) % (len(TILE_TEXT) - 9)
        if kind == "text":
            fr = msg_streams._frame(rng, 0x01, TILE_TEXT[:a])
        elif kind == "cont":
            fr = msg_streams._frame(rng, 0x00, TILE_TEXT[(a - 5) % len(TILE_TEXT):][:7])
        elif kind == "ping":
            fr = msg_streams._frame(rng, 0x89, b"p" * (j % 4))
        elif kind == "fin":
            fr = msg_streams._frame(rng, 0x80, TILE_TEXT[a:])
        elif kind == "binary":
            fr = msg_streams._frame(rng, 0x82, bytes([j & 0xFF]) * (j % 7))
        else:
            fr = msg_streams._frame(rng, 0x80, b"orphan"[:j % 6])
        wire += fr
        kinds.append(kind)
    return wire, kinds


def tile_seams(T):
    """Connections of T - 1, T, T + 1 and 2T + 1 frames at every phase of the
    pattern, whole and cut in the middle."""
    conns, kinds = [], []
    for n in (T - 1, T, T + 1, 2 * T + 1):
        for phase in range(6):
            wire, kd = tile_stream(n, phase)
            conns.append([wire])
            kinds.append(kd)
            conns.append(RC.batches(wire, [len(wire) // 2 + phase]))
            kinds.append(kd)
    return [(p, {}) for p in rounds(conns)], kinds, conns


def copy_seam_stream(S, d, seq, start, corrupt, seed=0x5EA4):
    """Two one-frame text messages: the first delivers bytes [0, S + d) of out,
    the second starts there. `seq` lies at out position `start` (it straddles
    S), ASCII elsewhere; corrupt: the byte at out position S becomes '('."""
    rng = streams.SplitMix(seed + S + 7 * (d + 3) + len(seq))
    total = S + d + 24
    data = bytearray(b"abcdefghijklmnopqrstuvwxyz"[q % 26] for q in range(total))
    data[start:start + len(seq)] = seq
    if corrupt:
        data[S] = 0x28
    data = bytes(data)
    return msg_streams._frame(rng, 0x81, data[:S + d]) + msg_streams._frame(rng, 0x81, data[S + d:])


def copy_seams(step):
    """Message ends at S + d, d = -3..3, S the copy step and the 16-byte line;
    every RC.SEAM_SEQS sequence straddling S, intact and corrupted; out at
    misalignment 0 and 5 (the seam is an address: out position S - omis)."""
    pieces, omis = [], []
    for S in (step, 16):
        for mis in (0, 5):
            for d in range(-3, 4):
                for seq in RC.SEAM_SEQS:
                    for start in sorted({S - mis - 1, S - mis - (len(seq) - 1)} if len(seq) > 1 else {S - mis - 1,
                                                                                                      S - mis}):
                        for corrupt in (False, True):
                            pieces.append(copy_seam_stream(S - mis, d, seq, start, corrupt))
                            omis.append(mis)
    return [(pieces, dict(omis=omis))]


def frag_stream(seq, k, seed=0xF4A6):
    """One text message of two fragments with a ping between them, seq[:k] the
    last bytes of the first and seq[k:] the first bytes of the second; then one
    more message."""
    rng = streams.SplitMix(seed + 17 * len(seq) + k + seq[0])
    return (msg_streams._frame(rng, 0x01, b"abc " + seq[:k]) + msg_streams._frame(rng, 0x89, b"pp") +
            msg_streams._frame(rng, 0x80, seq[k:] + b" xyz") + msg_streams._frame(rng, 0x81, b"next"))


SHIFTS = [(s, o) for s in (0, 1, 5, 15) for o in (0, 3, 14)]


def utf8_fragments():
    """Every RC.SEAM_SEQS sequence split between two fragments (one batch), and
    RC.seam_stream cut after each of its bytes in 2 and 3 sweeps; src and out
    misalignments cycle through SHIFTS."""
    conns = []
    for seq in RC.SEAM_SEQS:
        for k in range(1, len(seq)):
            conns.append([frag_stream(seq, k)])
        for completes in (True, False):
            wire, pos = RC.seam_stream(seq, completes)
            for p in pos + [pos[0] - 1]:
                for cuts in ([p], [p, p + 1], [p - 1, p], [p, len(wire) - 1]):
                    conns.append(RC.batches(wire, cuts))
    mis = [SHIFTS[i % len(SHIFTS)][0] for i in range(len(conns))]
    omis = [SHIFTS[i % len(SHIFTS)][1] for i in range(len(conns))]
    return [(p, dict(mis=mis, omis=omis)) for p in rounds(conns)], conns


def slab(G):
    """G + 3 connections of a few tens of bytes, each a two-fragment text
    message and a binary one, cut inside the first fragment: recv ranges and
    out ranges packed back to back, two sweeps."""
    rng = streams.SplitMix(0x51AB)
    conns = []
    for i in range(G + 3):
        wire = (msg_streams._frame(rng, 0x01, ("é€"[i % 2] * (2 + i % 5)).encode() + b"x" * (i % 3)) +
                msg_streams._frame(rng, 0x80, "𝄞".encode()[:4 if i % 7 else 3]) +
                msg_streams._frame(rng, 0x82, bytes([i & 0xFF]) * (i % 4)))
        conns.append(RC.batches(wire, [7 + i % 6]))
    return [(p, dict(packed=True)) for p in rounds(conns)], conns


def caps_and_nulls():
    """RC.caps_stream() under out_cap half, msg_cap 1 and both (first sweep),
    null out, null msgs, null mc, and a middle sweep without XYWS_REASM_UTF8;
    connection 0 is the uncapped run. Three sweeps of 7 connections; the
    null-mc run is a sweep list of its own."""
    wire, cuts = RC.caps_stream()
    parts = RC.batches(wire, cuts)
    half = len(parts[0]) // 2
    sweeps = []
    for r, p in enumerate(parts):
        kw = dict(out_caps=[None, half if r == 0 else None, None, half if r == 0 else None, None, None, None],
                  msg_caps=[None, None, 1 if r == 0 else None, 1 if r == 0 else None, None, None, None],
                  out_null=(4,) if r == 0 else (), msgs_null=(5,) if r == 0 else ())
        sweeps.append(([p] * 7, kw))
    noutf8 = [([p] * 2, dict(opts=M.REASM_UTF8 if r != 1 else 0)) for r, p in enumerate(parts)]
    nomc = [([p] * 2, dict(use_mc=False)) for p in parts]
    return sweeps, noutf8, nomc


def overflow_sweeps():
    """Five frames per connection; capacities 4 (t > cap), 6, a null frames
    pointer, 5; then a second sweep with room everywhere."""
    rng = streams.SplitMix(0x0F11)
    piece = b"".join(msg_streams._frame(rng, 0x81 if j != 2 else 0x01, b"m%d" % j) for j in range(5))
    return [([piece] * 4, dict(caps=[4, 6, None, 5])), ([piece] * 4, dict(caps=[9, 9, 9, 9]))]


def group_wires():
    return [msg_streams.message_stream(0x90 + i, nmsg=6)[0] for i in range(3)]

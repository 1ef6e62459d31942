"""Plain-Python model of xyws_broadcast_streams (include/xyws.h states the
semantics; the step numbers below are the header's): the deliverable test, a
room's wire, the fan-out image of every out range and all result rows. It
takes what the two calls before it wrote: stored message records
(tests/reasm_streams_model.py's Exp rows, or records made by hand) and reply
result rows (tests/reply_model.py's dicts). Below it, the scenarios shared by
the CPU test (tests/test_room_model.py) and the device test
(tests/test_gpu_room.py)."""
import numpy as np

import msg_streams
import reasm_model as M
import reasm_streams_model as SM
import reply_model as RM
import streams

NPOS = (1 << 64) - 1
NONE = 0xFFFFFFFF
ROOM_TRUNCATED, ROOM_BAD_MEMBER, ROOM_MSG_CAP = 0x1, 0x2, 0x4
BC_TRUNCATED, BC_NOT_RECEIVER, BC_NO_ROOM = 0x1, 0x2, 0x4
FIN, TEXT, BINARY, OP_MASK = 0x10, 0x1, 0x2, 0x0F
ENC_FRAME_OPCODE = 1
FILL = 0x5A  # message buffer bytes no record names


def header(flags, length):
    """The unmasked header in its minimal length form."""
    b0 = (0x80 if flags & FIN else 0) | (flags & OP_MASK)
    if length < 126:
        return bytes([b0, length])
    if length <= 0xFFFF:
        return bytes([b0, 126]) + length.to_bytes(2, "big")
    return bytes([b0, 127]) + length.to_bytes(8, "big")


class Conn:
    """What one connection brings to a broadcast call. buf: the out_cap bytes
    of its message buffer; recs: its stored records (first_frame, nframes,
    out_off, length, status, opcode), min(nmsgs, msg_cap) of them; reply: its
    xyws_reply_result as a dict, or None; send_cap: its send buffer's out_cap;
    prefix: what the send buffer holds before the call (the reply bytes)."""

    def __init__(self, buf=b"", recs=(), nmsgs=None, msg_cap=None, rsm_status=0, head=None, reply=None, room=NONE,
                 send_cap=0, prefix=b"", out_null=False, msgs_null=False):
        self.buf, self.recs = bytes(buf), [] if msgs_null else list(recs)
        self.out_cap = 0 if out_null else len(self.buf)
        self.nmsgs = len(self.recs) if nmsgs is None else nmsgs
        self.msg_cap = (len(self.recs) if msg_cap is None else msg_cap) if not msgs_null else 0
        assert len(self.recs) == min(self.nmsgs, self.msg_cap)
        self.rsm_status, self.head, self.reply, self.room = rsm_status, head, reply, room
        self.send_cap, self.prefix = send_cap, bytes(prefix)
        self.out_null, self.msgs_null = out_null, msgs_null

    @property
    def base(self):
        return self.reply["reply_len"] if self.reply is not None else 0

    def receiver(self):  # 4
        return self.reply is None or not self.reply["status"] & (RM.CLOSED | RM.OVERFLOW)


def skip_reason(rec, c):
    """None when record `rec` of connection c is deliverable (2), else why not."""
    first, _, off, length, st, _ = rec
    if st & M.CONTINUED:
        return "continued"
    if not st & M.COMPLETE:
        return "interrupted" if st & M.INTERRUPTED else "open"
    if st & M.TRUNCATED:
        return "truncated"
    if st & M.UTF8_BAD:
        return "utf8_bad"
    if off + length > c.out_cap:
        return "out_of_range"
    if c.rsm_status & SM.RSM_OVERFLOW:
        return "rsm_overflow"
    if c.reply is not None:
        if c.reply["status"] & RM.OVERFLOW:
            return "rpl_overflow"
        if c.reply["first_close"] != NPOS:
            if first >= c.reply["first_close"]:
                return "after_close"
        elif c.reply["status"] & RM.CLOSED:
            return "closed_earlier"
    return None


def frame_flags(flags, enc_opts, opcode):
    return (flags & ~OP_MASK) | opcode if enc_opts & ENC_FRAME_OPCODE else flags


def room_wire(conns, members, flags, enc_opts):
    """3: (the full wire, its frames as (member, record index, header, payload), result without TRUNCATED)."""
    wire, frames = bytearray(), []
    nmsgs = skipped = receivers = status = 0
    for i in members:
        if i >= len(conns):
            status |= ROOM_BAD_MEMBER
            continue
        c = conns[i]
        receivers += c.receiver()
        if c.nmsgs > c.msg_cap:
            status |= ROOM_MSG_CAP
        hd = c.head or b""
        for r, rec in enumerate(c.recs):
            if skip_reason(rec, c) is not None:
                skipped += 1
                continue
            payload = hd + c.buf[rec[2]:rec[2] + rec[3]]
            h = header(frame_flags(flags, enc_opts, rec[5]), len(payload))
            frames.append((i, r, h, payload))
            wire += h + payload
            nmsgs += 1
    return bytes(wire), frames, dict(wire_len=len(wire), nmsgs=nmsgs, skipped=skipped, receivers=receivers,
                                     status=status)


class Room:
    def __init__(self, members, wire_cap=None, wire_null=False):
        self.members, self.wire_cap, self.wire_null = list(members), wire_cap, wire_null


class Result:
    """rooms: per room (written wire bytes, frames, result dict, full wire);
    conns: per connection (offset of the first written byte in out, the bytes
    written there, result dict)."""


def broadcast(conns, rooms, flags=FIN | TEXT, enc_opts=0):
    res = Result()
    res.rooms, res.conns = [], []
    for rm in rooms:
        full, frames, rr = room_wire(conns, rm.members, flags, enc_opts)
        cap = 0 if rm.wire_null else (len(full) if rm.wire_cap is None else rm.wire_cap)
        if len(full) > cap:
            rr["status"] |= ROOM_TRUNCATED
        res.rooms.append((full[:cap], frames, rr, full))
    for c in conns:
        base, w, st, data = c.base, 0, 0, b""
        if c.room >= len(rooms):
            st = BC_NO_ROOM
        elif not c.receiver():
            st = BC_NOT_RECEIVER
        else:
            data = res.rooms[c.room][0]
            w = len(data)
        if base + w > c.send_cap:
            st |= BC_TRUNCATED
        lo, hi = min(base, c.send_cap), min(base + w, c.send_cap)
        res.conns.append((lo, data[lo - base:hi - base] if hi > lo else b"",
                          dict(send_len=base + w, bcast_len=w, status=st)))
    return res


def pack_room_result(r):
    return (r["wire_len"].to_bytes(8, "little") + r["nmsgs"].to_bytes(4, "little") +
            r["skipped"].to_bytes(4, "little") + r["receivers"].to_bytes(4, "little") +
            r["status"].to_bytes(4, "little") + bytes(8))


def pack_bcast_result(r):
    return (r["send_len"].to_bytes(8, "little") + r["bcast_len"].to_bytes(8, "little") +
            r["status"].to_bytes(4, "little") + bytes(12))


def pack_reply_result(r):
    return (r["reply_len"].to_bytes(8, "little") + r["first_close"].to_bytes(8, "little") +
            r["answered"].to_bytes(4, "little") + r["close_code"].to_bytes(2, "little") +
            r["status"].to_bytes(2, "little") + bytes(8))


class Coverage:
    """Counts of the situations the tests must reach (on the model)."""
    KEYS = ("continued", "open", "interrupted", "utf8_bad", "truncated", "rsm_overflow", "rpl_overflow",
            "before_close", "after_close", "closed_earlier", "hdr2", "hdr4", "hdr10", "bad_member", "msg_cap",
            "no_room", "empty_room")

    def __init__(self):
        self.n = dict.fromkeys(self.KEYS, 0)

    def add(self, conns, rooms, res):
        for rm, (_, frames, rr, _) in zip(rooms, res.rooms):
            self.n["bad_member"] += bool(rr["status"] & ROOM_BAD_MEMBER)
            self.n["msg_cap"] += bool(rr["status"] & ROOM_MSG_CAP)
            self.n["empty_room"] += not rm.members
            for i, r, h, _ in frames:
                self.n["hdr%d" % len(h)] += 1
                c = conns[i]
                if c.reply is not None and c.reply["first_close"] != NPOS:
                    self.n["before_close"] += 1
            for i in rm.members:
                if i >= len(conns):
                    continue
                c = conns[i]
                # (a connection whose table overflowed has no records: the member itself is counted)
                self.n["rsm_overflow"] += bool(c.rsm_status & SM.RSM_OVERFLOW)
                self.n["rpl_overflow"] += bool(c.reply is not None and c.reply["status"] & RM.OVERFLOW)
                for rec in c.recs:
                    why = skip_reason(rec, c)
                    if why in self.n and why not in ("rsm_overflow", "rpl_overflow"):
                        self.n[why] += 1
        self.n["no_room"] += sum(1 for c in conns if c.room >= len(rooms))
        return self

    def require(self, *keys):
        missing = [k for k in (keys or self.KEYS) if not self.n[k]]
        assert not missing, (missing, self.n)


# --------------------------------------------------------------------------- scenarios
# Each returns (conns, rooms, kwargs of broadcast) or a list of them. Placement
# hints for the device test ride on the objects: Conn.bmis (message buffer),
# Conn.hmis (head), Conn.smis (send buffer: the misalignment of out + base),
# Room.wmis (wire); `packed` send ranges are a kwarg the model ignores.

def text(n, salt=0):
    return bytes(0x61 + (q * 7 + salt) % 26 for q in range(n))


def speaker(lengths, head=None, statuses=None, opcodes=None, firsts=None, gap=3, **kw):
    """A connection whose message buffer holds messages of the given lengths,
    `gap` unnamed bytes between them, one record each."""
    buf, recs = bytearray(), []
    for k, ln in enumerate(lengths):
        buf += bytes([FILL]) * gap
        st = M.COMPLETE if statuses is None else statuses[k]
        op = TEXT if opcodes is None else opcodes[k]
        recs.append((k if firsts is None else firsts[k], 1, len(buf), ln, st, op))
        buf += text(ln, k + len(lengths))
    buf += bytes([FILL]) * gap
    return Conn(buf=buf, recs=recs, head=head, **kw)


HEAD24 = b"[2026-10-20 16:46] bob: "
assert len(HEAD24) == 24


def reply_row(reply_len=0, first_close=NPOS, status=0, code=0, answered=0):
    return RM.result(reply_len, first_close, answered, code, status)


def size_sends(conns, rooms, flags=FIN | TEXT, enc_opts=0, slack=7):
    """send_cap = base + the room's wire + slack, for those that have none yet."""
    res = broadcast(conns, rooms, flags, enc_opts)
    for c in conns:
        if not c.send_cap:
            w = len(res.rooms[c.room][3]) if c.room < len(rooms) else 0
            c.send_cap = c.base + w + slack
            c.prefix = text(min(c.base, c.send_cap), 5)
    return conns, rooms


def header_forms():
    """head_len 24 and 0; head + length 0, 1, 125, 126, 127, 65 535, 65 536."""
    a = speaker([0, 1, 125, 126, 127, 65535, 65536], head=None, room=0)
    b = speaker([101, 102, 103, 65511, 65512], head=HEAD24, room=0)
    c = Conn(room=0, reply=reply_row(9))  # a listener
    conns, rooms = size_sends([a, b, c], [Room([0, 1, 2])])
    return conns, rooms, {}


def alignment_matrix(S, L, packed=False):
    """16 rooms whose wires are misaligned 0..15 times 16 members whose out +
    base is misaligned 0..15, every wire cut to L bytes by its cap; message
    buffers and heads misaligned 0..15 for the wire build."""
    conns, rooms = [], []
    for r in range(16):
        for m in range(16):
            lens = [2 * S + 40] if m == 0 else [m + r]
            hd = HEAD24[:8 * ((m + r) % 4)] or None
            c = speaker(lens, head=hd, room=r, reply=reply_row(3 * m + r) if (m + r) % 5 else None)
            c.bmis, c.hmis, c.smis = (m + 3 * r) % 16, (5 * m + r) % 16, m
            conns.append(c)
        rm = Room(range(16 * r, 16 * r + 16), wire_cap=L)
        rm.wmis = r
        rooms.append(rm)
    for c in conns:
        c.send_cap = c.base + L + (c.smis % 3)
        c.prefix = text(c.base, 5)
    return conns, rooms, dict(packed=packed)


SKIPS = (M.COMPLETE, M.COMPLETE | M.CONTINUED, 0, M.INTERRUPTED, M.COMPLETE | M.UTF8_BAD, M.COMPLETE | M.TRUNCATED,
         M.COMPLETE | M.ORPHANS)


def tiles(T, msg_cap=5):
    """Rooms of 0, 1, T - 1, T, T + 1 and 2T + 3 members; members with 0, 1, 3
    and msg_cap stored records and one with nmsgs > msg_cap; every status of
    SKIPS among the records; binary and text."""
    conns, rooms = [], []
    for size in (0, 1, T - 1, T, T + 1, 2 * T + 3):
        lo = len(conns)
        for k in range(size):
            cnt = (1, 0, 3, msg_cap)[k % 4]
            sts = [SKIPS[(k + j) % len(SKIPS)] if (k + j) % 3 == 0 else M.COMPLETE for j in range(cnt)]
            ops = [BINARY if (k + j) % 5 == 0 else TEXT for j in range(cnt)]
            over = size == T + 1 and k == 7
            c = speaker([(3 * k + 5 * j) % 23 for j in range(cnt)], head=HEAD24[:k % 25] or None, statuses=sts,
                        opcodes=ops, room=len(rooms), gap=k % 4, nmsgs=cnt + 2 if over else None,
                        msg_cap=cnt if over else None)
            conns.append(c)
        rooms.append(Room(range(lo, lo + size)))
    conns, rooms = size_sends(conns, rooms, enc_opts=ENC_FRAME_OPCODE)
    return conns, rooms, dict(flags=FIN | TEXT, enc_opts=ENC_FRAME_OPCODE, packed=True)


def over_grid(G):
    """More rooms and more connections than the grid cap, all tiny."""
    conns = [speaker([k % 5], head=b"#" * (k % 3) or None, room=k) for k in range(G + 3)]
    rooms = [Room([k]) for k in range(G + 3)]
    for c in conns:
        c.send_cap = 2 + (len(c.head or b"")) + c.recs[0][3]
    return conns, rooms, dict(packed=True)


def wire_caps():
    """One frame (header 2, head 24, 9 message bytes) under every wire_cap from
    0 through its length + 1, a null wire, and the uncapped room."""
    flen = 2 + 24 + 9
    conns, rooms = [], []
    for cap in list(range(flen + 2)) + ["null", None]:
        r = len(rooms)
        conns += [speaker([9], head=HEAD24, room=r), Conn(room=r, reply=reply_row(4))]
        rooms.append(Room([2 * r, 2 * r + 1], wire_cap=cap if isinstance(cap, int) else None, wire_null=cap == "null"))
    for c in conns:
        c.send_cap = c.base + flen + 2
        c.prefix = text(c.base, 5)
    return conns, rooms, {}


def out_caps():
    """One room, one frame; listeners whose out_cap goes from base through base
    + the frame + 1 (base 0 and 6), one with base == out_cap, one with
    base > out_cap (a truncated reply), one with no send buffer room at all."""
    flen = 2 + 24 + 9
    conns = [speaker([9], head=HEAD24, room=0, send_cap=flen)]
    for base in (0, 6):
        for k in range(flen + 2):
            conns.append(Conn(room=0, reply=reply_row(base) if base else None, send_cap=base + k,
                              prefix=text(base, 5)))
    conns.append(Conn(room=0, reply=reply_row(11), send_cap=11, prefix=text(11, 5)))
    conns.append(Conn(room=0, reply=reply_row(40, status=RM.TRUNCATED), send_cap=13, prefix=text(13, 5)))
    conns.append(Conn(room=0, send_cap=0))
    return conns, [Room(range(len(conns)))], dict(packed=True)


def nulls_and_trivia():
    """Replies for some; a null head; a members[] entry >= n between two valid
    ones; a room field >= n_rooms; a listener outside every room; gates made by
    hand: reply overflow with stored records, closed earlier, closed in this
    sweep between two messages, reassembly overflow, a record that names bytes
    outside its buffer."""
    c0 = speaker([5, 6], head=None, room=0)
    c1 = speaker([7], head=HEAD24, room=0, reply=reply_row(4))
    c2 = speaker([3, 4], room=0, reply=reply_row(0, status=RM.OVERFLOW))
    c3 = speaker([3], room=0, reply=reply_row(0, status=RM.CLOSED, code=1000))
    c4 = speaker([8, 9, 10], room=0, firsts=[0, 2, 5], reply=reply_row(14, first_close=2, status=RM.CLOSED, code=1000))
    c5 = speaker([4], room=0, rsm_status=SM.RSM_OVERFLOW)
    c6 = speaker([4, 2], room=0)
    c6.recs[0] = (0, 1, len(c6.buf) - 2, 4, M.COMPLETE, TEXT)       # runs past the buffer
    c6.recs[1] = (1, 1, NPOS - 1, 2, M.COMPLETE, TEXT)              # wraps
    c7 = speaker([6], room=9)                                       # a room field >= n_rooms
    c8 = Conn(room=NONE, reply=reply_row(3))
    c9 = speaker([2], room=1, out_null=True)                        # a null message buffer: cap 0
    c10 = speaker([0, 3], room=1, msgs_null=True, nmsgs=2)
    conns = [c0, c1, c2, c3, c4, c5, c6, c7, c8, c9, c10]
    rooms = [Room([0, 1, 2, 3, 11, 4, 5, 6, 0xFFFFFFFE]), Room([9, 10]), Room([])]
    conns, rooms = size_sends(conns, rooms)
    return conns, rooms, {}


# --------------------------------------------------------------------------- the real sweep
def _f(rng, b0, payload):
    return msg_streams._frame(rng, b0, payload)


def sweep_streams():
    """Two sweeps of nine connections, two rooms and one connection outside.
    Returns (pieces per sweep, descriptor caps, room member lists, room of each)."""
    rng = streams.SplitMix(0xC4A7)
    bad = b"caf\xc3(" + b"!"
    s1 = [
        _f(rng, 0x89, b"hi") + _f(rng, 0x81, b"hello room") + _f(rng, 0x82, b"\x00\x01\x02"),          # 0 ping first
        _f(rng, 0x81, b"before") + _f(rng, 0x88, b"\x03\xe8") + _f(rng, 0x81, b"after the close"),      # 1 closes
        _f(rng, 0x81, b"bye") + _f(rng, 0x88, b""),                                                     # 2 closes
        b"".join(_f(rng, 0x81, b"m%d" % j) for j in range(6)),                                          # 3 overflows
        b"",                                                                                            # 4 spans sweeps
        _f(rng, 0x81, bad) + _f(rng, 0x81, "grüß".encode()),                                  # 5 invalid UTF-8
        _f(rng, 0x01, b"frag") + _f(rng, 0x89, b"") + _f(rng, 0x80, b"ments") + _f(rng, 0x01, b"open"),  # 6
        _f(rng, 0x81, b"x" * 130) + _f(rng, 0x01, b"one") + _f(rng, 0x81, b"two"),                      # 7 interrupted
        _f(rng, 0x81, b"outside"),                                                                      # 8 no room
    ]
    s2 = [
        _f(rng, 0x81, b"second sweep"),
        _f(rng, 0x81, b"speaks after its close"),
        _f(rng, 0x81, b"so does this one"),
        _f(rng, 0x81, b"still overflowed"),
        b"",
        _f(rng, 0x82, b"\xff\xfe") + _f(rng, 0x89, b"p"),
        _f(rng, 0x80, b" message") + _f(rng, 0x81, b"done"),
        b"",
        _f(rng, 0x81, b"outside again"),
    ]
    # connection 4: one message of three fragments, cut inside the second
    whole = _f(rng, 0x01, b"cut in ") + _f(rng, 0x00, b"two ") + _f(rng, 0x80, b"sweeps")
    s1[4], s2[4] = whole[:18], whole[18:]
    caps = [8, 8, 8, 5, 8, 8, 8, 8, 8]
    return [s1, s2], caps, [[0, 1, 2, 3, 4], [7, 6, 5]], [0, 0, 0, 0, 0, 1, 1, 1, NONE]


class SweepState:
    def __init__(self):
        self.sm = SM.State()
        self.rc = {}


REPLY_MODE = dict(policy=RM.POL_FRAGMENTS, flags=0, enc_opts=RM.ENC_FRAME_OPCODE, action_mask=1 << RM.ACT_PING)


def model_real_sweep(oracle, st, pieces, caps, members, room_of, flags=FIN | TEXT, enc_opts=0, exp=None,
                     send_cap=None, wire_cap=None, **sweep_kw):
    """decode -> reassemble -> reply (REPLY_MODE: pings answered as pongs,
    fragments allowed) -> broadcast of one sweep, on the models. exp: the
    reassembly rows when the caller has run SM.model_sweep on st.sm already.
    send_cap: one size for every send buffer (default: the reply's len + 13 or
    what the member is sent plus 5, whichever is more); wire_cap: one for every
    wire (default: its length). Returns (exp rows, reply rows, conns, rooms,
    broadcast result)."""
    if exp is None:
        exp = SM.model_sweep(oracle, st.sm, pieces, caps=caps, **sweep_kw)
    mode = REPLY_MODE
    conns, replies = [], []
    for k, e in enumerate(exp):
        rcap = len(e.piece) + 13 if send_cap is None else send_cap
        w, res, _, rc = RM.reply(oracle, e.host, e.frames, st.rc.get(k, RM.Carry()), rcap, 1 << 20, nframes=e.cnt,
                                 cap=e.cap, **mode)
        st.rc[k] = rc
        replies.append((w, res, rc))
        buf = e.out + bytes([FILL]) * (e.out_cap - len(e.out))
        conns.append(Conn(buf=buf, recs=e.recs, nmsgs=e.res["nmsgs"], msg_cap=e.msg_cap,
                          rsm_status=e.res["status"], head=HEAD24[:3 * k] or None, reply=res, room=room_of[k],
                          prefix=w))
    rooms = [Room(m, wire_cap=wire_cap) for m in members]
    res = broadcast(conns, rooms, flags, enc_opts)
    for c, e in zip(conns, exp):
        w = len(res.rooms[c.room][0]) if c.room < len(rooms) else 0
        c.send_cap = max(len(e.piece) + 13, c.base + w + 5) if send_cap is None else send_cap
    return exp, replies, conns, rooms, broadcast(conns, rooms, flags, enc_opts)

"""Plain-Python model of xyws_hold_streams (include/xyws.h states the
semantics; the step numbers below are the header's): per connection the view
records, the view row, the hold carry, the result row and the hold bytes. It
takes what xyws_reassemble_streams wrote (tests/reasm_streams_model.py's Exp
rows through from_exp, or inputs made by hand) and gives what
xyws_broadcast_streams reads (tests/room_model.py's Conn through view_conn).
Below it, the scenarios shared by the CPU test (tests/test_hold_model.py) and
the device test (tests/test_gpu_hold.py)."""
import msg_streams
import reasm_cases as RC
import reasm_model as M
import reasm_streams_model as SM
import room_model as R
import streams

DELIVERED, ACTIVE, LOST, DROPPED, TOO_LONG, PASSTHROUGH = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20
TEXT, BINARY = 1, 2
FILL = R.FILL
HOLD_FILL = 0x3C  # hold bytes nothing was copied to
MASK64 = (1 << 64) - 1


def half(hold_cap):
    return (hold_cap // 2) & ~15


class Carry:
    """xyws_hold_carry."""
    FIELDS = ("start", "held", "nframes", "status", "opcode")

    def __init__(self, start=0, held=0, nframes=0, status=0, opcode=0):
        self.start, self.held, self.nframes, self.status, self.opcode = start, held, nframes, status, opcode

    def pack(self):
        return (self.start.to_bytes(8, "little") + self.held.to_bytes(8, "little") +
                self.nframes.to_bytes(8, "little") + self.status.to_bytes(4, "little") + bytes([self.opcode, 0, 0, 0]))

    def key(self):
        return tuple(getattr(self, f) for f in self.FIELDS)

    def __eq__(self, other):
        return self.key() == other.key()

    def __repr__(self):
        return "HoldCarry(%s)" % ", ".join("%s=%d" % (f, getattr(self, f)) for f in self.FIELDS)


def pack_result(r):
    return (r["held"].to_bytes(8, "little") + r["delivered_len"].to_bytes(8, "little") +
            r["status"].to_bytes(4, "little") + bytes(12))


class In:
    """What one connection brings to a hold call: buf, the out_cap bytes of its
    reassembly range; recs, its stored records; row, its xyws_reasm_result."""

    def __init__(self, buf, recs, row, msg_cap, out_null=False, msgs_null=False):
        self.buf, self.recs, self.row, self.msg_cap = bytes(buf), list(recs), dict(row), msg_cap
        self.out_null, self.msgs_null = out_null, msgs_null
        assert len(self.recs) == (0 if msgs_null else min(row["nmsgs"], msg_cap))

    @property
    def out_cap(self):
        return len(self.buf)


def from_exp(e):
    return In(e.out + bytes([FILL]) * (e.out_cap - len(e.out)), e.recs, e.res, e.msg_cap, e.out_null, e.msgs_null)


class Out:
    """passthrough; view_recs (None when passed through: the input's row is
    used as it is); view_msg_cap; view_row; carry; result; hold (its bytes
    after the call); copies [(hold offset, out offset, length)]; events."""


def _in_range(off, length, cap):
    return off <= cap and length <= cap - off


def step(inp, carry, hold, hold_cap, vmsg_cap, hc_null=False, vmsgs_null=False):
    """One connection's share of a call. carry: Carry (ignored when hc_null);
    hold: the hold_cap bytes in front of out."""
    o = Out()
    o.inp, o.hold_cap, o.events, o.copies = inp, hold_cap, set(), []
    ev = o.events
    H = half(hold_cap)
    assert len(hold) == hold_cap
    if inp.out_null or hc_null or H == 0:  # 0
        ev.add("pt_out_null" if inp.out_null else "pt_hc_null" if hc_null else "pt_h0")
        o.passthrough, o.view_recs, o.view_msg_cap, o.view_row = True, None, inp.msg_cap, dict(inp.row)
        o.carry, o.hold, o.delivered = carry, bytes(hold), None
        o.result = dict(held=0, delivered_len=0, status=PASSTHROUGH)
        return o
    o.passthrough = False
    hold = bytearray(hold)
    recs, row = inp.recs, inp.row
    s, nmsgs = len(recs), row["nmsgs"]
    vcap = 0 if vmsgs_null else vmsg_cap
    vs = min(s, vcap)
    if vcap == 0 and s:
        ev.add("vmsg_cap0")
    elif vs < s:
        ev.add("vmsg_cap_short")
    # 1
    o.view_msg_cap = min(0 if inp.msgs_null else inp.msg_cap, vcap)
    o.view_row = dict(row, status=row["status"] | (SM.RSM_MSG_CAP if s > vcap else 0))
    view = [(f, n, (off + hold_cap) & MASK64, ln, st, op) for (f, n, off, ln, st, op) in recs[:vs]]
    c = Carry(*carry.key())
    if c.status & ACTIVE:
        c.status = ACTIVE
    else:
        c = Carry(status=c.status & LOST)
    st = 0
    delivered = None
    if row["status"] & SM.RSM_OVERFLOW:  # 2
        ev.add("overflow")
        if c.status & ACTIVE:
            st |= DROPPED
        c = Carry(status=LOST)
    else:
        has0 = s >= 1 and bool(recs[0][4] & M.CONTINUED)
        if c.status & ACTIVE and not has0:  # 5
            ev.add("rec0_unstored")
            st |= DROPPED
            c = Carry(status=LOST)
        if has0:  # 3
            _, n0, off0, len0, st0, _ = recs[0]
            if c.status & ACTIVE:
                if c.start not in (0, H) or c.held > H:
                    ev.add("bad_carry")
                    st |= DROPPED
                    c = Carry(status=LOST)
                elif st0 & M.TRUNCATED or not _in_range(off0, len0, inp.out_cap):
                    ev.add("truncated_append")
                    st |= DROPPED
                    c = Carry(status=LOST)
                elif c.held + len0 > H:
                    ev.add("too_long_append")
                    st |= DROPPED | TOO_LONG
                    c = Carry(status=LOST)
                else:
                    ev.add("append")
                    if c.held + len0 == H:
                        ev.add("append_fills_half")
                    dst = c.start + c.held
                    hold[dst:dst + len0] = inp.buf[off0:off0 + len0]
                    o.copies.append((dst, off0, len0))
                    c.held += len0
                    c.nframes += n0
            elif not c.status & LOST:
                ev.add("mid_join")
                st |= DROPPED
                c = Carry(status=LOST)
            if st0 & M.COMPLETE:
                if c.status & ACTIVE:
                    ev.add("delivered")
                    if st0 & M.UTF8_BAD:
                        ev.add("utf8_bad_delivered")
                    delivered = (0, c.nframes, c.start, c.held, st0 & ~M.CONTINUED, c.opcode)
                    st |= DELIVERED
                else:
                    ev.add("lost_cleared")
                c = Carry()
            elif st0 & M.INTERRUPTED:
                ev.add("interrupted")
                c = Carry()
        if row["status"] & SM.RSM_OPEN and nmsgs >= 1 and nmsgs - 1 < s:  # 4
            _, nl, offl, lenl, stl, opl = recs[nmsgs - 1]
            if not stl & (M.CONTINUED | M.COMPLETE | M.INTERRUPTED):
                if stl & M.TRUNCATED or not _in_range(offl, lenl, inp.out_cap):
                    ev.add("truncated_begin")
                    st |= DROPPED
                    c = Carry(status=LOST)
                elif lenl > H:
                    ev.add("too_long_begin")
                    st |= DROPPED | TOO_LONG
                    c = Carry(status=LOST)
                else:
                    target = H if delivered is not None and delivered[2] == 0 else 0
                    ev.add("begin_half1" if target else "begin_half0")
                    if lenl == H:
                        ev.add("begin_fills_half")
                    hold[target:target + lenl] = inp.buf[offl:offl + lenl]
                    o.copies.append((target, offl, lenl))
                    c = Carry(target, lenl, nl, ACTIVE, opl)
        if row["status"] & SM.RSM_OPEN:  # 5
            if not c.status & (ACTIVE | LOST):
                ev.add("last_unstored")
                st |= DROPPED
                c = Carry(status=LOST)
        else:
            c = Carry()
    if delivered is not None and vs:
        view[0] = delivered
    o.delivered = delivered
    o.view_recs, o.carry, o.hold = view, c, bytes(hold)
    o.result = dict(held=c.held, delivered_len=delivered[3] if delivered else 0, status=st | (c.status & (ACTIVE | LOST)))
    assert len(o.hold) == hold_cap
    return o


def view_conn(o, **kw):
    """What the broadcast reads of this connection through the view: a room_model.Conn."""
    inp = o.inp
    if o.passthrough:
        return R.Conn(buf=inp.buf, recs=inp.recs, nmsgs=inp.row["nmsgs"], msg_cap=inp.msg_cap,
                      rsm_status=inp.row["status"], out_null=inp.out_null, msgs_null=inp.msgs_null, **kw)
    return R.Conn(buf=o.hold + inp.buf, recs=o.view_recs, nmsgs=o.view_row["nmsgs"], msg_cap=o.view_msg_cap,
                  rsm_status=o.view_row["status"], **kw)


def plain_conn(inp, **kw):
    """The same connection without the hold call (the four-call sweep)."""
    return R.Conn(buf=inp.buf, recs=inp.recs, nmsgs=inp.row["nmsgs"], msg_cap=inp.msg_cap,
                  rsm_status=inp.row["status"], out_null=inp.out_null, msgs_null=inp.msgs_null, **kw)


class State:
    """The connections' hold carries and hold bytes across sweeps (model side)."""

    def __init__(self):
        self.hc, self.hold = {}, {}

    def sweep(self, ins, hold_caps, vmsg_caps=None, ids=None, hc_null=(), vmsgs_null=()):
        """One call: ins[k] is connection ids[k]'s In. Returns the Outs."""
        outs = []
        for k, inp in enumerate(ins):
            i = k if ids is None else ids[k]
            cap = hold_caps[k] if isinstance(hold_caps, (list, tuple)) else hold_caps
            vcap = len(inp.recs) + 1 if vmsg_caps is None or vmsg_caps[k] is None else vmsg_caps[k]
            hold = self.hold.get(i, bytes([HOLD_FILL]) * cap)
            o = step(inp, self.hc.get(i, Carry()), hold, cap, vcap, hc_null=k in hc_null, vmsgs_null=k in vmsgs_null)
            o.carry_in, o.hold_in, o.vmsg_cap, o.hc_null, o.vmsgs_null = self.hc.get(i, Carry()), hold, vcap, \
                k in hc_null, k in vmsgs_null
            if not o.hc_null:
                self.hc[i] = o.carry
            self.hold[i] = o.hold
            outs.append(o)
        return outs


class Coverage:
    """The branches the tests must reach (on the model)."""
    KEYS = ("append", "append_fills_half", "delivered", "begin_half0", "begin_half1", "begin_fills_half",
            "too_long_begin", "too_long_append", "truncated_begin", "truncated_append", "rec0_unstored",
            "last_unstored", "vmsg_cap0", "vmsg_cap_short", "mid_join", "interrupted", "utf8_bad_delivered",
            "overflow", "lost_cleared", "bad_carry", "pt_out_null", "pt_hc_null", "pt_h0", "close_at_frame0")

    def __init__(self):
        self.n = dict.fromkeys(self.KEYS, 0)

    def add(self, outs):
        for o in outs:
            for e in o.events:
                self.n[e] += 1
        return self

    def require(self, *keys):
        missing = [k for k in (keys or self.KEYS) if not self.n[k]]
        assert not missing, (missing, self.n)


# --------------------------------------------------------------------------- inputs made by hand
def made(parts, lead=0, gap=3, out_cap=None, msg_cap=None, rsm=0, nmsgs=None, **kw):
    """parts: (length, status[, opcode[, nframes]]) per record; the message
    bytes lie `lead` bytes into the buffer, `gap` unnamed bytes between them.
    XYWS_RSM_OPEN is set when the last part has neither COMPLETE nor
    INTERRUPTED. msg_cap: records stored (default all)."""
    buf, recs = bytearray(bytes([FILL]) * lead), []
    for k, p in enumerate(parts):
        ln, st = p[0], p[1]
        op = p[2] if len(p) > 2 else TEXT
        nf = p[3] if len(p) > 3 else 1 + k % 2
        recs.append((M.NPOS if st & M.CONTINUED else k, nf, len(buf), ln, st, op))
        buf += R.text(ln, k + 3 * len(parts) + lead)
        buf += bytes([FILL]) * gap
    if out_cap is not None:
        buf = buf[:out_cap] + bytes([FILL]) * (out_cap - len(buf))
    n = len(recs) if nmsgs is None else nmsgs
    cap = n if msg_cap is None else msg_cap
    status = rsm | (SM.RSM_OPEN if parts and not parts[-1][1] & (M.COMPLETE | M.INTERRUPTED) else 0) | \
        (SM.RSM_MSG_CAP if n > cap else 0)
    row = dict(out_len=sum(p[0] for p in parts), nmsgs=n, completed=sum(1 for r in recs[:cap] if r[4] & M.COMPLETE),
               status=status)
    return In(buf, recs[:cap], row, cap, **kw)


OPEN, CONT, DONE = 0, M.CONTINUED, M.COMPLETE


def loss_and_passthrough(H0=64):
    """Every loss path and every pass-through cause, one connection each, over
    three sweeps; hold_cap 2 * H0 (H == H0). Returns (sweeps, kwargs per
    sweep): sweeps[r][k] is connection k's In."""
    H = H0
    rows = [
        # 0 TOO_LONG on begin: H + 1
        [made([(5, DONE), (H + 1, OPEN)]), made([(3, CONT | DONE)]), made([])],
        # 1 begin of exactly H, then TOO_LONG on append
        [made([(H, OPEN)]), made([(1, CONT)]), made([(2, CONT | DONE)])],
        # 2 held + length == H passes and is delivered
        [made([(H - 7, OPEN)]), made([(7, CONT | DONE)]), made([])],
        # 3 a TRUNCATED part on begin
        [made([(9, OPEN | M.TRUNCATED)]), made([(4, CONT | DONE)]), made([])],
        # 4 a TRUNCATED part on append
        [made([(9, OPEN)]), made([(4, CONT | M.TRUNCATED)]), made([(4, CONT | DONE)])],
        # 5 msg_cap leaves record 0 unstored
        [made([(9, OPEN)]), made([(4, CONT | DONE), (6, OPEN)], msg_cap=0), made([(3, CONT | DONE)])],
        # 6 msg_cap leaves the last record unstored
        [made([(4, DONE), (5, DONE), (6, OPEN)], msg_cap=2), made([(3, CONT | DONE)]), made([])],
        # 7 vmsg_cap 0: the carry is exact, nothing is delivered by the view
        [made([(4, DONE), (6, OPEN)]), made([(3, CONT | DONE), (5, DONE)]), made([])],
        # 8 vmsg_cap s - 1
        [made([(4, DONE), (6, OPEN)]), made([(3, CONT | DONE), (5, DONE), (2, OPEN)]), made([(1, CONT | DONE)])],
        # 9 a carry joined mid-message
        [made([(4, CONT)]), made([(3, CONT | DONE), (5, OPEN)]), made([(2, CONT | DONE)])],
        # 10 INTERRUPTED
        [made([(6, OPEN)]), made([(3, CONT | M.INTERRUPTED), (5, DONE)]), made([])],
        # 11 UTF8_BAD completing
        [made([(6, OPEN)]), made([(3, CONT | DONE | M.UTF8_BAD)]), made([])],
        # 12 OVERFLOW with a message held; it stays LOST
        [made([(6, OPEN)]), made([], rsm=SM.RSM_OVERFLOW), made([], rsm=SM.RSM_OVERFLOW)],
        # 13 a part that names bytes outside its range
        [made([(6, OPEN)]), made([(30, CONT | DONE)], out_cap=20), made([])],
        # 14 pass-through: a null out
        [made([(6, OPEN)], out_null=True), made([(3, CONT | DONE)], out_null=True), made([])],
        # 15 pass-through: a null carry
        [made([(6, OPEN)]), made([(3, CONT | DONE)]), made([(4, DONE)])],
        # 16 pass-through: H == 0 (hold_cap 31)
        [made([(6, OPEN)]), made([(3, CONT | DONE)]), made([(4, DONE)])],
        # 17 a null vmsgs
        [made([(6, OPEN)]), made([(3, CONT | DONE)]), made([(4, DONE)])],
        # 18 a carry that does not fit this hold_cap
        [made([(6, OPEN)]), made([(3, CONT | DONE)]), made([])],
        # 19 a message that stays open over a whole sweep (an empty CONTINUED record)
        [made([(6, OPEN, BINARY)]), made([(0, CONT, BINARY, 0)]), made([(5, CONT | DONE, BINARY), (4, OPEN)])],
    ]
    n = len(rows)
    sweeps = [[rows[k][r] for k in range(n)] for r in range(3)]
    caps = [2 * H] * n
    caps[16] = 31
    kws = []
    for r in range(3):
        vm = [None] * n
        vm[7] = 0
        vm[8] = len(rows[8][r].recs) - 1 if rows[8][r].recs else None
        kws.append(dict(hold_caps=caps, vmsg_caps=vm, hc_null=(15,), vmsgs_null=(17,)))
    return sweeps, kws


def bad_carry_for(st, k=18):
    """Connection k's carry after sweep 0 replaced by one whose start is no half."""
    st.hc[k] = Carry(start=8, held=st.hc[k].held, nframes=1, status=ACTIVE, opcode=TEXT)


SEAM_KINDS = ("begin_half0", "begin_half1", "append_half0", "append_half1")


def seam_call(step, kind):
    """The copy seams of one kind (SEAM_KINDS), a connection for every part
    length (0, 1, 15, 16, 17, step - 1, step, step + 1, 2 * step + 1) x out
    misalignment 0..15 x hold_cap in {2 * H0, + 1, + 15, + 31} x source out_off
    misalignment 0..15. begin: the message open at the end starts a hold, in
    half 1 when the same call delivers a message out of half 0; append: the
    part joins a held message at held in {1, 15, 16, 17} (cycled). Returns
    (ins, carries in, hold_caps, out misalignments)."""
    lengths = [0, 1, 15, 16, 17, step - 1, step, step + 1, 2 * step + 1]
    H0 = 2 * step + 64
    ins, carries, caps, hints = [], [], [], []
    q = 0
    for L in lengths:
        for omis in range(16):
            for extra in (0, 1, 15, 31):
                for smis in range(16):
                    cap = 2 * H0 + extra
                    q += 1
                    if kind == "begin_half1":  # a message out of half 0 delivered by the same call
                        ins.append(made([(3, CONT | DONE), (L, OPEN)], gap=smis + 13))
                        carries.append(Carry(0, 5, 1, ACTIVE, TEXT))
                    elif kind == "begin_half0":
                        ins.append(made([(L, OPEN)], lead=smis))
                        carries.append(Carry())
                    else:
                        ins.append(made([(L, CONT)], lead=smis))
                        carries.append(Carry(half(cap) if kind == "append_half1" else 0, (1, 15, 16, 17)[q % 4], 2,
                                             ACTIVE, BINARY))
                    caps.append(cap)
                    hints.append(omis)
    return ins, carries, caps, hints


def row_calls():
    """Record rows: s in {0, 1, 2, 63, 64, 65, 129} with vmsg_cap in {0, 1, s - 1, s}."""
    ins, vcaps = [], []
    for s in (0, 1, 2, 63, 64, 65, 129):
        for v in sorted({0, 1, max(s - 1, 0), s}):
            parts = [((3 * j + s) % 11, DONE if j % 4 else DONE | M.UTF8_BAD, BINARY if j % 3 == 0 else TEXT)
                     for j in range(s)]
            if s >= 2:  # a delivered record 0 and a begin among them
                parts[0] = (4, CONT | DONE)
                parts[-1] = (6, OPEN)
            ins.append(made(parts, gap=1))
            vcaps.append(v)
    carries = [Carry(0, 3, 1, ACTIVE, TEXT) if len(i.recs) >= 2 else Carry() for i in ins]
    return ins, carries, vcaps


def over_grid(G):
    """G + 3 tiny connections, every third one spanning: it delivers and begins."""
    ins, carries = [], []
    for k in range(G + 3):
        if k % 3 == 0:
            ins.append(made([(1 + k % 5, CONT | DONE), (2 + k % 3, OPEN)], gap=0))
            carries.append(Carry(32 * (k % 2), 2 + k % 7, 1, ACTIVE, TEXT))
        else:
            ins.append(made([(k % 4, DONE)], gap=0))
            carries.append(Carry())
    return ins, carries


# --------------------------------------------------------------------------- streams
def three_fragments():
    """One three-fragment text message (with a ping between fragments), then a
    one-frame message."""
    rng = streams.SplitMix(0x401D)
    f = msg_streams._frame
    return (f(rng, 0x01, "héllo ".encode()) + f(rng, 0x89, b"pp") + f(rng, 0x00, "wörld € ".encode()) +
            f(rng, 0x80, "𝄞 done".encode()) + f(rng, 0x81, b"next"))


def every_cut():
    """three_fragments() cut at every byte position into 2 and into 3 sweeps, a
    connection per cut list. Returns (sweeps of pieces, wires)."""
    wire = three_fragments()
    conns = [RC.batches(wire, [c]) for c in range(len(wire) + 1)]
    conns += [RC.batches(wire, [c, c + 1]) for c in range(len(wire))]
    conns += [RC.batches(wire, [c, min(len(wire), c + 9)]) for c in range(len(wire))]
    return SM.rounds(conns), [wire] * len(conns)


def back_to_back(k=6):
    """k messages, every recv boundary inside one: each sweep completes a
    message and begins the next."""
    rng = streams.SplitMix(0xB2B)
    wire, cuts = b"", []
    for j in range(k):
        payload = R.text(20 + 3 * j, j)
        fr = msg_streams._frame(rng, 0x01, payload[:9]) + msg_streams._frame(rng, 0x80, payload[9:])
        cuts.append(len(wire) + len(fr) - 4 - j)
        wire += fr
    conns = [RC.batches(wire, cuts[:-1] + [len(wire) - 2])]
    return SM.rounds(conns), [wire]


# --------------------------------------------------------------------------- the real sweep
def real_sweep(oracle, st, hst, pieces, caps, members, room_of, hold_cap, flags=R.FIN | R.TEXT, enc_opts=0, exp=None,
               send_cap=None, wire_cap=None, **sweep_kw):
    """decode -> reassemble -> hold -> reply -> broadcast of one sweep, on the
    models: R.model_real_sweep (the four-call sweep) and the same broadcast on
    the view. st: R.SweepState, hst: State. Returns (exp rows, reply rows, the
    four-call sweep's conns, the view's conns, rooms, the four-call result, the
    five-call result, the hold call's Outs)."""
    exp, replies, conns, rooms, plain = R.model_real_sweep(oracle, st, pieces, caps, members, room_of, flags,
                                                           enc_opts, exp=exp, send_cap=send_cap, wire_cap=wire_cap,
                                                           **sweep_kw)
    outs = hst.sweep([from_exp(e) for e in exp], hold_cap, vmsg_caps=[e.msg_cap for e in exp])
    vconns = [view_conn(o, head=c.head, reply=c.reply, room=c.room, prefix=c.prefix) for o, c in zip(outs, conns)]
    res = R.broadcast(vconns, rooms, flags, enc_opts)
    for c, e in zip(vconns, exp):
        w = len(res.rooms[c.room][0]) if c.room < len(rooms) else 0
        c.send_cap = max(len(e.piece) + 13, c.base + w + 5) if send_cap is None else send_cap
    return exp, replies, conns, vconns, rooms, plain, R.broadcast(vconns, rooms, flags, enc_opts), outs

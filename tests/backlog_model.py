"""Plain-Python model of xyws_backlog_streams (include/xyws.h states the
semantics; the step numbers below are the header's): the fold of a sweep's
frames into a room's log and carry, and the delivery to joiners. It is built
on tests/room_model.py, which supplies the wire, the room rows and the
deliverable test. Below it, the scenarios shared by the CPU test
(tests/test_backlog_model.py) and the device test (tests/test_gpu_backlog.py)."""
import room_model as R

MAX = 16
BL_PASSTHROUGH, BL_BAD_CARRY, BL_MISMATCH, BL_GAP, BL_EVICTED, BL_TOO_LONG = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20
BL_JOIN = 0x1
BLC_JOINED, BLC_TRUNCATED, BLC_NO_ROOM, BLC_NOT_RECEIVER = 0x1, 0x2, 0x4, 0x8
LOG_FILL = 0xA7  # log bytes no fold has written


def half(log_cap):
    return (log_cap // 2) & ~15


def cap_for(B):
    """The sizing rule: a log that always holds B bytes."""
    return 2 * B + 30


class Carry:
    def __init__(self, start=0, len=0, count=0, gaps=0, total=0, flen=()):
        self.start, self.len, self.count, self.gaps, self.total = start, len, count, gaps, total
        self.flen = (list(flen) + [0] * MAX)[:MAX]

    def copy(self):
        return Carry(self.start, self.len, self.count, self.gaps, self.total, self.flen)

    def pack(self):
        return (self.start.to_bytes(8, "little") + self.len.to_bytes(8, "little") +
                self.count.to_bytes(4, "little") + self.gaps.to_bytes(4, "little") +
                self.total.to_bytes(8, "little") + b"".join(f.to_bytes(8, "little") for f in self.flen) + bytes(32))

    def valid(self, H):  # 2
        return (self.start in (0, H) and self.len <= H and self.count <= MAX and
                sum(self.flen[:self.count]) == self.len)


class BRoom:
    """One room's backlog: the log's bytes, its carry, keep. log_null / bc_null:
    the pass-through forms."""

    def __init__(self, log_cap, keep=10, log_null=False, bc_null=False, carry=None):
        self.log_cap, self.keep, self.log_null, self.bc_null = log_cap, keep, log_null, bc_null
        self.log = bytearray([LOG_FILL]) * log_cap
        self.carry = carry or Carry()

    @property
    def H(self):
        return 0 if self.log_null else half(self.log_cap)

    def passthrough(self):  # 0
        return self.log_null or self.bc_null or self.keep == 0 or self.H == 0

    def held(self):
        """What a joiner is sent (9): a carry that names nothing readable counts as empty."""
        c, H = self.carry, self.H
        if c.start not in (0, H) or c.len > H:
            return b""
        return bytes(self.log[c.start:c.start + c.len])


def room_result(len=0, count=0, folded=0, dropped=0, status=0):
    return dict(len=len, count=count, folded=folded, dropped=dropped, status=status)


def pack_room_result(r):
    return (r["len"].to_bytes(8, "little") + r["count"].to_bytes(4, "little") + r["folded"].to_bytes(4, "little") +
            r["dropped"].to_bytes(4, "little") + r["status"].to_bytes(4, "little") + bytes(8))


def pack_result(r):
    return (r["send_len"].to_bytes(8, "little") + r["backlog_len"].to_bytes(8, "little") +
            r["status"].to_bytes(4, "little") + bytes(12))


def fold(br, sizes, wire, row, wire_cap=None):
    """One room's fold. sizes: the deliverable frames' sizes as recounted from
    the tables, in wire order; wire: the bytes the wire build wrote (its first
    min(wire_len, wire_cap)); row: the room row the caller passes (wire_len,
    nmsgs, status). Mutates br; returns (result row, why) with why the rule
    that decided."""
    if br.passthrough():
        return room_result(status=BL_PASSTHROUGH), "passthrough"
    c, H = br.carry, br.H
    keep = min(br.keep, MAX)
    N = row["nmsgs"]
    if N == 0:  # 1
        return room_result(c.len, c.count), "n0"
    st = 0
    old = c.copy()
    if not old.valid(H):
        st |= BL_BAD_CARRY
        old = Carry(gaps=c.gaps, total=c.total)
    cap = len(wire) if wire_cap is None else wire_cap
    why = None
    if len(sizes) != N or sum(sizes) != row["wire_len"]:  # 3
        st |= BL_MISMATCH | BL_GAP
        why = "mismatch"
    elif row["status"] & R.ROOM_TRUNCATED or row["wire_len"] > cap:  # 4
        st |= BL_GAP
        why = "truncated"
    if why:
        br.carry = Carry(gaps=old.gaps + 1, total=old.total)
        return room_result(0, 0, 0, old.count, st), why
    cand = [("old", s) for s in old.flen[:old.count]] + [("new", s) for s in sizes]  # 5
    taken, nbytes = [], 0
    for kind, s in reversed(cand):
        if len(taken) >= keep:
            break
        if nbytes + s > H:
            st |= BL_EVICTED | (0 if taken else BL_TOO_LONG)
            break
        taken.append((kind, s))
        nbytes += s
    taken.reverse()
    olds = [s for k, s in taken if k == "old"]
    news = [s for k, s in taken if k == "new"]
    b_old, b_new = sum(olds), sum(news)
    target = H if (taken and old.count and old.start == 0) else 0  # 6
    data = bytes(br.log[old.start + old.len - b_old:old.start + old.len]) + \
        bytes(wire[row["wire_len"] - b_new:row["wire_len"]])
    assert len(data) == nbytes
    br.log[target:target + nbytes] = data
    br.carry = Carry(target, nbytes, len(taken), old.gaps, old.total + len(news), olds + news)  # 7
    why = "too_long" if st & BL_TOO_LONG else "evicted" if st & BL_EVICTED else "kept"
    return room_result(nbytes, len(taken), len(news), old.count - len(olds), st), why


class JConn:
    """What one connection brings to the delivery: send_cap, the prefix its
    send buffer holds, its broadcast and reply rows (dicts or None), the room
    joined and whether it joins."""

    def __init__(self, send_cap=0, bcast=None, reply=None, room=R.NONE, join=False, out_null=False):
        self.send_cap, self.bcast, self.reply, self.room, self.join = send_cap, bcast, reply, room, join
        self.out_null = out_null

    @property
    def base(self):
        if self.bcast is not None:
            return self.bcast["send_len"]
        return self.reply["reply_len"] if self.reply is not None else 0

    def receiver(self):
        if self.reply is not None and self.reply["status"] & (R.RM.CLOSED | R.RM.OVERFLOW):
            return False
        return not (self.bcast is not None and self.bcast["status"] & R.BC_NOT_RECEIVER)


def deliver(jconns, brooms):
    """9: per connection (offset of the first written byte in out, the bytes written there, result dict)."""
    out = []
    for j in jconns:
        base, data, st = j.base, b"", 0
        cap = 0 if j.out_null else j.send_cap
        if j.join:
            if j.room >= len(brooms) or brooms[j.room].passthrough():
                st = BLC_NO_ROOM
            elif not j.receiver():
                st = BLC_NOT_RECEIVER
            else:
                data, st = brooms[j.room].held(), BLC_JOINED
        w = len(data)
        if st & BLC_JOINED and base + w > cap:
            st |= BLC_TRUNCATED
        lo, hi = min(base, cap), min(base + w, cap)
        out.append((lo, data[lo - base:hi - base] if hi > lo else b"",
                    dict(send_len=base + w, backlog_len=w, status=st)))
    return out


def sizes_of(conns, members):
    """The deliverable frames' sizes of a room, recounted from the tables (3)."""
    _, frames, _ = R.room_wire(conns, members, R.FIN | R.TEXT, 0)
    return [len(h) + len(p) for _, _, h, p in frames]


def backlog(conns, rooms, bres, brooms, jconns=None, rows=None):
    """The whole call on the models: conns, rooms and bres are a broadcast
    call's inputs and its R.Result; rows overrides the room rows passed.
    Returns (room rows, whys, delivery or None)."""
    rres, whys = [], []
    for r, (rm, br) in enumerate(zip(rooms, brooms)):
        written, _, rr, _ = bres.rooms[r]
        row = rr if rows is None or rows[r] is None else rows[r]
        cap = 0 if rm.wire_null else (rr["wire_len"] if rm.wire_cap is None else rm.wire_cap)
        res, why = fold(br, sizes_of(conns, rm.members), written, row, cap)
        rres.append(res)
        whys.append(why)
    return rres, whys, (deliver(jconns, brooms) if jconns is not None else None)


class Coverage:
    """Counts of the situations the tests must reach (on the model)."""
    KEYS = ("passthrough", "n0", "bad_carry", "mismatch", "truncated", "evicted", "too_long", "kept", "keep_ended",
            "old_kept", "old_dropped", "to_half0", "to_halfH", "hdr2", "hdr4", "hdr10", "joined", "join_truncated",
            "join_no_room", "join_not_receiver", "non_joiner", "empty_join")

    def __init__(self):
        self.n = dict.fromkeys(self.KEYS, 0)

    def add_fold(self, br, res, why, sizes=()):
        self.n[why] += 1
        self.n["bad_carry"] += bool(res["status"] & BL_BAD_CARRY)
        if why in ("kept", "evicted"):
            self.n["keep_ended"] += res["count"] == min(br.keep, MAX) and not res["status"] & BL_EVICTED
            self.n["old_kept"] += res["count"] > res["folded"]
            self.n["old_dropped"] += res["dropped"] > 0
            if res["count"]:
                self.n["to_halfH" if br.carry.start else "to_half0"] += 1
            for s in sizes:
                p = s - 2 if s - 2 < 126 else s - 4 if s - 4 <= 0xFFFF else s - 10
                self.n["hdr%d" % (s - p)] += 1
        return self

    def add_delivery(self, jconns, dl):
        for j, (_, _, r) in zip(jconns, dl):
            st = r["status"]
            self.n["joined"] += bool(st & BLC_JOINED)
            self.n["join_truncated"] += bool(st & BLC_TRUNCATED)
            self.n["join_no_room"] += bool(st & BLC_NO_ROOM)
            self.n["join_not_receiver"] += bool(st & BLC_NOT_RECEIVER)
            self.n["non_joiner"] += not j.join
            self.n["empty_join"] += bool(st & BLC_JOINED) and r["backlog_len"] == 0
        return self

    def require(self, *keys):
        missing = [k for k in (keys or self.KEYS) if not self.n[k]]
        assert not missing, (missing, self.n)


# --------------------------------------------------------------------------- scenarios
def talk(lengths_per_member, heads=None):
    """One room whose members each speak messages of the given lengths:
    (conns, rooms) for R.broadcast."""
    conns = [R.speaker(ls, head=(heads[k] if heads else None), room=0) for k, ls in enumerate(lengths_per_member)]
    return conns, [R.Room(range(len(conns)))]


def run_sweeps(br, sweeps, cov=None, wire_cap=None):
    """Fold a sequence of sweeps (each a list of per-member length lists) into
    br. Returns per sweep (result, why, frames as bytes)."""
    out = []
    for lens in sweeps:
        conns, rooms = talk(lens)
        rooms[0].wire_cap = wire_cap
        bres = R.broadcast(conns, rooms)
        rres, whys, _ = backlog(conns, rooms, bres, [br])
        frames = [h + p for _, _, h, p in bres.rooms[0][1]]
        if cov is not None:
            cov.add_fold(br, rres[0], whys[0], [len(f) for f in frames])
        out.append((rres[0], whys[0], frames))
    return out


# --------------------------------------------------------------------------- cases for the device test
class Call:
    """One xyws_backlog_streams call after a broadcast over conns and rooms.
    jconns: one JConn per connection or None (a null dev_jconns); a JConn's
    use_bcast / use_reply say which of the connection's rows it names; rows:
    per room a row dict passed in place of the broadcast's, or None."""

    def __init__(self, conns, rooms, jconns=None, rows=None, kw=None):
        self.conns, self.rooms, self.jconns, self.rows, self.kw = conns, rooms, jconns, rows, kw or {}


class Case:
    """Calls that share their rooms' logs and carries. lmis: the misalignment
    of each log, None: the logs abut."""

    def __init__(self, name, brooms, calls, lmis=None):
        self.name, self.brooms, self.calls, self.lmis = name, brooms, calls, lmis


def joiner(conn, room, join=True, use_bcast=True, use_reply=True, send_cap=None):
    j = JConn(conn.send_cap if send_cap is None else send_cap, room=room, join=join)
    j.use_bcast, j.use_reply = use_bcast, use_reply
    return j


def resolve(call, bres):
    """The rows a call's JConns name, out of the broadcast's results."""
    if call.jconns is None:
        return None
    for k, (j, c) in enumerate(zip(call.jconns, call.conns)):
        j.bcast = bres.conns[k][2] if j.use_bcast else None
        j.reply = c.reply if j.use_reply else None
    return call.jconns


def run_call(case, call, cov=None):
    """The model over one call; mutates the case's rooms. Returns (broadcast
    result, room rows, whys, delivery or None)."""
    bres = R.broadcast(call.conns, call.rooms, **{k: v for k, v in call.kw.items() if k in ("flags", "enc_opts")})
    jc = resolve(call, bres)
    rres, whys, dl = backlog(call.conns, call.rooms, bres, case.brooms, jc, call.rows)
    if cov is not None:
        for r, br in enumerate(case.brooms):
            cov.add_fold(br, rres[r], whys[r], sizes_of(call.conns, call.rooms[r].members)
                         if whys[r] in ("kept", "evicted") else ())
        if dl is not None:
            cov.add_delivery(jc, dl)
    return bres, rres, whys, dl


def filled(br, start, flens, salt=0):
    """br with a hand-made valid carry of the given frame lengths, the held bytes some text."""
    n = sum(flens)
    br.log[start:start + n] = R.text(n, salt)
    br.carry = Carry(start, n, len(flens), 0, len(flens), flens)
    return br


OLD_SUFFIX = (0, 1, 15, 16, 17, 33)


def fold_seams():
    """Log misaligned 0..15 x the new suffix's start in the wire mod 16 x an
    old suffix of OLD_SUFFIX bytes; three new frames of 3..40 bytes: all
    three behind a surviving old frame, the last two when there is none (an old
    frame survives only when every new one is taken); the old half alternates."""
    conns, rooms, brooms, lmis = [], [], [], []
    for a in range(16):
        for w in range(16):
            for o in OLD_SUFFIX:
                r = len(rooms)
                lens = [1 + (a + 3 * w + o) % 38, 1 + (5 * a + w + 2 * o) % 38, 1 + (a * w + o) % 38]
                c = R.speaker(lens, room=r)
                c.bmis = (a + w + o) % 16
                conns.append(c)
                rm = R.Room([r])
                rm.wmis = w if o else (w - (2 + lens[0])) % 16
                rooms.append(rm)
                br = BRoom(320 + (r % 7), keep=4 if o else 2)
                x = 3 + (5 * a + w) % 16
                filled(br, br.H * ((a + w + o) % 2), [x, o] if o else [x], r)
                brooms.append(br)
                lmis.append(a)
    R.size_sends(conns, rooms)
    return Case("fold_seams", brooms, [Call(conns, rooms)], lmis)


def frame_sizes():
    """head_len + length at 125, 126, 65 535 and 65 536, with a head and without."""
    conns, rooms, brooms = [], [], []
    for total in (125, 126, 65535, 65536):
        for head in (None, R.HEAD24):
            r = len(rooms)
            conns.append(R.speaker([7, total - len(head or b"")], head=head, room=r))
            rooms.append(R.Room([r]))
            brooms.append(filled(BRoom(cap_for(66000), keep=2), 0, [5], r))
    R.size_sends(conns, rooms)
    return Case("frame_sizes", brooms, [Call(conns, rooms)], [3 * r for r in range(len(rooms))])


def member_tiles(T):
    """Rooms of T - 1, T, T + 1 and 2T + 3 members (speakers with 1, 0, 3 and 5
    records, every skip status among them), a members[] entry >= n, and two
    rooms in which one member alone holds more than keep records."""
    conns, rooms, brooms = [], [], []
    for size in (T - 1, T, T + 1, 2 * T + 3):
        lo = len(conns)
        for k in range(size):
            cnt = (1, 0, 3, 5)[k % 4]
            sts = [R.SKIPS[(k + j) % len(R.SKIPS)] if (k + j) % 3 == 0 else R.M.COMPLETE for j in range(cnt)]
            conns.append(R.speaker([(3 * k + 5 * j) % 23 for j in range(cnt)], head=R.HEAD24[:k % 25] or None,
                                   statuses=sts, room=len(rooms), gap=k % 4))
        rooms.append(R.Room(range(lo, lo + size)))
        brooms.append(filled(BRoom(cap_for(800), keep=10), 0, [4, 9], size))
    lo = len(conns)
    conns += [R.speaker([3], room=len(rooms)), R.speaker(list(range(1, 21)), room=len(rooms)),
              R.speaker([], room=len(rooms))]
    rooms.append(R.Room([lo, 0xFFFFFFFE, lo + 1, lo + 2]))
    brooms.append(BRoom(cap_for(800), keep=10))
    conns += [R.speaker([6, 5, 4, 3, 2], room=len(rooms)), R.speaker([9], room=len(rooms), rsm_status=R.SM.RSM_OVERFLOW)]
    rooms.append(R.Room([lo + 3, lo + 4]))
    brooms.append(BRoom(cap_for(100), keep=3))
    R.size_sends(conns, rooms)
    return Case("member_tiles", brooms, [Call(conns, rooms, kw=dict(packed=True))])


def rules():
    """Every status bit and every clear path over four chained calls; the logs abut."""
    plan = [  # (room, per-sweep talk)
        (BRoom(cap_for(700), keep=1), [[[3, 4]], [[5]], [[6], [7]], [[8]]]),
        (BRoom(cap_for(700), keep=10), [[[3, 4]], [[5] * 6], [[6], [7]], [[8] * 5]]),
        (BRoom(cap_for(700), keep=16), [[[3] * 9], [[5] * 6], [[6] * 3, [7]], [[8]]]),
        (BRoom(cap_for(700), keep=17), [[[3] * 9], [[5] * 9], [[6] * 17], [[8]]]),
        (BRoom(203, log_null=True), [[[3]]] * 4),
        (BRoom(203, bc_null=True), [[[3]]] * 4),
        (BRoom(203, keep=0), [[[3]]] * 4),
        (BRoom(31), [[[3]]] * 4),
        (BRoom(2 * 48 + 9), [[[10, 10, 10]], [[11]], [[46]], [[4, 47]]]),
        (BRoom(cap_for(90)), [[[5, 6]], [[]], [[7]], [[]]]),
        (filled(BRoom(cap_for(90)), 16, [5]), [[[5]], [[6]], [[7]], [[8]]]),
        (BRoom(cap_for(90)), [[[5]], [[6]], [[7]], [[8]]]),   # 11: nmsgs + 1 in sweep 2
        (BRoom(cap_for(90)), [[[5]], [[6]], [[7]], [[8]]]),   # 12: wire_len - 1 in sweep 3
        (BRoom(cap_for(90)), [[[5]], [[6]], [[7]], [[8]]]),   # 13: a short wire in sweep 2
        (filled(BRoom(cap_for(90)), 0, [5]), [[[5]], [[6]], [[7]], [[8]]]),
        (filled(BRoom(cap_for(90)), 0, [5, 4]), [[[5]], [[6]], [[7]], [[8]]]),
        (filled(BRoom(cap_for(90)), 0, [5]), [[[5]], [[6]], [[7]], [[8]]]),
    ]
    plan[14][0].carry.count = MAX + 1
    plan[15][0].carry.flen[1] = 3
    plan[16][0].carry.len = plan[16][0].H + 1
    brooms = [p[0] for p in plan]
    calls = []
    for s in range(4):
        conns, rooms = [], []
        for r, (_, talks) in enumerate(plan):
            lo = len(conns)
            conns += [R.speaker(ls, room=r, head=R.HEAD24[:r % 8] or None) for ls in talks[s]]
            rm = R.Room(range(lo, len(conns)))
            if r == 13 and s == 1:
                rm.wire_cap = 5
            rooms.append(rm)
        R.size_sends(conns, rooms)
        rows = [None] * len(plan)
        bres = R.broadcast(conns, rooms)
        if s == 1:
            rows[11] = dict(bres.rooms[11][2], nmsgs=bres.rooms[11][2]["nmsgs"] + 1)
        if s == 2:
            rows[12] = dict(bres.rooms[12][2], wire_len=bres.rooms[12][2]["wire_len"] - 1)
        calls.append(Call(conns, rooms, rows=rows))
    return Case("rules", brooms, calls)


def over_grid(G):
    """More rooms and more connections than the grid cap plus 3, all tiny; every third connection joins."""
    conns, rooms, _ = R.over_grid(G)
    brooms = [BRoom(64 + k % 5, keep=1 + k % 3) for k in range(len(rooms))]
    for c in conns:
        c.send_cap += 9
    jc = [joiner(c, (k + 1) % len(rooms), join=k % 3 == 0) for k, c in enumerate(conns)]
    return Case("over_grid", brooms, [Call(conns, rooms, jc, kw=dict(packed=True))])


LENGTHS = tuple(range(1, 41)) + (4096 + 16 + 5,)


def delivery_matrix():
    """(out + base) misaligned 0..15 x (log + start) misaligned 0..15, backlogs of LENGTHS bytes; nobody speaks."""
    conns, rooms, brooms, lmis, jc = [], [], [], [], []
    for a in range(16):
        for n in LENGTHS:
            r = len(rooms)
            br = BRoom(cap_for(n) + r % 3)
            brooms.append(filled(br, br.H * (r % 2), [n], r))
            lmis.append(a)
            lo = len(conns)
            for m in range(16):
                base = (3 * m + r) % 11
                c = R.Conn(room=R.NONE, reply=R.reply_row(base) if base else None, send_cap=base + n + m % 3,
                           prefix=R.text(base, 5))
                c.smis = m
                conns.append(c)
                jc.append(joiner(c, r, use_bcast=(m + r) % 2 == 0))
            rooms.append(R.Room([]))
    return Case("delivery_matrix", brooms, [Call(conns, rooms, jc)], lmis)


def delivery_rules():
    """One spoken-in room and one backlog of 35 + 12 bytes: out_cap below, at
    and above base and send_len, in a packed slab; closed and overflowed
    replies; bcast and reply null in every combination; non-joiners; rooms
    that do not exist or pass through."""
    sp = R.speaker([9], head=R.HEAD24, room=0)
    conns, jc = [sp], [joiner(sp, 0, join=False)]
    brooms = [filled(BRoom(cap_for(64)), 0, [12]), BRoom(100, keep=0), BRoom(100)]
    flen = 35 + 12
    sp.send_cap = 35
    for base in (0, 6):
        for k in range(-1, 35 + flen + 2):
            c = R.Conn(room=0, reply=R.reply_row(base) if base else None, send_cap=max(base + k, 0),
                       prefix=R.text(base, 5))
            conns.append(c)
            jc.append(joiner(c, 0))
    for ub in (False, True):
        for ur in (False, True):
            for st in (0, R.RM.CLOSED, R.RM.OVERFLOW, R.RM.TRUNCATED):
                for join in (False, True):
                    c = R.Conn(room=0, reply=R.reply_row(5, status=st, code=1000 if st == R.RM.CLOSED else 0),
                               send_cap=5 + 35 + flen + 1, prefix=R.text(5, 5))
                    conns.append(c)
                    jc.append(joiner(c, 0, join=join, use_bcast=ub, use_reply=ur))
    for room in (1, 2, 3, R.NONE):  # pass-through, empty, not there, none
        c = R.Conn(room=0, send_cap=35 + flen)
        conns.append(c)
        jc.append(joiner(c, room))
    rooms = [R.Room(range(len(conns))), R.Room([]), R.Room([])]
    case = Case("delivery_rules", brooms, [Call(conns, rooms, jc, kw=dict(packed=True)),
                                           Call(conns, rooms, None, kw=dict(packed=True))])
    return case


def all_cases(T, G):
    return [fold_seams(), frame_sizes(), member_tiles(T), rules(), over_grid(G), delivery_matrix(), delivery_rules()]


# --------------------------------------------------------------------------- the real sweep
def sweep_streams():
    """R.sweep_streams() (sweep 2 completes a message that spans sweeps 1 and
    2) and a third sweep. Connection 8, outside every room before, joins room
    0 in sweep 2 and is its member in sweep 3. Returns (pieces per sweep,
    descriptor caps, member lists per sweep, room of each per sweep, joiners
    per sweep as (connection, room) pairs)."""
    sweeps, caps, members, room_of = R.sweep_streams()
    rng = R.streams.SplitMix(0xB10C)
    s3 = [R._f(rng, 0x81, b"third sweep"), b"", b"", b"", R._f(rng, 0x81, b"more from four") + R._f(rng, 0x81, b"and more"),
          R._f(rng, 0x81, b"room one talks"), b"", b"", R._f(rng, 0x81, b"the newcomer speaks")]
    joined = [members[0] + [8], members[1]]
    return (sweeps + [s3], caps, [members, members, joined], [room_of, room_of, room_of[:8] + [0]],
            [[], [(8, 0)], []])


def real_jconns(vconns, res, joiners):
    """The delivery's connections of one real sweep: every row named, the joiners flagged."""
    out = []
    for i, c in enumerate(vconns):
        room = dict(joiners).get(i, R.NONE)
        j = JConn(c.send_cap, bcast=res.conns[i][2], reply=c.reply, room=room, join=i in dict(joiners))
        out.append(j)
    return out

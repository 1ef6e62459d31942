"""Plain-Python model of xyws_roster_streams (include/xyws.h states the
semantics; the rule numbers below are the header's): the events of a sweep,
every room's member list after it, the notice wires and what each connection is
sent. Below it, the scenarios shared by the CPU test (tests/test_roster_model.py)
and the device test (tests/test_gpu_roster.py)."""
NONE = 0xFFFFFFFF
NAME_MAX, TEXT_MAX = 256, 32
FIN, TEXT = 0x10, 0x01
JOIN, LEAVE, JOIN_ON_ACCEPT, LEAVE_ON_CLOSE = 0x1, 0x2, 0x4, 0x8
RS_TRUNCATED, RS_FULL, RS_BAD_MEMBER = 0x10, 0x20, 0x40
(RSC_TRUNCATED, RSC_NOT_RECEIVER, RSC_NO_ROOM, RSC_MEMBER, RSC_JOINED, RSC_LEFT, RSC_FULL, RSC_ALREADY,
 RSC_BAD_NAME) = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40, 0x80, 0x100
RPL_TRUNCATED, RPL_CLOSED, RPL_OVERFLOW = 0x1, 0x2, 0x4
BC_TRUNCATED, BC_NOT_RECEIVER, BC_NO_ROOM = 0x1, 0x2, 0x4
ACC_ACCEPTED, ACC_REJECTED, ACC_TRUNCATED = 0x1, 0x2, 0x4
BL_JOIN = 0x1


class Text:
    def __init__(self, head, joined, left):
        self.head, self.joined, self.left = bytes(head), bytes(joined), bytes(left)


# byte for byte the reference's strings (example/websocket/websocket_chat.cpp:51-52, 68-69)
REF = Text(b"|        SERVER       |:", b" has joined the chat\n", b" has left the chat\n")


def header(flags, L):
    """The server frame header xyws_broadcast_streams builds, for L < 65 536."""
    b0 = (0x80 if flags & FIN else 0) | (flags & 0x0F)
    return bytes([b0, L]) if L < 126 else bytes([b0, 126, L >> 8, L & 0xFF])


def notice(flags, text, name, tail):
    body = text.head + name + tail
    return header(flags, len(body)) + body


class Conn:
    """What one connection brings to the call: its name (None: a null
    pointer; name_len overrides the length the row states), its send buffer
    (send_cap, out_null, the prefix it holds), this sweep's rows (dicts or
    None), the room it asks for and its flags, and cur: dev_bconns[i].room."""

    def __init__(self, name=b"", flags=0, room=NONE, cur=NONE, send_cap=0, bcast=None, reply=None, accept=None,
                 name_len=None, out_null=False, prefix=b""):
        self.name, self.flags, self.room, self.cur, self.send_cap = name, flags, room, cur, send_cap
        self.bcast, self.reply, self.accept, self.out_null, self.prefix = bcast, reply, accept, out_null, prefix
        self.name_len = (0 if name is None else len(name)) if name_len is None else name_len

    @property
    def base(self):  # 4
        if self.bcast is not None:
            return self.bcast["send_len"]
        if self.reply is not None:
            return self.reply["reply_len"]
        if self.accept is not None:
            return self.accept["resp_len"] if self.accept["status"] & (ACC_ACCEPTED | ACC_REJECTED) else 0
        return 0

    def notice_name(self):  # 1: a null name or a length above NAME_MAX counts as 0
        if self.name is None or self.name_len > NAME_MAX:
            return b""
        return bytes(self.name[:self.name_len])


class Room:
    """members: dev_rooms[r].members[0 .. n_members); member_cap; notes_cap
    (None: as long as the notices need); the null forms."""

    def __init__(self, members=(), member_cap=None, notes_cap=None, notes_null=False, members_null=False, seen=True):
        self.members = list(members)
        self.member_cap = len(self.members) if member_cap is None else member_cap
        self.notes_cap, self.notes_null, self.members_null = notes_cap, notes_null, members_null
        self.seen = seen  # a `seen` row is named: it receives the list as the call found it (5.)


def bcast_row(send_len, status=0):
    return dict(send_len=send_len, status=status)


def reply_row(reply_len, status=0):
    return dict(reply_len=reply_len, status=status)


def accept_row(status, resp_len):
    return dict(status=status, resp_len=resp_len)


class Result:
    """rooms: per room (notes bytes written, row dict, the list after the
    call); conns: per connection (offset of the first written byte in out, the
    bytes written there, row dict); cur: dev_bconns[i].room after the call;
    jconns: per connection (room, flags) of the backlog's word; want: the events
    as ('leave' | room | None)."""

    def __init__(self):
        self.rooms, self.conns, self.cur, self.jconns, self.want, self.seen = [], [], [], [], [], []


def roster(conns, rooms, text=REF, flags=FIN | TEXT):
    n, nr = len(conns), len(rooms)
    res = Result()
    st, room_of, leaves, receiver = [0] * n, [NONE] * n, [False] * n, [True] * n
    for i, c in enumerate(conns):  # 1
        closed = c.reply is not None and c.reply["status"] & RPL_CLOSED
        leave = bool(c.flags & LEAVE or (c.flags & LEAVE_ON_CLOSE and closed))
        on_accept = bool(c.flags & JOIN_ON_ACCEPT) and c.accept is not None
        accepted = on_accept and bool(c.accept["status"] & ACC_ACCEPTED)
        joins = not leave and c.room < nr and bool(c.flags & JOIN or accepted)
        member = c.cur < nr
        if c.name is not None and c.name_len > NAME_MAX:  # (a null name's length is not looked at)
            st[i] |= RSC_BAD_NAME
        want = None
        if leave:
            want = "leave"
        else:
            if member:
                st[i] |= RSC_MEMBER
                room_of[i] = c.cur
            if joins:
                if member:
                    st[i] |= RSC_ALREADY
                else:
                    want = c.room
        leaves[i] = leave
        res.want.append(want)
        rcv = not leave  # 4
        if c.reply is not None and c.reply["status"] & (RPL_CLOSED | RPL_OVERFLOW):
            rcv = False
        if c.bcast is not None and c.bcast["status"] & BC_NOT_RECEIVER:
            rcv = False
        if on_accept and not accepted:
            rcv = False
        receiver[i] = rcv
    asking = {}
    for i, w in enumerate(res.want):
        if w is not None and w != "leave":
            asking.setdefault(w, []).append(i)
    res.cur = [c.cur for c in conns]
    res.jconns = [(NONE, 0)] * n
    note_off = [0] * n
    notes_all = []
    for r, rm in enumerate(rooms):  # 2, 3
        old = [] if rm.members_null else rm.members
        kept, wire, status, left = [], b"", 0, 0
        for m in old:
            if m >= n:
                status |= RS_BAD_MEMBER
            elif leaves[m]:
                left += 1
                wire += notice(flags, text, conns[m].notice_name(), text.left)
                st[m] |= RSC_LEFT
                room_of[m] = r
                res.cur[m] = NONE
            else:
                kept.append(m)
        welcome_off = len(wire)
        cap = 0 if rm.members_null else rm.member_cap
        joiners = asking.get(r, [])  # (ascending table index)
        admitted = joiners[:max(cap - len(kept), 0)]
        for i in joiners[len(admitted):]:
            st[i] |= RSC_FULL
            status |= RS_FULL
        for i in admitted:
            note_off[i] = len(wire)
            wire += notice(flags, text, conns[i].notice_name(), text.joined)
            st[i] |= RSC_JOINED
            room_of[i] = r
            res.cur[i] = r
            res.jconns[i] = (r, BL_JOIN)
        ncap = 0 if rm.notes_null else len(wire) if rm.notes_cap is None else rm.notes_cap
        if len(wire) > ncap:
            status |= RS_TRUNCATED
        members = kept + admitted
        row = dict(notes_len=len(wire), welcome_off=welcome_off, joined=len(admitted), left=left,
                   n_members=len(members), status=status)
        res.rooms.append((wire[:ncap], row, members))
        res.seen.append(list(old[:cap]) if rm.seen else None)  # 5: for this sweep's backlog fold
        notes_all.append((wire, ncap))
    for i, c in enumerate(conns):  # 4
        base, data, off = c.base, b"", note_off[i]  # (an admitted joiner's: where its welcome begins, sent or not)
        cap = 0 if c.out_null else c.send_cap
        if not receiver[i]:
            st[i] |= RSC_NOT_RECEIVER
        elif st[i] & (RSC_MEMBER | RSC_JOINED):
            wire, ncap = notes_all[room_of[i]]
            data = wire[:ncap][off:]
        else:
            st[i] |= RSC_NO_ROOM
        if base + len(data) > cap:
            st[i] |= RSC_TRUNCATED
        lo, hi = min(base, cap), min(base + len(data), cap)
        res.conns.append((lo, data[lo - base:hi - base] if hi > lo else b"",
                          dict(send_len=base + len(data), note_len=len(data), status=st[i], room=room_of[i],
                               note_off=off)))
    return res


def apply(conns, rooms, res):
    """The resident tables after the call: the next sweep reads them."""
    for c, cur in zip(conns, res.cur):
        c.cur = cur
    for rm, (_, _, members) in zip(rooms, res.rooms):
        if not rm.members_null:
            rm.members = list(members)


def pack_room_result(r):
    return (r["notes_len"].to_bytes(8, "little") + r["welcome_off"].to_bytes(8, "little") +
            r["joined"].to_bytes(4, "little") + r["left"].to_bytes(4, "little") +
            r["n_members"].to_bytes(4, "little") + r["status"].to_bytes(4, "little"))


def pack_result(r):
    return (r["send_len"].to_bytes(8, "little") + r["note_len"].to_bytes(8, "little") +
            r["status"].to_bytes(4, "little") + r["room"].to_bytes(4, "little") + r["note_off"].to_bytes(8, "little"))


# --------------------------------------------------------------------------- the reference's room, restated
class RefRoom:
    """chat_room (websocket_chat.cpp:31-105) without its messages: a
    participant list, join (insert, the welcome to everyone including the
    newcomer) and leave (erase, the farewell to the rest). sent[i]: what
    participant i's writer sends, frame after frame."""

    def __init__(self, names, flags=FIN | TEXT):
        self.names, self.flags, self.participants, self.sent = names, flags, [], {}

    def _say(self, line):
        frame = header(self.flags, len(line)) + line
        for p in self.participants:
            self.sent[p] = self.sent.get(p, b"") + frame

    def join(self, i):
        self.participants.append(i)
        self._say(REF.head + self.names[i] + REF.joined)

    def leave(self, i):
        self.participants.remove(i)
        self._say(REF.head + self.names[i] + REF.left)


# --------------------------------------------------------------------------- scenarios
def name_of(i, length=None):
    """An address text like socket_address::to_str()'s, or `length` bytes that differ per i."""
    if length is None:
        return b"10.%d.%d.%d:%d" % (i >> 16 & 255, i >> 8 & 255, i & 255, 40000 + i % 20000)
    return bytes((0x41 + (i * 7 + k * 3) % 53) for k in range(length))


def ample(conns, rooms, text=REF, flags=FIN | TEXT, limit=None):
    """Send buffers that hold exactly what the call appends; limit(i): a smaller cap for connection i, or None."""
    for c in conns:
        c.send_cap = 1 << 60
    res = roster(conns, rooms, text, flags)
    for i, (c, (_, _, row)) in enumerate(zip(conns, res.conns)):
        c.send_cap = row["send_len"]
        if limit is not None and limit(i) is not None:
            c.send_cap = min(c.send_cap, limit(i))
    return conns, rooms


class Case:
    """One call (or a chain of calls on the same tables). nmis / smis / wmis:
    the misalignment of each name, send buffer and notice buffer (None: they
    abut)."""

    def __init__(self, name, conns, rooms, text=REF, flags=FIN | TEXT, nmis=None, smis=None, wmis=None, jconns=True):
        self.name, self.conns, self.rooms, self.text, self.flags = name, conns, rooms, text, flags
        self.nmis, self.smis, self.wmis, self.jconns = nmis, smis, wmis, jconns


def member_counts(T):
    """Rooms of 0, 1, T - 1, T, T + 1 and 2T + 1 members with leavers at the
    first, the last and both seam positions of a tile; a room that all leave;
    an empty room that T + 1 join; a bad entry."""
    conns, rooms = [], []
    for size in (0, 1, T - 1, T, T + 1, 2 * T + 1):
        lo, r = len(conns), len(rooms)
        gone = {0, size - 1, T - 1, T, 2 * T - 1, 2 * T} if size else set()
        for k in range(size):
            conns.append(Conn(name_of(lo + k), LEAVE if k in gone else 0, cur=r))
        rooms.append(Room(range(lo, lo + size)))
    lo, r = len(conns), len(rooms)
    conns += [Conn(name_of(lo + k), LEAVE, cur=r) for k in range(T + 3)]
    rooms.append(Room(range(lo, lo + T + 3)))
    lo, r = len(conns), len(rooms)
    first = lo
    conns += [Conn(name_of(lo + k), JOIN, room=r) for k in range(T + 1)]
    rooms.append(Room([], member_cap=T + 1))
    lo, r = len(conns), len(rooms)
    conns += [Conn(name_of(lo + k), LEAVE if k == 1 else 0, cur=r) for k in range(3)]
    rooms.append(Room([lo, 0xFFFFFFFE, lo + 1, len(conns) + 5, lo + 2]))
    # (of the T + 1 newcomers every 97th and the last have room for all they are sent)
    return Case("member_counts", *ample(conns, rooms, limit=lambda i: 70 if first <= i < first + T and (i - first) % 97 else None))


def joiner_scan(n, S):
    """n connections; joiners at index 0 and n - 1 and around every seam of the
    scan's step S, alternating between two rooms; one member in each room."""
    conns = [Conn(name_of(i)) for i in range(n)]
    rooms = [Room([], member_cap=n), Room([], member_cap=n)]
    picks = sorted({0, n - 1} | {k for s in range(S, n, S) for k in (s - 1, s) if 0 <= k < n})
    for t, i in enumerate(picks):
        conns[i].flags, conns[i].room = JOIN, t % 2
    for r in (0, 1):  # a member that stays, where there is a free slot
        free = [i for i in range(n) if not conns[i].flags and conns[i].cur == NONE]
        if free:
            conns[free[len(free) // 2]].cur = r
            rooms[r].members = [free[len(free) // 2]]
    return Case("joiner_scan_%d" % n, *ample(conns, rooms))


def member_caps():
    """member_cap exactly reached, exceeded by one and by many; a leaver frees a slot in the same sweep."""
    conns, rooms = [], []
    for extra, joiners in ((0, 3), (1, 3), (9, 3), (0, 0)):
        lo, r = len(conns), len(rooms)
        conns += [Conn(name_of(lo + k), LEAVE if k == 1 else 0, cur=r) for k in range(4)]
        conns += [Conn(name_of(lo + 4 + k), JOIN, room=r) for k in range(joiners + extra)]
        rooms.append(Room(range(lo, lo + 4), member_cap=max(3 + joiners, 4), seen=extra != 1))
    lo, r = len(conns), len(rooms)
    conns += [Conn(name_of(lo + k), JOIN, room=r) for k in range(2)]
    rooms.append(Room([], members_null=True))
    return Case("member_caps", *ample(conns, rooms))


NAME_LENGTHS = (0, 1, 15, 16, 17, 256, 257)


def header_seam_lengths(text=REF):
    """The name lengths either side of L = 125 / 126, for the welcome and the farewell."""
    return sorted({125 - len(text.head) - len(t) + d for t in (text.joined, text.left) for d in (0, 1)})


def name_lengths():
    """One room per name length: a member with that name leaves and a joiner
    with it joins; a null name; every alignment of names, notes and out."""
    conns, rooms, nmis, smis, wmis = [], [], [], [], []
    lengths = list(NAME_LENGTHS) + header_seam_lengths() + [None]
    for a in range(16):
        for k, ln in enumerate(lengths):
            lo, r = len(conns), len(rooms)
            nm = None if ln is None else name_of(lo, ln)
            kw = dict(name_len=7) if ln is None else {}
            conns += [Conn(name_of(lo), cur=r), Conn(nm, LEAVE, cur=r, **kw), Conn(nm, JOIN, room=r, **kw)]
            rooms.append(Room([lo, lo + 1], member_cap=2))
            nmis += [a, (a + k) % 16, (a + 5 * k + 3) % 16]
            smis += [(a + 3 * k) % 16, 0, (a + 7 * k + 1) % 16]
            wmis.append((a + 11 * k) % 16 if k % 2 else a)
    return Case("name_lengths", *ample(conns, rooms), nmis=nmis, smis=smis, wmis=wmis)


def notes_caps():
    """A leaver and two joiners per room; notes_cap 0, inside the first header,
    inside a name, exact, exact + 1 and at every byte between; a null notes; a
    member whose out_cap cuts inside what it is sent, at every byte."""
    conns, rooms = [], []
    full = len(notice(FIN | TEXT, REF, name_of(0), REF.left)) + 2 * len(notice(FIN | TEXT, REF, name_of(0), REF.joined))

    def room(notes_cap, notes_null=False, send_cap=None):
        lo, r = len(conns), len(rooms)
        conns.extend([Conn(name_of(0), cur=r, reply=reply_row(3), prefix=b"abc"), Conn(name_of(0), LEAVE, cur=r),
                      Conn(name_of(0), JOIN, room=r), Conn(name_of(0), JOIN, room=r)])
        rooms.append(Room([lo, lo + 1], member_cap=4, notes_cap=notes_cap, notes_null=notes_null))
        for c in conns[lo:]:
            c.send_cap = c.base + full + 2 if send_cap is None else send_cap
    for cap in range(0, full + 2):
        room(cap)
    room(full, notes_null=True)
    for cap in range(0, 3 + full + 2):
        room(None, send_cap=cap)
    return Case("notes_caps", conns, rooms)


def bases():
    """Each source of base, the receivers and the non-receivers, in one room of members and one of joiners."""
    conns = []
    rows = [dict(), dict(accept=accept_row(ACC_ACCEPTED, 129)), dict(accept=accept_row(ACC_REJECTED, 66)),
            dict(accept=accept_row(0, 77)), dict(reply=reply_row(9)), dict(reply=reply_row(9), accept=accept_row(1, 129)),
            dict(bcast=bcast_row(40)), dict(bcast=bcast_row(40), reply=reply_row(9), accept=accept_row(1, 129)),
            dict(reply=reply_row(4, RPL_CLOSED)), dict(reply=reply_row(4, RPL_OVERFLOW)), dict(reply=reply_row(4, RPL_TRUNCATED)),
            dict(bcast=bcast_row(11, BC_NOT_RECEIVER)), dict(bcast=bcast_row(11, BC_TRUNCATED | BC_NO_ROOM))]
    for kw in rows:  # members of room 0 that stay (a closed one leaves only with LEAVE_ON_CLOSE)
        conns.append(Conn(name_of(len(conns)), cur=0, **kw))
    for kw in rows:
        conns.append(Conn(name_of(len(conns)), LEAVE_ON_CLOSE, cur=0, **kw))
    members = list(range(len(conns)))
    for kw in rows:  # joiners of room 1, by flag and on accept
        conns.append(Conn(name_of(len(conns)), JOIN, room=1, **kw))
    for kw in rows:
        conns.append(Conn(name_of(len(conns)), JOIN_ON_ACCEPT, room=1, **kw))
    conns += [Conn(name_of(1), JOIN | LEAVE, room=1, cur=0),      # leave wins
              Conn(name_of(2), JOIN, room=1, cur=0),              # already a member
              Conn(name_of(3), JOIN, room=2), Conn(name_of(4), JOIN, room=NONE),  # no such room
              Conn(name_of(5), LEAVE), Conn(name_of(6), 0),       # a leaver nobody lists; nothing at all
              Conn(name_of(7), JOIN, room=1, out_null=True)]
    members += [len(conns) - 7, len(conns) - 6]
    for c in conns:
        c.prefix = name_of(9, min(c.base, 200))
    rooms = [Room(members, member_cap=len(members)), Room([], member_cap=len(conns))]
    return Case("bases", *ample(conns, rooms))


def custom_text():
    """Strings of 0 and 32 bytes, a binary frame without FIN; no dev_jconns."""
    t = Text(b"", bytes(range(0x30, 0x50)), bytes(range(0x50, 0x70)))
    conns = [Conn(name_of(0, 40), cur=0), Conn(name_of(1, 99), LEAVE, cur=0), Conn(name_of(2, 61), JOIN, room=0)]
    return Case("custom_text", *ample(conns, [Room([0, 1], member_cap=2)], t, 0x02), text=t, flags=0x02, jconns=False)


def over_grid(G):
    """More rooms than the grid cap plus 3, a member, a leaver and a joiner each."""
    conns, rooms = [], []
    for r in range(G + 3):
        lo = len(conns)
        conns += [Conn(name_of(lo), cur=r), Conn(name_of(lo + 1), LEAVE, cur=r), Conn(name_of(lo + 2), JOIN, room=r)]
        rooms.append(Room([lo, lo + 1], member_cap=2))
    return Case("over_grid", *ample(conns, rooms))


def three_sweeps():
    """One room set over three sweeps: (join; talk and join; close and leave).
    Per sweep the flags and rows of 8 slot-stable connections; the talk itself
    is the broadcast's business: here a bcast row stands for it."""
    n = 8
    names = [name_of(i) for i in range(n)]
    sweeps = [
        {1: dict(flags=JOIN, room=0), 2: dict(flags=JOIN, room=0), 5: dict(flags=JOIN, room=1)},
        {1: dict(bcast=bcast_row(30)), 2: dict(bcast=bcast_row(37)), 5: dict(bcast=bcast_row(0)),
         3: dict(flags=JOIN_ON_ACCEPT, room=0, accept=accept_row(ACC_ACCEPTED, 129)),
         6: dict(flags=JOIN_ON_ACCEPT, room=1, accept=accept_row(0, 0))},
        {1: dict(flags=LEAVE_ON_CLOSE, reply=reply_row(4, RPL_CLOSED), bcast=bcast_row(4, BC_NOT_RECEIVER)),
         2: dict(flags=LEAVE_ON_CLOSE, reply=reply_row(0), bcast=bcast_row(21)),
         3: dict(flags=LEAVE_ON_CLOSE, bcast=bcast_row(21)), 5: dict(flags=LEAVE)},
    ]
    return n, names, sweeps

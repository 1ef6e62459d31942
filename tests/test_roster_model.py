"""The roster model (tests/roster_model.py) held to a restatement of the
reference's room (chat_room::join, leave, welcome, farewell,
example/websocket/websocket_chat.cpp:34-39, 49-87) run sequentially over each
sweep's leaves, then its joins; then every rule of include/xyws.h's
xyws_roster_streams section on its own. CPU only."""
import random

import roster_model as M


def run_against_reference(n, n_rooms, sweeps, seed):
    """Random joins and leaves over `sweeps` sweeps on slot-stable tables:
    per connection the concatenated notices it is sent, per room the list."""
    rng = random.Random(seed)
    names = [M.name_of(i, rng.choice((0, 1, 9, 21, 80, 81, 82, 83, 200))) for i in range(n)]
    refs = [M.RefRoom(names) for _ in range(n_rooms)]
    conns = [M.Conn(names[i]) for i in range(n)]
    rooms = [M.Room([], member_cap=n) for _ in range(n_rooms)]
    events = 0
    for _ in range(sweeps):
        for i, c in enumerate(conns):
            c.flags, c.room, c.reply = 0, M.NONE, None
            roll = rng.random()
            if c.cur != M.NONE and roll < 0.3:
                if rng.random() < 0.5:
                    c.flags = M.LEAVE
                else:
                    c.flags, c.reply = M.LEAVE_ON_CLOSE, M.reply_row(0, M.RPL_CLOSED)
            elif c.cur == M.NONE and roll < 0.4:
                c.flags, c.room = M.JOIN, rng.randrange(n_rooms)
        M.ample(conns, rooms)
        res = M.roster(conns, rooms)
        before = [dict(ref.sent) for ref in refs]
        for r, (ref, rm) in enumerate(zip(refs, rooms)):  # the sweep's leaves, in list order, before its joins
            for m in list(rm.members):
                if res.want[m] == "leave":
                    ref.leave(m)
                    events += 1
            for i in range(n):
                if res.want[i] == r:
                    ref.join(i)
                    events += 1
        for i, (lo, data, row) in enumerate(res.conns):
            heard = b"".join(ref.sent.get(i, b"")[len(before[r].get(i, b"")):] for r, ref in enumerate(refs))
            if res.want[i] == "leave":
                # (the reference erases first: a leaver hears nothing of this sweep, its own farewell included)
                assert data == b"" and row["status"] & M.RSC_NOT_RECEIVER
            else:
                assert data == heard, (i, row)
            assert row["note_len"] == len(data) and not row["status"] & M.RSC_TRUNCATED
        for ref, (_, row, members) in zip(refs, res.rooms):
            assert members == ref.participants and row["n_members"] == len(members)
        M.apply(conns, rooms, res)
    return events


def test_model_is_the_references_room():
    assert run_against_reference(24, 3, 12, 1) > 50
    assert run_against_reference(5, 1, 30, 2) > 20
    assert run_against_reference(64, 2, 6, 3) > 50


def test_the_strings_are_the_references():
    src = open(__file__.replace("tests/test_roster_model.py", "include/xyws.h")).read()
    assert "websocket_chat.cpp" in src
    assert M.REF.head == b"|        SERVER       |:" and len(M.REF.head) == 24
    assert M.REF.joined == b" has joined the chat\n" and M.REF.left == b" has left the chat\n"
    assert M.notice(M.FIN | M.TEXT, M.REF, b"1.2.3.4:5", M.REF.joined) == \
        b"\x81\x36|        SERVER       |:1.2.3.4:5 has joined the chat\n"


def one(conns, rooms, **kw):
    M.ample(conns, rooms, **kw)
    return M.roster(conns, rooms, **kw)


def test_leave_wins_and_already():
    conns = [M.Conn(b"a", M.JOIN | M.LEAVE, room=1, cur=0), M.Conn(b"b", M.JOIN, room=1, cur=0),
             M.Conn(b"c", M.LEAVE), M.Conn(b"d", M.JOIN | M.LEAVE, room=1)]
    res = one(conns, [M.Room([0, 1], member_cap=4), M.Room([], member_cap=4)])
    assert res.want == ["leave", None, "leave", "leave"]
    assert res.rooms[0][2] == [1] and res.rooms[1][2] == []
    assert res.conns[0][2]["status"] == M.RSC_LEFT | M.RSC_NOT_RECEIVER and res.cur[0] == M.NONE
    assert res.conns[0][2]["room"] == 0
    assert res.conns[1][2]["status"] == M.RSC_MEMBER | M.RSC_ALREADY and res.cur[1] == 0
    assert res.conns[1][1] == M.notice(0x11, M.REF, b"a", M.REF.left)      # it stays and hears the farewell
    assert res.conns[2][2]["status"] == M.RSC_NOT_RECEIVER                 # a leave nobody lists: no effect
    assert res.conns[2][2]["room"] == M.NONE and res.cur[2] == M.NONE
    assert res.rooms[0][1]["left"] == 1 and res.rooms[1][1]["joined"] == 0
    assert res.jconns == [(M.NONE, 0)] * 4


def test_full_admits_a_prefix():
    conns = [M.Conn(b"m", cur=0)] + [M.Conn(b"j%d" % k, M.JOIN, room=0) for k in range(5)]
    res = one(conns, [M.Room([0], member_cap=3)])
    assert res.rooms[0][2] == [0, 1, 2] and res.rooms[0][1]["status"] == M.RS_FULL
    assert res.rooms[0][1]["joined"] == 2
    assert [r["status"] for _, _, r in res.conns] == [M.RSC_MEMBER, M.RSC_JOINED, M.RSC_JOINED] + \
        [M.RSC_FULL | M.RSC_NO_ROOM] * 3
    assert res.cur == [0, 0, 0, M.NONE, M.NONE, M.NONE]
    assert res.jconns == [(M.NONE, 0), (0, M.BL_JOIN), (0, M.BL_JOIN)] + [(M.NONE, 0)] * 3
    w1, w2 = (M.notice(0x11, M.REF, b"j%d" % k, M.REF.joined) for k in (0, 1))
    assert res.rooms[0][0] == w1 + w2                    # no welcome for the refused
    assert [d for _, d, _ in res.conns] == [w1 + w2, w1 + w2, w2, b"", b"", b""]
    assert res.conns[2][2]["note_off"] == len(w1)
    # a leaver frees its slot in the same sweep
    conns = [M.Conn(b"m", M.LEAVE, cur=0), M.Conn(b"j", M.JOIN, room=0)]
    res = one(conns, [M.Room([0], member_cap=1)])
    assert res.rooms[0][2] == [1] and res.rooms[0][1]["status"] == 0
    # a null member array admits nobody
    res = one([M.Conn(b"j", M.JOIN, room=0)], [M.Room([], members_null=True)])
    assert res.rooms[0][1]["status"] == M.RS_FULL and res.conns[0][2]["status"] == M.RSC_FULL | M.RSC_NO_ROOM


def test_bad_name_and_bad_member():
    long = M.name_of(0, 257)
    conns = [M.Conn(long, M.LEAVE, cur=0), M.Conn(long, M.JOIN, room=0), M.Conn(long[:256], M.JOIN, room=0),
             M.Conn(None, M.JOIN, room=0, name_len=999)]
    res = one(conns, [M.Room([7, 0, 4], member_cap=8)])
    assert res.rooms[0][2] == [1, 2, 3]                  # the event still happens; the bad entries are gone
    assert res.rooms[0][1]["status"] == M.RS_BAD_MEMBER and res.rooms[0][1]["left"] == 1
    assert res.conns[0][2]["status"] == M.RSC_LEFT | M.RSC_NOT_RECEIVER | M.RSC_BAD_NAME
    assert res.conns[1][2]["status"] == M.RSC_JOINED | M.RSC_BAD_NAME
    assert res.conns[2][2]["status"] == M.RSC_JOINED and res.conns[3][2]["status"] == M.RSC_JOINED
    bare = lambda t: M.notice(0x11, M.REF, b"", t)
    assert res.rooms[0][0] == bare(M.REF.left) + bare(M.REF.joined) + \
        M.notice(0x11, M.REF, long[:256], M.REF.joined) + bare(M.REF.joined)
    assert len(M.notice(0x11, M.REF, long[:256], M.REF.joined)) == 4 + 24 + 256 + 21


def test_header_forms():
    assert M.header_seam_lengths() == [80, 81, 82, 83]
    for ln, tail, h in ((80, M.REF.joined, 2), (81, M.REF.joined, 4), (82, M.REF.left, 2), (83, M.REF.left, 4)):
        f = M.notice(0x11, M.REF, b"x" * ln, tail)
        assert len(f) == h + 24 + ln + len(tail) and f[1] == (126 if h == 4 else 125)
        assert h == 2 or (f[2] << 8 | f[3]) == 126


def test_truncation():
    full = len(M.notice(0x11, M.REF, b"a", M.REF.left)) + 2 * len(M.notice(0x11, M.REF, b"b", M.REF.joined))
    for cap in (0, 1, 30, full - 1, full, full + 1):
        conns = [M.Conn(b"m", cur=0), M.Conn(b"a", M.LEAVE, cur=0), M.Conn(b"b", M.JOIN, room=0),
                 M.Conn(b"b", M.JOIN, room=0)]
        res = one(conns, [M.Room([0, 1], member_cap=4, notes_cap=cap)])
        wire, row, members = res.rooms[0]
        assert len(wire) == min(cap, full) and row["notes_len"] == full and members == [0, 2, 3]   # exact whatever the cap
        assert row["welcome_off"] == len(M.notice(0x11, M.REF, b"a", M.REF.left))
        assert bool(row["status"] & M.RS_TRUNCATED) == (cap < full)
        assert res.conns[0][1] == wire
        off = res.conns[3][2]["note_off"]
        assert res.conns[3][2]["note_len"] == max(min(cap, full) - off, 0) and res.conns[3][1] == wire[off:]
    # out_cap inside the delivered suffix
    conns = [M.Conn(b"m", cur=0, reply=M.reply_row(5)), M.Conn(b"a", M.LEAVE, cur=0)]
    rooms = [M.Room([0, 1])]
    M.ample(conns, rooms)
    conns[0].send_cap = 5 + 10
    lo, data, row = M.roster(conns, rooms).conns[0]
    assert lo == 5 and len(data) == 10 and row["status"] == M.RSC_MEMBER | M.RSC_TRUNCATED
    assert row["send_len"] == 5 + len(M.notice(0x11, M.REF, b"a", M.REF.left))


def test_the_base_chain_and_the_receivers():
    case = M.bases()
    res = M.roster(case.conns, case.rooms)
    by_base = {}
    for c, (_, _, row) in zip(case.conns, res.conns):
        src = "bcast" if c.bcast is not None else "reply" if c.reply is not None else \
            "accept" if c.accept is not None else "none"
        by_base.setdefault(src, set()).add(c.base)
        assert row["send_len"] == c.base + row["note_len"]
    assert by_base == {"none": {0}, "accept": {129, 66, 0}, "reply": {9, 4}, "bcast": {40, 11}}
    k = len(res.conns) // 4
    st = [r["status"] for _, _, r in res.conns]
    # members that stay: closed, overflowed and not-receivers get nothing, the others the whole wire
    assert [bool(s & M.RSC_NOT_RECEIVER) for s in st[:13]] == [False] * 8 + [True, True, False, True, False]
    assert all(s & M.RSC_MEMBER for s in st[:13])
    # LEAVE_ON_CLOSE: only the closed one leaves
    assert [bool(s & M.RSC_LEFT) for s in st[13:26]] == [False] * 8 + [True] + [False] * 4
    # JOIN_ON_ACCEPT: accepted rows join; a rejected or incomplete row makes a non-receiver; no row, no effect
    on = st[39:52]
    assert [bool(s & M.RSC_JOINED) for s in on] == [False, True, False, False, False, True, False, True] + [False] * 5
    assert on[2] & M.RSC_NOT_RECEIVER and on[3] & M.RSC_NOT_RECEIVER and on[0] == M.RSC_NO_ROOM
    tail = st[52:]
    assert tail[0] & M.RSC_LEFT and tail[1] == M.RSC_MEMBER | M.RSC_ALREADY
    assert tail[2] == M.RSC_NO_ROOM and tail[3] == M.RSC_NO_ROOM and tail[4] == M.RSC_NOT_RECEIVER
    assert tail[5] == M.RSC_NO_ROOM and tail[6] == M.RSC_JOINED | M.RSC_TRUNCATED
    assert k  # (the case has four blocks of rows)


def test_talk_then_close_and_a_joiner_that_spoke_through_roster_and_backlog():
    """Rule 5: the backlog's fold recounts the room's frames from the list the
    broadcast read. A member that says something and closes in the same sweep
    leaves; a joiner has messages of its own in the sweep's tables. With the
    `seen` list the fold keeps the room's history; with the rewritten list it
    is a mismatch and the backlog is lost."""
    import backlog_model as B
    import room_model as R
    closed = R.reply_row(4, first_close=1, status=R.RM.CLOSED, code=1000)
    conns = [R.speaker([3], room=0), R.speaker([], room=0), R.speaker([4], room=0, reply=closed),
             R.speaker([5], room=R.NONE)]
    rooms = [R.Room([0, 1, 2])]
    R.size_sends(conns, rooms)
    bres = R.broadcast(conns, rooms)
    written, frames, row, _ = bres.rooms[0]
    assert row["nmsgs"] == 2 and [i for i, _, _, _ in frames] == [0, 2]   # the closing member's text is in the wire
    mconns = [M.Conn(b"a", M.LEAVE_ON_CLOSE, cur=0), M.Conn(b"b", M.LEAVE_ON_CLOSE, cur=0),
              M.Conn(b"c", M.LEAVE_ON_CLOSE, cur=0, reply=M.reply_row(4, M.RPL_CLOSED)),
              M.Conn(b"d", M.JOIN, room=0)]
    mrooms = [M.Room([0, 1, 2], member_cap=4)]
    res = one(mconns, mrooms)
    assert res.seen == [[0, 1, 2]] and res.rooms[0][2] == [0, 1, 3]
    br = B.filled(B.BRoom(B.cap_for(200), keep=10), 0, [6])
    got, why = B.fold(br, B.sizes_of(conns, res.seen[0]), written, row)
    assert (why, got["status"], got["count"], got["folded"], got["dropped"]) == ("kept", 0, 3, 2, 0)
    assert br.carry.count == 3 and br.carry.flen[:3] == [6] + [len(h) + len(p) for _, _, h, p in frames]
    assert br.held()[6:] == written and br.carry.gaps == 0 and br.carry.total == 3
    # the rewritten list instead: the leaver's frame is missed, the joiner's counted: the history is lost
    lost = B.filled(B.BRoom(B.cap_for(200), keep=10), 0, [6])
    got, why = B.fold(lost, B.sizes_of(conns, res.rooms[0][2]), written, row)
    assert why == "mismatch" and got["status"] == B.BL_MISMATCH | B.BL_GAP and lost.carry.count == 0
    # a room without a seen row names none
    assert M.roster(mconns, [M.Room([0, 1, 2], member_cap=4, seen=False)]).seen == [None]
    # the seen list is cut at member_cap, bad entries included
    assert M.roster(mconns, [M.Room([0, 9, 1, 2], member_cap=3)]).seen == [[0, 9, 1]]


def test_three_sweeps_chained():
    n, names, sweeps = M.three_sweeps()
    conns = [M.Conn(names[i]) for i in range(n)]
    rooms = [M.Room([], member_cap=4), M.Room([], member_cap=4)]
    lists = []
    for ev in sweeps:
        for i, c in enumerate(conns):
            e = ev.get(i, {})
            c.flags, c.room = e.get("flags", 0), e.get("room", M.NONE)
            c.bcast, c.reply, c.accept = e.get("bcast"), e.get("reply"), e.get("accept")
        M.ample(conns, rooms)
        res = M.roster(conns, rooms)
        M.apply(conns, rooms, res)
        lists.append([list(rm.members) for rm in rooms])
    assert lists == [[[1, 2], [5]], [[1, 2, 3], [5]], [[2, 3], []]]
    assert [c.cur for c in conns] == [M.NONE, M.NONE, 0, 0, M.NONE, M.NONE, M.NONE, M.NONE]
    # the last sweep: 2 and 3 hear 1's farewell behind the room's wire
    assert res.conns[2][0] == 21 and res.conns[2][1] == M.notice(0x11, M.REF, names[1], M.REF.left)
    assert res.conns[3][1] == res.conns[2][1] and res.conns[1][1] == b""

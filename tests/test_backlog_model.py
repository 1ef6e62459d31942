"""The backlog model (tests/backlog_model.py) held to a restatement of the
reference's room, and every rule of xyws_backlog_streams on its own.

The reference (example/websocket/websocket_chat.cpp:34-47, 89-95): deliver
pushes each message onto m_recent_messages and pops the front past 10; join
sends the deque's contents to the newcomer. Restated below as a
collections.deque(maxlen=10) of framed messages."""
import collections

import pytest

import backlog_model as B
import room_model as R


def reference_room(sweeps):
    """Per sweep: what a joiner after that sweep's messages is sent."""
    recent = collections.deque(maxlen=10)
    out = []
    for frames in sweeps:
        for f in frames:
            recent.append(f)
        out.append(b"".join(recent))
    return out


SCENARIOS = [
    [[[5], [7, 9]], [[]], [[3, 3, 3, 3], [4, 4, 4, 4], [1, 2, 3]], [[130], [0]], [[2] * 12], [[6]]],
    [[[1]] * 11, [[]], [[2, 200, 70000]], [[9]] * 9, [[4], [], [5]]],
    [[[k % 7 for k in range(40)]], [[8]], [[9]], [[10]], [[11]]],
]


@pytest.mark.parametrize("k", range(len(SCENARIOS)))
def test_model_is_the_reference_deque(k):
    br = B.BRoom(B.cap_for(1 << 20), keep=10)
    cov = B.Coverage()
    runs = B.run_sweeps(br, SCENARIOS[k], cov)
    want = reference_room([frames for _, _, frames in runs])
    br2 = B.BRoom(B.cap_for(1 << 20), keep=10)
    for s, lens in enumerate(SCENARIOS[k]):
        B.run_sweeps(br2, [lens])
        j = B.JConn(send_cap=1 << 21, room=0, join=True)
        (lo, data, res), = B.deliver([j], [br2])
        assert data == want[s] and lo == 0, (k, s)
        assert res == dict(send_len=len(want[s]), backlog_len=len(want[s]), status=B.BLC_JOINED)
    assert br2.carry.total == sum(min(len(f), 10) for _, _, f in runs) and br2.carry.gaps == 0


def one(br, lens, **kw):
    (res, why, frames), = B.run_sweeps(br, [lens], **kw)
    return res, why, frames


def test_no_new_message_leaves_everything():
    br = B.BRoom(B.cap_for(100))
    one(br, [[5, 6]])
    log, carry = bytes(br.log), br.carry.pack()
    res, why, _ = one(br, [[]])
    assert why == "n0" and res == B.room_result(br.carry.len, 2) and bytes(br.log) == log and br.carry.pack() == carry
    # (the carry is not checked when N == 0)
    br.carry.start = 7
    bad = br.carry.pack()
    res, why, _ = one(br, [[]])
    assert why == "n0" and res["status"] == 0 and br.carry.pack() == bad
    assert br.held() == b""


@pytest.mark.parametrize("field", ["start", "len", "count", "flen"])
def test_bad_carry_counts_as_empty(field):
    br = B.BRoom(B.cap_for(100), keep=4)
    one(br, [[5, 6]])
    H = br.H
    if field == "start":
        br.carry.start = 16
    elif field == "len":
        br.carry.len = H + 1
    elif field == "count":
        br.carry.count = B.MAX + 1
    else:
        br.carry.flen[0] += 1
    br.carry.gaps, br.carry.total = 3, 40
    res, why, frames = one(br, [[9]])
    assert res == B.room_result(len(frames[0]), 1, 1, 0, B.BL_BAD_CARRY) and why == "kept"
    assert (br.carry.start, br.carry.gaps, br.carry.total) == (0, 3, 41) and br.held() == frames[0]


def test_mismatch_and_truncated_wire_clear():
    for how in ("nmsgs", "wire_len", "truncated", "cap"):
        br = B.BRoom(B.cap_for(100), keep=4)
        one(br, [[5, 6]])
        conns, rooms = B.talk([[7], [8]])
        if how == "cap":
            rooms[0].wire_cap = 10
        bres = R.broadcast(conns, rooms)
        row = dict(bres.rooms[0][2])
        if how == "nmsgs":
            row["nmsgs"] += 1
        elif how == "wire_len":
            row["wire_len"] -= 1
        elif how == "truncated":
            row["status"] |= R.ROOM_TRUNCATED
        rres, whys, _ = B.backlog(conns, rooms, bres, [br], rows=[row])
        gap = B.BL_GAP | (B.BL_MISMATCH if how in ("nmsgs", "wire_len") else 0)
        assert rres[0] == B.room_result(0, 0, 0, 2, gap), how
        assert whys[0] == ("mismatch" if gap & B.BL_MISMATCH else "truncated")
        c = br.carry
        assert (c.start, c.len, c.count, c.gaps, c.total, c.flen) == (0, 0, 0, 1, 2, [0] * B.MAX)
        assert br.held() == b""


def test_eviction_by_bytes():
    br = B.BRoom(2 * 48, keep=10)  # H = 48
    assert br.H == 48
    _, _, f1 = one(br, [[10, 10, 10]])     # three frames of 12
    assert br.carry.count == 3 and br.carry.len == 36
    res, why, f2 = one(br, [[11]])         # 13 more: 49 > 48, the oldest goes
    assert why == "evicted" and res == B.room_result(37, 3, 1, 1, B.BL_EVICTED)
    assert br.held() == f1[1] + f1[2] + f2[0]


def test_a_frame_of_exactly_h_and_of_h_plus_one():
    br = B.BRoom(2 * 48, keep=10)
    one(br, [[5]])
    res, why, f = one(br, [[46]])          # 2 + 46 == H
    assert why == "evicted" and res == B.room_result(48, 1, 1, 1, B.BL_EVICTED) and br.held() == f[0]
    res, why, f = one(br, [[4, 47]])       # the newest is H + 1
    assert why == "too_long" and res == B.room_result(0, 0, 0, 1, B.BL_EVICTED | B.BL_TOO_LONG)
    c = br.carry
    assert (c.start, c.len, c.count, c.gaps, c.total) == (0, 0, 0, 0, 2) and c.flen == [0] * B.MAX


@pytest.mark.parametrize("keep", [1, 16, 17])
def test_keep(keep):
    br = B.BRoom(B.cap_for(4096), keep=keep)
    frames, k = [], min(keep, 16)
    for lens in ([[1, 2, 3]], [[4] * 9], [[5] * 7, [6]]):
        frames += one(br, lens)[2]
    assert br.carry.count == k and br.held() == b"".join(frames[-k:])
    assert br.carry.total == min(3, k) + min(9, k) + min(8, k)
    res, _, f = one(br, [[9] * 20])
    assert res["folded"] == k and res["dropped"] == k and br.held() == b"".join(f[-k:])


def test_halves_alternate_over_four_sweeps():
    br = B.BRoom(B.cap_for(200), keep=3)
    starts, frames = [], []
    for s in range(4):
        frames += one(br, [[10 + s, 20 + s]])[2]
        starts.append(br.carry.start)
        assert br.held() == b"".join(frames[-3:])
    assert starts == [0, br.H, 0, br.H]


def test_sizing_rule():
    for Bb in range(1, 65):
        assert B.half(B.cap_for(Bb)) >= Bb
    assert any(B.half(2 * Bb + 29) < Bb for Bb in range(1, 65))  # (30 is needed)


def test_passthrough_forms_and_delivery_rules():
    rooms = [B.BRoom(200, log_null=True), B.BRoom(200, bc_null=True), B.BRoom(200, keep=0), B.BRoom(31),
             B.BRoom(200)]
    cov = B.Coverage()
    for br in rooms:
        res, why, _ = one(br, [[5]], cov=cov)
        assert (why == "passthrough") == (br is not rooms[4])
        if br is not rooms[4]:
            assert res == B.room_result(status=B.BL_PASSTHROUGH) and br.carry.pack() == B.Carry().pack()
            assert bytes(br.log) == bytes([B.LOG_FILL]) * br.log_cap
    closed = R.reply_row(4, status=R.RM.CLOSED)
    nr = dict(send_len=9, bcast_len=0, status=R.BC_NOT_RECEIVER)
    js = [B.JConn(20, room=r, join=True) for r in range(6)] + [
        B.JConn(20, room=4, join=False, reply=R.reply_row(3)),
        B.JConn(20, room=4, join=True, reply=closed),
        B.JConn(20, room=4, join=True, bcast=nr, reply=R.reply_row(3)),
        B.JConn(20, room=4, join=True, bcast=dict(send_len=15, bcast_len=6, status=0), reply=R.reply_row(9)),
        B.JConn(20, room=4, join=True, reply=R.reply_row(25)),
        B.JConn(20, room=4, join=True, out_null=True),
        B.JConn(20, room=3, join=True, reply=closed)]
    dl = B.deliver(js, rooms)
    cov.add_delivery(js, dl)
    st = [r["status"] for _, _, r in dl]
    assert st[:4] == [B.BLC_NO_ROOM] * 4 and st[5] == B.BLC_NO_ROOM and st[4] == B.BLC_JOINED
    assert dl[4][:2] == (0, rooms[4].held()) and len(rooms[4].held()) == 7
    assert dl[6] == (3, b"", dict(send_len=3, backlog_len=0, status=0))
    assert dl[7][2] == dict(send_len=4, backlog_len=0, status=B.BLC_NOT_RECEIVER)
    assert dl[8][2] == dict(send_len=9, backlog_len=0, status=B.BLC_NOT_RECEIVER)
    assert dl[9] == (15, rooms[4].held()[:5], dict(send_len=22, backlog_len=7, status=B.BLC_JOINED | B.BLC_TRUNCATED))
    assert dl[10] == (20, b"", dict(send_len=32, backlog_len=7, status=B.BLC_JOINED | B.BLC_TRUNCATED))
    assert dl[11] == (0, b"", dict(send_len=7, backlog_len=7, status=B.BLC_JOINED | B.BLC_TRUNCATED))
    assert st[12] == B.BLC_NO_ROOM
    cov.require("passthrough", "joined", "join_truncated", "join_no_room", "join_not_receiver", "non_joiner")


def test_scenarios_reach_every_cell():
    """The generators the device test shares must reach every Coverage cell."""
    cov = B.Coverage()
    for case in B.all_cases(T=1024, G=8192):
        for call in case.calls:
            B.run_call(case, call, cov)
    cov.require()

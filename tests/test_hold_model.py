"""The model of xyws_hold_streams (tests/hold_model.py) held to the reference:
for every connection of every scenario the messages the view delivers over all
sweeps (the records tests/room_model.py's skip_reason accepts, their bytes read
through the view base) are, as a sequence, the whole valid messages of the
oracle's reassembly of the unsplit stream; those the view names as a whole
message of one sweep are the records that lie inside a sweep. The bar holds
when hold_cap, msg_cap, vmsg_cap and out_cap suffice; every loss path and
pass-through cause is checked against its stated outcome, and a coverage
object requires that each branch was reached."""
import pytest

import hold_model as HM
import reasm_cases as RC
import reasm_model as M
import reasm_streams_model as SM
import reply_model as RM
import room_model as R
from hold_model import ACTIVE, DELIVERED, DROPPED, LOST, PASSTHROUGH, TOO_LONG


@pytest.fixture()
def cov():
    return HM.Coverage()


def valid_messages(oracle, wire):
    """(bytes, opcode, data frames) of the unsplit stream's whole valid messages."""
    out, recs, _ = RC.unsplit(oracle, wire)
    pos, valid = 0, []
    for _, nfr, _, length, st, op in recs:
        if st & M.COMPLETE and not st & (M.UTF8_BAD | M.TRUNCATED):
            valid.append((out[pos:pos + length], op, nfr))
        pos += length
    return valid


def check_connection(oracle, wire, outs):
    got = []
    for o in outs:
        c, plain = HM.view_conn(o), HM.plain_conn(o.inp)
        inside = [(f, n, off + o.hold_cap, ln, st, op) for (f, n, off, ln, st, op) in o.inp.recs
                  if R.skip_reason((f, n, off, ln, st, op), plain) is None]
        whole = []
        for j, rec in enumerate(c.recs):
            if R.skip_reason(rec, c) is None:
                got.append((c.buf[rec[2]:rec[2] + rec[3]], rec[5], rec[1]))
                if not (j == 0 and o.delivered is not None):
                    whole.append(rec)
        assert whole == inside
        assert not o.result["status"] & (DROPPED | TOO_LONG | PASSTHROUGH)
    assert got == valid_messages(oracle, wire), (got, valid_messages(oracle, wire))
    return got


def run_streams(oracle, sweeps, wires, hold_cap, cov):
    st, hst = SM.State(), HM.State()
    per = [[] for _ in wires]
    for pieces in sweeps:
        exp = SM.model_sweep(oracle, st, pieces)
        outs = hst.sweep([HM.from_exp(e) for e in exp], hold_cap)
        cov.add(outs)
        for i, o in enumerate(outs):
            per[i].append(o)
    return [check_connection(oracle, w, per[i]) for i, w in enumerate(wires)], per


def test_three_fragments_cut_at_every_byte(oracle, cov):
    sweeps, wires = HM.every_cut()
    assert len(sweeps) == 3
    got, per = run_streams(oracle, sweeps, wires, 2 * len(wires[0]) + 30, cov)
    assert all(len(g) == 2 and g[0][2] == 3 for g in got)
    assert sum(1 for outs in per for o in outs if o.delivered is not None) > len(wires[0])
    # a message held over a whole sweep of one byte: the middle sweep appends it
    assert any(o[1].events >= {"append"} and o[2].delivered is not None for o in per if len(o) == 3)


def test_short_stream_every_cut(oracle, cov):
    for middle in (False, True):
        sweeps, wires, _ = SM.short_every_cut(middle)
        run_streams(oracle, [p for p, _ in sweeps], wires, 2 * len(wires[0]) + 30, cov)


def test_back_to_back_halves_alternate(oracle, cov):
    sweeps, wires = HM.back_to_back(6)
    hold_cap = 2 * 64 + 30
    H = HM.half(hold_cap)
    got, per = run_streams(oracle, sweeps, wires, hold_cap, cov)
    assert len(got[0]) == 6
    starts = [o.carry.start for o in per[0] if o.carry.status & ACTIVE]
    assert len(starts) >= 5 and set(starts) == {0, H}
    assert all(a != b for a, b in zip(starts, starts[1:]))  # each sweep delivers from one half, begins in the other
    assert all(o.carry.start in (0, H) for o in per[0])


def test_the_sizing_rule(oracle):
    """hold_cap = 2 * L + 30 holds a message of L bytes whatever L; one byte less need not."""
    for L in range(1, 70):
        assert HM.half(2 * L + 30) >= L
    assert HM.half(2 * 17 + 29) < 17


def status_of(o):
    return o.result["status"]


def test_every_loss_path_and_pass_through(cov):
    H = 64
    sweeps, kws = HM.loss_and_passthrough(H)
    hst = HM.State()
    runs = []
    for r, (ins, kw) in enumerate(zip(sweeps, kws)):
        outs = hst.sweep(ins, **kw)
        cov.add(outs)
        runs.append(outs)
        if r == 0:
            HM.bad_carry_for(hst)
        for o in outs:  # the view is always a table the broadcast can take
            c = HM.view_conn(o)
            for rec in c.recs:
                R.skip_reason(rec, c)
    s0, s1, s2 = ([status_of(o) for o in outs] for outs in runs)
    delivered = [[o.delivered for o in outs] for outs in runs]
    # 0 TOO_LONG on begin
    assert s0[0] == DROPPED | TOO_LONG | LOST and s1[0] == 0 and not delivered[1][0] and "lost_cleared" in runs[1][0].events
    # 1 exactly H begins; one more byte is TOO_LONG on append
    assert s0[1] == ACTIVE and runs[0][1].result["held"] == H and s1[1] == DROPPED | TOO_LONG | LOST and s2[1] == 0
    # 2 held + length == H passes
    assert s1[2] == DELIVERED and runs[1][2].result["delivered_len"] == H and "append_fills_half" in runs[1][2].events
    # 3, 4 TRUNCATED parts
    assert s0[3] == DROPPED | LOST and s1[3] == 0 and s1[4] == DROPPED | LOST and s2[4] == 0
    assert not any(delivered[r][k] for r in range(3) for k in (3, 4))
    # 5 record 0 unstored: the held message and the one opened behind it are lost
    assert s0[5] == ACTIVE and s1[5] == DROPPED | LOST and s2[5] == 0 and not delivered[2][5]
    # 6 the last record unstored
    assert s0[6] == DROPPED | LOST and s1[6] == 0 and not delivered[1][6]
    # 7 vmsg_cap 0: the carry and the result are exact, the view stores nothing
    assert s0[7] == ACTIVE and s1[7] == DELIVERED and runs[1][7].view_recs == []
    assert runs[1][7].view_row["status"] & SM.RSM_MSG_CAP and runs[1][7].carry == HM.Carry()
    # 8 vmsg_cap s - 1
    o = runs[1][8]
    assert status_of(o) == DELIVERED | ACTIVE and len(o.view_recs) == 2 and o.view_recs[0][:4] == (0, 3, 0, 9)
    assert o.carry == HM.Carry(H, 2, 1, ACTIVE, 1) and s2[8] == DELIVERED and runs[2][8].view_recs == []
    # 9 a carry joined mid-message loses that message and holds the next
    assert s0[9] == DROPPED | LOST and s1[9] == ACTIVE and s2[9] == DELIVERED and runs[2][9].result["delivered_len"] == 7
    # 10 INTERRUPTED
    assert s1[10] == 0 and not delivered[1][10] and "interrupted" in runs[1][10].events
    # 11 UTF8_BAD completing: delivered to the view, skipped by the broadcast's rule
    o = runs[1][11]
    assert status_of(o) == DELIVERED and o.view_recs[0][4] == M.COMPLETE | M.UTF8_BAD
    assert R.skip_reason(o.view_recs[0], HM.view_conn(o)) == "utf8_bad"
    # 12 OVERFLOW is sticky
    assert s1[12] == DROPPED | LOST and s2[12] == LOST and runs[2][12].carry == HM.Carry(status=LOST)
    # 13 a part outside its range
    assert s1[13] == DROPPED and not delivered[1][13]
    # 14-16 pass-through; 17 a null vmsgs
    for k in (14, 15, 16):
        assert s0[k] == s1[k] == PASSTHROUGH and runs[1][k].view_recs is None
    assert s2[14] == 0 and s2[15] == s2[16] == PASSTHROUGH
    assert s1[17] == DELIVERED and runs[1][17].view_recs == [] and runs[1][17].view_msg_cap == 0
    # 18 a carry that does not fit the hold
    assert s1[18] == DROPPED and "bad_carry" in runs[1][18].events
    # 19 open over a whole sweep, then delivered while the next begins in the other half
    o = runs[2][19]
    assert s1[19] == ACTIVE and status_of(o) == DELIVERED | ACTIVE and o.view_recs[0] == (0, 2, 0, 11, M.COMPLETE, 2)
    assert o.carry.start == H and o.hold[:11] == runs[0][19].inp.buf[0:6] + o.inp.buf[0:5]
    # carries without ACTIVE compare bit-exactly: only status is set
    for outs in runs:
        for o in outs:
            if not o.passthrough and not o.carry.status & ACTIVE:
                assert o.carry.key()[:3] == (0, 0, 0) and o.carry.opcode == 0 and o.carry.status in (0, LOST)


def test_close_at_frame_0_drops_the_delivered_message(cov):
    """The documented approximation: the delivered record has first_frame 0, so
    a sweep whose frame 0 is the close frame does not deliver it."""
    hst = HM.State()
    hst.sweep([HM.made([(6, HM.OPEN)])], 158)
    o, = hst.sweep([HM.made([(3, HM.CONT | HM.DONE)])], 158)
    assert o.delivered is not None
    closed = HM.view_conn(o, reply=R.reply_row(4, first_close=0, status=RM.CLOSED, code=1000))
    later = HM.view_conn(o, reply=R.reply_row(4, first_close=1, status=RM.CLOSED, code=1000))
    assert R.skip_reason(o.view_recs[0], closed) == "after_close" and R.skip_reason(o.view_recs[0], later) is None
    cov.n["close_at_frame0"] += 1


@pytest.mark.parametrize("enc_opts", [0, R.ENC_FRAME_OPCODE])
def test_the_real_sweep_delivers_the_cut_message(oracle, cov, enc_opts):
    sweeps, caps, members, room_of = R.sweep_streams()
    st, hst = R.SweepState(), HM.State()
    seen = []
    for pieces in sweeps:
        run = HM.real_sweep(oracle, st, hst, pieces, caps, members, room_of, 2 * 64 + 30, enc_opts=enc_opts)
        cov.add(run[7])
        seen.append(run)
    (_, _, c1, v1, _, p1, r1, o1), (_, _, c2, v2, _, p2, r2, o2) = seen
    # sweep 1: the hold changes nothing on the wire; connections 4 and 6 begin a hold
    assert [rm[3] for rm in p1.rooms] == [rm[3] for rm in r1.rooms]
    assert o1[4].result["status"] == ACTIVE and o1[6].result["status"] == ACTIVE
    # sweep 2: connection 4's message reaches room 0
    frame = R.header(R.FIN | R.TEXT, 12 + len("cut in two sweeps")) + R.HEAD24[:12] + b"cut in two sweeps"
    assert frame in r2.rooms[0][3] and frame not in p2.rooms[0][3]
    assert r2.rooms[0][2]["skipped"] == p2.rooms[0][2]["skipped"] - 1
    assert r2.rooms[0][2]["nmsgs"] == p2.rooms[0][2]["nmsgs"] + 1
    assert o2[4].result == dict(held=0, delivered_len=17, status=DELIVERED) and o2[4].view_recs[0][1] == 3
    # ... and connection 6's ("fragments message", cut between two fragments) reaches room 1
    frame6 = R.header(R.FIN | R.TEXT, 18 + len("open message")) + R.HEAD24[:18] + b"open message"
    assert frame6 in r2.rooms[1][3] and frame6 not in p2.rooms[1][3]
    for i in (0, 4):  # every receiver of room 0 gets it
        lo, data, _ = r2.conns[i]
        assert frame in data
    # the overflowed connection's carry is LOST and stays so
    assert o1[3].carry == o2[3].carry == HM.Carry(status=LOST)


def test_every_branch_was_reached(oracle):
    """The scenarios above, on one coverage object, reach every branch."""
    cov = HM.Coverage()
    test_three_fragments_cut_at_every_byte(oracle, cov)
    test_short_stream_every_cut(oracle, cov)
    test_back_to_back_halves_alternate(oracle, cov)
    test_every_loss_path_and_pass_through(cov)
    test_close_at_frame_0_drops_the_delivered_message(cov)
    test_the_real_sweep_delivers_the_cut_message(oracle, cov, 0)
    cov.require()

"""The model of xyws_broadcast_streams (tests/room_model.py) held to an
independent statement of the reference's room (chat_room::deliver and
chat_session::writer, example/websocket/websocket_chat.cpp:89-101, 148-175):
every room's wire, decoded by the oracle's decode_stream, is exactly the
expected (head + message) payloads in member-then-record order under the
builder's headers; what a member sends is its reply bytes followed by the
wire; the counts are exact whatever the caps; and the scenarios the device
test shares reach every situation it counts on."""
import ctypes as C

import numpy as np
import pytest

import reasm_model as M
import reply_model as RM
import room_model as R
import xynet_amd._lib as L


def geometry():
    g = (C.c_uint64 * 4)()
    assert L.load().xyws_debug_broadcast_geometry(g) == 0
    return list(g)


@pytest.fixture(scope="module")
def reference():
    from oracle.oracle import Reference
    try:
        return Reference()
    except (FileNotFoundError, OSError):
        return None


def expected_payloads(conns, members):
    """The room as the reference runs it: every whole message of this sweep,
    of every participant in order, with the session's head before it."""
    out = []
    for i in members:
        if i >= len(conns):
            continue
        c = conns[i]
        for rec in c.recs:
            if R.skip_reason(rec, c) is None:
                out.append(((c.head or b"") + c.buf[rec[2]:rec[2] + rec[3]], rec[5], len(c.head or b"") + rec[3]))
    return out


def check(oracle, reference, conns, rooms, kw, cov):
    kw = {k: v for k, v in kw.items() if k != "packed"}
    flags, enc = kw.get("flags", R.FIN | R.TEXT), kw.get("enc_opts", 0)
    res = R.broadcast(conns, rooms, **kw)
    free = R.broadcast(conns, [R.Room(rm.members) for rm in rooms], **kw)
    cov.add(conns, rooms, res)
    for r, rm in enumerate(rooms):
        written, frames, rr, full = res.rooms[r]
        want = expected_payloads(conns, rm.members)
        # the wire, decoded as a peer would decode it
        buf = np.frombuffer(full, np.uint8).copy() if full else np.zeros(0, np.uint8)
        fr, _, cnt = oracle.decode_stream(buf, cap=len(want) + 2)
        assert cnt == len(fr) == len(want) == rr["nmsgs"], r
        pos = 0
        for f, (payload, op, total) in zip(fr, want):
            f_flags = R.frame_flags(flags, enc, op)
            hdr = oracle.header_build(f_flags, None, total)
            assert full[pos:pos + len(hdr)] == hdr and f.frame_off == pos and f.hdr_len == len(hdr), r
            if reference is not None:
                assert reference.header_ctor(f_flags, total) == hdr
            assert f.payload_len == len(payload) == total and f.flags == f_flags, r
            assert full[f.payload_off:f.payload_off + f.payload_len] == payload, r
            pos = f.payload_off + f.payload_len
        assert pos == len(full) == rr["wire_len"]
        assert rr["skipped"] == sum(len(conns[i].recs) for i in rm.members if i < len(conns)) - len(want)
        # carry-free exactness: the counts do not depend on the cap
        fr_ = free.rooms[r][2]
        assert (rr["wire_len"], rr["nmsgs"], rr["skipped"], rr["receivers"]) == \
            (fr_["wire_len"], fr_["nmsgs"], fr_["skipped"], fr_["receivers"])
        assert written == full[:len(written)] and bool(rr["status"] & R.ROOM_TRUNCATED) == (len(written) < len(full))
    for i, c in enumerate(conns):
        lo, data, cr = res.conns[i]
        # what the member sends: its reply bytes, then the wire
        image = bytearray(c.prefix[:c.send_cap].ljust(min(c.base, c.send_cap), b"\0"))
        image[lo:lo + len(data)] = data
        if c.room < len(rooms) and c.receiver():
            sent = (c.prefix[:c.base].ljust(c.base, b"\0") + res.rooms[c.room][0])[:c.send_cap]
            assert bytes(image) == sent[:len(image)] and len(image) == min(cr["send_len"], c.send_cap), i
            assert cr["bcast_len"] == len(res.rooms[c.room][0])
        else:
            assert not data and cr["bcast_len"] == 0 and cr["send_len"] == c.base, i
        assert bool(cr["status"] & R.BC_TRUNCATED) == (cr["send_len"] > c.send_cap), i
    return res


def test_scenarios_against_the_reference_statement(oracle, reference):
    T, S, G, _ = geometry()
    cov = R.Coverage()
    check(oracle, reference, *R.header_forms(), cov)
    for length in (1, 15, 16, 17, 31, 33, S - 1, S, S + 1, 2 * S + 5):
        check(oracle, reference, *R.alignment_matrix(S, length), cov)
    check(oracle, reference, *R.tiles(T), cov)
    check(oracle, reference, *R.over_grid(G), cov)
    check(oracle, reference, *R.wire_caps(), cov)
    check(oracle, reference, *R.out_caps(), cov)
    res = check(oracle, reference, *R.nulls_and_trivia(), cov)
    rr = res.rooms[0][2]
    assert rr["status"] == R.ROOM_BAD_MEMBER and rr["receivers"] == 4 and rr["nmsgs"] == 4 and rr["skipped"] == 8
    assert res.rooms[1][2] == dict(wire_len=0, nmsgs=0, skipped=1, receivers=2, status=R.ROOM_MSG_CAP)
    assert res.conns[7][2]["status"] == R.BC_NO_ROOM and res.conns[8][2]["status"] == R.BC_NO_ROOM
    assert res.conns[2][2]["status"] == R.BC_NOT_RECEIVER
    cov.require("truncated", "rsm_overflow", "rpl_overflow", "before_close", "after_close", "closed_earlier", "hdr2",
                "hdr4", "hdr10", "bad_member", "msg_cap", "no_room", "empty_room", "continued", "open", "interrupted",
                "utf8_bad")


REAL = ("continued", "open", "interrupted", "utf8_bad", "rsm_overflow", "rpl_overflow", "before_close", "after_close",
        "closed_earlier", "hdr2", "hdr4", "no_room")


@pytest.mark.parametrize("enc_opts", [0, R.ENC_FRAME_OPCODE])
def test_the_real_sweep(oracle, reference, enc_opts):
    sweeps, caps, members, room_of = R.sweep_streams()
    st, cov = R.SweepState(), R.Coverage()
    seen = []
    for pieces in sweeps:
        exp, replies, conns, rooms, _ = R.model_real_sweep(oracle, st, pieces, caps, members, room_of,
                                                           enc_opts=enc_opts)
        res = check(oracle, reference, conns, rooms, dict(enc_opts=enc_opts), cov)
        seen.append((exp, replies, conns, res))
    cov.require(*REAL)
    (e1, p1, c1, r1), (e2, p2, c2, r2) = seen
    assert p1[0][1]["reply_len"] > 0 and p1[0][1]["answered"] == 1                    # a pong before the wire
    assert p1[1][1]["first_close"] == 1 and p2[1][1]["status"] == RM.CLOSED          # closed mid-sweep, then earlier
    assert p1[3][1]["status"] & RM.OVERFLOW and e1[3].res["status"] & 4 and p2[3][1]["status"] & RM.OVERFLOW
    assert e2[4].recs[0][4] & M.CONTINUED and e2[4].recs[0][4] & M.COMPLETE           # the message that spans sweeps
    # binary messages go out under their own opcode only with XYWS_ENC_FRAME_OPCODE
    ops = {h[0] & 0x0F for rm in r1.rooms + r2.rooms for _, _, h, _ in rm[1]}
    assert ops == ({1, 2} if enc_opts else {1})
    # the closing connection's message from before its close frame is delivered, the one after it is not
    got = [p for i, _, _, p in r1.rooms[0][1] if i == 1]
    assert got == [(c1[1].head or b"") + b"before"]
    # nothing is delivered to or from a connection closed by an earlier sweep
    assert not any(i in (1, 2, 3) for i, _, _, _ in r2.rooms[0][1])
    assert all(r2.conns[i][2]["status"] & R.BC_NOT_RECEIVER for i in (1, 2, 3))

"""The semantics of xyws_reply_streams, checked on the CPU: the Python model
(tests/reply_model.py) of a stream cut into calls against the oracle on the
unsplit stream (oracle.classify + oracle.encode_frames, then the close frame),
in the reference's mode and the RFC mode; the len + 13 capacity bound; and the
reply carry's frame_remaining against the decode carry's payload_remaining."""
import pytest

import reply_cases as RC
import reply_model as M
import streams

MODES = ["reference", "rfc"]


def check_split(oracle, wire, cuts, mode, want):
    calls = M.run_split(oracle, wire, cuts, mode, RC.MAX_PAYLOAD)
    got = b"".join(c[3] for c in calls)
    assert got == want, (mode, cuts)
    closed = False
    for piece, fr, dc, w, res, vd, rc in calls:
        assert res["reply_len"] == len(w) <= piece.size + 13, (mode, cuts)  # out_cap = len + 13 never truncates
        assert not res["status"] & M.TRUNCATED
        closed = closed or rc.close_code != 0
        if not closed:
            assert rc.frame_remaining == dc.payload_remaining, (mode, cuts)
            assert rc.frames_seen == dc.frames_total
    return calls


@pytest.mark.parametrize("mode", MODES)
def test_random_streams_random_splits(oracle, mode):
    rng = streams.SplitMix(0x5917)
    worst = 0
    for s in range(60):
        wire = RC.echo_stream(1000 + s, 1 + rng.below(30), close=s % 3 != 0, big=s % 10 == 0)
        want = M.unsplit(oracle, wire, mode, RC.MAX_PAYLOAD)
        for _ in range(4):
            calls = check_split(oracle, wire, RC.random_cuts(rng, len(wire), rng.below(8)), mode, want)
            worst = max(worst, max(c[4]["reply_len"] - c[0].size for c in calls))
    assert worst <= 13


@pytest.mark.parametrize("mode", MODES)
def test_byte_at_a_time(oracle, mode):
    for s in range(4):
        wire = RC.echo_stream(77 + s, 6, close=True)[:700]
        want = M.unsplit(oracle, wire, mode, RC.MAX_PAYLOAD)
        check_split(oracle, wire, list(range(1, len(wire))), mode, want)


@pytest.mark.parametrize("mode", MODES)
def test_named_streams_and_header_cuts(oracle, mode):
    rng = streams.SplitMix(0xC0C0)
    for name, wire in RC.named_streams().items():
        want = M.unsplit(oracle, wire, mode, RC.MAX_PAYLOAD)
        assert want, name
        for _ in range(3):
            check_split(oracle, wire, RC.random_cuts(rng, len(wire), 5), mode, want)
        for cuts in RC.header_cuts(wire, RC.frame_starts(oracle, wire)[:6]):
            check_split(oracle, wire, cuts, mode, want)


def test_bound_is_reached_by_its_parts(oracle):
    """len + 13 = a 10-byte reply header for a frame whose last header byte
    alone is in the batch (+9), and the close frame (+4)."""
    import msg_streams
    rng = streams.SplitMix(5)
    wire = streams.header(0x82, 70000, rng.bytes(4))
    tail = msg_streams.close_frame(rng, 1000)
    # the header's last byte, then (payload_len 0 in the batch) a second stream: header carried + a close
    calls = M.run_split(oracle, wire, [13], "rfc", RC.MAX_PAYLOAD)
    assert calls[1][4]["reply_len"] - calls[1][0].size == 9
    short = streams.header(0x82, 0, rng.bytes(4), form=64) + tail
    calls = M.run_split(oracle, short, [13], "rfc", RC.MAX_PAYLOAD)
    # (a non-minimal 14-byte header answered by 2 bytes, then the close: 1 byte + 8 in, 2 + 4 out)
    assert calls[1][4]["reply_len"] == 6 and calls[1][0].size == 1 + len(tail)


def test_closed_and_overflow_are_sticky(oracle):
    import msg_streams
    rng = streams.SplitMix(9)
    wire = streams.frame(rng, 0x81, 5) + msg_streams.close_frame(rng, 1000) + streams.frame(rng, 0x81, 7)
    buf = M.as_array(wire)
    fr, _, _ = oracle.decode_stream(buf)
    kw = M.MODES["rfc"]
    w, res, vd, rc = M.reply(oracle, buf, fr, M.Carry(), 100, RC.MAX_PAYLOAD, **kw)
    assert res["first_close"] == 1 and res["close_code"] == 1000 and res["status"] == M.CLOSED and res["answered"] == 1
    assert w == bytes([0x81, 5]) + buf[fr[0].payload_off:][:5].tobytes() + bytes([0x88, 2, 0x03, 0xE8])
    assert len(vd) == 3 and rc.frames_seen == 3
    w2, res2, vd2, rc2 = M.reply(oracle, buf, fr, rc, 100, RC.MAX_PAYLOAD, **kw)
    assert w2 == b"" and vd2 is None and res2 == M.result(close_code=1000, status=M.CLOSED)
    assert rc2.as_tuple() == rc.as_tuple()
    # a table larger than its capacity: nothing answered, sticky
    w, res, vd, rc = M.reply(oracle, buf, fr, M.Carry(), 100, RC.MAX_PAYLOAD, cap=2, **kw)
    assert w == b"" and res == M.result(status=M.OVERFLOW) and rc.status == M.OVERFLOW and rc.frames_seen == 0
    w, res, vd, rc = M.reply(oracle, buf, fr[:1], rc, 100, RC.MAX_PAYLOAD, **kw)
    assert w == b"" and res["status"] == M.OVERFLOW


def test_truncation_keeps_the_carry_exact(oracle):
    rng = streams.SplitMix(11)
    wire = streams.frame(rng, 0x81, 40) + streams.frame(rng, 0x82, 300)
    cut = len(wire) - 100
    full = M.run_split(oracle, wire, [cut], "rfc", RC.MAX_PAYLOAD)
    for cap in (0, 1, 5, 41):
        calls = M.run_split(oracle, wire, [cut], "rfc", RC.MAX_PAYLOAD, out_caps=[cap, cap])
        for a, b in zip(calls, full):
            assert a[3] == b[3][:cap] and a[6].as_tuple() == b[6].as_tuple()
            assert a[4]["reply_len"] == b[4]["reply_len"] and a[4]["status"] == (M.TRUNCATED if b[4]["reply_len"] > cap else 0)

"""tests/inbox_model.py held to hand-computed answers, rule by rule of
include/xyws.h (xyws_inbox_streams). No library, no GPU.

The model is deliberately independent of the library, so these tests would pass
on a tree without xyws_inbox_streams too (the one that asks the library asks
xyws_accept_request, which is older): they hold the yardstick, and
tests/test_inbox_abi.py, tests/test_inbox_rows_text.py and
tests/test_gpu_inbox.py are the ones that fail without the feature."""
import random

import inbox_model as M


def conn(cap=64, carry=None, flags=0, aresult=None):
    return dict(cap=cap, carry=carry, flags=flags, aresult=aresult)


def ent(c, off, n, at, flags=0):
    return dict(conn=c, off=off, len=n, at=at, flags=flags)


def run(conns, entries, pack_len=1000, m_cap=None, head_m=None, pack_cap=None):
    head_m = len(entries) if head_m is None else head_m
    return M.inbox(conns, head_m, pack_len, entries, len(entries) if m_cap is None else m_cap,
                   pack_len if pack_cap is None else pack_cap)


def test_rule_1_entries_behind_m_and_bad_entries():
    conns = [conn(), conn()]
    es = [ent(0, 0, 4, 0), ent(2, 0, 4, 0), ent(1, 996, 5, 0), ent(1, 0, 3, 0)]
    res, s, rows, car, writes = run(conns, es, head_m=3)
    # the fourth entry is behind head.m; conn 2 is ignored; [996, 1001) leaves the pack and breaks connection 1
    assert s == dict(n_entries=3, bytes=4, n_conns=2, n_opened=0, n_eof=0, n_broken=1, n_bad_entries=2,
                     status=M.S_BAD_ENTRIES | M.S_BROKEN)
    assert res[0] == dict(len=4, lead=0, n_entries=1, status=0)
    assert res[1] == dict(len=0, lead=0, n_entries=1, status=M.R_BAD_RANGE)
    assert writes == [(0, 0, 0, 4)]
    # head.m above m_cap: clipped; the pack is cut at pack_cap too
    res, s, *_ = run(conns, es, head_m=9, m_cap=1, pack_cap=3)
    assert s["n_entries"] == 1 and s["status"] == M.S_CLIPPED | M.S_BAD_ENTRIES | M.S_BROKEN
    assert res[0]["status"] == M.R_BAD_RANGE and s["n_bad_entries"] == 1
    # off + len wraps: a bad range
    res, s, *_ = run([conn()], [ent(0, 8, (1 << 64) - 4, 0)])
    assert res[0]["status"] == M.R_BAD_RANGE


def test_rule_2_order_of_a_connections_entries_does_not_matter():
    es = [ent(0, 10, 3, 5), ent(0, 0, 5, 0), ent(0, 20, 2, 8)]
    res, s, rows, car, writes = run([conn()], es)
    assert res[0] == dict(len=10, lead=0, n_entries=3, status=0)
    assert sorted(writes) == [(0, 0, 0, 5), (0, 5, 10, 3), (0, 8, 20, 2)]
    assert car[0] == dict(http_len=10, bytes_total=10, state=M.HTTP, status=0)
    assert rows[0] == dict(conn_off=0, conn_len=0, aconn_len=10)


def test_rule_3_state_step():
    http7 = dict(http_len=7, bytes_total=7, state=M.HTTP, status=0)
    # dead: dropped, nothing written
    res, s, rows, car, writes = run([conn(carry=dict(http7, state=M.DEAD))], [ent(0, 0, 4, 0)])
    assert res[0] == dict(len=0, lead=0, n_entries=1, status=M.R_DROPPED) and writes == []
    assert rows[0] == dict(conn_off=0, conn_len=0, aconn_len=0) and car[0]["state"] == M.DEAD
    # NO_HANDSHAKE: open at once, placed at 0
    res, s, rows, car, writes = run([conn(flags=M.NO_HANDSHAKE)], [ent(0, 0, 4, 0)])
    assert rows[0] == dict(conn_off=0, conn_len=4, aconn_len=0) and car[0]["state"] == M.OPEN and s["n_opened"] == 0
    # refused
    res, s, rows, car, writes = run([conn(carry=http7, aresult=dict(status=M.ACC_REJECTED, consumed=7))],
                                    [ent(0, 0, 4, 0)])
    assert res[0]["status"] == M.R_REFUSED | M.R_DROPPED and car[0]["state"] == M.DEAD and writes == []
    assert car[0]["status"] == M.R_REFUSED and s["n_broken"] == 0
    # accepted, the whole request consumed: kept 0, lead 0, the new bytes at 0
    acc = dict(status=M.ACC_ACCEPTED, consumed=7)
    res, s, rows, car, writes = run([conn(carry=http7, aresult=acc)], [ent(0, 0, 4, 0)])
    assert res[0] == dict(len=4, lead=0, n_entries=1, status=M.R_OPENED) and writes == [(0, 0, 0, 4)]
    assert rows[0] == dict(conn_off=0, conn_len=4, aconn_len=0) and s["n_opened"] == 1
    assert car[0] == dict(http_len=0, bytes_total=11, state=M.OPEN, status=0)
    # accepted with 2 frame bytes behind the request: they stay, the new bytes go behind them
    res, s, rows, car, writes = run([conn(carry=http7, aresult=dict(status=M.ACC_ACCEPTED, consumed=5))],
                                    [ent(0, 0, 4, 0)])
    assert res[0] == dict(len=4, lead=5, n_entries=1, status=M.R_OPENED) and writes == [(0, 7, 0, 4)]
    assert rows[0] == dict(conn_off=5, conn_len=6, aconn_len=0)
    # ... and it opens without any entry too
    res, s, rows, car, writes = run([conn(carry=http7, aresult=dict(status=M.ACC_ACCEPTED, consumed=5))], [])
    assert rows[0] == dict(conn_off=5, conn_len=2, aconn_len=0) and s["n_opened"] == 1 and s["n_conns"] == 0
    # consumed above http_len: broken
    res, s, rows, car, writes = run([conn(carry=http7, aresult=dict(status=M.ACC_ACCEPTED, consumed=8))], [])
    assert res[0]["status"] == M.R_BAD_CONSUMED and car[0]["state"] == M.DEAD and s["n_broken"] == 1
    assert s["n_opened"] == 0
    # neither bit: stays HTTP, appended behind http_len
    res, s, rows, car, writes = run([conn(carry=http7, aresult=dict(status=0, consumed=0))], [ent(0, 0, 4, 0)])
    assert writes == [(0, 7, 0, 4)] and rows[0] == dict(conn_off=0, conn_len=0, aconn_len=11)


def test_rule_4_broken_connections():
    # S != T: a gap
    res, s, rows, car, writes = run([conn(), conn()], [ent(0, 0, 4, 1), ent(1, 4, 4, 0)])
    assert res[0]["status"] == M.R_BAD_TILING and res[0]["len"] == 0 and car[0]["state"] == M.DEAD
    assert writes == [(1, 0, 4, 4)] and s["n_broken"] == 1 and s["bytes"] == 4
    # an exact fit, and overflow by one byte (behind 60 request bytes)
    http60 = dict(http_len=60, bytes_total=60, state=M.HTTP, status=0)
    res, s, rows, car, writes = run([conn(carry=http60)], [ent(0, 0, 4, 0)])
    assert res[0]["status"] == 0 and car[0]["http_len"] == 64
    res, s, rows, car, writes = run([conn(carry=http60)], [ent(0, 0, 5, 0)])
    assert res[0] == dict(len=0, lead=0, n_entries=1, status=M.R_OVERFLOW) and writes == []
    assert rows[0] == dict(conn_off=0, conn_len=0, aconn_len=0)
    # the bits stay, and the next sweep's entries are dropped
    res2, s2, rows2, car2, writes2 = run([conn(carry=car[0])], [ent(0, 0, 1, 0)])
    assert res2[0]["status"] == M.R_OVERFLOW | M.R_DROPPED and writes2 == [] and s2["n_broken"] == 0
    # every bit that applies
    res, s, *_ = run([conn(cap=2)], [ent(0, 0, 4, 1), ent(0, 999, 2, 0)])
    assert res[0]["status"] == M.R_BAD_TILING | M.R_OVERFLOW | M.R_BAD_RANGE and s["n_broken"] == 1


def test_rule_5_an_idle_connection_ends_with_len_0():
    res, s, rows, car, writes = run([conn()], [ent(0, 0, 9, 0)])
    assert rows[0]["aconn_len"] == 9
    res, s, rows, car2, writes = run([conn(carry=car[0])], [])
    assert rows[0] == dict(conn_off=0, conn_len=0, aconn_len=0) and car2[0]["http_len"] == 9
    opened = dict(http_len=0, bytes_total=20, state=M.OPEN, status=0)
    res, s, rows, car, writes = run([conn(carry=opened)], [])
    assert rows[0] == dict(conn_off=0, conn_len=0, aconn_len=0)
    res, s, rows, car, writes = run([conn(carry=opened)], [ent(0, 3, 6, 0)])
    assert rows[0] == dict(conn_off=0, conn_len=6, aconn_len=0) and car[0]["bytes_total"] == 26


def test_rule_6_eof_with_and_without_bytes():
    opened = dict(http_len=0, bytes_total=0, state=M.OPEN, status=0)
    res, s, rows, car, writes = run([conn(carry=opened), conn(carry=opened)],
                                    [ent(0, 0, 4, 0, M.EOF_E), ent(1, 0, 0, 0, M.EOF_E)])
    assert res[0] == dict(len=4, lead=0, n_entries=1, status=M.R_EOF) and writes == [(0, 0, 0, 4)]
    assert res[1] == dict(len=0, lead=0, n_entries=1, status=M.R_EOF) and s["n_eof"] == 2
    assert car[1]["status"] == M.R_EOF and car[1]["state"] == M.OPEN
    # sticky in the row, counted once
    res, s, *_ = run([conn(carry=car[1])], [])
    assert res[0]["status"] == M.R_EOF and s["n_eof"] == 0


def test_accept_reports_a_row_without_bytes_as_incomplete():
    """Rule 5 relies on it: a row with len 0 is incomplete, nothing is answered, in the model and in the library."""
    import ctypes as C

    import accept_model as A
    import xynet_amd._lib as L
    for policy in (0, A.REFERENCE):
        res, out = A.accept(b"", policy=policy)
        assert res["status"] == 0 and res["resp_len"] == 0 and res["consumed"] == 0 and out == b""
        row = L.AcceptResult()
        assert L.load().xyws_accept_request(b"", 0, 1024, policy, None, 0, C.byref(row)) == 0
        assert bytes(row) == A.pack_result(res)


def test_apply_and_cut():
    pack = bytes(range(40))
    ranges = M.apply([(0, 2, 10, 3), (1, 0, 0, 2)], pack, [bytearray(8), bytearray(4)])
    assert ranges == [bytearray(b"\0\0\x0a\x0b\x0c\0\0\0"), bytearray(b"\x00\x01\0\0")]
    rng = random.Random(1)
    for total, pieces in ((0, 3), (10, 1), (100, 4), (5, 0)):
        runs = M.cut(total, pieces, rng)
        assert len(runs) == pieces and (sum(runs) == total or not pieces) and min(runs, default=0) >= 0

"""The outbox model (tests/outbox_model.py) against hand-computed answers: the
length chain, the flags, offsets as independent prefix sums, idempotence and
the capacity cases of include/xyws.h's rules. No library, no GPU."""
import copy
import random

import outbox_model as M


def conn(n=64, **rows):
    return dict(out=bytes((7 * k + 1) & 0xFF or 1 for k in range(n)), **rows)


def test_length_chain_takes_the_first_row_given():
    rows = dict(backlog=dict(send_len=40), bcast=dict(send_len=30), reply=dict(reply_len=20, status=0),
                accept=dict(status=M.ACC_ACCEPTED, resp_len=10))
    assert M.full_len(conn(**rows)) == 40
    del rows["backlog"]
    assert M.full_len(conn(**rows)) == 30
    del rows["bcast"]
    assert M.full_len(conn(**rows)) == 20
    del rows["reply"]
    assert M.full_len(conn(**rows)) == 10
    assert M.full_len(conn(accept=dict(status=M.ACC_REJECTED, resp_len=64))) == 64
    assert M.full_len(conn(accept=dict(status=0, resp_len=99))) == 0  # incomplete: nothing was written
    assert M.full_len(conn(accept=dict(status=4, resp_len=99))) == 0  # TRUNCATED alone is neither
    assert M.full_len(conn()) == 0
    # a row in front hides the ones behind it even when it says 0
    assert M.full_len(conn(backlog=dict(send_len=0), bcast=dict(send_len=30))) == 0


def test_flags_by_hand():
    assert M.flags_of(conn(reply=dict(reply_len=4, status=M.RPL_CLOSED))) == M.CLOSE
    assert M.flags_of(conn(reply=dict(reply_len=0, status=M.RPL_OVERFLOW))) == M.OVERFLOW
    assert M.flags_of(conn(reply=dict(reply_len=0, status=M.RPL_CLOSED | M.RPL_OVERFLOW | 1))) == M.CLOSE | M.OVERFLOW
    assert M.flags_of(conn(accept=dict(status=M.ACC_REJECTED, resp_len=64))) == M.CLOSE
    assert M.flags_of(conn(accept=dict(status=M.ACC_ACCEPTED, resp_len=64))) == 0
    # the flags look at reply and accept even when a row in front gives the length
    assert M.flags_of(conn(bcast=dict(send_len=8), reply=dict(reply_len=4, status=M.RPL_CLOSED))) == M.CLOSE
    assert M.flags_of(conn(n=64, bcast=dict(send_len=64))) == 0
    assert M.flags_of(conn(n=64, bcast=dict(send_len=65))) == M.TRUNCATED
    assert M.flags_of(dict(out=None, bcast=dict(send_len=1))) == M.TRUNCATED
    assert M.flags_of(dict(out=b"abcdef", out_cap=4, reply=dict(reply_len=5, status=0))) == M.TRUNCATED


def test_list_offsets_and_pack_by_hand():
    conns = [conn(n=64, bcast=dict(send_len=17)),                      # 0: 17 bytes, slot 32
             conn(),                                                     # 1: every pointer null: never listed
             conn(reply=dict(reply_len=0, status=M.RPL_CLOSED)),         # 2: the sticky close, len 0
             conn(n=8, bcast=dict(send_len=9)),                          # 3: truncated to 8, slot 16
             conn(reply=dict(reply_len=0, status=0)),                    # 4: silent
             conn(n=64, accept=dict(status=M.ACC_REJECTED, resp_len=64))]  # 5: the refusal, then close
    entries, summary, writes = M.outbox(conns, 4096)
    assert entries == [dict(conn=0, flags=0, off=0, len=17, full_len=17),
                       dict(conn=2, flags=M.CLOSE, off=32, len=0, full_len=0),
                       dict(conn=3, flags=M.TRUNCATED, off=32, len=8, full_len=9),
                       dict(conn=5, flags=M.CLOSE, off=48, len=64, full_len=64)]
    assert summary == dict(n_entries=4, pack_len=112, packed_len=112, send_bytes=89, n_close=2, n_truncated=1,
                           n_deferred=0, status=M.S_TRUNCATED)
    assert writes == {0: conns[0]["out"][:17] + bytes(15), 32: conns[3]["out"][:8] + bytes(8), 48: conns[5]["out"]}


def random_conns(rng, n):
    conns = []
    for _ in range(n):
        c = conn(n=rng.choice((0, 1, 15, 16, 17, 40, 100)))
        if not c["out"]:
            c["out"] = None
        if rng.random() < 0.3:
            c["backlog"] = dict(send_len=rng.randrange(0, 120))
        if rng.random() < 0.5:
            c["bcast"] = dict(send_len=rng.randrange(0, 120))
        if rng.random() < 0.6:
            c["reply"] = dict(reply_len=rng.randrange(0, 50), status=rng.choice((0, 0, 1, 2, 4, 6)))
        if rng.random() < 0.3:
            c["accept"] = dict(status=rng.choice((0, 1, 2, 6)), resp_len=rng.choice((0, 64, 129)))
        conns.append(c)
    return conns


def test_offsets_are_prefix_sums_whatever_the_capacity():
    rng = random.Random(5)
    conns = random_conns(rng, 200)
    lens = [min(M.full_len(c), M.out_cap_of(c)) for c in conns]
    listed = [i for i, c in enumerate(conns) if lens[i] or M.flags_of(c)]
    ref = None
    for cap in (None, 0, 16, 100, 1000, 1 << 20):
        entries, summary, writes = M.outbox(conns, cap)
        assert [e["conn"] for e in entries] == listed
        for e in entries:
            before = [j for j in listed if j < e["conn"]]
            assert e["off"] == sum((lens[j] + 15) // 16 * 16 for j in before) and e["off"] % 16 == 0
            assert e["len"] == lens[e["conn"]]
        core = [dict(e, flags=e["flags"] & ~M.DEFERRED) for e in entries]
        exact = {k: v for k, v in summary.items() if k not in ("packed_len", "n_deferred", "status")}
        ref = ref or (core, exact)
        assert (core, exact) == ref  # nothing but DEFERRED and its counts depends on the capacity
        assert summary["pack_len"] == sum((n + 15) // 16 * 16 for n in lens)
        assert summary["send_bytes"] == sum(lens)


def test_capacity_cases():
    conns = [conn(n=64, bcast=dict(send_len=n)) for n in (20, 0, 16, 33)]  # slots 32, -, 16, 48 at 0, 32, 48
    for cap, deferred, packed_len in ((None, [0, 2, 3], 0), (0, [0, 2, 3], 0), (31, [0, 2, 3], 0), (32, [2, 3], 32),
                                      (47, [2, 3], 32), (48, [3], 48), (95, [3], 48), (96, [], 96), (111, [], 96),
                                      (1 << 30, [], 96)):
        entries, summary, writes = M.outbox(conns, cap)
        assert [e["conn"] for e in entries if e["flags"] & M.DEFERRED] == deferred, cap
        assert summary["packed_len"] == packed_len and summary["pack_len"] == 96
        assert summary["n_deferred"] == len(deferred) and summary["status"] == (M.S_DEFERRED if deferred else 0)
        assert sorted(writes) == [e["off"] for e in entries if not e["flags"] & M.DEFERRED]
        assert all(off + len(b) <= (cap or 0) for off, b in writes.items())
    # an entry without bytes is never deferred
    entries, summary, _ = M.outbox([conn(reply=dict(reply_len=0, status=M.RPL_CLOSED))], None)
    assert entries[0]["flags"] == M.CLOSE and summary["n_deferred"] == 0 and summary["status"] == 0


def test_idempotent_and_inputs_unchanged():
    rng = random.Random(9)
    conns = random_conns(rng, 64)
    before = copy.deepcopy(conns)
    first = M.outbox(conns, 512)
    image = M.apply(first[2], bytearray(b"\xA5" * 4096))
    second = M.outbox(conns, 512)
    assert first == second and conns == before
    assert M.apply(second[2], bytearray(image)) == image
    assert all(b == 0xA5 for b in image[first[1]["packed_len"]:])

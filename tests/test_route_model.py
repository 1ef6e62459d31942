"""tests/route_model.py held against expectations written by hand from the
rules of include/xyws.h: no library and no GPU."""
import pytest

import accept_model as AM
import route_cases as RC
import route_model as M

ROOT, NOROOT = M.table(RC.TABLES["root"]), M.table(RC.TABLES["noroot"])
T = dict(RC.TARGETS)
E, B = M.MATCHED, M.MATCHED | M.BY_PREFIX


def got(tab, target):
    r = M.lookup(tab, target)
    return r["status"], (None if r["room"] == M.ROOM_NONE else r["room"]), r["key_len"]


def test_root_prefix_is_a_catch_all_and_a_prefix_ends_at_a_slash():
    assert got(ROOT, b"/") == (E, 0, 1)
    assert got(ROOT, b"/zzz") == (B, 0, 4)
    assert got(ROOT, b"/ab") == (B, 0, 3)         # /a does not match /ab: the root does
    assert got(NOROOT, b"/ab") == (M.MISS, None, 3)
    assert got(NOROOT, b"/a/b") == (B, 1, 4)
    assert got(NOROOT, b"/") == (M.MISS, None, 1)
    assert got(NOROOT, b"/roomsx") == (M.MISS, None, 7)
    assert got(NOROOT, b"x/y") == (B, 12, 3)       # a one-byte prefix key that is not the root
    assert got(NOROOT, b"xy") == (M.MISS, None, 2)


def test_trailing_slash():
    assert got(NOROOT, b"/a/") == (E, 1, 2)
    assert got(NOROOT, b"/exact/") == (E, 5, 6)
    assert got(NOROOT, b"/slash") == (E, 6, 6) and got(NOROOT, b"/slash/") == (E, 6, 6)  # the key was given as /slash/
    assert got(NOROOT, b"/a//") == (E, 11, 3)      # one slash is dropped, not two: the key /a/
    assert got(NOROOT, b"/a///") == (B, 11, 4)
    assert M.key_of(b"/") == b"/" and M.key_of(b"//") == b"/"


def test_query_and_fragment_at_the_start_in_the_middle_and_at_the_end():
    assert got(ROOT, b"?x=1") == (M.MISS, None, 0) and got(ROOT, b"#") == (M.MISS, None, 0)
    assert got(NOROOT, b"/a?x=1") == (E, 1, 2) and got(NOROOT, b"/a#top") == (E, 1, 2)
    assert got(NOROOT, b"/a?") == (E, 1, 2) and got(NOROOT, b"/a/?x") == (E, 1, 2)
    assert got(NOROOT, b"/a?/rooms/b") == (E, 1, 2)  # nothing behind the `?` is looked at
    assert got(NOROOT, b"/rooms/b?x=1") == (E, 3, 8)


def test_a_target_without_a_leading_slash_and_double_slashes():
    assert got(ROOT, b"chat") == (E, 7, 4)
    assert got(ROOT, b"chatx") == (M.MISS, None, 5)   # the root route needs a leading slash
    assert got(ROOT, b"chat/x") == (M.MISS, None, 6)  # chat is exact
    assert got(ROOT, b"//") == (E, 0, 1)
    assert got(ROOT, b"//a") == (B, 0, 3) and got(NOROOT, b"//a") == (M.MISS, None, 3)
    assert got(NOROOT, b"/a//b") == (B, 11, 5)         # /a/ is longer than /a


def test_keys_of_255_256_and_257_bytes():
    assert got(NOROOT, RC.K255) == (E, 8, 255) and got(NOROOT, RC.K256) == (E, 9, 256)
    assert got(NOROOT, RC.K256 + b"m") == (M.MISS, None, 257)   # no exact match above 256
    assert got(NOROOT, RC.K256 + b"/") == (E, 9, 256)            # 257 bytes, 256 after its slash is dropped
    assert got(NOROOT, RC.K256 + b"?q") == (E, 9, 256)           # the `?` is the window's last byte
    assert got(NOROOT, RC.K256 + b"/x") == (B, 9, 258)           # a prefix candidate that ends with the window
    assert got(NOROOT, RC.K255 + b"x") == (M.MISS, None, 256)
    with pytest.raises(ValueError):
        M.table([(RC.K256 + b"m", 0, 0)])
    assert len(M.table([(RC.K256, 0, 0)])) == 1


def test_a_300_byte_target_under_a_prefix_route():
    assert got(NOROOT, T["long_300"]) == (B, 10, 300)
    assert got(NOROOT, T["long_300_query_late"]) == (B, 10, 300)  # a `?` behind the window is not looked for
    assert got(NOROOT, T["flat_300"]) == (M.MISS, None, 300) and got(ROOT, T["flat_300"]) == (B, 0, 300)
    assert got(NOROOT, T["pairs_300"]) == (B, 1, 300)


def test_nested_exact_and_prefix_routes_the_longest_wins():
    assert got(ROOT, b"/rooms") == (E, 2, 6)
    assert got(ROOT, b"/rooms/b") == (E, 3, 8)
    assert got(ROOT, b"/rooms/b/c") == (B, 2, 10)          # /rooms/b is exact: /rooms takes what lies below it
    assert got(ROOT, b"/rooms/b/deep") == (E, 4, 13)
    assert got(ROOT, b"/rooms/b/deep/er/still") == (B, 4, 22)
    assert M.lookup(ROOT, b"/rooms/b/c")["route"] == 2 and M.lookup(NOROOT, b"/rooms/b/c")["route"] == 1


def test_what_the_build_refuses():
    for bad in ([(b"", 0, 0)], [(b"/a?b", 0, 0)], [(b"/a#", 0, 0)], [(b"/a", 0, 0), (b"/a/", 1, M.PREFIX)],
                [(b"/a", 0, 2)], [(b"/", 0, 0), (b"/", 1, 0)]):
        with pytest.raises(ValueError):
            M.table(bad)
    for slots in (3, 1, 2, 6):
        with pytest.raises(ValueError):
            M.table([(b"/a", 0, 0), (b"/b", 1, 0)], slots)
    assert M.table([(b"/a", 0, 0), (b"/b", 1, 0)], 4) and M.table([], 1) == {}
    assert RC.smallest_slots(0) == 1 and RC.smallest_slots(63) == 64 and RC.smallest_slots(64) == 128


def test_rows_of_the_call():
    req = b"GET /nope?x HTTP/1.1\r\nHost: a\r\n\r\n"
    acc = dict(status=AM.ACCEPTED, http_status=101, reason=0, consumed=len(req), resp_len=129, path_off=4, path_len=7,
               key_off=AM.NO_KEY)
    none = dict(status=M.NOT_ACCEPTED, room=M.ROOM_NONE, route=M.NO_ROUTE, key_off=0, key_len=0)
    assert M.route(NOROOT, req, len(req), dict(acc, status=0), 200, 0, 1) == (none, dict(acc, status=0), None, None)
    assert M.route(NOROOT, req, len(req), dict(acc, status=AM.REJECTED), 200, 0, 1)[0] == none
    row, ares, out, stored = M.route(NOROOT, req, len(req), acc, 200, 0, 1, default_room=9)
    assert (row["status"], row["room"], row["route"], row["key_off"], row["key_len"]) == (M.MISS, 9, M.NO_ROUTE, 4, 5)
    assert ares == acc and out is None and stored == 9
    row, ares, out, stored = M.route(NOROOT, req, len(req), acc, 63, 0, 1, default_room=9, policy=M.MISS_404)
    assert (row["status"], row["room"]) == (M.MISS | M.NOT_FOUND, M.ROOM_NONE) and stored == M.ROOM_NONE
    assert out == M.RESP_404[:63] and ares == dict(status=AM.REJECTED | AM.TRUNCATED, http_status=404, reason=11,
                                                   consumed=len(req), resp_len=64, path_off=0, path_len=0,
                                                   key_off=AM.NO_KEY)
    assert M.route(NOROOT, req, len(req), acc, 64, 0, 1, policy=M.MISS_404)[1]["status"] == AM.REJECTED
    # rconn: none wanted, and out of range
    assert M.route(NOROOT, req, len(req), acc, 64, M.NO_ROW, 1)[3] is None
    row, _, _, stored = M.route(ROOT, req, len(req), acc, 64, 1, 1)
    assert row["status"] == M.MATCHED | M.BY_PREFIX | M.BAD_ROW and stored is None
    # an accept row that names bytes behind the request: nothing but the route row
    row, ares, out, stored = M.route(ROOT, req, 10, acc, 64, 0, 1, default_room=3, policy=M.MISS_404)
    assert (row["status"], row["room"], row["key_len"]) == (M.MISS | M.BAD_ROW | M.NOT_FOUND, M.ROOM_NONE, 0)
    assert ares == acc and out is None and stored is None
    assert M.route(ROOT, req, 10, acc, 64, 0, 1, default_room=3)[0]["room"] == 3
    # a table that is none
    row = M.route(ROOT, req, len(req), acc, 64, 0, 1, bad_table=True)[0]
    assert row["status"] == M.MISS | M.BAD_TABLE
    assert len(M.pack_result(row)) == 32

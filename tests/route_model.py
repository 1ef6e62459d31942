"""xyws_route_build, xyws_route_lookup and xyws_route_streams in plain Python,
from the rules of include/xyws.h alone: the table is a dict of keys in normal
form, and a match is found by trying the key P of a target and each cut of P
in front of a `/`. Also the 404 and the accept row a miss under MISS_404
leaves, from tests/accept_model.py's rows."""
import accept_model as AM

KEY_MAX, WINDOW = 256, 257
PREFIX = 0x1
NO_ROW = NO_ROUTE = ROOM_NONE = 0xFFFFFFFF
MISS_404 = 0x1
MATCHED, BY_PREFIX, MISS, NOT_FOUND, NOT_ACCEPTED, BAD_ROW, BAD_TABLE = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40
R_NOT_FOUND = 11
RESP_404 = b"HTTP/1.1 404 Not Found\r\nConnection: close\r\nContent-Length: 0\r\n\r\n"
assert len(RESP_404) == 64


def normal(key):
    return key[:-1] if len(key) > 1 and key.endswith(b"/") else key


def table(routes, slots=0):
    """{key in normal form: (room, index, flags)} of (key, room, flags)
    triples; ValueError for what xyws_route_build refuses."""
    if slots and (slots & (slots - 1) or slots <= len(routes)):
        raise ValueError("slots")
    tab = {}
    for index, (key, room, flags) in enumerate(routes):
        if not 1 <= len(key) <= KEY_MAX or b"?" in key or b"#" in key or flags & ~PREFIX or normal(key) in tab:
            raise ValueError("route %d" % index)
        tab[normal(key)] = (room, index, flags)
    return tab


def key_of(target):
    """The key P of a request target: up to the first `?` or `#` among its
    first WINDOW bytes, one trailing `/` dropped where that byte is among
    them."""
    w = target[:WINDOW]
    cuts = [i for i, c in enumerate(w) if c in b"?#"]
    p = target[:cuts[0]] if cuts else target
    if 1 < len(p) <= len(w) and p.endswith(b"/"):
        p = p[:-1]
    return p


def lookup(tab, target, bad_table=False):
    """xyws_route_lookup's result row (a dict) for `target` over the dict
    `tab` (None: no table at all); bad_table: bytes were given that are none."""
    p = key_of(target)
    best = None
    if tab and not bad_table:
        if len(p) <= KEY_MAX and p in tab:
            best = p
        for j in range(min(len(p) - 1, KEY_MAX), 0, -1):  # the cuts of P, the longest first
            if best is None and (p[j:j + 1] == b"/" or (j == 1 and p[:1] == b"/")):
                if p[:j] in tab and tab[p[:j]][2] & PREFIX:
                    best = p[:j]
    bad = BAD_TABLE if bad_table else 0
    if best is None:
        return dict(status=MISS | bad, room=ROOM_NONE, route=NO_ROUTE, key_off=0, key_len=len(p))
    room, index, _ = tab[best]
    return dict(status=MATCHED | (BY_PREFIX if len(best) < len(p) else 0) | bad, room=room, route=index, key_off=0,
                key_len=len(p))


def route(tab, req, length, ares, out_cap, rconn, n_rconns, default_room=ROOM_NONE, policy=0, bad_table=False):
    """One row of xyws_route_streams: the connection sent req[:length], its
    accept row is the dict `ares`. Returns (route row, the accept row after
    the call, the bytes written to out or None, the room stored to roster row
    `rconn` or None)."""
    if not ares["status"] & AM.ACCEPTED:
        return dict(status=NOT_ACCEPTED, room=ROOM_NONE, route=NO_ROUTE, key_off=0, key_len=0), ares, None, None
    off, plen = ares["path_off"], ares["path_len"]
    if off + plen > min(length, AM.MAX_REQUEST):  # a lying row: nothing is read, the route row alone is written
        row = dict(status=MISS | BAD_ROW | (BAD_TABLE if bad_table else 0), room=ROOM_NONE, route=NO_ROUTE, key_off=0,
                   key_len=0)
        if policy & MISS_404:
            row["status"] |= NOT_FOUND
        else:
            row["room"] = default_room
        return row, ares, None, None
    row = lookup(tab, req[off:off + plen], bad_table)
    row["key_off"] = off
    out = None
    if row["status"] & MISS:
        if policy & MISS_404:
            row["status"] |= NOT_FOUND
            out = RESP_404[:out_cap]
            ares = dict(ares, status=AM.REJECTED | (AM.TRUNCATED if out_cap < 64 else 0), http_status=404,
                        reason=R_NOT_FOUND, resp_len=64, path_off=0, path_len=0, key_off=AM.NO_KEY)
        else:
            row["room"] = default_room
    stored = row["room"] if rconn != NO_ROW and rconn < n_rconns else None
    if rconn != NO_ROW and rconn >= n_rconns:
        row["status"] |= BAD_ROW
    return row, ares, out, stored


def pack_result(r):
    """The 32 bytes of an xyws_route_result."""
    return b"".join(r[f].to_bytes(4, "little") for f in ("status", "room", "route", "key_off", "key_len")) + bytes(12)

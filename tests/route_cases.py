"""Route tables and request targets shared by the CPU and GPU tests of
xyws_route_streams: TABLES = {name: [(key, room, flags)]}, TARGETS = [(name,
target bytes)]; every target is looked up in every table. Key lengths sit
around the kernel's boundaries: 4 bytes per lane, 16 per staged line, 256 in
the window."""
import random

import route_model as M

P = M.PREFIX
K255, K256 = b"/" + b"k" * 254, b"/" + b"m" * 255
EDGE_LENGTHS = (2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)


def edge_key(n):
    return (b"/e%d" % n + b"p" * n)[:n]


ROUTES = [
    (b"/", 0, P),                # the catch-all
    (b"/a", 1, P),
    (b"/rooms", 2, P),
    (b"/rooms/b", 3, 0),         # exact, nested in a prefix route
    (b"/rooms/b/deep", 4, P),
    (b"/exact", 5, 0),
    (b"/slash/", 6, 0),          # given with its slash: /slash
    (b"chat", 7, 0),             # no leading slash
    (K255, 8, 0),
    (K256, 9, P),
    (b"/long", 10, P),
    (b"/a//", 11, P),            # /a/
    (b"x", 12, P),               # one byte, not the root
] + [(edge_key(n), 100 + n, 0) for n in EDGE_LENGTHS]
assert all(len(edge_key(n)) == n for n in EDGE_LENGTHS)

TABLES = {"root": ROUTES, "noroot": ROUTES[1:], "one": [(b"/rooms/b", 3, 0)], "none": []}

TARGETS = [
    ("root", b"/"), ("below_root", b"/zzz"), ("a", b"/a"), ("ab", b"/ab"), ("a_slash", b"/a/"), ("a_b", b"/a/b"),
    ("a_query", b"/a?x=1"), ("a_query_end", b"/a?"), ("a_slash_query", b"/a/?x"), ("a_fragment", b"/a#top"),
    ("query_first", b"?x=1"), ("fragment_first", b"#"), ("query_then_slash", b"/a?/rooms/b"),
    ("rooms_b_query", b"/rooms/b?x=1"), ("rooms_b_slash", b"/rooms/b/"), ("rooms_b_c", b"/rooms/b/c"),
    ("rooms_b_deep", b"/rooms/b/deep"), ("rooms_b_deeper", b"/rooms/b/deep/er/still"), ("rooms", b"/rooms"),
    ("roomsx", b"/roomsx"), ("exact", b"/exact"), ("exact_slash", b"/exact/"), ("exact_below", b"/exact/x"),
    ("slash", b"/slash"), ("slash_slash", b"/slash/"), ("chat", b"chat"), ("chat_below", b"chat/x"),
    ("chatx", b"chatx"), ("x", b"x"), ("x_below", b"x/y"), ("double", b"//"), ("double_a", b"//a"),
    ("a_double_b", b"/a//b"), ("a_double", b"/a//"), ("a_triple", b"/a///"), ("nope", b"/nope"),
    ("k255", K255), ("k255_slash", K255 + b"/"), ("k256", K256), ("k256_slash", K256 + b"/"),
    ("k256_query", K256 + b"?q"), ("k256_below", K256 + b"/x"), ("k257", K256 + b"m"), ("k257_slash", K256 + b"m/"),
    ("k256_slash_query", K256 + b"/?q"), ("k255_x", K255 + b"x"),
    ("long_300", b"/long/" + b"z" * 294), ("long_300_query_late", b"/long/" + b"z" * 274 + b"?" + b"q" * 19),
    ("flat_300", b"/" + b"q" * 299), ("slashes_300", b"/" * 300), ("pairs_300", b"/a" * 150),
] + [("edge_%d" % n, edge_key(n)) for n in EDGE_LENGTHS] + \
    [("edge_%d_slash" % n, edge_key(n) + b"/") for n in (4, 16, 64)] + \
    [("edge_%d_short" % n, edge_key(n)[:-1]) for n in (4, 16, 17, 64)]
NAMES = [n for n, _ in TARGETS]
assert len(set(NAMES)) == len(NAMES)
assert len(dict(TARGETS)["long_300"]) == len(dict(TARGETS)["long_300_query_late"]) == 300


def smallest_slots(n_routes):
    """The next power of two above n_routes: the smallest xyws_route_build takes."""
    s = 1
    while s <= n_routes:
        s <<= 1
    return s


def random_keys(n, seed=0x707E):
    rng = random.Random(seed)
    keys = set()
    while len(keys) < n:
        keys.add(b"/r/" + bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz0123456789-_") for _ in range(rng.randint(1, 40))))
    return sorted(keys)

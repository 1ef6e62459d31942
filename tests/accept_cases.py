"""Handshake requests shared by the CPU and GPU tests of xyws_accept_streams
and by tests/golden/gen_handshake_golden.py, which runs the reference's
websocket_request_handler on every one of them: CASES is a list of
(name, request bytes). TRUNCATED names the three whose every truncation the
fixtures hold."""
import random

RFC_KEY = b"dGhlIHNhbXBsZSBub25jZQ=="
RFC_ACCEPT = b"s3pPLMBiTxaQ9kYGzzhZRbK+xOo="
NO_KEY_ACCEPT = b"PqANCZjv3XGbmDfyXk3WqicE950="

# RFC 6455 1.3
RFC = (b"GET /chat HTTP/1.1\r\nHost: server.example.com\r\nUpgrade: websocket\r\nConnection: Upgrade\r\n"
       b"Sec-WebSocket-Key: dGhlIHNhbXBsZSBub25jZQ==\r\nOrigin: http://example.com\r\n"
       b"Sec-WebSocket-Protocol: chat, superchat\r\nSec-WebSocket-Version: 13\r\n\r\n")


def browser(key=b"x3JJHMbDL1EzLkh9GBhXDw==", path=b"/rooms/lobby"):
    """A browser-shaped request: 13 headers, 499 bytes with the default path."""
    req = (b"GET " + path + b" HTTP/1.1\r\n"
           b"Host: chat.example.org:8443\r\n"
           b"Connection: Upgrade\r\n"
           b"Pragma: no-cache\r\n"
           b"Cache-Control: no-cache\r\n"
           b"User-Agent: Mozilla/5.0 (X11; Linux x86_64) AppleWebKit/537.36 Chrome/120.0.0.0 "
           b"Safari/537.36\r\n"
           b"Upgrade: websocket\r\n"
           b"Origin: https://chat.example.org\r\n"
           b"Sec-WebSocket-Version: 13\r\n"
           b"Accept-Encoding: gzip, deflate, br\r\n"
           b"Accept-Language: en-GB,en;q=0.9,de;q=0.8\r\n"
           b"Sec-WebSocket-Key: " + key + b"\r\n"
           b"Sec-WebSocket-Extensions: permessage-deflate\r\n"
           b"Cookie: sid=3f9a1c; theme=dark\r\n\r\n")
    return req


BROWSER = browser()
assert len(BROWSER) == 499, len(BROWSER)


def req(line=b"GET /chat HTTP/1.1", headers=None, end=b"\r\n", eol=b"\r\n", lead=b"", tail=b""):
    """A request from its parts; the default headers are the minimal valid set."""
    if headers is None:
        headers = MINIMAL
    return lead + line + eol + b"".join(h + eol for h in headers) + end + tail


H_HOST, H_UP, H_CONN = b"Host: a", b"Upgrade: websocket", b"Connection: Upgrade"
H_KEY, H_VER = b"Sec-WebSocket-Key: " + RFC_KEY, b"Sec-WebSocket-Version: 13"
MINIMAL = [H_HOST, H_UP, H_CONN, H_KEY, H_VER]


def without(h):
    return [x for x in MINIMAL if x is not h]


def swapped(h, new):
    return [new if x is h else x for x in MINIMAL]


def many_headers(n, key_at=None):
    """n header lines, the minimal set among X-i fillers; the key at line key_at (default: in its usual place)."""
    fill = [b"X-%d: v%d" % (i, i) for i in range(n)]
    core = [H_HOST, H_UP, H_CONN, H_VER] if key_at is not None else list(MINIMAL)
    hs = core + fill[:n - len(core) - (key_at is not None)]
    if key_at is not None:
        hs.insert(key_at, H_KEY)
    assert len(hs) == n
    return hs


KEY_80 = bytes([0x80 + i for i in range(22)]) + b"\t\xff"  # 24 bytes >= 0x80 and an HT (not trailing)

CASES = [
    ("rfc", RFC),
    ("browser", BROWSER),
    ("minimal", req()),
    ("frames_behind", req(tail=b"\x81\x85\x37\xfa\x21\x3d\x7f\x9f\x4d\x51\x58")),
    ("second_request_behind", req(tail=b"GET / HTTP/1.1\r\n\r\n")),
    ("garbage_behind", req(tail=b"\x00\x01\x7f\r\r\n:")),
    # leading line
    ("lead_crlf", req(lead=b"\r\n")),
    ("lead_lf", req(lead=b"\n")),
    ("lead_two_crlf", req(lead=b"\r\n\r\n")),
    ("lead_cr_only", req(lead=b"\rX")),
    ("lead_sp", req(lead=b" ")),
    # line ends
    ("lf_only", req(eol=b"\n", end=b"\n")),
    ("lf_mixed", req(eol=b"\n", end=b"\r\n")),
    ("request_line_cr_x", b"GET / HTTP/1.1\rX\r\n\r\n"),
    ("header_cr_x", req(headers=swapped(H_HOST, b"Host: a\rb"))),
    ("end_cr_x", req(end=b"\rX")),
    # method and target
    ("post", req(line=b"POST /chat HTTP/1.1")),
    ("get_lower", req(line=b"get /chat HTTP/1.1")),
    ("method_long", req(line=b"GETT /chat HTTP/1.1")),
    ("method_ctl", req(line=b"G\x01T /chat HTTP/1.1")),
    ("method_del", req(line=b"G\x7fT /chat HTTP/1.1")),
    ("method_high", req(line=b"G\xc3\xa9T /chat HTTP/1.1")),
    ("method_ht", req(line=b"GET\t/chat HTTP/1.1")),
    ("target_ctl", req(line=b"GET /ch\x1fat HTTP/1.1")),
    ("target_del", req(line=b"GET /ch\x7fat HTTP/1.1")),
    ("target_high", req(line=b"GET /r\xc3\xa4ume/\xff HTTP/1.1")),
    ("target_long", req(line=b"GET /" + b"a" * 300 + b"?q=1 HTTP/1.1")),
    ("target_star", req(line=b"GET * HTTP/1.1")),
    ("no_target", req(line=b"GET HTTP/1.1")),
    ("no_method", req(line=b" /chat HTTP/1.1")),
    ("target_lf", req(line=b"GET /chat\nHTTP/1.1")),
    # spaces
    ("spaces_runs", req(line=b"GET    /chat     HTTP/1.1")),
    ("space_after_version", req(line=b"GET /chat HTTP/1.1 ")),
    ("ht_between", req(line=b"GET /chat\tHTTP/1.1")),
    # version
    ("http10", req(line=b"GET /chat HTTP/1.0")),
    ("http12", req(line=b"GET /chat HTTP/1.2")),
    ("http19", req(line=b"GET /chat HTTP/1.9")),
    ("http20", req(line=b"GET /chat HTTP/2.0")),
    ("http1x", req(line=b"GET /chat HTTP/1.x")),
    ("http_lower", req(line=b"GET /chat http/1.1")),
    ("http_11_long", req(line=b"GET /chat HTTP/1.11")),
    ("version_short_wrong", b"GET /chat XTTP/1\r\n"),
    ("version_9_wrong", b"GET /chat XTTP/1.1"),
    ("version_8_right", b"GET /chat HTTP/1.1"),
    # header names
    ("name_lower", req(headers=[b"host: a", b"upgrade: websocket", b"connection: Upgrade",
                                b"sec-websocket-key: " + RFC_KEY, b"sec-websocket-version: 13"])),
    ("name_upper", req(headers=[b"HOST: a", b"UPGRADE: websocket", b"CONNECTION: Upgrade",
                                b"SEC-WEBSOCKET-KEY: " + RFC_KEY, b"SEC-WEBSOCKET-VERSION: 13"])),
    ("name_lower_bad_values", req(headers=[b"Host: a", b"upgrade: h2c", b"connection: close",
                                           b"sec-websocket-key: short", b"sec-websocket-version: 8"])),
    ("name_empty", req(headers=swapped(H_HOST, b": a"))),
    ("name_sp_colon", req(headers=swapped(H_HOST, b"Host : a"))),
    ("name_no_colon", req(headers=swapped(H_HOST, b"Host a"))),
    ("name_bad_char", req(headers=swapped(H_HOST, b"Ho(st: a"))),
    ("name_high", req(headers=swapped(H_HOST, b"H\xf6st: a"))),
    ("name_all_token", req(headers=MINIMAL + [b"!#$%&'*+-.^_`|~09AZaz: v"])),
    ("name_at", req(headers=MINIMAL + [b"a@b: v"])),
    ("first_header_sp", req(headers=[b" Host: a"] + MINIMAL[1:])),
    ("first_header_ht", req(headers=[b"\tHost: a"] + MINIMAL[1:])),
    # header values
    ("value_no_sp", req(headers=[b"Host:a", b"Upgrade:websocket", b"Connection:Upgrade",
                                 b"Sec-WebSocket-Key:" + RFC_KEY, b"Sec-WebSocket-Version:13"])),
    ("value_sp_ht", req(headers=[b"Host: \t a", b"Upgrade:\t websocket \t", b"Connection:  Upgrade\t\t ",
                                 b"Sec-WebSocket-Key: \t" + RFC_KEY + b" \t ", b"Sec-WebSocket-Version:\t13 "])),
    ("value_empty", req(headers=MINIMAL + [b"X-Empty:", b"X-Spaces:  \t "])),
    ("value_ctl", req(headers=MINIMAL + [b"X: a\x01b"])),
    ("value_nul", req(headers=MINIMAL + [b"X: a\x00b"])),
    ("value_del", req(headers=MINIMAL + [b"X: a\x7fb"])),
    ("value_ht_inside", req(headers=MINIMAL + [b"X: a\tb"])),
    ("value_high", req(headers=MINIMAL + [b"X: gr\xfc\xdf\x80\xff"])),
    ("value_colons", req(headers=MINIMAL + [b"X: a:b: c"])),
    # folded lines
    ("folded_after_all", req(headers=MINIMAL + [b" folded"])),
    ("folded_ht", req(headers=MINIMAL + [b"\tfolded: x"])),
    ("folded_hides_bad_version", req(headers=[H_HOST, H_UP, b" more", H_CONN, H_KEY, b"Sec-WebSocket-Version: 8"])),
    ("folded_hides_key", req(headers=[H_HOST, H_UP, H_CONN, H_VER, b" more", H_KEY])),
    ("folded_hides_short_key", req(headers=[H_HOST, H_UP, H_CONN, H_VER, b"\tmore", b"Sec-WebSocket-Key: short"])),
    ("folded_empty_value", req(headers=MINIMAL + [b" "])),
    ("bad_version_then_folded", req(headers=[H_HOST, H_UP, H_CONN, H_KEY, b"Sec-WebSocket-Version: 8", b" x"])),
    # header counts
    ("headers_63", req(headers=many_headers(63))),
    ("headers_64", req(headers=many_headers(64))),
    ("headers_65", req(headers=many_headers(65))),
    ("headers_100", req(headers=many_headers(100))),
    ("headers_101", req(headers=many_headers(101))),
    ("headers_100_key_last", req(headers=many_headers(100, key_at=99))),
    ("headers_100_folded_last", req(headers=many_headers(99) + [b" f"])),
    ("headers_101_folded_last", req(headers=many_headers(100) + [b" f"])),
    ("key_first", req(headers=[H_KEY, H_HOST, H_UP, H_CONN, H_VER])),
    ("key_line_64", req(headers=many_headers(80, key_at=63))),
    ("key_line_65", req(headers=many_headers(80, key_at=64))),
    ("no_headers", req(headers=[])),
    # the four checked headers
    ("no_host", req(headers=without(H_HOST))),
    ("no_upgrade", req(headers=without(H_UP))),
    ("no_connection", req(headers=without(H_CONN))),
    ("no_key", req(headers=without(H_KEY))),
    ("no_version", req(headers=without(H_VER))),
    ("only_host", req(headers=[H_HOST])),
    ("upgrade_case", req(headers=swapped(H_UP, b"Upgrade: WebSocket"))),
    ("upgrade_list", req(headers=swapped(H_UP, b"Upgrade: h2c, \twebsocket\t ,x"))),
    ("upgrade_other", req(headers=swapped(H_UP, b"Upgrade: h2c"))),
    ("upgrade_prefix", req(headers=swapped(H_UP, b"Upgrade: websocket/13"))),
    ("upgrade_empty", req(headers=swapped(H_UP, b"Upgrade:"))),
    ("upgrade_commas", req(headers=swapped(H_UP, b"Upgrade: ,,websocket,,"))),
    ("upgrade_two_headers", req(headers=[H_HOST, b"Upgrade: h2c", H_UP, H_CONN, H_KEY, H_VER])),
    ("upgrade_two_headers_bad_last", req(headers=[H_HOST, H_UP, b"Upgrade: h2c", H_CONN, H_KEY, H_VER])),
    ("connection_list", req(headers=swapped(H_CONN, b"Connection: keep-alive, Upgrade"))),
    ("connection_lower", req(headers=swapped(H_CONN, b"Connection: upgrade"))),
    ("connection_close", req(headers=swapped(H_CONN, b"Connection: close"))),
    ("connection_inner_sp", req(headers=swapped(H_CONN, b"Connection: Up grade"))),
    ("version_8", req(headers=swapped(H_VER, b"Sec-WebSocket-Version: 8"))),
    ("version_013", req(headers=swapped(H_VER, b"Sec-WebSocket-Version: 013"))),
    ("version_list", req(headers=swapped(H_VER, b"Sec-WebSocket-Version: 13, 8"))),
    ("version_twice", req(headers=MINIMAL + [H_VER])),
    ("version_twice_bad_first", req(headers=[H_HOST, H_UP, H_CONN, H_KEY, b"Sec-WebSocket-Version: 8", H_VER])),
    ("version_8_and_post", req(line=b"POST /chat HTTP/1.1", headers=swapped(H_VER, b"Sec-WebSocket-Version: 8"))),
    ("version_8_no_key", req(headers=[H_HOST, H_UP, H_CONN, b"Sec-WebSocket-Version: 8"])),
    # the key
    ("key_twice", req(headers=MINIMAL + [b"Sec-WebSocket-Key: AAAAAAAAAAAAAAAAAAAAAA=="])),
    ("key_twice_short_first", req(headers=[b"Sec-WebSocket-Key: short"] + MINIMAL)),
    ("key_twice_short_last", req(headers=MINIMAL + [b"Sec-WebSocket-Key: short"])),
    ("key_23", req(headers=swapped(H_KEY, b"Sec-WebSocket-Key: " + RFC_KEY[:23]))),
    ("key_25", req(headers=swapped(H_KEY, b"Sec-WebSocket-Key: " + RFC_KEY + b"="))),
    ("key_empty", req(headers=swapped(H_KEY, b"Sec-WebSocket-Key:"))),
    ("key_high_ht", req(headers=swapped(H_KEY, b"Sec-WebSocket-Key: " + KEY_80))),
    ("key_24_not_base64", req(headers=swapped(H_KEY, b"Sec-WebSocket-Key: !!!!!!!!!!!!!!!!!!!!!!=="))),
    ("key_bad_last_char", req(headers=swapped(H_KEY, b"Sec-WebSocket-Key: dGhlIHNhbXBsZSBub25jZR=="))),
    ("key_one_pad", req(headers=swapped(H_KEY, b"Sec-WebSocket-Key: dGhlIHNhbXBsZSBub25jZQA="))),
    ("key_no_pad", req(headers=swapped(H_KEY, b"Sec-WebSocket-Key: dGhlIHNhbXBsZSBub25jZQAA"))),
    ("key_plus_slash", req(headers=swapped(H_KEY, b"Sec-WebSocket-Key: ++++////++++////++++/w=="))),
    ("key_trailing_sp_24", req(headers=swapped(H_KEY, b"Sec-WebSocket-Key: " + RFC_KEY[:22] + b"  "))),
    ("key_placeholder_itself", req(headers=swapped(H_KEY, b"Sec-WebSocket-Key: XXXXXXXXXXXXXXXXXXXXXX=="))),
    # ignored: subprotocols and extensions
    ("protocol_extensions", req(headers=MINIMAL + [b"Sec-WebSocket-Protocol: chat",
                                                   b"Sec-WebSocket-Extensions: permessage-deflate"])),
    # not a request at all
    ("tls_hello", b"\x16\x03\x01\x02\x00\x01\x00\x01\xfc\x03\x03" + bytes(range(40))),
    ("frame_first", b"\x81\x85\x37\xfa\x21\x3d\x7f\x9f\x4d\x51\x58"),
    ("spaces_only", b"          "),
    ("lf_only_bytes", b"\n\n\n"),
    ("empty", b""),
]

NAMES = [n for n, _ in CASES]
assert len(set(NAMES)) == len(NAMES)
BY_NAME = dict(CASES)
TRUNCATED = ["rfc", "value_sp_ht", "key_twice_short_last"]
# one request that is refused for its grammar, for the launch of all its truncations
REJECTED_FOR_GRAMMAR = "value_ctl"


def random_keys(n, seed=0x5EED):
    """n canonical Sec-WebSocket-Key values."""
    import base64
    rng = random.Random(seed)
    return [base64.b64encode(bytes(rng.randrange(256) for _ in range(16))) for _ in range(n)]

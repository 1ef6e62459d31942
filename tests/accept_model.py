"""A plain-Python model of xyws_accept_streams / xyws_accept_request
(include/xyws.h, "many connections, one opening handshake call"): the
sequential walk of picohttpparser's phr_parse_request as a fresh http_parser
runs it, the two policies' checks and the three responses. The accept value
comes from hashlib and base64, so the library's own SHA-1 and base64 have an
independent check. Nothing here is shared with the library's source."""
import base64
import functools
import hashlib

ACCEPTED, REJECTED, TRUNCATED = 0x1, 0x2, 0x4
REFERENCE = 0x100
(R_NONE, R_PARSE, R_TOO_LONG, R_METHOD, R_VERSION, R_FOLDED, R_HOST, R_UPGRADE, R_CONNECTION, R_KEY,
 R_WS_VERSION) = range(11)
MAX_REQUEST = 8192
NO_KEY = 0xFFFFFFFF
GUID = b"258EAFA5-E914-47DA-95CA-C5AB0DC85B11"
PLACEHOLDER = b"XXXXXXXXXXXXXXXXXXXXXX=="

RESP_400_REF = b"HTTP/1.1 400 Bad Request\r\n"
RESP_400 = b"HTTP/1.1 400 Bad Request\r\nConnection: close\r\nContent-Length: 0\r\n\r\n"
RESP_426 = (b"HTTP/1.1 426 Upgrade Required\r\nSec-WebSocket-Version: 13\r\nConnection: close\r\n"
            b"Content-Length: 0\r\n\r\n")

TOKEN = set(b"!#$%&'*+-.^_`|~0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz")
B64 = set(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/")


def accept_value(key):
    return base64.b64encode(hashlib.sha1(bytes(key) + GUID).digest())


def response_101(key):
    return (b"HTTP/1.1 101 Switching Protocols\r\nUpgrade: websocket\r\nConnection: Upgrade\r\n"
            b"Sec-WebSocket-Accept: " + accept_value(key) + b"\r\n\r\n")


class Incomplete(Exception):
    pass


class Bad(Exception):
    pass


def parse(b):
    """phr_parse_request over all of b: (consumed, method, (path_off, path_len),
    minor, headers); headers are (name or None, name_off, value_off, value).
    Raises Incomplete (-2) or Bad (-1)."""
    E, p = len(b), 0

    def at(q):
        if q == E:
            raise Incomplete()
        return b[q]

    def eol(q):  # behind a CR
        if at(q) != 10:
            raise Bad()
        return q + 1

    c = at(p)
    if c == 13:
        p = eol(p + 1)
    elif c == 10:
        p += 1
    toks = []
    for _ in range(2):
        t0 = p
        while True:
            c = at(p)
            if c == 32:
                break
            if c < 32 or c == 127:
                raise Bad()
            p += 1
        toks.append((t0, p - t0))
        p += 1
        while p < E and b[p] == 32:
            p += 1
    if toks[0][1] == 0 or toks[1][1] == 0:
        raise Bad()
    if E - p < 9:
        raise Incomplete()
    if b[p:p + 7] != b"HTTP/1." or not 48 <= b[p + 7] <= 57:
        raise Bad()
    minor = b[p + 7] - 48
    p += 8
    if b[p] == 13:
        p = eol(p + 1)
    elif b[p] == 10:
        p += 1
    else:
        raise Bad()
    headers = []
    while True:
        c = at(p)
        if c == 13:
            p = eol(p + 1)
            break
        if c == 10:
            p += 1
            break
        if len(headers) == 100:
            raise Bad()
        name, n0 = None, p
        if not (headers and c in (32, 9)):
            while True:
                c = b[p]
                if c == 58:
                    break
                if c not in TOKEN:
                    raise Bad()
                p += 1
                at(p)
            if p == n0:
                raise Bad()
            name = bytes(b[n0:p])
            p += 1
            while at(p) in (32, 9):
                p += 1
        v0 = p
        while True:
            c = at(p)
            if (c < 32 and c != 9) or c == 127:
                break
            p += 1
        if c == 13:
            p = eol(p + 1)
            v1 = p - 2
        elif c == 10:
            v1 = p
            p += 1
        else:
            raise Bad()
        headers.append((name, n0, v0, bytes(b[v0:v1]).rstrip(b" \t")))
    return p, bytes(b[toks[0][0]:toks[0][0] + toks[0][1]]), toks[1], minor, headers


@functools.lru_cache(maxsize=1024)
def parse_event(b):
    """parse(b) as a value (both policies of one input share it): ("parsed", ...), ("incomplete",) or ("bad",)."""
    try:
        return ("parsed",) + parse(b)
    except Incomplete:
        return ("incomplete",)
    except Bad:
        return ("bad",)


def elements(value):
    return [e.strip(b" \t").lower() for e in value.split(b",")]


def key_is_canonical(v):
    return (len(v) == 24 and all(c in B64 for c in v[:21]) and v[21:22] in (b"A", b"Q", b"g", b"w")
            and v[22:] == b"==")


def failing_checks(policy, method, minor, headers):
    """(the failing XYWS_ACR_* checks, the offset of the key that is hashed)."""
    fail, key_off = set(), NO_KEY
    if method != b"GET":
        fail.add(R_METHOD)
    if policy & REFERENCE:
        if minor != 1:
            fail.add(R_VERSION)
        for name, _, v0, value in headers:
            if name is None:  # http_parser::headers() ends at the first nameless header
                break
            if name == b"Connection" and value != b"Upgrade":
                fail.add(R_CONNECTION)
            elif name == b"Upgrade" and value != b"websocket":
                fail.add(R_UPGRADE)
            elif name == b"Sec-WebSocket-Version" and value != b"13":
                fail.add(R_WS_VERSION)
            elif name == b"Sec-WebSocket-Key":
                if len(value) == 24:
                    key_off = v0
                else:
                    fail.add(R_KEY)
        return fail, key_off
    if minor < 1:
        fail.add(R_VERSION)
    if any(name is None for name, _, _, _ in headers):
        fail.add(R_FOLDED)
    named = [(name.lower(), v0, value) for name, _, v0, value in headers if name is not None]
    if not any(nm == b"host" for nm, _, _ in named):
        fail.add(R_HOST)
    if not any(nm == b"upgrade" and b"websocket" in elements(v) for nm, _, v in named):
        fail.add(R_UPGRADE)
    if not any(nm == b"connection" and b"upgrade" in elements(v) for nm, _, v in named):
        fail.add(R_CONNECTION)
    keys = [(v0, v) for nm, v0, v in named if nm == b"sec-websocket-key"]
    if len(keys) != 1 or not key_is_canonical(keys[0][1]):
        fail.add(R_KEY)
    else:
        key_off = keys[0][0]
    versions = [v for nm, _, v in named if nm == b"sec-websocket-version"]
    if len(versions) != 1 or versions[0] != b"13":
        fail.add(R_WS_VERSION)
    return fail, key_off


def accept(req, policy=0, max_request=1024, out_cap=1 << 20, length=None):
    """(result dict, the bytes written) for a connection that has sent `req`
    (length: its len when it is more than the bytes given, as only the first
    max_request are looked at)."""
    req = bytes(req)
    length = len(req) if length is None else length
    b = req[:min(length, max_request)]
    res = dict(status=0, http_status=0, reason=0, consumed=0, resp_len=0, path_off=0, path_len=0, key_off=NO_KEY)
    ev = parse_event(b)
    if ev[0] == "incomplete":
        if length < max_request:
            return res, b""
        reason, resp = R_TOO_LONG, None
    elif ev[0] == "bad":
        reason, resp = R_PARSE, None
    else:
        consumed, method, path, minor, headers = ev[1:]
        fail, key_off = failing_checks(policy, method, minor, headers)
        reason = min(fail) if fail else 0
        res["consumed"] = consumed  # (also when a check refuses it: the request still ends there)
        if not reason:
            key = b[key_off:key_off + 24] if key_off != NO_KEY else PLACEHOLDER
            resp = response_101(key)
            res.update(status=ACCEPTED, http_status=101, consumed=consumed, path_off=path[0], path_len=path[1],
                       key_off=key_off)
    if reason:
        if policy & REFERENCE:
            resp, http = RESP_400_REF, 400
        elif reason == R_WS_VERSION:
            resp, http = RESP_426, 426
        else:
            resp, http = RESP_400, 400
        res.update(status=REJECTED, http_status=http, reason=reason)
    res["resp_len"] = len(resp)
    if len(resp) > out_cap:
        res["status"] |= TRUNCATED
    return res, resp[:out_cap]


def pack_result(r):
    """The 32 bytes of an xyws_accept_result."""
    return (r["status"].to_bytes(4, "little") + r["http_status"].to_bytes(2, "little") +
            r["reason"].to_bytes(2, "little") + r["consumed"].to_bytes(4, "little") +
            r["resp_len"].to_bytes(4, "little") + r["path_off"].to_bytes(4, "little") +
            r["path_len"].to_bytes(4, "little") + r["key_off"].to_bytes(4, "little") + bytes(4))

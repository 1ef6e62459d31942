"""XYWS_ACC_DEFLATE: the handshake agrees to an offer of permessage-deflate (RFC 7692 7.1). CPU cases through
xyws_accept_request; one gpu case runs the same table through xyws_accept_streams."""
import ctypes as C

import pytest

import xynet_amd._lib as L

HEAD = b"GET /chat HTTP/1.1\r\nHost: x\r\nUpgrade: websocket\r\nConnection: Upgrade\r\n" \
       b"Sec-WebSocket-Key: dGhlIHNhbXBsZSBub25jZQ==\r\nSec-WebSocket-Version: 13\r\n"
LINE = b"Sec-WebSocket-Extensions: permessage-deflate; server_no_context_takeover; client_no_context_takeover\r\n"
PLAIN = b"HTTP/1.1 101 Switching Protocols\r\nUpgrade: websocket\r\nConnection: Upgrade\r\n" \
        b"Sec-WebSocket-Accept: s3pPLMBiTxaQ9kYGzzhZRbK+xOo=\r\n"


def ext(*values):
    return b"".join(b"Sec-WebSocket-Extensions: " + v + b"\r\n" for v in values)


CASES = {  # name: (extension headers, taken)
    "plain_offer": (ext(b"permessage-deflate"), True),
    "chrome": (ext(b"permessage-deflate; client_max_window_bits"), True),
    "behind_another_extension": (ext(b"x-webkit-deflate-frame, permessage-deflate; client_max_window_bits=12"), True),
    "two_headers": (ext(b"foo; bar=1", b"permessage-deflate"), True),
    "case_and_padding": (b"sec-websocket-EXTENSIONS:  \t PerMessage-Deflate ;\tCLIENT_NO_CONTEXT_TAKEOVER ; "
                         b"server_max_window_bits = \"10\" \r\n", True),
    "second_offer_passes": (ext(b"permessage-deflate; server_max_window_bits=7, permessage-deflate"), True),
    "no_offer": (ext(b"permessage-deflate-not, x"), False),
    "unknown_parameter": (ext(b"permessage-deflate; window=9"), False),
    "repeated_parameter": (ext(b"permessage-deflate; client_max_window_bits; client_max_window_bits=9"), False),
    "server_bits_7": (ext(b"permessage-deflate; server_max_window_bits=7"), False),
    "server_bits_16": (ext(b"permessage-deflate; server_max_window_bits=16"), False),
    "server_bits_bare": (ext(b"permessage-deflate; server_max_window_bits"), False),
    "client_bits_valued": (ext(b"permessage-deflate; client_max_window_bits=\"15\""), True),
    "client_bits_99": (ext(b"permessage-deflate; client_max_window_bits=99"), False),
    "takeover_with_a_value": (ext(b"permessage-deflate; client_no_context_takeover=foo"), False),
    "offer_inside_a_quoted_string": (ext(b"foo; x=\"a, permessage-deflate\", bar; y=\"\\\", permessage-deflate\""), False),
}


def accept(req, policy, cap=240):
    res, out = L.AcceptResult(), (C.c_uint8 * cap)()
    assert L.load().xyws_accept_request(req, len(req), 1024, policy, out, cap, C.byref(res)) == 0
    return res, bytes(out[:min(res.resp_len, cap)])


@pytest.mark.parametrize("policy", [L.ACC_DEFLATE, L.ACC_DEFLATE | L.ACC_REFERENCE], ids=["rfc", "reference"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_offer(name, policy):
    headers, taken = CASES[name]
    res, resp = accept(HEAD + headers + b"\r\n", policy)
    assert resp == PLAIN + (LINE if taken else b"") + b"\r\n" and res.resp_len == (231 if taken else 129)
    assert res.status == L.ACC_ACCEPTED | (L.ACC_DEFLATED if taken else 0) and res.http_status == 101
    assert accept(HEAD + headers + b"\r\n", policy & L.ACC_REFERENCE)[1] == PLAIN + b"\r\n"  # without the bit: as before


def test_rejected_and_truncated():
    bad = HEAD.replace(b"Version: 13", b"Version: 12") + CASES["plain_offer"][0] + b"\r\n"
    for policy in (0, L.ACC_DEFLATE):
        res, resp = accept(bad, policy)
        assert res.status == L.ACC_REJECTED and res.http_status == 426 and b"Extensions" not in resp and res.resp_len == 98
    res, resp = accept(HEAD + CASES["chrome"][0] + b"\r\n", L.ACC_DEFLATE, cap=144)  # the inbox's default response range
    assert res.status == L.ACC_ACCEPTED | L.ACC_DEFLATED | L.ACC_TRUNCATED and res.resp_len == 231
    assert resp == (PLAIN + LINE + b"\r\n")[:144]
    # without a result row nobody learns whether the extension was agreed: refused on the arguments alone
    req, out, fake = HEAD + b"\r\n", (C.c_uint8 * 240)(), C.cast(C.create_string_buffer(64), C.c_void_p)
    for policy in (L.ACC_DEFLATE, L.ACC_DEFLATE | L.ACC_REFERENCE):
        assert L.load().xyws_accept_request(req, len(req), 1024, policy, out, 240, None) == -1
        assert L.load().xyws_accept_streams(fake, fake, 1, 1024, policy, None, None) == -1
        assert L.load().xyws_accept_streams(fake, None, 0, 1024, policy, fake, None) == 0  # n == 0 with one: nothing launched


@pytest.mark.gpu
def test_the_same_table_on_the_device():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from xynet_amd import websocket as ws
    names = sorted(CASES)
    reqs = [HEAD + CASES[n][0] + b"\r\n" for n in names]
    grp = ws.connection_group(len(reqs))
    for policy in (L.ACC_DEFLATE, 0):
        bufs = [torch.tensor(list(r), dtype=torch.uint8, device="cuda") for r in reqs]
        outs = [torch.full((240,), 0xA5, dtype=torch.uint8, device="cuda") for _ in reqs]
        acc = grp.accept(bufs, outs, policy=policy)
        for k, n in enumerate(names):
            want, wres = accept(reqs[k], policy)[1], accept(reqs[k], policy)[0]
            assert acc.response(k) == want and acc.result(k).status == wres.status and acc.result(k).resp_len == len(want), n
            assert (outs[k][len(want):].cpu().numpy() == 0xA5).all(), n

"""XYWS_ACC_DEFLATE_SERVER_TAKEOVER through xyws_accept_request (the source xyws_accept_streams compiles): the four forms
of the extension line against the offers that select them, status bits, resp_len; without the bit every response is what it was."""
import ctypes as C

import pytest

from xynet_amd import _lib

D, CT, ST = _lib.ACC_DEFLATE, _lib.ACC_DEFLATE_TAKEOVER, _lib.ACC_DEFLATE_SERVER_TAKEOVER
S_NCT, C_NCT = "; server_no_context_takeover", "; client_no_context_takeover"
OFFERS = ["permessage-deflate", "permessage-deflate; client_max_window_bits", "permessage-deflate; server_no_context_takeover",
          "permessage-deflate; client_no_context_takeover",
          "permessage-deflate; client_no_context_takeover; server_no_context_takeover", None]


def accept(offer, policy):
    req = ("GET /chat HTTP/1.1\r\nHost: a\r\nUpgrade: websocket\r\nConnection: Upgrade\r\n"
           "Sec-WebSocket-Key: dGhlIHNhbXBsZSBub25jZQ==\r\nSec-WebSocket-Version: 13\r\n" +
           (f"Sec-WebSocket-Extensions: {offer}\r\n" if offer else "") + "\r\n").encode()
    out, res = C.create_string_buffer(256), _lib.AcceptResult()
    assert _lib.load().xyws_accept_request(req, len(req), 1024, policy, out, len(out), C.byref(res)) == 0
    return out.raw[:res.resp_len], res


@pytest.mark.parametrize("offer", OFFERS)
@pytest.mark.parametrize("policy", [D | ST, D | ST | CT, D | ST | _lib.ACC_REFERENCE, ST, 0, D, D | CT, _lib.ACC_REFERENCE | D])
def test_the_four_forms(offer, policy):
    """(Without the new bit the line keeps server_no_context_takeover: 102 or 74 bytes, 231 or 203 in all, as before.)"""
    resp, res = accept(offer, policy)
    agreed = bool(offer) and bool(policy & D)
    server = agreed and bool(policy & ST) and "server_no" not in offer
    client = agreed and bool(policy & CT) and "client_no" not in offer
    line = "Sec-WebSocket-Extensions: permessage-deflate" + ("" if server else S_NCT) + ("" if client else C_NCT) + "\r\n"
    want = _lib.ACC_ACCEPTED | (_lib.ACC_DEFLATED if agreed else 0) | (_lib.ACC_SERVER_TAKEOVER if server else 0) | \
        (_lib.ACC_TAKEOVER if client else 0)
    assert res.status == want and res.resp_len == len(resp) == 129 + (len(line) if agreed else 0)
    assert resp.endswith((line if agreed else "").encode() + b"\r\n") and resp.count(b"Extensions") == int(agreed)
    assert len(line) == 102 - 28 * (server + client) and res.resp_len <= _lib.ACCEPT_RESP_MAX
    assert resp[:129 - 2] == accept(None, 0)[0][:129 - 2]  # the 101 in front of the line is the plain one

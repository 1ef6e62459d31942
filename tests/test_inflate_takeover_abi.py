"""CPU checks of client context takeover's boundary: the export, the fields the inflate's rows gained inside their
reserved bytes (row sizes unchanged, offsets as xyws_rows.h computes them from include/xyws.h), and the handshake's
answer under XYWS_ACC_DEFLATE_TAKEOVER, byte for byte, through xyws_accept_request (no device)."""
import ctypes as C
import os
import subprocess

import pytest

import xynet_amd._lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [("xyws_inflate_conn", L.InflateConn, "window", 8), ("xyws_inflate_carry", L.InflateCarry, "win_len", 4),
          ("xyws_inflate_carry", L.InflateCarry, "win_pos", 4), ("xyws_inflate_result", L.InflateResult, "n_history", 4)]


def test_export_and_refusals():
    assert "xyws_inflate_windows_streams" in L.declared_symbols()
    lib, p = L.load(), C.cast(C.create_string_buffer(64), C.c_void_p)
    assert lib.xyws_inflate_windows_streams(None, p, p, p, p, p, 1, 0, p, p, p, None) == -1
    assert lib.xyws_inflate_windows_streams(p, p, p, p, p, p, 1, 2, p, p, p, None) == -1  # no new opts bit
    assert lib.xyws_inflate_windows_streams(p, None, None, None, None, None, 0, 1, None, None, None, None) == 0
    assert (L.INFC_TAKEOVER, L.ACC_DEFLATE_TAKEOVER, L.ACC_TAKEOVER) == (0x2, 0x400, 0x10)


def test_new_fields_lie_where_the_header_has_them(tmp_path):
    """The C structs through xyws_rows.h (whose asserts hold the fields to their words) against _lib.py's names."""
    lines = "".join(f'  printf("%zu %zu %zu\\n", sizeof({s}), offsetof({s}, {f}), sizeof((({s}*)0)->{f}));\n' for s, _, f, _ in FIELDS)
    src = tmp_path / "offsets.cpp"
    src.write_text('#include <stdio.h>\n#include "xyws_rows.h"\nint main() {\n' + lines + "  return 0;\n}\n")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(ROOT, "xynet_amd", "csrc"), str(src), "-o", str(tmp_path / "offsets")], check=True)
    got = [tuple(map(int, ln.split())) for ln in subprocess.run([str(tmp_path / "offsets")], check=True, capture_output=True,
                                                               text=True).stdout.splitlines()]
    assert got == [(C.sizeof(t), getattr(t, f).offset, size) for _, t, f, size in FIELDS]
    assert [g[0] for g in got] == [64, 32, 32, 32] and all(getattr(t, f).size == size for _, t, f, size in FIELDS)
    row = L.InflateConn()
    row.window = 0x7F0000001230
    assert row.window == row.reserved[0] == 0x7F0000001230 and L.InflateResult().n_history == 0


HEAD = ("GET /chat HTTP/1.1\r\nHost: h\r\nUpgrade: websocket\r\nConnection: Upgrade\r\n"
        "Sec-WebSocket-Key: dGhlIHNhbXBsZSBub25jZQ==\r\nSec-WebSocket-Version: 13\r\n")
LINE, NCT = "Sec-WebSocket-Extensions: permessage-deflate; server_no_context_takeover", "; client_no_context_takeover"
OFFERS = {  # name: (the header's value or None, the 101's extension line with the policy bit, XYWS_ACC_TAKEOVER)
    "plain": ("permessage-deflate", LINE, True),
    "client_no_context_takeover": ("permessage-deflate; client_no_context_takeover", LINE + NCT, False),
    "client_max_window_bits": ("permessage-deflate; client_max_window_bits", LINE, True),
    "two_alternatives": ("permessage-deflate; client_no_context_takeover; client_max_window_bits=10, permessage-deflate", LINE + NCT, False),
    "second_alternative_taken": ("permessage-deflate; server_max_window_bits, permessage-deflate", LINE, True),
    "no_offer": (None, None, False),
}


def accept(req, policy):
    out, res = C.create_string_buffer(256), L.AcceptResult()
    assert L.load().xyws_accept_request(req, len(req), 1024, policy, out, 256, C.byref(res)) == 0
    return out.raw[:res.resp_len], res.status


@pytest.mark.parametrize("name", OFFERS)
def test_the_101_under_the_takeover_policy(name):
    value, line, keeps = OFFERS[name]
    req = (HEAD + (f"Sec-WebSocket-Extensions: {value}\r\n" if value else "") + "\r\n").encode()
    base = ("HTTP/1.1 101 Switching Protocols\r\nUpgrade: websocket\r\nConnection: Upgrade\r\n"
            "Sec-WebSocket-Accept: s3pPLMBiTxaQ9kYGzzhZRbK+xOo=\r\n")
    today = (base + (LINE + NCT + "\r\n" if value else "") + "\r\n").encode(), L.ACC_ACCEPTED | (L.ACC_DEFLATED if value else 0)
    assert accept(req, L.ACC_DEFLATE) == today  # without the policy bit: today's bytes and status
    assert accept(req, 0) == accept(req, L.ACC_DEFLATE_TAKEOVER) == ((base + "\r\n").encode(), L.ACC_ACCEPTED)  # alone: nothing
    want = (base + (line + "\r\n" if line else "") + "\r\n").encode()
    assert accept(req, L.ACC_DEFLATE | L.ACC_DEFLATE_TAKEOVER) == (want, today[1] | (L.ACC_TAKEOVER if keeps else 0))

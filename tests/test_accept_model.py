"""The semantics of xyws_accept_streams, checked on the CPU: the Python model
(tests/accept_model.py) under XYWS_ACC_REFERENCE against what the reference's
websocket_request_handler answered (tests/golden/handshake.json: every case of
tests/accept_cases.py and every truncation of three of them), and the default
policy against hand-written expectations for each reason code."""
import pytest

import accept_cases as AC
import accept_model as M
from conftest import load_golden

GOLD = load_golden("handshake.json")


def input_of(e):
    return bytes.fromhex(e["req"]) if "req" in e else AC.BY_NAME[e["of"]][:e["len"]]


def test_fixtures_cover_every_case_and_truncation():
    whole = [e for e in GOLD if "req" in e]
    assert [e["name"] for e in whole] == AC.NAMES
    for e in whole:
        assert bytes.fromhex(e["req"]) == AC.BY_NAME[e["name"]], e["name"]
    cuts = [(e["of"], e["len"]) for e in GOLD if "of" in e]
    assert cuts == [(n, k) for n in AC.TRUNCATED for k in range(len(AC.BY_NAME[n]) + 1)]
    assert len(AC.BROWSER) == 499 and AC.BROWSER.count(b"\r\n") == 15  # request line, 13 headers, blank line


def test_model_equals_the_reference_on_every_fixture():
    """status, consumed and response bytes; a reference return of -2 is
    incomplete here (the one stated departure: the reference answers it with
    its 400), -1 the 26-byte 400."""
    seen = {"accepted": 0, "rejected_by_checks": 0, "parse": 0, "incomplete": 0}
    for e in GOLD:
        req = input_of(e)
        what = e.get("name") or (e["of"], e["len"])
        res, resp = M.accept(req, M.REFERENCE, max_request=M.MAX_REQUEST)
        ref_resp = bytes.fromhex(e["resp"])
        if e["parse"] == -2:
            assert ref_resp == M.RESP_400_REF, what
            assert (res["status"], res["http_status"], res["consumed"], resp) == (0, 0, 0, b""), what
            seen["incomplete"] += 1
        elif e["parse"] == -1:
            assert ref_resp == M.RESP_400_REF, what
            assert (res["status"], res["reason"], res["consumed"]) == (M.REJECTED, M.R_PARSE, 0), what
            assert resp == ref_resp, what
            seen["parse"] += 1
        else:
            assert e["parse"] > 0, what
            assert resp == ref_resp, what
            if len(ref_resp) == 129:
                assert (res["status"], res["http_status"], res["consumed"]) == (M.ACCEPTED, 101, e["parse"]), what
                seen["accepted"] += 1
            else:
                assert (res["status"], res["http_status"], res["consumed"]) == (M.REJECTED, 400, e["parse"]), what
                assert res["reason"] >= M.R_METHOD, what
                seen["rejected_by_checks"] += 1
    assert all(v >= 20 for v in seen.values()), seen


def test_known_accept_values():
    res, resp = M.accept(AC.RFC, M.REFERENCE)
    assert resp[97:125] == AC.RFC_ACCEPT and res["key_off"] == AC.RFC.index(AC.RFC_KEY)
    assert M.accept(AC.RFC, 0)[1] == resp and len(resp) == 129
    res, resp = M.accept(AC.BY_NAME["no_key"], M.REFERENCE)
    assert resp[97:125] == AC.NO_KEY_ACCEPT and res["key_off"] == M.NO_KEY
    assert (len(M.RESP_400_REF), len(M.RESP_400), len(M.RESP_426)) == (26, 66, 98)


# name -> (http status, reason) under the default policy; every case not listed is a 101
DEFAULT_EXPECT = {
    **{n: (400, M.R_PARSE) for n in (
        "lead_two_crlf", "lead_cr_only", "lead_sp", "request_line_cr_x", "header_cr_x", "end_cr_x", "method_ctl",
        "method_del", "method_ht", "target_ctl", "target_del", "no_target", "no_method", "target_lf",
        "space_after_version", "ht_between", "http20", "http1x", "http_lower", "http_11_long", "name_empty",
        "name_sp_colon", "name_no_colon", "name_bad_char", "name_high", "name_at", "first_header_sp",
        "first_header_ht", "value_ctl", "value_nul", "value_del", "headers_101", "headers_101_folded_last",
        "tls_hello", "frame_first", "lf_only_bytes")},
    **{n: (0, 0) for n in ("version_short_wrong", "version_9_wrong", "version_8_right", "spaces_only", "empty")},
    **{n: (400, M.R_METHOD) for n in ("post", "get_lower", "method_long", "method_high", "version_8_and_post")},
    "http10": (400, M.R_VERSION),
    **{n: (400, M.R_FOLDED) for n in (
        "folded_after_all", "folded_ht", "folded_hides_bad_version", "folded_hides_key", "folded_hides_short_key",
        "folded_empty_value", "bad_version_then_folded", "headers_100_folded_last")},
    **{n: (400, M.R_HOST) for n in ("no_headers", "no_host")},
    **{n: (400, M.R_UPGRADE) for n in ("no_upgrade", "only_host", "upgrade_other", "upgrade_prefix", "upgrade_empty",
                                       "name_lower_bad_values")},
    **{n: (400, M.R_CONNECTION) for n in ("no_connection", "connection_close", "connection_inner_sp")},
    **{n: (400, M.R_KEY) for n in (
        "no_key", "version_8_no_key", "key_twice", "key_twice_short_first", "key_twice_short_last", "key_23", "key_25",
        "key_empty", "key_high_ht", "key_24_not_base64", "key_bad_last_char", "key_one_pad", "key_no_pad",
        "key_trailing_sp_24", "key_placeholder_itself")},
    **{n: (426, M.R_WS_VERSION) for n in ("no_version", "version_8", "version_013", "version_list", "version_twice",
                                          "version_twice_bad_first")},
}


def test_default_policy_by_hand():
    assert set(DEFAULT_EXPECT) <= set(AC.NAMES)
    assert {r for _, r in DEFAULT_EXPECT.values()} == set(range(11)) - {M.R_TOO_LONG}  # TOO_LONG: below
    for name, req in AC.CASES:
        http, reason = DEFAULT_EXPECT.get(name, (101, 0))
        res, resp = M.accept(req, 0, max_request=M.MAX_REQUEST)
        assert (res["http_status"], res["reason"]) == (http, reason), name
        if http == 101:
            assert res["status"] == M.ACCEPTED and len(resp) == 129 and resp.startswith(b"HTTP/1.1 101 "), name
            assert req[res["consumed"] - 1:res["consumed"]] == b"\n", name
            assert req[res["path_off"]:res["path_off"] + res["path_len"]] in (
                b"/chat", b"*", b"/r\xc3\xa4ume/\xff", b"/" + b"a" * 300 + b"?q=1", b"/rooms/lobby"), name
        elif http == 0:
            assert res["status"] == 0 and resp == b"", name
        else:
            assert res["status"] == M.REJECTED and resp == (M.RESP_426 if http == 426 else M.RESP_400), name
    # what lies behind the blank line is the connection's, not the request's
    tail = AC.BY_NAME["frames_behind"]
    assert tail[M.accept(tail)[0]["consumed"]:] == b"\x81\x85\x37\xfa\x21\x3d\x7f\x9f\x4d\x51\x58"


@pytest.mark.parametrize("policy", [0, M.REFERENCE])
def test_too_long_and_truncated(policy):
    req = AC.RFC
    L = len(req)
    bad = M.RESP_400_REF if policy else M.RESP_400
    # max_request one less than the request: TOO_LONG; exactly its length: accepted
    res, resp = M.accept(req, policy, max_request=L - 1)
    assert (res["status"], res["http_status"], res["reason"], resp) == (M.REJECTED, 400, M.R_TOO_LONG, bad)
    assert M.accept(req, policy, max_request=L)[0]["status"] == M.ACCEPTED
    # a shorter piece of it is incomplete until max_request bytes are there
    assert M.accept(req[:50], policy, max_request=51)[0]["status"] == 0
    assert M.accept(req[:50], policy, max_request=50)[0]["reason"] == M.R_TOO_LONG
    # a grammar error before max_request stays PARSE
    assert M.accept(b"GET\x01" + req, policy, max_request=8)[0]["reason"] == M.R_PARSE
    for cap in (0, 25, 26, 128, 129, 130):
        res, resp = M.accept(req, policy, out_cap=cap)
        assert res["resp_len"] == 129 and resp == M.response_101(AC.RFC_KEY)[:cap]
        assert bool(res["status"] & M.TRUNCATED) == (cap < 129)

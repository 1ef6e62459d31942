"""xyws_accept_streams on the device: the opening handshakes of many
connections parsed, checked and answered by one launch. Expected values: the
Python model (tests/accept_model.py: a sequential walk, hashlib, base64).
Bar: bit-exact result rows and send ranges; not a guard byte changed around
any out range or behind row n; every input unchanged; the device error word 0
at the end.

Plumbing: a launch's requests lie in ONE guard-filled device buffer at chosen
misalignments, its out ranges in another (at chosen misalignments, or abutting
so that neighbours share 16-byte lines); the result rows have a guard row
behind them. The grid cap comes from xyws_debug_accept_geometry."""
import ctypes as C

import numpy as np
import pytest

import accept_cases as AC
import accept_model as M
from xynet_amd import _lib

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
GUARD = 0xA5
POLICIES = [0, M.REFERENCE]


@pytest.fixture(scope="module")
def ws():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from xynet_amd import websocket
    return websocket


@pytest.fixture()
def ctx(ws):
    """A context of the test's own; the device error word must read 0 at the end."""
    c = ws.Context(0)
    yield c
    assert c.last_device_error() == 0
    c.close()


def geometry():
    out = (C.c_uint64 * 4)()
    assert _lib.load().xyws_debug_accept_geometry(out) == 0
    return list(out)


class Entry:
    """One connection of a launch: `req` lies in the request buffer whole, len
    is `length` (default all of it; the bytes behind it are there and must not
    matter); its out range has out_cap bytes (out=False: a null pointer, with
    out_cap 0)."""

    def __init__(self, req, length=None, out_cap=129, bmis=0, omis=0, abut=False, out=True):
        self.req, self.length = bytes(req), len(req) if length is None else length
        self.out_cap, self.bmis, self.omis, self.abut, self.out = out_cap, bmis, omis, abut, out
        assert self.length <= len(self.req) and (out or not out_cap)


class Launch:
    """The tables and buffers of one xyws_accept_streams call and the model's
    answer to every entry."""

    def __init__(self, entries, policy, max_request, results=True):
        self.entries, self.policy, self.max_request = entries, policy, max_request
        n = self.n = len(entries)
        self.exp = [M.accept(e.req, policy, max_request, e.out_cap, length=e.length) for e in entries]
        pos, self.boffs = 64, []
        for e in entries:
            pos = (pos + 15) // 16 * 16 + 32 + e.bmis
            self.boffs.append(pos)
            pos += len(e.req)
        self.in_image = np.full(pos + 64, GUARD, np.uint8)
        for e, o in zip(entries, self.boffs):
            self.in_image[o:o + len(e.req)] = np.frombuffer(e.req, np.uint8)
        pos, self.ooffs = 64, []
        for e in entries:
            if not e.abut:
                pos = (pos + 15) // 16 * 16 + 32 + e.omis
            self.ooffs.append(pos)
            pos += e.out_cap
        self.out_image = np.full(pos + 64, GUARD, np.uint8)
        for (res, resp), o in zip(self.exp, self.ooffs):
            self.out_image[o:o + len(resp)] = np.frombuffer(resp, np.uint8)
        self.in_t = torch.from_numpy(self.in_image.copy()).cuda()
        self.out_t = torch.full((self.out_image.size,), GUARD, dtype=torch.uint8, device="cuda")
        tab = np.zeros((max(n, 1), 4), np.uint64)
        for k, e in enumerate(entries):
            tab[k] = (self.in_t.data_ptr() + self.boffs[k], e.length,
                      self.out_t.data_ptr() + self.ooffs[k] if e.out else 0, e.out_cap)
        self.tab_t = torch.from_numpy(tab.view(np.int64)).cuda()
        self.res_t = torch.full((32 * (n + 1),), GUARD, dtype=torch.uint8, device="cuda") if results else None

    def run(self, ctx, stream=None):
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        rc = ctx.L.xyws_accept_streams(ctx.h, C.c_void_p(self.tab_t.data_ptr()), self.n, self.max_request, self.policy,
                                       C.c_void_p(self.res_t.data_ptr()) if self.res_t is not None else None,
                                       C.c_void_p(s))
        assert rc == 0
        return self

    def check(self, what=""):
        out = self.out_t.cpu().numpy()
        bad = np.flatnonzero(out != self.out_image)
        if bad.size:
            k = max(i for i, o in enumerate(self.ooffs) if o <= bad[0] + 16) if self.ooffs else -1
            raise AssertionError((what, "out byte", int(bad[0]), "near entry", k, self.exp[k][0] if k >= 0 else None))
        if self.res_t is not None:
            rows = self.res_t.cpu().numpy().tobytes()
            for k, (res, _) in enumerate(self.exp):
                got = rows[32 * k:32 * k + 32]
                assert got == M.pack_result(res), (what, k, res, _lib.AcceptResult.from_buffer_copy(got).status,
                                                   got.hex())
            assert rows[32 * self.n:] == bytes([GUARD]) * 32, what  # the row behind n
        assert np.array_equal(self.in_t.cpu().numpy(), self.in_image), what  # every input unchanged
        return self


# --------------------------------------------------------------------------- 1. every case, both policies
@pytest.mark.parametrize("max_request", [1024, 8192])
@pytest.mark.parametrize("policy", POLICIES)
def test_every_case(ctx, policy, max_request):
    """All of accept_cases.py in one launch (the 63, 64, 65, 100 and 101 header
    lines, the key first, last, in line 64 and 65 among them); with
    max_request 1024 the long ones are TOO_LONG."""
    entries = [Entry(req, bmis=k % 16, omis=(5 * k) % 16) for k, (_, req) in enumerate(AC.CASES)]
    la = Launch(entries, policy, max_request).run(ctx).check()
    reasons = {res["reason"] for res, _ in la.exp}
    assert reasons >= (set(range(11)) - {M.R_TOO_LONG} if not policy else {0, 1, 3, 4, 7, 8, 9, 10})
    assert (M.R_TOO_LONG in reasons) == (max_request == 1024)


# --------------------------------------------------------------------------- 2. n and the grid stride
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_connection_counts(ctx, n):
    keys = AC.random_keys(n, seed=n)
    Launch([Entry(AC.browser(k), bmis=i % 16, abut=True) for i, k in enumerate(keys)], 0, 1024).run(ctx).check()


def test_past_the_grid_cap(ctx):
    """grid cap + 1 connections with tiny requests: the last one is the first
    workgroup's second connection."""
    cap = geometry()[3]
    tiny = [b"\n\n\n", b"GET", AC.BY_NAME["minimal"], b"", b"GET / HTTP/1.1\r\n\r\n", AC.BY_NAME["post"]]
    entries = [Entry(tiny[k % len(tiny)], out_cap=(26, 129, 66)[k % 3], bmis=k % 16, abut=True) for k in range(cap + 1)]
    la = Launch(entries, 0, 1024).run(ctx).check()
    assert la.n == cap + 1 and {r["status"] & 3 for r, _ in la.exp} == {0, M.ACCEPTED, M.REJECTED}


# --------------------------------------------------------------------------- 3. alignments, shared lines
def test_every_alignment(ctx):
    """Every buf alignment with every out alignment; each out group is an
    abutting 129-byte 101 and 26-byte 400 (the reference's), so neighbours share
    their first and last 16-byte lines. The key's 24 bytes straddle a line at
    most alignments."""
    entries = []
    for bm in range(16):
        for om in range(16):
            entries.append(Entry(AC.RFC, out_cap=129, bmis=bm, omis=om))
            entries.append(Entry(AC.BY_NAME["post"], out_cap=26, bmis=(bm + 7) % 16, abut=True))
            entries.append(Entry(AC.BY_NAME["no_key"], out_cap=129, bmis=(bm + 3) % 16, abut=True))
    la = Launch(entries, M.REFERENCE, 1024).run(ctx).check()
    assert [r["resp_len"] for r, _ in la.exp[:3]] == [129, 26, 129]


# --------------------------------------------------------------------------- 4. lengths
def sized(total, key_at=None):
    """A valid request of exactly `total` bytes (the target padded); key_at: the
    offset at which the key's 24 bytes begin (an X-Pad header in front of it)."""
    if key_at is None:
        base = AC.req(line=b"GET /p HTTP/1.1")
        return AC.req(line=b"GET /p" + b"a" * (total - len(base)) + b" HTTP/1.1")
    head = b"GET /p HTTP/1.1\r\nHost: a\r\nX-Pad: "
    name = b"\r\nSec-WebSocket-Key: "
    pad = key_at - len(head) - len(name)
    req = (head + b"p" * pad + name + AC.RFC_KEY + b"\r\nUpgrade: websocket\r\nConnection: Upgrade\r\n"
           b"Sec-WebSocket-Version: 13\r\n\r\n")
    assert req.index(AC.RFC_KEY) == key_at
    assert total >= len(req)
    return req + (b"\x81\x80abcd" * total)[:total - len(req)]  # (frame bytes behind the blank line)


@pytest.mark.parametrize("policy", POLICIES)
def test_lengths_around_a_line_and_around_one_line_per_lane(ctx, policy):
    short = [Entry(AC.RFC, length=k, bmis=b) for k in (0, 1, 15, 16, 17) for b in (0, 1, 15)]
    Launch(short, policy, 1024).run(ctx).check("short")
    for mr in (1024, 2048):
        entries = [Entry(sized(L), bmis=b) for L in (1023, 1024, 1025) for b in (0, 9, 15)]
        # len past the request: 1023..1025 bytes sent so far of which the request is the first part
        entries += [Entry(sized(1025, key_at=400), length=L, bmis=3) for L in (1023, 1024, 1025)]
        # the key's bytes across the 1024-byte mark, and ending exactly on it
        entries += [Entry(sized(1200, key_at=k), bmis=b) for k in (1000, 1012, 1023, 1024) for b in (0, 4)]
        la = Launch(entries, policy, mr).run(ctx).check(mr)
        want = [M.ACCEPTED, M.ACCEPTED, M.REJECTED if mr == 1024 else M.ACCEPTED]
        assert [la.exp[3 * i][0]["status"] for i in range(3)] == want
        assert la.exp[6][0]["reason"] == (M.R_TOO_LONG if mr == 1024 else 0)
        assert all(r["status"] == M.ACCEPTED for r, _ in la.exp[9:12])
        assert all((r["status"] == M.ACCEPTED) == (mr == 2048) for r, _ in la.exp[12:])


@pytest.mark.parametrize("policy", POLICIES)
def test_max_request_at_the_request_length(ctx, policy):
    for req in (AC.RFC, AC.BROWSER, AC.BY_NAME["headers_100"]):
        L = len(req)
        for mr, status, reason in ((L, M.ACCEPTED, 0), (L - 1, M.REJECTED, M.R_TOO_LONG), (8192, M.ACCEPTED, 0)):
            la = Launch([Entry(req, bmis=b) for b in (0, 11)], policy, mr).run(ctx).check((L, mr))
            assert (la.exp[0][0]["status"], la.exp[0][0]["reason"]) == (status, reason)


# --------------------------------------------------------------------------- 5. every truncation
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", ["rfc", AC.REJECTED_FOR_GRAMMAR, "key_twice_short_last"])
def test_every_truncation(ctx, name, policy):
    """L + 1 entries, one launch: the first event of the walk decides, and the
    bytes behind len never matter."""
    req = AC.BY_NAME[name]
    entries = [Entry(req, length=k, bmis=k % 16, omis=(3 * k) % 16) for k in range(len(req) + 1)]
    la = Launch(entries, policy, 1024).run(ctx).check(name)
    statuses = [r["status"] for r, _ in la.exp]
    assert statuses[0] == 0 and statuses[-1] == (M.ACCEPTED if name == "rfc" else M.REJECTED)
    first = next(k for k, s in enumerate(statuses) if s)
    assert all(s == statuses[-1] for s in statuses[first:]) and not any(statuses[:first])


# --------------------------------------------------------------------------- 6. capacities
@pytest.mark.parametrize("policy", POLICIES)
def test_out_capacities(ctx, policy):
    entries = []
    for name in ("rfc", "post", "version_8", "version_9_wrong"):
        for cap in (0, 25, 26, 128, 129):
            entries.append(Entry(AC.BY_NAME[name], out_cap=cap, omis=cap % 16))
            entries.append(Entry(AC.BY_NAME[name], out_cap=cap, abut=True))
        entries.append(Entry(AC.BY_NAME[name], out_cap=0, out=False))
    la = Launch(entries, policy, 1024).run(ctx).check()
    assert la.exp[0][0]["status"] == M.ACCEPTED | M.TRUNCATED and la.exp[8][0]["status"] == M.ACCEPTED


# --------------------------------------------------------------------------- 7. SHA-1 and base64 against hashlib
def test_random_keys(ctx):
    keys = AC.random_keys(64)
    la = Launch([Entry(AC.browser(k), bmis=i % 16, abut=True) for i, k in enumerate(keys)], 0, 1024).run(ctx).check()
    for (res, resp), k in zip(la.exp, keys):
        assert resp == M.response_101(k) and res["key_off"] == AC.browser(k).index(k)
    # any 24 bytes under the reference's policy, the placeholder with no key
    odd = [AC.BY_NAME[n] for n in ("key_high_ht", "key_24_not_base64", "no_key", "key_twice", "folded_hides_key")]
    la = Launch([Entry(r, bmis=i) for i, r in enumerate(odd)], M.REFERENCE, 1024).run(ctx).check()
    assert la.exp[2][1][97:125] == AC.NO_KEY_ACCEPT == la.exp[4][1][97:125]
    assert la.exp[0][1] == M.response_101(AC.KEY_80)


# --------------------------------------------------------------------------- 8. null results
def test_null_results(ctx):
    entries = [Entry(req, bmis=k % 16, abut=True, out_cap=129) for k, (_, req) in enumerate(AC.CASES[:40])]
    Launch(entries, 0, 1024, results=False).run(ctx).check()


# --------------------------------------------------------------------------- 9. capture
def test_captured_and_replayed(ctx):
    """The call captured into a graph (a linear chain: one kernel), replayed
    twice with the request bytes changed in between; each replay equals the
    eager call on the same bytes."""
    keys = AC.random_keys(24, seed=7)
    sets = [[AC.browser(k) for k in keys[:12]], [AC.browser(k, path=b"/rooms/other") for k in keys[12:]]]
    sets[1][5] = sets[1][5].replace(b"GET ", b"PUT ")
    assert all(len(a) == len(b) for a, b in zip(*sets))
    eager = [Launch([Entry(r, bmis=i) for i, r in enumerate(s)], 0, 1024).run(ctx).check() for s in sets]
    la = Launch([Entry(r, bmis=i) for i, r in enumerate(sets[0])], 0, 1024)
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        la.run(ctx, s.cuda_stream)
    torch.cuda.synchronize()
    assert bool((la.out_t == GUARD).all()) and bool((la.res_t == GUARD).all())  # (capture ran nothing)
    for want in eager:
        with torch.cuda.stream(s):
            la.in_t.copy_(want.in_t)
            la.out_t.fill_(GUARD)
            la.res_t.fill_(GUARD)
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(la.out_t, want.out_t) and torch.equal(la.res_t, want.res_t)
        la.exp, la.in_image, la.out_image = want.exp, want.in_image, want.out_image
        la.check("replay")


# --------------------------------------------------------------------------- 10. the Python layer
def test_connection_group_accept(ws, ctx):
    grp = ws.connection_group(4, cap=4, ctx=ctx)
    reqs = [AC.BY_NAME["frames_behind"], AC.RFC[:100], AC.BY_NAME["version_8"], AC.BROWSER]
    bufs = [torch.from_numpy(np.frombuffer(r, np.uint8).copy()).cuda() for r in reqs]
    outs = [torch.full((160,), GUARD, dtype=torch.uint8, device="cuda") for _ in reqs]
    acc = grp.accept(bufs, outs)
    for k, r in enumerate(reqs):
        res, resp = M.accept(r, 0, 1024, 160)
        assert bytes(acc.result(k)) == M.pack_result(res) and acc.response(k) == resp
        assert outs[k].cpu().numpy().tobytes() == resp + bytes([GUARD]) * (160 - len(resp))
    first = acc.result(0)
    assert reqs[0][first.consumed:] == b"\x81\x85\x37\xfa\x21\x3d\x7f\x9f\x4d\x51\x58"  # the first decode() input
    assert reqs[3][acc.result(3).path_off:][:acc.result(3).path_len] == b"/rooms/lobby"
    ref = grp.accept([(7, bufs[2])], [outs[2]], policy=_lib.ACC_REFERENCE, max_request=2048)
    assert ref.ids == [7] and ref.response(0) == M.RESP_400_REF

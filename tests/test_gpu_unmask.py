"""xyws_unmask (k_unmask_range) and xyws_mask_bytes against expected bytes
over the kernel's whole tile geometry: ranges long enough that a workgroup
walks a chain of two and of three tiles (the prefetch of the next tile, the
claim one ahead, the counter's reset), with edge tiles at either end, in the
three forms a launch takes: tiles claimed from the stream's counter (eager),
static tiles (captured into a graph), and static tiles again when every
scratch slot of the context is bound to another stream.

Every comparison is of all bytes (np.array_equal) of the guarded buffer, the
0xA5 guards before and after the range included, after an ODD number of
applications: expected bytes are oracle.mask's on a host copy
(tests/test_oracle.py holds it to the plain formula and to the reference at
these very sizes). Sizes follow the kernel (xyws_debug_unmask_geometry
through tests/unmask_cases.py): T bytes per tile, G workgroups at most.
"""
import ctypes as C

import numpy as np
import pytest

import unmask_cases as uc
from test_gpu_parity import dev_bytes, host, torch
from xynet_amd import websocket as ws

pytestmark = pytest.mark.gpu

GUARD = 32
ERR_CAPACITY = -4


class Env:
    pass


@pytest.fixture(scope="module")
def env():
    """The geometry, the case tables and the one long source (host, and
    uploaded once: each case clones its prefix on the device)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ws.context(0)  # (the thread's context exists before any capture begins)
    e = Env()
    e.T, _, wpc, e.slots = uc.geometry()
    e.G = torch.cuda.get_device_properties(0).multi_processor_count * wpc
    e.long = uc.long_cases(e.T, e.G)
    e.short = uc.short_cases(e.T, e.G)
    e.src = uc.source(max(n for n, _, _ in uc.all_ranges(e.T, e.G)))
    e.src_dev = torch.from_numpy(e.src).cuda()
    torch.cuda.synchronize()
    return e


def place(env, n, m):
    """src[:n] at misalignment m of a guarded device buffer: (view, whole)."""
    whole = torch.full((m + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 16 == 0
    whole[m:m + n] = env.src_dev[:n]
    return whole[m:m + n], whole


def expected(oracle, env, n, m, *masks):
    """The guarded buffer after the masks (key, phase) were applied in turn."""
    want = np.full(m + n + GUARD, 0xA5, np.uint8)
    body = want[m:m + n]
    body[:] = env.src[:n]
    for key, phase in masks:
        assert oracle.mask(body, key, phase) == phase + n
    return want


def unmask(ctx, view, key, phase, stream):
    """xyws_unmask on `stream` of `ctx`: the returned phase."""
    out = C.c_uint64()
    ws.check(ctx.L.xyws_unmask(ctx.h, C.c_void_p(view.data_ptr()), view.numel(), key_bytes(key), phase, C.byref(out),
                               C.c_void_p(stream.cuda_stream)), "xyws_unmask")
    return out.value


def key_bytes(key):
    return (C.c_uint8 * 4)(*key.to_bytes(4, "little"))


def same(whole, want):
    return np.array_equal(whole.cpu().numpy(), want)


def assert_long(env, c):
    """A geometry change must break these tests, not empty them."""
    assert c.K in (env.G + 1, 2 * env.G + 3)
    assert c.n > (2 if c.K == 2 * env.G + 3 else 1) * env.G * env.T, c


# --------------------------------------------------------------------------- 1
@pytest.mark.parametrize("chain", [2, 3])
def test_claimed_tiles_long_ranges(env, oracle, chain):
    """Eager calls: G + 1 tiles (some workgroup takes two) and 2G + 3 tiles
    (three), at start misalignments 0, 1, 15 and ends 0, 1, 17, T - 1 bytes
    past the last whole tile; m = 0, tail = 0 never leaves the whole-tile
    branch, every other case has an edge tile at one or both ends."""
    K = {2: env.G + 1, 3: 2 * env.G + 3}[chain]
    cases = [c for c in env.long if c.K == K]
    assert len(cases) == 12
    for c in cases:
        assert_long(env, c)
        view, whole = place(env, c.n, c.m)
        assert ws.websocket_mask(view, c.key, c.phase) == c.phase + c.n, c
        assert same(whole, expected(oracle, env, c.n, c.m, (c.key, c.phase))), c
    assert ws.context(0).last_device_error() == 0


# --------------------------------------------------------------------------- 2
def test_static_tiles_captured_and_replayed_once(env, oracle):
    """A captured launch takes tiles b, b + grid, b + 2 grid: 2G + 3 tiles,
    captured on a fresh stream and replayed ONCE."""
    K = 2 * env.G + 3
    for m in (0, 15):
        for tail in (1, env.T - 1):
            c = uc.pick(env.long, K, m, tail)
            assert_long(env, c)
            view, whole = place(env, c.n, c.m)
            s = torch.cuda.Stream()
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):
                assert ws.websocket_mask(view, c.key, c.phase) == c.phase + c.n
            torch.cuda.synchronize()
            assert same(whole, expected(oracle, env, c.n, c.m)), c  # (capture ran nothing)
            g.replay()
            torch.cuda.synchronize()
            assert same(whole, expected(oracle, env, c.n, c.m, (c.key, c.phase))), c
            del g


# --------------------------------------------------------------------------- 3
def test_static_tiles_when_every_slot_is_bound_to_another_stream(env, oracle):
    """A context whose scratch slots are all bound (one 64-byte unmask on as
    many streams as it has slots), then 2G + 3 tiles on one more stream: that
    call takes static tiles, binds no slot and evicts none, and the first
    streams' next calls find their counters as they left them."""
    ctx = ws.Context(0)
    streams_ = [torch.cuda.Stream() for _ in range(env.slots + 1)]
    assert len({s.cuda_stream for s in streams_}) == env.slots + 1
    n0, ph0, k0 = env.short["slot"]
    n1, ph1, k1 = env.short["slot2"]
    assert n1 == n0 and k1 != k0
    small = [place(env, n0, 5) for _ in range(env.slots)]
    c = uc.pick(env.long, 2 * env.G + 3, 1, 17)
    assert_long(env, c)
    view, whole = place(env, c.n, c.m)
    torch.cuda.synchronize()
    for s, (v, _) in zip(streams_, small):
        assert unmask(ctx, v, k0, ph0, s) == ph0 + n0
    assert unmask(ctx, view, c.key, c.phase, streams_[-1]) == c.phase + c.n
    for s, (v, _) in zip(streams_, small):
        assert unmask(ctx, v, k1, ph1, s) == ph1 + n1
    torch.cuda.synchronize()
    assert same(whole, expected(oracle, env, c.n, c.m, (c.key, c.phase))), c
    want = expected(oracle, env, n0, 5, (k0, ph0), (k1, ph1))
    for k, (_, w) in enumerate(small):
        assert same(w, want), k
    # (a stream's debug words are its slot's: the first streams still have theirs, the last one never got one)
    words = (C.c_uint64 * 5)()
    for s in streams_[:-1]:
        assert ctx.L.xyws_debug_lattice(ctx.h, C.c_void_p(s.cuda_stream), words) == 0
    assert ctx.L.xyws_debug_lattice(ctx.h, C.c_void_p(streams_[-1].cuda_stream), words) == -1
    assert ctx.last_device_error() == 0
    ctx.close()


# --------------------------------------------------------------------------- 4
def test_claim_counter_across_calls_on_one_stream(env, oracle):
    """2G + 3 tiles, 1 byte, T + 1 bytes, 2G + 3 tiles again, queued on one
    stream with nothing between them: a counter the last workgroup out did
    not reset makes the next call skip tiles."""
    ctx = ws.Context(0)
    s = torch.cuda.Stream()
    K = 2 * env.G + 3
    a, b = uc.pick(env.long, K, 1, 1), uc.pick(env.long, K, 15, 17)
    calls = [(a.n, a.m, a.key, a.phase), (env.short["one"][0], 7, env.short["one"][2], env.short["one"][1]),
             (env.short["tile1"][0], 0, env.short["tile1"][2], env.short["tile1"][1]), (b.n, b.m, b.key, b.phase)]
    assert_long(env, a), assert_long(env, b)
    assert [n for n, _, _, _ in calls[1:3]] == [1, env.T + 1]
    bufs = [place(env, n, m) for n, m, _, _ in calls]
    torch.cuda.synchronize()
    for (n, m, key, phase), (v, _) in zip(calls, bufs):
        assert unmask(ctx, v, key, phase, s) == phase + n
    torch.cuda.synchronize()
    for k, ((n, m, key, phase), (_, w)) in enumerate(zip(calls, bufs)):
        assert same(w, expected(oracle, env, n, m, (key, phase))), k
    assert ctx.last_device_error() == 0
    ctx.close()


# --------------------------------------------------------------------------- 5
def test_two_claim_counters_at_once(env, oracle):
    """Two streams of one context, 2G + 3 tiles with a key of its own queued
    on each, synchronized only afterwards: each stream claims from its own
    slot's counter."""
    ctx = ws.Context(0)
    K = 2 * env.G + 3
    cases = [uc.pick(env.long, K, 1, 17), uc.pick(env.long, K, 15, env.T - 1)]
    assert cases[0].key != cases[1].key
    streams_ = [torch.cuda.Stream(), torch.cuda.Stream()]
    assert streams_[0].cuda_stream != streams_[1].cuda_stream
    bufs = [place(env, c.n, c.m) for c in cases]
    torch.cuda.synchronize()
    for c, s, (v, _) in zip(cases, streams_, bufs):
        assert_long(env, c)
        assert unmask(ctx, v, c.key, c.phase, s) == c.phase + c.n
    torch.cuda.synchronize()
    for c, (_, w) in zip(cases, bufs):
        assert same(w, expected(oracle, env, c.n, c.m, (c.key, c.phase))), c
    assert ctx.last_device_error() == 0
    ctx.close()


# --------------------------------------------------------------------------- 6
def test_replay_beside_eager_unmask_is_exact(env, oracle):
    """A captured unmask replayed on stream B while eager unmasks run on the
    capture stream A, three of each: both buffers are the once-masked bytes
    (the even-count form of this is in tests/test_gpu_graph.py)."""
    K = 2 * env.G + 3
    ca, cb = uc.pick(env.long, K, 0, 1), uc.pick(env.long, K, 1, env.T - 1)
    assert_long(env, ca), assert_long(env, cb)
    (va, wa), (vb, wb) = place(env, ca.n, ca.m), place(env, cb.n, cb.m)
    n0, ph0, k0 = env.short["slot"]
    warm, _ = place(env, n0, 0)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(sa):
        ws.websocket_mask(warm, k0, ph0)  # (eager on A first: A's slot and counter exist)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=sa):
        ws.websocket_mask(va, ca.key, ca.phase)
    torch.cuda.synchronize()
    for _ in range(3):
        with torch.cuda.stream(sb):
            g.replay()
        with torch.cuda.stream(sa):
            assert ws.websocket_mask(vb, cb.key, cb.phase) == cb.phase + cb.n
    torch.cuda.synchronize()
    assert same(wa, expected(oracle, env, ca.n, ca.m, (ca.key, ca.phase))), ca
    assert same(wb, expected(oracle, env, cb.n, cb.m, (cb.key, cb.phase))), cb
    assert ws.context(0).last_device_error() == 0


# --------------------------------------------------------------------------- 7
def mask_bytes(ctx, ptr, n, key, phase, stream):
    """xyws_mask_bytes: (return code, phase_out)."""
    out = C.c_uint64(0xDEAD)
    rc = ctx.L.xyws_mask_bytes(ctx.h, C.c_void_p(ptr) if ptr else None, n, key_bytes(key), phase, C.byref(out),
                               C.c_void_p(stream.cuda_stream))
    return rc, out.value


def mask_bytes_sizes(env):
    sizes = [env.short[k] for k in ("below", "above", "stage")]
    assert [n for n, _, _ in sizes] == [env.T - 1, env.T + 1, env.G * env.T + env.T + 5]
    return sizes


def test_mask_bytes_on_host_bytes_at_an_odd_address(env, oracle):
    """Host bytes through the context's device stage: T - 1 and T + 1 bytes,
    then more tiles than workgroups (the stage grows each time, the last run
    on it is a chain of tiles)."""
    ctx = ws.Context(0)
    s = torch.cuda.Stream()
    for n, phase, key in mask_bytes_sizes(env):
        buf = np.full(n + 2 * GUARD + 2, 0xA5, np.uint8)
        off = GUARD + (1 - buf.ctypes.data % 2)
        data = buf[off:off + n]
        assert data.ctypes.data % 2 == 1
        data[:] = env.src[:n]
        want = buf.copy()
        assert oracle.mask(want[off:off + n], key, phase) == phase + n
        assert mask_bytes(ctx, data.ctypes.data, n, key, phase, s) == (0, phase + n)
        assert np.array_equal(buf, want), n
    assert ctx.last_device_error() == 0
    ctx.close()


def test_mask_bytes_on_device_bytes_is_done_when_it_returns(env, oracle):
    """Device bytes at misalignment 3 on a stream of their own: the copy back
    (another stream, nothing waited for) sees the whole result."""
    ctx = ws.Context(0)
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
    for n, phase, key in mask_bytes_sizes(env):
        view, whole = place(env, n, 3)
        torch.cuda.synchronize()  # (the buffer is filled before the call; nothing after it)
        assert mask_bytes(ctx, view.data_ptr(), n, key, phase, s) == (0, phase + n)
        assert same(whole, expected(oracle, env, n, 3, (key, phase))), n
    assert ctx.last_device_error() == 0
    ctx.close()


def test_mask_bytes_arguments(env, oracle):
    """len == 0 with a null pointer is a call that does nothing; a capturing
    stream is refused (the call is synchronous by contract) with nothing
    written to host or device bytes."""
    ctx = ws.Context(0)
    s = torch.cuda.Stream()
    assert mask_bytes(ctx, None, 0, 0x01020304, 7, s) == (0, 7)
    n, phase, key = env.short["slot"]
    hbuf = env.src[:n].copy()
    view, whole = place(env, n, 3)
    other, _ = dev_bytes(env.src[:n].tobytes())
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        unmask(ctx, other, key, phase, s)  # (allowed under capture: the graph is not empty)
        assert mask_bytes(ctx, hbuf.ctypes.data, n, key, phase, s)[0] == ERR_CAPACITY
        assert mask_bytes(ctx, view.data_ptr(), n, key, phase, s)[0] == ERR_CAPACITY
    torch.cuda.synchronize()
    assert np.array_equal(hbuf, env.src[:n])
    assert same(whole, expected(oracle, env, n, 3))
    assert host(other) == env.src[:n].tobytes()  # (captured, never replayed)
    assert ctx.last_device_error() == 0
    ctx.close()

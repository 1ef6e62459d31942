"""hipGraph capture of the decode path (xyws_ctx_reserve's promise: after a
reserve, calls allocate nothing and can be captured), replayed and checked
against the oracle.

- A decode with descriptors captured on a stream the context has never seen
  (the reserve's spare slot, include/xyws.h), replayed: bytes, frames, count.
- A decode with descriptors captured on a stream whose previous calls chose
  the run decoder's 256-thread geometry (echo-sized batches of small frames
  of mixed sizes: four runs per CU), within the reserve.
- xyws_unmask captured and replayed an even number of times (a captured
  unmask takes static tiles: no counter outside the launch): the buffer comes
  back unchanged, an odd count unmasks; a replay on another stream runs
  concurrently with eager unmasks on the capture stream.
- The other half of the rule: outside capture every scratch buffer of a
  context grows when a call needs more than it has. For each buffer, a call
  that fits its floor and then one that does not, queued back to back on one
  stream with nothing between them, both checked against the oracle.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import streams  # noqa: E402
from xynet_amd._lib import OPT_LATTICE  # noqa: E402


@pytest.mark.gpu
def test_decode_with_descriptors_captured_on_a_new_stream():
    import torch
    from oracle.oracle import Oracle
    from xynet_amd import websocket as ws
    orc = Oracle()
    src = streams.case_bytes("random_frames_200")
    host = np.frombuffer(src, np.uint8).copy()
    ofr, _, on = orc.decode_stream(host)
    ctx = ws.Context(0)
    ctx.reserve(1 << 20, 4096)
    dec = ws.frame_decoder(ctx=ctx)
    buf = torch.frombuffer(bytearray(src), dtype=torch.uint8).cuda()
    orig = buf.clone()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        r = dec.decode(buf, cap=on + 2, carry=False)  # (within the reserve's 4096 frames)
    # (capture ran nothing: the bytes are untouched)
    torch.cuda.synchronize()
    assert torch.equal(buf, orig)
    for rep in range(3):
        buf.copy_(orig)
        g.replay()
        torch.cuda.synchronize()
        assert buf.cpu().numpy().tobytes() == host.tobytes(), rep
        assert r.nframes == on
        got = [(f.frame_off, f.payload_off, f.payload_len, bytes(f.key), f.flags, f.hdr_len, f.status)
               for f in r.frames()]
        want = [(f.frame_off, f.payload_off, f.payload_len, bytes(f.key), f.flags, f.hdr_len, f.status)
                for f in ofr]
        assert got == want, rep
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,phase", [(1 << 22, 0), ((1 << 22) + 13, 3)])
def test_unmask_captured_and_replayed(n, phase):
    import torch
    from xynet_amd import websocket as ws
    g0 = torch.Generator().manual_seed(5)
    data = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g0).cuda()
    orig = data.clone()
    mask = 0x1F2E3D4C
    view = data[5:]  # (misaligned start)
    ws.context(0).reserve(n + 64)  # (the claim counter of a stream new to the context)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        ws.websocket_mask(view, mask, phase)
    torch.cuda.synchronize()
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(data, orig)
    g.replay()
    torch.cuda.synchronize()
    kb = np.frombuffer(mask.to_bytes(4, "little"), np.uint8)
    want = orig.cpu().numpy().copy()
    idx = (phase + np.arange(n - 5)) % 4
    want[5:] ^= kb[idx]
    assert np.array_equal(data.cpu().numpy(), want)


@pytest.mark.gpu
def test_decode_captured_after_mid_geometry_calls():
    """the reserve must cover the 256-thread geometry's run count
    (ncu * 4 runs on 16 KiB segments), which the decoder choice gives a
    stream after calls of small frames of mixed sizes."""
    import torch
    from oracle.oracle import Oracle
    from xynet_amd import websocket as ws
    orc = Oracle()
    rng = streams.SplitMix(0x6D1D)
    b = bytearray()
    while len(b) < (4 << 20) - 1100:
        b += streams.frame(rng, 0x81, rng.next() % 1001)
    src = bytes(b)
    host = np.frombuffer(src, np.uint8).copy()
    ofr, _, on = orc.decode_stream(host, cap=len(src) // 6 + 2)
    ctx = ws.Context(0)
    ctx.reserve(4 << 20, 16384)
    dec = ws.frame_decoder(ctx=ctx)
    orig = torch.frombuffer(bytearray(src), dtype=torch.uint8).cuda()
    buf = orig.clone()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(2):  # (eager: the policy words now say small frames of mixed sizes)
            buf.copy_(orig)
            r = dec.decode(buf, cap=on + 2, carry=False)
            assert r.nframes == on
    torch.cuda.synchronize()
    from xynet_amd._lib import POL_FSMAX, POL_FSMIN, POL_WORDS
    pol = (__import__("ctypes").c_uint64 * POL_WORDS)()
    assert ctx.L.xyws_debug_policy(ctx.h, __import__("ctypes").c_void_p(s.cuda_stream), pol) == 0
    assert pol[POL_FSMAX] < 2048 and pol[POL_FSMIN] != pol[POL_FSMAX], list(pol)
    g = torch.cuda.CUDAGraph()
    buf.copy_(orig)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        r = dec.decode(buf, cap=on + 2, carry=False)
    torch.cuda.synchronize()
    for rep in range(2):
        buf.copy_(orig)
        g.replay()
        torch.cuda.synchronize()
        assert buf.cpu().numpy().tobytes() == host.tobytes(), rep
        assert r.nframes == on
        got = [(f.frame_off, f.payload_off, f.payload_len, bytes(f.key), f.flags, f.hdr_len, f.status)
               for f in r.frames()]
        want = [(f.frame_off, f.payload_off, f.payload_len, bytes(f.key), f.flags, f.hdr_len, f.status)
                for f in ofr]
        assert got == want, rep
    ctx.close()


@pytest.mark.gpu
def test_unmask_replay_concurrent_with_eager_unmask_on_the_capture_stream():
    """A captured unmask replayed on stream B while eager unmasks run on the
    capture stream A: the replay shares no counter with them."""
    import torch
    from xynet_amd import websocket as ws
    n = 96 << 20
    g0 = torch.Generator().manual_seed(9)
    a = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g0).cuda()
    b = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g0).cuda()
    a0, b0 = a.clone(), b.clone()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(sa):
        ws.websocket_mask(b, 0x01020304, 0)  # (eager on A first: A's slot and counter exist)
        ws.websocket_mask(b, 0x01020304, 0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=sa):
        ws.websocket_mask(a, 0xA5C3E1F0, 1)
    torch.cuda.synchronize()
    for _ in range(3):
        with torch.cuda.stream(sb):
            g.replay()
            g.replay()
        with torch.cuda.stream(sa):
            ws.websocket_mask(b, 0x01020304, 0)
            ws.websocket_mask(b, 0x01020304, 0)
    torch.cuda.synchronize()
    assert torch.equal(a, a0)
    assert torch.equal(b, b0)


def _tuples(fr):
    return [(f.frame_off, f.payload_off, f.payload_len, bytes(f.key), f.flags, f.hdr_len, f.status) for f in fr]


def _frames(seed, n, size, mixed=False):
    """n masked binary frames with payloads of `size` bytes (mixed: of fewer than `size`, at random)."""
    rng = streams.SplitMix(seed)
    return b"".join(streams.frame(rng, 0x82, rng.below(size) if mixed else size) for _ in range(n))


# (decoder arguments, the call within the floor, the call past it); floors: xyws_ctx.h, xyws_stream.h
GROW_DECODES = {
    # frame table, 1024 entries: the serial scan asks for len / 2 + 2
    "table": (dict(serial=True), lambda: _frames(1, 3, 300), lambda: _frames(2, 1100, 300)),
    # run scratch, 64 runs, and the descriptor regions with it: one run per KiB in the small-segment geometry
    "runs": (dict(small_segments=True), lambda: _frames(3, 7, 280, True), lambda: _frames(4, 320, 500, True)),
    # lattice scratch, 64 segments: one per KiB of equal frames, the lattice decoder first
    "lattice": (dict(small_segments=True, opts=OPT_LATTICE), lambda: _frames(5, 100, 200), lambda: _frames(6, 500, 200)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(GROW_DECODES))
def test_decode_scratch_grows_between_two_queued_calls(oracle, which):
    import torch
    from xynet_amd import websocket as ws
    kw, small, large = GROW_DECODES[which]
    srcs = [small(), large()]
    assert {"table": len(srcs[0]) // 2 + 2 <= 1024 < len(srcs[1]) // 2 + 2,
            "runs": len(srcs[0]) <= 2048 and len(srcs[1]) > 65536,
            "lattice": len(srcs[0]) < 64 * 1024 < len(srcs[1])}[which]
    want = []
    for src in srcs:
        h = np.frombuffer(src, np.uint8).copy()
        ofr, _, on = oracle.decode_stream(h)
        want.append((h.tobytes(), _tuples(ofr), on))
    ctx = ws.Context(0)
    dec = ws.frame_decoder(ctx=ctx, **kw)
    bufs = [torch.frombuffer(bytearray(src), dtype=torch.uint8).cuda() for src in srcs]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        res = [dec.decode(b, cap=w[2] + 2, carry=False) for b, w in zip(bufs, want)]
    torch.cuda.synchronize()
    for k, (b, r, (data, frames, on)) in enumerate(zip(bufs, res, want)):
        assert r.nframes == on, k
        assert b.cpu().numpy().tobytes() == data, k
        assert _tuples(r.frames()) == frames, k
    assert ctx.last_device_error() == 0
    ctx.close()


@pytest.mark.gpu
def test_iov_staging_grows_between_two_queued_calls(oracle):
    """The staging buffer's floor is 1 MiB: a staged sequence of 4 KiB, then one
    just over 1 MiB (descriptors asked for: several pieces are staged)."""
    import torch
    from xynet_amd import websocket as ws
    srcs = [_frames(7, 8, 500, True), _frames(8, 2200, 1000, True)]
    assert len(srcs[0]) <= 4096 and 1 << 20 < len(srcs[1]) < (1 << 20) + (128 << 10)
    want, seqs = [], []
    for src in srcs:
        h = np.frombuffer(src, np.uint8).copy()
        ofr, _, on = oracle.decode_stream(h)
        want.append((h.tobytes(), _tuples(ofr), on))
        cuts = [0, len(src) // 5, len(src) // 2 + 3, len(src)]
        seqs.append([torch.frombuffer(bytearray(src[a:b]), dtype=torch.uint8).cuda() for a, b in zip(cuts, cuts[1:])])
    ctx = ws.Context(0)
    dec = ws.frame_decoder(ctx=ctx)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        res = [dec.decode_iov(v, cap=w[2] + 2, carry=False) for v, w in zip(seqs, want)]
    torch.cuda.synchronize()
    for k, (views, r, (data, frames, on)) in enumerate(zip(seqs, res, want)):
        assert r.nframes == on, k
        assert b"".join(v.cpu().numpy().tobytes() for v in views) == data, k
        assert _tuples(r.frames()) == frames, k
    ctx.close()


@pytest.mark.gpu
def test_frame_list_scratch_grows_between_two_queued_calls(oracle):
    """The frame-list scratch's floor is 64 KiB, 8 bytes per frame and some: an
    encode of 16 frames, then one of more than 8192 frames of 4-byte payloads."""
    import ctypes as C
    import torch
    from xynet_amd import websocket as ws
    ctx = ws.Context(0)
    dec = ws.frame_decoder(ctx=ctx)
    work = []
    for src in (_frames(9, 16, 4), _frames(10, 8300, 4)):
        h = np.frombuffer(src, np.uint8).copy()
        ofr, _, on = oracle.decode_stream(h)
        want, _, total = oracle.encode_frames(h, ofr, 0x12)
        t = torch.frombuffer(bytearray(src), dtype=torch.uint8).cuda()
        r = dec.decode(t, cap=on, carry=False)
        assert r.nframes == on
        out = torch.full((total + 32,), 0xA5, dtype=torch.uint8, device="cuda")
        work.append((t, r.frames_t, on, out, torch.zeros(1, dtype=torch.int64, device="cuda"), want, total))
    assert work[0][2] == 16 and work[1][2] > 8192
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    for t, frames_t, n, out, olen, _, total in work:  # (no offsets of the caller's: they live in the scratch)
        ws.check(ctx.L.xyws_encode_frames(ctx.h, C.c_void_p(t.data_ptr()), t.numel(), C.c_void_p(frames_t.data_ptr()), n,
                                          None, 0x12, 0, None, None, 0, C.c_void_p(out.data_ptr()), total, None,
                                          C.c_void_p(olen.data_ptr()), C.c_void_p(s.cuda_stream)))
    torch.cuda.synchronize()
    for k, (_, _, _, out, olen, want, total) in enumerate(work):
        assert int(olen.item()) == total, k
        assert out[:total].cpu().numpy().tobytes() == want, k
        assert out[total:].tolist() == [0xA5] * 32, k
    assert ctx.last_device_error() == 0
    ctx.close()


@pytest.mark.gpu
def test_host_stage_grows_between_two_calls(oracle):
    """xyws_mask_bytes on host bytes goes through the context's device stage,
    4 KiB at the least: 1 KiB, then 8 KiB."""
    import ctypes as C
    import torch
    from xynet_amd import websocket as ws
    ctx = ws.Context(0)
    s = torch.cuda.Stream()
    rng = streams.SplitMix(11)
    for n, phase in ((1024, 1), (8192, 2)):
        key = rng.next() & 0xFFFFFFFF
        data = np.frombuffer(rng.bytes(n), np.uint8).copy()
        want = data.copy()
        assert oracle.mask(want, key, phase) == phase + n
        out = C.c_uint64()
        ws.check(ctx.L.xyws_mask_bytes(ctx.h, C.c_void_p(data.ctypes.data), n, (C.c_uint8 * 4)(*key.to_bytes(4, "little")),
                                       phase, C.byref(out), C.c_void_p(s.cuda_stream)))
        assert out.value == phase + n
        assert data.tobytes() == want.tobytes(), n
    ctx.close()

"""xyws_reassemble_stream on the device (frame_decoder.decode +
message_assembler.feed per batch) against the model (tests/reasm_model.py,
itself held to the unsplit stream's xyws_reassemble by
tests/test_reasm_model.py): out[:total], the stored records, the count and
the 64 carry bytes of every call, byte for byte; then the acceptance property
on the device's own records: folded over the calls they are the unsplit
stream's records.

Sizes: a few hundred bytes to ~300 KiB. The tile-seam streams cross the
gather tile (16 KiB) and the UTF-8 tile (64 KiB) of xyws_frames.hip at every
offset -3..3; nothing here needs more than one scan block (the scans are
xyws_reassemble's own, tests/test_frames_scale.py)."""
import pytest

import msg_streams
import reasm_cases as RC
import reasm_model as M
import streams

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 0xEE


@pytest.fixture(scope="module")
def ws():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from xynet_amd import websocket
    return websocket


def _records(raw, cnt):
    from oracle.oracle import Message
    arr = (Message * max(len(raw) // 40, 1)).from_buffer_copy(raw.cpu().numpy().tobytes().ljust(40, b"\0"))
    return [arr[i].as_tuple() for i in range(cnt)]


def run_device(ws, calls, opts=M.REASM_UTF8, out_caps=None, msg_caps=None, opts_per=None, src_shift=0, out_shift=0,
               check=True):
    """Each call's batch decoded and fed on the device; compared with the
    model's answer (calls: RC.run_model with the same caps and options).
    Returns the device's records per call."""
    dec = ws.frame_decoder()
    asm = ws.message_assembler(opts=opts)
    got = []
    for k, c in enumerate(calls):
        ln = len(c.wire)
        big = torch.zeros(ln + src_shift + 16, dtype=torch.uint8, device="cuda")
        t = big[src_shift:src_shift + ln]
        if ln:
            t.copy_(torch.frombuffer(bytearray(c.wire), dtype=torch.uint8))
        cap = ln // 2 + 2
        r = dec.decode(t, cap=cap)
        n = r.nframes
        assert n == len(c.frames)
        assert t.cpu().numpy().tobytes() == c.host.tobytes()
        oc = ln if out_caps is None or out_caps[k] is None else out_caps[k]
        mc = n + 1 if msg_caps is None or msg_caps[k] is None else msg_caps[k]
        obig = torch.full((oc + out_shift + 32,), GUARD, dtype=torch.uint8, device="cuda")
        out = obig[out_shift:out_shift + max(oc, 1)]
        if opts_per is not None:
            asm.opts = opts_per[k]
        o, mt, cnt = asm.feed(t, r.frames_t, n, out=out, out_cap=oc, msg_cap=mc)
        nm = int(cnt.item())
        recs = _records(mt, min(nm, mc))
        got.append(recs)
        if check:
            host_out = obig.cpu().numpy()
            assert nm == c.nm, (k, nm, c.nm)
            assert recs == c.recs, (k, recs, c.recs)
            assert host_out[out_shift:out_shift + len(c.out)].tobytes() == c.out, k
            # nothing outside the bytes delivered is written
            assert (host_out[:out_shift] == GUARD).all() and (host_out[out_shift + len(c.out):] == GUARD).all(), k
            assert bytes(asm.carry()) == c.carry.pack(), (k, M.Carry.unpack(bytes(asm.carry())), c.carry)
    return got


# --------------------------------------------------------------------------- 1. every cut of a short stream

def test_short_stream_every_cut(ws, oracle):
    wire, marks = RC.short_stream()
    kinds = set()
    for cut in range(len(wire) + 1):
        kinds |= RC.short_cut_kinds(marks, cut)
        calls = RC.run_model(oracle, RC.batches(wire, [cut]))
        got = run_device(ws, calls)
        RC.check_fold(oracle, wire, calls, records=got)
    assert kinds == {"header", "after_header", "member", "control", "orphan", "boundary"}


def test_short_stream_one_byte_middle_batch(ws, oracle):
    wire, _ = RC.short_stream()
    for cut in range(len(wire)):
        calls = RC.run_model(oracle, RC.batches(wire, [cut, cut + 1]))
        got = run_device(ws, calls)
        RC.check_fold(oracle, wire, calls, records=got)


# --------------------------------------------------------------------------- 2. generator streams

@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_generator_streams(ws, oracle, seed):
    wire, _ = msg_streams.message_stream(seed, nmsg=60)
    continued = pending = 0
    for cuts in RC.generator_splits(oracle, seed, wire):
        calls = RC.run_model(oracle, RC.batches(wire, cuts))
        got = run_device(ws, calls)
        RC.check_fold(oracle, wire, calls, records=got)
        continued += sum(1 for g in got for r in g if r[4] & M.CONTINUED)
        pending += sum(1 for c in calls if c.carry.opcode == 0 and c.carry.status & M.ORPHANS)
    assert continued and pending


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_generator_streams_one_byte_batches(ws, oracle, seed):
    wire = RC.whole_frame_prefix(oracle, msg_streams.message_stream(seed, nmsg=60)[0])
    calls = RC.run_model(oracle, RC.batches(wire, range(1, len(wire))))
    got = run_device(ws, calls)
    RC.check_fold(oracle, wire, calls, records=got)


# --------------------------------------------------------------------------- 3. UTF-8 seam

SHIFTS = [(s, o) for s in (0, 1, 5, 15) for o in (0, 3, 14)]


@pytest.mark.parametrize("seq", RC.SEAM_SEQS, ids=lambda s: s.hex())
def test_utf8_seam(ws, oracle, seq):
    """The sequence at the end of a fragment's bytes, cut after each of its
    bytes, in 2 and 3 batches, the message completing later or staying open;
    src and out taken at every shift pair in turn (views into larger
    tensors)."""
    k = 0
    for completes in (True, False):
        wire, pos = RC.seam_stream(seq, completes)
        for p in pos + [pos[0] - 1]:
            for cuts in ([p], [p, p + 1], [p - 1, p], [p, len(wire) - 1]):
                calls = RC.run_model(oracle, RC.batches(wire, cuts))
                s, o = SHIFTS[k % len(SHIFTS)]
                k += 1
                got = run_device(ws, calls, src_shift=s, out_shift=o)
                RC.check_fold(oracle, wire, calls, records=got)
    assert k >= len(SHIFTS)


# --------------------------------------------------------------------------- 4. tile seams

@pytest.mark.parametrize("base", [65536, 2 * 65536, 16384, 5 * 16384])
def test_tile_seams(ws, oracle, base):
    """The gathered bytes of the middle batch start at base + d and end at
    base + 65536 + d (d = -3..3): around a UTF-8 tile end (64 KiB) and a
    gather tile end (16 KiB) of out[], inside multi-byte sequences."""
    wire, text, spans = RC.tile_stream()
    for d in range(-3, 4):
        a = RC.wire_pos_of_payload(spans, base + d)
        b = RC.wire_pos_of_payload(spans, base + 65536 + d)
        calls = RC.run_model(oracle, RC.batches(wire, [a, b]))
        got = run_device(ws, calls)
        folded = RC.check_fold(oracle, wire, calls, records=got)
        assert folded[0][4] == M.COMPLETE


@pytest.mark.parametrize("base", [65536, 5 * 16384])
def test_tile_seams_corrupted_after_the_seam(ws, oracle, base):
    for d in (0, 1, 2):
        wire, text, spans = RC.tile_stream(corrupt_at=base + d)
        calls = RC.run_model(oracle, RC.batches(wire, [RC.wire_pos_of_payload(spans, base)]))
        got = run_device(ws, calls)
        folded = RC.check_fold(oracle, wire, calls, records=got)
        assert folded[0][4] == M.COMPLETE | M.UTF8_BAD and not got[0][0][4] & M.UTF8_BAD


# --------------------------------------------------------------------------- 5. whole frames, zero carry

@pytest.mark.parametrize("seed", [1, 2, 3])
def test_whole_frames_zero_carry_equals_reassemble(ws, oracle, seed):
    from xynet_amd import _lib
    wire, _ = msg_streams.message_stream(seed, nmsg=80)
    t = torch.frombuffer(bytearray(wire), dtype=torch.uint8).cuda()
    r = ws.frame_decoder().decode(t, cap=len(wire) // 2 + 2)
    n = r.nframes
    out, mt, cnt = ws.reassemble(t, r.frames_t, n, _lib.REASM_UTF8)
    ws.context().last_device_error()  # (clears bit 0x200: xyws_reassemble reports trailing orphans there)
    asm = ws.message_assembler()
    sout, smt, scnt = asm.feed(t, r.frames_t, n, msg_cap=max(n, 1))
    nm = int(cnt.item())
    assert int(scnt.item()) == nm
    recs = _records(smt, nm)
    assert recs == _records(mt, nm)
    assert not any(x[4] & M.CONTINUED for x in recs)
    assert torch.equal(sout, out)
    c = M.Carry.unpack(bytes(asm.carry()))
    last = recs[-1]
    if last[4] & (M.COMPLETE | M.INTERRUPTED):
        pending = c.status
        assert c == M.Carry(frames_seen=n, status=pending) and pending in (0, M.ORPHANS)
    else:
        assert (c.opcode, c.length, c.nframes, c.first_frame, c.frame_remaining, c.frames_seen) == \
            (last[5], last[3], last[1], last[0], 0, n)
    assert ws.context().last_device_error() == 0


# --------------------------------------------------------------------------- 6. caps

@pytest.mark.parametrize("which", ["out_cap", "msg_cap", "both"])
def test_caps(ws, oracle, which):
    """out_cap half of a batch that ends inside an open text message, msg_cap 1
    with the open message the third record: the structural carry is the
    uncapped run's, UNCHECKED sticks to the message's later records, the next
    message is unaffected, *dev_nmsgs is exact."""
    wire, cuts = RC.caps_stream()
    parts = RC.batches(wire, cuts)
    out_caps = [len(parts[0]) // 2, None, None] if which != "msg_cap" else None
    msg_caps = [1, None, None] if which != "out_cap" else None
    free = RC.run_model(oracle, parts)
    capped = RC.run_model(oracle, parts, out_caps=out_caps, msg_caps=msg_caps)
    got = run_device(ws, capped, out_caps=out_caps, msg_caps=msg_caps)
    assert capped[0].nm == 3 and len(got[0]) == (3 if which == "out_cap" else 1)
    for a, b in zip(free, capped):
        sa, sb = a.carry, b.carry
        assert (sa.opcode, sa.length, sa.nframes, sa.first_frame, sa.frame_remaining, sa.frame_member,
                sa.frames_seen) == (sb.opcode, sb.length, sb.nframes, sb.first_frame, sb.frame_remaining,
                                    sb.frame_member, sb.frames_seen)
    assert got[1][0][4] & M.UNCHECKED and got[2][0][4] & M.UNCHECKED
    assert got[2][0][4] & (M.CONTINUED | M.COMPLETE | M.UTF8_BAD) == M.CONTINUED | M.COMPLETE
    assert got[2][1] == free[2].recs[1] and got[2][1][4] == M.COMPLETE


def test_call_without_utf8_option_abandons_validation(ws, oracle):
    wire, cuts = RC.caps_stream()
    parts = RC.batches(wire, cuts)
    opts_per = [M.REASM_UTF8, 0, M.REASM_UTF8]
    calls = RC.run_model(oracle, parts, opts_per=opts_per)
    got = run_device(ws, calls, opts_per=opts_per)
    assert not got[1][0][4] & M.UNCHECKED and got[2][0][4] & M.UNCHECKED and not got[2][0][4] & M.UTF8_BAD


# --------------------------------------------------------------------------- 7. capture

def test_decode_and_feed_captured_in_one_graph(ws, oracle):
    """decode + feed captured once (one stream, fixed buffers, both carries
    aliased in == out) after one eager call of the same sizes, replayed over 4
    successive batches copied into the fixed buffer; nothing reads the carries
    back in between."""
    wire, _ = msg_streams.message_stream(2, nmsg=60)
    B = len(wire) // 4
    parts = [wire[k * B:(k + 1) * B] for k in range(4)]
    calls = RC.run_model(oracle, parts)
    cap = B // 2 + 2
    ctx = ws.Context(0)
    ctx.reserve(1 << 20, 4096)
    dec = ws.frame_decoder(ctx=ctx)
    asm = ws.message_assembler(ctx=ctx)
    buf = torch.zeros(B, dtype=torch.uint8, device="cuda")
    out = torch.zeros(B, dtype=torch.uint8, device="cuda")
    msgs = torch.zeros((cap + 1) * 40, dtype=torch.uint8, device="cuda")
    stage = [torch.frombuffer(bytearray(p), dtype=torch.uint8).cuda() for p in parts]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        buf.copy_(stage[0])
        r = dec.decode(buf, cap=cap)
        asm.feed(buf, r.frames_t, cap, dev_n=r.nframes_t, out=out, msgs=msgs)
    torch.cuda.synchronize()
    dec.reset()
    asm.reset()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        r = dec.decode(buf, cap=cap)
        o, mt, cnt = asm.feed(buf, r.frames_t, cap, dev_n=r.nframes_t, out=out, msgs=msgs)
    torch.cuda.synchronize()
    results = []
    for k in range(4):
        buf.copy_(stage[k])
        out.fill_(GUARD)
        g.replay()
        results.append((out.clone(), mt.clone(), cnt.clone()))  # (device copies: no host read of the carries)
    torch.cuda.synchronize()
    for k, (o, m, c) in enumerate(results):
        nm = int(c.item())
        assert nm == calls[k].nm
        assert _records(m, nm) == calls[k].recs, k
        assert o.cpu().numpy()[:len(calls[k].out)].tobytes() == calls[k].out, k
    assert bytes(asm.carry()) == calls[3].carry.pack()
    ctx.close()


# --------------------------------------------------------------------------- 8. error word

def test_clipped_frame_and_trailing_orphans_leave_the_error_word_clear(ws, oracle):
    rng = streams.SplitMix(9)
    wire = msg_streams._frame(rng, 0x81, b"whole") + msg_streams._frame(rng, 0x80, b"orphan") + \
        msg_streams._frame(rng, 0x80, b"a clipped orphan continuation")
    ws.context().last_device_error()  # (clear)
    calls = RC.run_model(oracle, [wire[:-10]])
    run_device(ws, calls)
    assert calls[0].carry.status == M.ORPHANS and calls[0].carry.frame_remaining == 10
    assert ws.context().last_device_error() == 0
    calls = RC.run_model(oracle, [wire[:len(wire) - 40]])
    run_device(ws, calls)
    assert ws.context().last_device_error() == 0

"""CPU: the model of xyws_reassemble_stream (tests/reasm_model.py) against the
existing checker. For every stream and cut list: the batches are decoded with
the carry chained, fed to the model with its carry chained, and the records
folded (a CONTINUED record merges into the message before it) must equal
xyws_reassemble's records of the UNSPLIT stream, the outputs concatenated its
output, and UTF8_BAD must be monotone within a message. Also here: the
xyws_msg_carry layout, the exported symbol, and the C++ shim's
message_assembler."""
import ctypes as C
import os
import subprocess

import pytest

import msg_streams
import reasm_cases as RC
import reasm_model as M
import xynet_amd._lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_msg_carry_layout_and_symbol():
    assert C.sizeof(L.MsgCarry) == 64
    off = {f[0]: getattr(L.MsgCarry, f[0]).offset for f in L.MsgCarry._fields_}
    assert off == {"length": 0, "nframes": 8, "first_frame": 16, "frame_remaining": 24, "frames_seen": 32,
                   "status": 40, "opcode": 44, "frame_member": 45, "utf8_len": 46, "utf8": 47, "reserved": 50}
    assert (L.MSG_CONTINUED, L.MSG_UNCHECKED) == (0x20, 0x40) == (M.CONTINUED, M.UNCHECKED)
    assert "xyws_reassemble_stream" in L.declared_symbols()
    assert hasattr(L.load(), "xyws_reassemble_stream")
    c = M.Carry(length=5, nframes=2, first_frame=9, frame_remaining=3, frames_seen=11, status=0x42, opcode=1,
                frame_member=1, utf8=b"\xe2\x82")
    raw = c.pack()
    s = L.MsgCarry.from_buffer_copy(raw)
    assert (s.length, s.nframes, s.first_frame, s.frame_remaining, s.frames_seen, s.status, s.opcode,
            s.frame_member, s.utf8_len, bytes(s.utf8)) == (5, 2, 9, 3, 11, 0x42, 1, 1, 2, b"\xe2\x82\0")
    assert M.Carry.unpack(raw) == c and M.Carry().pack() == bytes(64)


def test_null_arguments_rejected():
    lib = L.load()
    assert lib.xyws_reassemble_stream(None, None, 0, None, 0, None, 0, None, None, None, 0, None, 0, None, None) == -1


def test_short_stream_every_cut(oracle):
    wire, marks = RC.short_stream()
    assert 200 <= len(wire) <= 320
    kinds, continued, pending = set(), 0, 0
    for cut in range(len(wire) + 1):
        kinds |= RC.short_cut_kinds(marks, cut)
        calls = RC.run_model(oracle, RC.batches(wire, [cut]))
        folded = RC.check_fold(oracle, wire, calls)
        continued += any(r[4] & M.CONTINUED for r in calls[1].recs)
        pending += calls[0].carry.opcode == 0 and bool(calls[0].carry.status & M.ORPHANS)
        # the last message ends in a cut sequence and completes: invalid, whichever call saw its bytes
        assert folded[-1][4] & (M.COMPLETE | M.UTF8_BAD) == M.COMPLETE | M.UTF8_BAD
        assert calls[-1].carry == M.Carry(frames_seen=9)
    assert kinds == {"header", "after_header", "member", "control", "orphan", "boundary"}
    assert continued > 50 and pending > 5


def test_short_stream_one_byte_middle_batch(oracle):
    wire, _ = RC.short_stream()
    for cut in range(len(wire)):
        calls = RC.run_model(oracle, RC.batches(wire, [cut, cut + 1]))
        RC.check_fold(oracle, wire, calls)


SEEDS = [1, 2, 3, 4]


@pytest.mark.parametrize("seed", SEEDS)
def test_generator_streams(oracle, seed):
    wire, _ = msg_streams.message_stream(seed, nmsg=60)
    continued = pending = 0
    for cuts in RC.generator_splits(oracle, seed, wire):
        calls = RC.run_model(oracle, RC.batches(wire, cuts))
        RC.check_fold(oracle, wire, calls)
        continued += sum(1 for c in calls for r in c.recs if r[4] & M.CONTINUED)
        pending += sum(1 for c in calls if c.carry.opcode == 0 and c.carry.status & M.ORPHANS)
    assert continued and pending, (continued, pending)


@pytest.mark.parametrize("seed", SEEDS)
def test_generator_streams_one_byte_batches(oracle, seed):
    """The first 400 bytes, extended to the next frame boundary (the unsplit
    reference then sees only whole frames), one byte per batch."""
    wire, _ = msg_streams.message_stream(seed, nmsg=60)
    wire = RC.whole_frame_prefix(oracle, wire)
    calls = RC.run_model(oracle, RC.batches(wire, range(1, len(wire))))
    RC.check_fold(oracle, wire, calls)


@pytest.mark.parametrize("seq", RC.SEAM_SEQS, ids=lambda s: s.hex())
@pytest.mark.parametrize("completes", [True, False])
def test_utf8_seam(oracle, seq, completes):
    wire, pos = RC.seam_stream(seq, completes)
    for p in pos + [pos[0] - 1]:
        for cuts in ([p], [p, p + 1], [p - 1, p], [p, len(wire) - 1]):
            cuts = [c for c in cuts if 0 <= c <= len(wire)]
            calls = RC.run_model(oracle, RC.batches(wire, cuts))
            folded = RC.check_fold(oracle, wire, calls)
            try:
                (b"abc " + seq + b" xyz").decode()
                ok = True
            except UnicodeDecodeError:
                ok = False
            if completes:
                assert folded[0][4] & (M.COMPLETE | M.UTF8_BAD) == M.COMPLETE | (0 if ok else M.UTF8_BAD)


def test_tile_seams(oracle):
    wire, text, spans = RC.tile_stream()
    for base in (65536, 2 * 65536, 16384, 5 * 16384):
        for d in range(-3, 4):
            a = RC.wire_pos_of_payload(spans, base + d)
            b = RC.wire_pos_of_payload(spans, base + 65536 + d)
            calls = RC.run_model(oracle, RC.batches(wire, [a, b]))
            folded = RC.check_fold(oracle, wire, calls)
            assert folded[0][4] == M.COMPLETE and len(folded) == 1
    for base in (65536, 5 * 16384):
        for d in (0, 1, 2):
            cwire, ctext, cspans = RC.tile_stream(corrupt_at=base + d)
            a = RC.wire_pos_of_payload(cspans, base)
            calls = RC.run_model(oracle, RC.batches(cwire, [a]))
            folded = RC.check_fold(oracle, cwire, calls)
            assert folded[0][4] == M.COMPLETE | M.UTF8_BAD
            assert not any(r[4] & M.UTF8_BAD for r in calls[0].recs)


def test_caps_keep_the_structural_carry(oracle):
    """out_cap half of a batch that ends inside an open text message, msg_cap 1
    with the open message the third record: the structural carry is the
    uncapped run's, UNCHECKED sticks, the next message is unaffected."""
    wire, cuts = RC.caps_stream()
    parts = RC.batches(wire, cuts)
    free = RC.run_model(oracle, parts)
    for out_caps, msg_caps in (([len(parts[0]) // 2, None, None], None), (None, [1, None, None]),
                               ([len(parts[0]) // 2, None, None], [1, None, None])):
        capped = RC.run_model(oracle, parts, out_caps=out_caps, msg_caps=msg_caps)
        for a, b in zip(free, capped):
            sa, sb = a.carry, b.carry
            assert (sa.opcode, sa.length, sa.nframes, sa.first_frame, sa.frame_remaining, sa.frame_member,
                    sa.frames_seen) == (sb.opcode, sb.length, sb.nframes, sb.first_frame, sb.frame_remaining,
                                        sb.frame_member, sb.frames_seen)
            assert a.nm == b.nm
        assert capped[0].nm == 3 and capped[0].carry.status & M.UNCHECKED and capped[0].carry.utf8 == b""
        assert capped[1].recs[0][4] & M.UNCHECKED and capped[1].carry.status & M.UNCHECKED
        r0 = capped[2].recs[0]
        assert r0[4] & (M.CONTINUED | M.COMPLETE | M.UNCHECKED) == M.CONTINUED | M.COMPLETE | M.UNCHECKED
        assert not r0[4] & M.UTF8_BAD  # (the FF arrived after validation was abandoned)
        assert capped[2].recs[1] == free[2].recs[1] and capped[2].recs[1][4] == M.COMPLETE
    assert free[2].recs[0][4] & M.UTF8_BAD


SHIM_PROG = r"""
#include <cstdio>
#include "xyws/websocket.hpp"
using namespace xyws;
static_assert(sizeof(xyws_msg_carry) == 64);
int main() {
  try {
    context ctx(0);
    message_assembler as(ctx, nullptr, XYWS_REASM_UTF8);
    as.feed({}, {}, nullptr, {}, {}, nullptr);
    reassemble(ctx, {}, {}, nullptr, 0, {}, {}, nullptr);
    std::puts("device");
    return 0;
  } catch (const error& e) {
    std::printf("error %d\n", e.code());
    return 0;
  }
}
"""


def test_cpp_shim_message_assembler_compiles_and_fails_loudly(tmp_path):
    src = tmp_path / "shim_asm.cpp"
    src.write_text(SHIM_PROG)
    exe = tmp_path / "shim_asm"
    libdir = os.path.dirname(L.lib_path())
    r = subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", str(exe), "-L", libdir, "-lxyws", f"-Wl,-rpath,{libdir}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    assert out.stdout.strip() == ("device" if has_gpu else "error -2")

"""The model of xyws_reassemble_streams (tests/reasm_streams_model.py) on the
inputs the device tests use (the same scenario functions and seeds): per
connection the calls' records fold to the unsplit stream's, overflow is sticky
and leaves the rest of the carry alone, the default capacities never truncate,
and the scenarios reach every situation the device tests count on."""
import ctypes as C

import reasm_cases as RC
import reasm_model as M
import reasm_streams_model as SM
import xynet_amd._lib as L


def geometry():
    g = (C.c_uint64 * 4)()
    assert L.load().xyws_debug_reasm_streams_geometry(g) == 0
    return list(g)


def run(oracle, sweeps, cov=None):
    st, out = SM.State(), []
    for pieces, kw in sweeps:
        kw = {k: v for k, v in kw.items() if k not in ("mis", "omis", "packed")}
        exp = SM.model_sweep(oracle, st, pieces, **kw)
        if cov is not None:
            cov.add(exp)
        out.append(exp)
    return out


class FoldCall:
    def __init__(self, e):
        self.recs, self.frames, self.out = e.recs, e.frames, e.out


def check_folds(oracle, sweeps_exp, wires):
    for i, wire in enumerate(wires):
        RC.check_fold(oracle, wire, [FoldCall(exp[i]) for exp in sweeps_exp])


def never_truncated(sweeps_exp):
    for exp in sweeps_exp:
        for e in exp:
            assert not e.res["status"] & (SM.RSM_TRUNCATED | SM.RSM_MSG_CAP | SM.RSM_OVERFLOW), e.id
            assert len(e.out) == e.res["out_len"] <= len(e.piece) and len(e.recs) == e.res["nmsgs"] <= e.cnt + 1
            assert not any(r[4] & M.TRUNCATED for r in e.recs)


def test_short_stream_every_cut(oracle):
    cov = SM.Coverage()
    for middle in (False, True):
        sweeps, wires, _ = SM.short_every_cut(middle)
        got = run(oracle, sweeps, cov)
        check_folds(oracle, got, wires)
        never_truncated(got)
    cov.require("continued", "closing", "orphans_carried", "tail1", "tail2", "interrupted")


def test_generator_streams(oracle):
    cov = SM.Coverage()
    sweeps, wires, _ = SM.generator(oracle)
    got = run(oracle, sweeps, cov)
    check_folds(oracle, got, wires)
    never_truncated(got)
    cov.require("continued", "orphans_carried", "interrupted")


def test_all_scenarios_reach_every_situation(oracle):
    T, step, grid, _ = geometry()
    cov = SM.Coverage()
    for sweeps in (SM.short_every_cut()[0], SM.generator(oracle)[0], SM.tile_seams(T)[0], SM.copy_seams(step),
                   SM.utf8_fragments()[0]):
        never_truncated(run(oracle, sweeps, cov))
    cov.require()


def test_tile_seam_streams_hold_the_seams(oracle):
    T = geometry()[0]
    sweeps, kinds, conns = SM.tile_seams(T)
    got = run(oracle, sweeps)
    assert sorted({e.cnt for e in got[0] if len(conns[e.id]) == 1}) == [T - 1, T, T + 1, 2 * T + 1]
    long = [kd for kd in kinds if len(kd) > T + 1]
    assert any(kd[T - 1] == "text" and kd[T] == "cont" for kd in long)       # starts in one tile, ends in the next
    assert any(kd[T - 1] == "cont" and kd[T] == "ping" and kd[T + 1] == "fin" for kd in long)  # ping at the edge
    assert any(kd[T - 2] == "cont" and kd[T - 1] == "ping" and kd[T] == "fin" for kd in long)
    assert any(kd[T - 1] == "binary" and kd[T] == "orphan" for kd in long)   # an orphan as a tile's first frame
    # the message across the edge is one record
    for e in got[0]:
        kd = kinds[e.id]
        if len(conns[e.id]) == 1 and len(kd) > T + 2 and kd[T - 1] == "text":
            r = [r for r in e.recs if r[0] == T - 1][0]
            assert r[1] == 3 and r[4] & M.COMPLETE


def test_copy_seams_hold_the_seams(oracle):
    step = geometry()[1]
    (pieces, kw), = SM.copy_seams(step)
    exp = run(oracle, [(pieces, kw)])[0]
    ends = {(e.recs[0][3] + kw["omis"][e.id]) for e in exp}
    assert {step + d for d in range(-3, 4)} <= ends and {16 + d for d in range(-3, 4)} <= ends
    assert all(len(e.recs) == 2 and e.recs[1][2] == e.recs[0][3] for e in exp)
    bad = sum(1 for e in exp for r in e.recs if r[4] & M.UTF8_BAD)
    assert 0 < bad < 2 * len(exp)


def test_slab_two_sweeps(oracle):
    grid = geometry()[2]
    sweeps, conns = SM.slab(grid)
    cov = SM.Coverage()
    got = run(oracle, sweeps, cov)
    assert len(got) == 2 and len(got[0]) == grid + 3
    never_truncated(got)
    cov.require("continued", "tail1")


def test_caps_nulls_and_the_structural_carry(oracle):
    sweeps, noutf8, nomc = SM.caps_and_nulls()
    got = run(oracle, sweeps)
    assert got[0][0].res["nmsgs"] == 3
    assert got[0][1].res["status"] & SM.RSM_TRUNCATED and got[0][2].res["status"] & SM.RSM_MSG_CAP
    assert got[0][4].out == b"" and got[0][4].res["status"] & SM.RSM_TRUNCATED
    assert got[0][5].recs == [] and got[0][5].res["status"] & SM.RSM_MSG_CAP
    for exp in got:
        free = exp[0].carry
        for e in exp[1:]:
            c = e.carry
            assert (c.opcode, c.length, c.nframes, c.first_frame, c.frame_remaining, c.frame_member, c.frames_seen) == \
                (free.opcode, free.length, free.nframes, free.first_frame, free.frame_remaining, free.frame_member,
                 free.frames_seen)
    for k in (1, 2, 3, 4, 5):
        assert got[1][k].recs[0][4] & M.UNCHECKED and got[2][k].recs[0][4] & M.UNCHECKED
    assert got[2][0].recs[0][4] & M.UTF8_BAD and not got[2][0].recs[0][4] & M.UNCHECKED
    g2 = run(oracle, noutf8)
    assert not g2[1][0].recs[0][4] & M.UNCHECKED and g2[2][0].recs[0][4] & M.UNCHECKED
    g3 = run(oracle, nomc)
    assert all(e.carry_in is None for exp in g3 for e in exp)
    assert not any(r[4] & M.CONTINUED for exp in g3 for e in exp for r in e.recs)


def test_overflow_is_sticky_and_leaves_the_carry(oracle):
    first, second = run(oracle, SM.overflow_sweeps())
    assert [e.res["status"] & SM.RSM_OVERFLOW for e in first] == [4, 0, 4, 0]
    assert [e.res["status"] & SM.RSM_OVERFLOW for e in second] == [4, 0, 4, 0]
    for k in (0, 2):
        assert first[k].out == b"" and first[k].recs == [] and first[k].res["out_len"] == 0
        want = SM.copy_carry(first[k].carry_in)
        want.status |= SM.MSG_OVERFLOW
        assert first[k].carry == want and second[k].carry == want  # the rest of the carry as it was
    assert first[1].res == first[3].res and first[1].res["completed"] == 4 and second[1].carry.frames_seen == 10
    # a carry with other state keeps it
    mc = M.Carry(length=5, nframes=2, first_frame=7, frame_remaining=3, frames_seen=9, status=M.UTF8_BAD, opcode=1,
                 frame_member=1)
    out, recs, co, res = SM.feed(b"abc", [], M.REASM_UTF8, mc, 3, 1, nframes=1, cap=0)
    assert (out, recs, res["status"]) == (b"", [], SM.RSM_OVERFLOW)
    assert co.status == M.UTF8_BAD | SM.MSG_OVERFLOW and co.pack()[:40] == mc.pack()[:40] and \
        co.pack()[44:] == mc.pack()[44:]


def test_empty_batch_with_a_message_open(oracle):
    mc = M.Carry(length=4, nframes=1, first_frame=0, frames_seen=1, opcode=1)
    out, recs, co, res = SM.feed(b"", [], M.REASM_UTF8, mc, 1, 1)
    assert out == b"" and recs == [(M.NPOS, 0, 0, 0, M.CONTINUED, 1)] and co == SM.copy_carry(mc)
    assert res["nmsgs"] == 1 and res["status"] & SM.RSM_OPEN

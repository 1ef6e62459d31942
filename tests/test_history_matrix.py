"""The history matrix of test_gpu_history.py through the host-side plan
(xyws_debug_plan: no HIP call, no GPU): the primers' policy words and the
probes' lengths must reach every plan shape the history can steer a call into.
A condition on the test's inputs, not on the decoder: a shape the matrix never
plans is a path the GPU matrix never runs."""
import history
import xynet_amd._lib as L
from test_plan import LSEG, LSEG5, MID, PROD, SMALL, WG512, plan

MODES = {"normal": 0, "small": L.OPT_SMALL_SEG}


def plans():
    """(history, mode, probe name, plan) for the first piece of every probe, at
    the probe's device offset, with descriptors."""
    P = history.primers()
    for h in history.HISTORIES:
        for mode, opts in MODES.items():
            for probe in history.probes(mode):
                n = len(probe.pieces[0])
                yield h, mode, probe, plan(P[h].policy(), probe.offset, probe.offset + n, cap=n // 2 + 2, opts=opts)


def test_primer_words_are_the_states_the_issue_names():
    P = history.primers()
    assert set(history.HISTORIES) == set(P)
    assert P["fresh"].policy()[L.POL_EPOCH] == 0
    for name in ("equal_264_lat", "equal_264_runs"):
        w = P[name].policy()
        assert w[L.POL_FSMIN] == w[L.POL_FSMAX] == 264
    assert P["equal_264_lat"].policy()[L.POL_DECODER] == L.DEC_LATTICE
    assert P["equal_264_runs"].policy()[L.POL_DECODER] in (L.DEC_RUNS, L.DEC_RUNS512)
    w = P["equal_127"].policy()
    assert w[L.POL_FSMIN] == w[L.POL_FSMAX] == 127 < 128  # LAT_FMIN
    w = P["equal_65550"].policy()
    assert w[L.POL_FSMIN] == w[L.POL_FSMAX] == 65550 and w[L.POL_DECODER] == L.DEC_LATTICE
    w = P["mixed_small"].policy()
    assert w[L.POL_FSMIN] != w[L.POL_FSMAX] and w[L.POL_FSMAX] < 2048        # DENSE0_MAX_FRAME
    w = P["mixed_big"].policy()
    assert w[L.POL_FSMIN] != w[L.POL_FSMAX] and w[L.POL_FSMAX] >= 16384      # BIGSCAN_MIN_FRAME
    w = P["no_frame"].policy()
    assert w[L.POL_EPOCH] != 0 and w[L.POL_FSMIN] == w[L.POL_FSMAX] == 0
    for p in P.values():
        assert all(len(src) <= 4 << 20 for src, _ in p.calls)


def test_primers_plan_in_the_geometries_their_words_assume():
    """A primer's own second call, planned from the words its first one left
    (the ones it states), runs the decoder it names."""
    P = history.primers()
    for name, geom, lat in (("equal_264_lat", WG512, 1), ("equal_264_runs", WG512, 0), ("equal_127", WG512, 0),
                            ("equal_65550", PROD, 1), ("mixed_small", MID, 0), ("mixed_big", PROD, 0),
                            ("no_frame", PROD, 0)):
        p = P[name]
        n = len(p.calls[-1][0])
        q = plan(p.policy(), 0, n, opts=p.opts)
        assert (q["geom"], q["want_lat"]) == (geom, lat), (name, q)
        assert p.words[3] == (L.DEC_LATTICE if lat else L.DEC_RUNS512 if geom == WG512 else L.DEC_RUNS)


def test_mixed_primers_hold_two_sizes_only(oracle):
    """The layout behind the mixed primers' words, on the oracle's frames:
    whole frames of the two stated sizes only, each with a payload, the small
    one alone over the first 256 KiB (two runs of every geometry), the big one
    alone over the last."""
    import numpy as np
    P = history.primers()
    for name in ("mixed_small", "mixed_big"):
        src = P[name].calls[-1][0]
        fr, _, n = oracle.decode_stream(np.frombuffer(src, np.uint8).copy(), cap=len(src) // 2 + 2)
        spans = [(f.frame_off, f.payload_off + f.payload_len) for f in fr]
        assert spans[0][0] == 0 and spans[-1][1] == len(src) and all(f.payload_len for f in fr)
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        _, fsmin, fsmax, _ = P[name].words
        assert {b - a for a, b in spans} == {fsmin, fsmax}
        assert {b - a for a, b in spans if a < 256 << 10} == {fsmin}
        assert {b - a for a, b in spans if b > len(src) - (256 << 10)} == {fsmax}


def test_matrix_reaches_every_plan_shape():
    seen = set()
    spans = {}
    for h, mode, probe, p in plans():
        hint = "pfs" if p["pfs"] else "dense0" if p["dense0"] else "bigscan" if p["bigscan"] else "none"
        assert bool(p["pfs"]) + p["dense0"] + p["bigscan"] <= 1, (h, mode, probe.name, p)
        seen.add((p["geom"], hint, p["want_lat"], h))
        # (long_lengths ends where its seed draws the 2^31-byte length: 64 KiB, one run)
        if probe.kind not in ("edge", "split") and not probe.name.startswith("long_lengths"):
            spans.setdefault((h, mode), []).append(p["nruns"])
        if p["want_lat"]:
            assert (p["lseg0"], p["lseg1"]) == (LSEG5, LSEG)
    shapes = [
        (MID, "dense0", 0, "mixed_small"),      # 16 KiB segments with dense0
        (WG512, "pfs", 1, "equal_264_lat"),     # 64 KiB segments with pfs and the lattice first
        (WG512, "pfs", 1, "equal_264_runs"),
        (WG512, "pfs", 0, "equal_127"),         # 64 KiB segments with pfs, no lattice
        (PROD, "none", 1, "fresh"),             # 128 KiB segments, the lattice first, a fresh stream
        (PROD, "none", 1, "equal_65550"),       # ...after large equal frames: no pfs (65550 > seg / 4)
        (PROD, "bigscan", 0, "mixed_big"),      # 128 KiB segments with bigscan
        (PROD, "none", 0, "no_frame"),          # 128 KiB segments, no hint (FSMAX == 0)
        (SMALL, "pfs", 0, "equal_127"),         # small segments with pfs (127 <= 1024 / 4; 264 is not)
        (SMALL, "dense0", 0, "mixed_small"),    # small segments with dense0
        (SMALL, "bigscan", 0, "mixed_big"),     # small segments with bigscan
    ]
    for s in shapes:
        assert s in seen, (s, sorted(seen))
    # the generated probes span several runs in the geometry each history
    # selects: 8 segments at least (16 of 64 KiB, 64 of 16 KiB, ~200 of 1 KiB)
    for (h, mode), nruns in spans.items():
        assert min(nruns) >= (8 if mode == "normal" else 190), (h, mode, min(nruns))

"""The stream decode's host-side plan (plan_decode, plan_reserve in
xyws_stream.hip) through xyws_debug_plan: integer arithmetic on {compute
units, policy words, lo, hi, cap, opts}, no HIP call, so no GPU.

Anchor rows are derived by hand from the choice as DESIGN §4.3 states it
(the derivation stands beside each); the properties run over a seeded sweep.
The last one is xyws_ctx_reserve's promise: whatever a call of a reserved size
plans, the reserve computation covers it."""
import ctypes as C
import random

import pytest

import xynet_amd._lib as L

NCU = 256
# geometries (xyws_stream.hip): segment bytes, threads, runs per CU
SMALL, MID, WG512, PROD = 0, 1, 2, 3
SEG = {SMALL: 1024, MID: 16384, WG512: 65536, PROD: 131072}
THREADS = {SMALL: 64, MID: 256, WG512: 512, PROD: 1024}
PER_CU = {MID: 4, WG512: 2, PROD: 1}
MAX_RUNS = 1024
LSEG5, LSEG = 76800, 122880  # the lattice decoder's 75 KiB / 120 KiB segments
OPT_PARSE_ONLY, OPT_WG256 = L.OPT_PARSE_ONLY, L.OPT_WG256
FIELDS = ("geom", "seg", "threads", "nruns", "rbytes", "nflat", "want_lat", "lnseg", "lgrid", "lseg0", "lseg1",
          "pfs", "dense0", "bigscan", "rcap", "need_runs", "need_fmem", "need_lat")



def policy(epoch, nbytes, fsmin, fsmax, decoder):
    """The policy words a call leaves (L.POL_*)."""
    words = [0] * L.POL_WORDS
    words[L.POL_EPOCH], words[L.POL_BYTES], words[L.POL_FSMIN], words[L.POL_FSMAX] = epoch, nbytes, fsmin, fsmax
    words[L.POL_DECODER] = decoder
    return words


FRESH = policy(0, 0, 0, 0, 0)            # no call has finished on the stream
EQUAL_264 = policy(7, 1 << 28, 264, 264, L.DEC_LATTICE)
EQUAL_127 = policy(7, 1 << 20, 127, 127, L.DEC_RUNS512)
MIXED_1000 = policy(3, 4 << 20, 2, 1006, L.DEC_RUNS)    # 0-1000 B payloads
MIXED_1M = policy(3, 128 << 20, 100, 1 << 20, L.DEC_RUNS)
POLICIES = [None, FRESH, EQUAL_264, EQUAL_127, MIXED_1000, MIXED_1M]


def plan(pol, lo, hi, cap=0, opts=0, ncu=NCU):
    lib = L.load()
    out = (C.c_uint64 * len(FIELDS))()
    words = (C.c_uint64 * L.POL_WORDS)(*pol) if pol is not None else None
    assert lib.xyws_debug_plan(ncu, words, lo, hi, cap, opts, out) == 0
    return dict(zip(FIELDS, out))


def reserve(batch, frames, ncu=NCU):
    out = (C.c_uint64 * 3)()
    assert L.load().xyws_debug_plan_reserve(ncu, batch, frames, out) == 0
    return tuple(out)


def test_first_call_on_a_stream_2gib():
    # no previous call: the lattice decoder first, in 75 KiB segments for the
    # grid (the kernel may take 120 KiB ones), one workgroup per CU; no frame
    # sizes known: the default geometry, 2^31 / 128 KiB = 16384 segments over
    # 256 runs of 2^31 / 256 = 8388608 bytes
    p = plan(FRESH, 0, 1 << 31)
    assert (p["want_lat"], p["lseg0"], p["lseg1"], p["lgrid"]) == (1, LSEG5, LSEG, 256)
    assert p["lnseg"] == 27963  # ceil(2147483648 / 76800) = ceil(27962.03)
    assert (p["geom"], p["seg"], p["threads"]) == (PROD, 131072, 1024)
    assert (p["nruns"], p["rbytes"], p["nflat"]) == (256, 8388608, 512)
    assert (p["pfs"], p["dense0"], p["bigscan"], p["rcap"]) == (0, 0, 0, 0)
    assert (p["need_runs"], p["need_fmem"], p["need_lat"]) == (256, 0, 27963)
    # 5 bytes past the 16-byte line: ceil((2^31 + 5) / 256) = 8388609, rounded up to 16
    p = plan(FRESH, 5, (1 << 31) + 5)
    assert (p["nruns"], p["rbytes"]) == (256, 8388624)


def test_after_equal_264_byte_frames():
    # one size >= LAT_FMIN (128): the lattice; under WG512_MAX_FRAME (2048)
    # and one size: two 512-thread workgroups per CU on 64 KiB segments, 2^28 /
    # 64 KiB = 4096 segments over 512 runs of 2^28 / 512 bytes; 264 <= 65536 /
    # 4: the lattice entry hint; one size: no dense0
    p = plan(EQUAL_264, 0, 1 << 28)
    assert (p["want_lat"], p["lnseg"], p["lgrid"]) == (1, 3496, 256)  # ceil(268435456 / 76800) = ceil(3495.25)
    assert (p["geom"], p["seg"], p["threads"]) == (WG512, 65536, 512)
    assert (p["nruns"], p["rbytes"]) == (512, 524288)
    assert (p["pfs"], p["dense0"], p["bigscan"]) == (264, 0, 0)


def test_after_small_mixed_frames_4mib():
    # mixed sizes under 2048 and a batch of at most 32 KiB per CU (8 MiB): four
    # 256-thread workgroups per CU on 16 KiB segments; 4 MiB / 16 KiB = 256
    # segments <= min(4 * 256, 1024) runs: one segment per run
    p = plan(MIXED_1000, 0, 4 << 20, cap=1000)
    assert (p["geom"], p["seg"], p["threads"]) == (MID, 16384, 256)
    assert (p["nruns"], p["rbytes"]) == (256, 16384)
    assert (p["want_lat"], p["pfs"], p["dense0"], p["bigscan"]) == (0, 0, 1, 0)
    # regions of 2 * ceil(1000 / 256) + 1024 entries; the need 8 * (4 * cap + 2052 * nruns)
    assert (p["rcap"], p["need_fmem"]) == (1032, 8 * (4000 + 2052 * 256))
    # at the threshold 512 segments, one each
    assert plan(MIXED_1000, 0, 8 << 20)["nruns"] == 512
    # the cap: forced on 64 MiB, 4096 segments over 1024 runs of 64 KiB
    p = plan(MIXED_1000, 0, 64 << 20, opts=OPT_WG256)
    assert (p["geom"], p["nruns"], p["rbytes"]) == (MID, 1024, 65536)


def test_after_small_mixed_frames_64mib():
    # past 8 MiB not the 256-thread geometry; mixed sizes take the 512-thread
    # one only under one 128 KiB segment per CU (32 MiB): the default, 512
    # segments over 256 runs of 256 KiB
    p = plan(MIXED_1000, 0, 64 << 20)
    assert (p["geom"], p["nruns"], p["rbytes"]) == (PROD, 256, 262144)
    assert (p["want_lat"], p["dense0"]) == (0, 1)
    # under 32 MiB, over 8 MiB: 16 MiB / 64 KiB = 256 segments, one per run
    p = plan(MIXED_1000, 0, 16 << 20)
    assert (p["geom"], p["nruns"], p["rbytes"]) == (WG512, 256, 65536)


def test_after_mixed_frames_up_to_1mib():
    # a last frame of BIGSCAN_MIN_FRAME (16384) or more, mixed: the one-pass entry scans
    p = plan(MIXED_1M, 0, 128 << 20)
    assert (p["geom"], p["nruns"], p["rbytes"]) == (PROD, 256, 524288)
    assert (p["want_lat"], p["pfs"], p["dense0"], p["bigscan"]) == (0, 0, 0, 1)


def test_equal_frames_under_lat_fmin():
    p = plan(EQUAL_127, 0, 1 << 20)
    assert (p["want_lat"], p["geom"], p["pfs"]) == (0, WG512, 127)


@pytest.mark.parametrize("opt", [L.OPT_RUNS, L.OPT_NO_LATDEC, OPT_PARSE_ONLY])
def test_options_that_keep_the_lattice_out(opt):
    assert plan(FRESH, 0, 1 << 24)["want_lat"] == 1
    assert plan(FRESH, 0, 1 << 24, opts=opt)["want_lat"] == 0
    assert plan(EQUAL_264, 0, 1 << 24, opts=opt)["want_lat"] == 0


def test_small_segment_mode():
    # 1 KiB segments, a run each: ceil(100003 / 1024) = 98; the lattice only forced
    p = plan(FRESH, 3, 100003, opts=L.OPT_SMALL_SEG)
    assert (p["geom"], p["seg"], p["threads"], p["nruns"], p["rbytes"]) == (SMALL, 1024, 64, 98, 1024)
    assert p["want_lat"] == 0
    assert plan(EQUAL_264, 3, 100003, opts=L.OPT_SMALL_SEG)["want_lat"] == 0
    p = plan(FRESH, 3, 100003, opts=L.OPT_SMALL_SEG | L.OPT_LATTICE)
    assert (p["want_lat"], p["lseg0"], p["lseg1"], p["lnseg"], p["lgrid"]) == (1, 1024, 1024, 98, 64)
    assert p["nruns"] == 98


def test_no_policy_words():
    p = plan(None, 0, 1 << 28)
    assert (p["want_lat"], p["geom"], p["nruns"]) == (0, PROD, 256)
    assert (p["pfs"], p["dense0"], p["bigscan"]) == (0, 0, 0)


def test_empty_call():
    for pol in POLICIES:
        p = plan(pol, 7, 7, cap=100)
        assert (p["nruns"], p["want_lat"], p["rcap"]) == (0, 0, 0)
        assert (p["need_runs"], p["need_fmem"], p["need_lat"]) == (0, 0, 0)


def test_reserve_covers_the_batch_one_run_short():
    # 1024 descriptors over 1023 runs take regions of 2 * 2 + 1024 entries,
    # over 1024 runs of 2 * 1 + 1024: the smaller batch's regions total more
    # (8 * 2046 * 1028 > 8 * 2048 * 1026 bytes), and the reserve for the larger
    # batch still covers it
    p = plan(None, 0, 1023 * 16384, cap=1024, opts=OPT_WG256)
    q = plan(None, 0, 1024 * 16384, cap=1024, opts=OPT_WG256)
    assert (p["nruns"], p["rcap"], q["nruns"], q["rcap"]) == (1023, 1028, 1024, 1026)
    assert 8 * p["nflat"] * p["rcap"] > 8 * q["nflat"] * q["rcap"]
    assert 8 * p["nflat"] * p["rcap"] <= p["need_fmem"] <= reserve(1024 * 16384 - 15, 1024)[1]


FORCED = [0, L.OPT_WG1024, L.OPT_WG512, OPT_WG256, L.OPT_LATTICE, L.OPT_RUNS, L.OPT_SMALL_SEG,
          L.OPT_SMALL_SEG | L.OPT_LATTICE]


def sweep(n=4000):
    rng = random.Random(0x9E3779B9)
    for i in range(n):
        length = max(1, int(2 ** rng.uniform(0, 34)))
        if i % 5 == 0:  # (on and around the segment multiples)
            length = max(1, rng.choice([16384, 65536, 131072, 76800]) * rng.randrange(1, 3000) + rng.randrange(-1, 2))
        lo = rng.randrange(16)
        cap = rng.choice([0, 0, 1, 1023, 1024, 1025, rng.randrange(1, 1 << 20)])
        ncu = rng.choice([NCU, NCU, 304, 64, 1])
        yield ncu, rng.choice(POLICIES), lo, lo + length, cap, rng.choice(FORCED), rng


def test_properties_over_a_sweep():
    for ncu, pol, lo, hi, cap, opts, rng in sweep():
        p = plan(pol, lo, hi, cap, opts, ncu)
        what = (ncu, pol, lo, hi, cap, hex(opts), p)
        g = p["geom"]
        assert (p["seg"], p["threads"]) == (SEG[g], THREADS[g]), what
        assert p["nruns"] * p["rbytes"] >= hi, what
        assert (p["nruns"] - 1) * p["rbytes"] < hi, what
        assert p["rbytes"] % 16 == 0 and p["rbytes"] >= p["seg"], what
        assert p["nflat"] == 2 * p["nruns"], what
        if g != SMALL:
            assert p["nruns"] <= min(PER_CU[g] * ncu, MAX_RUNS), what
        assert p["lgrid"] <= max(ncu, 64), what
        if p["want_lat"]:
            assert p["lgrid"] >= 1 and p["lnseg"] * p["lseg0"] >= hi > (p["lnseg"] - 1) * p["lseg0"], what
        # the needs cover what the launch uses
        assert p["need_runs"] == p["nruns"], what
        assert p["need_lat"] == (p["lnseg"] if p["want_lat"] else 0), what
        assert (p["rcap"] != 0) == (cap != 0) and p["need_fmem"] >= 8 * p["nflat"] * p["rcap"], what
        if cap:
            assert p["rcap"] >= 2 * cap // p["nruns"] + 1024, what
        # the reserve property: a reserve for (B, F) covers every call of at
        # most B bytes (at any alignment) and F descriptors
        if g != SMALL:
            length = hi - lo
            for batch, frames in ((length, cap), (length + rng.randrange(1 << 24), cap + rng.randrange(4096))):
                r = reserve(batch, frames, ncu)
                need = (p["need_runs"], p["need_fmem"], p["need_lat"])
                assert all(a <= b for a, b in zip(need, r)), (what, batch, frames, r)

"""xyws_decode_stream under controlled stream histories: every edge stream
after every state a previous call can leave in the (context, stream) slot.

The history (history.py) is the pinned policy words plan_decode reads and the
device policy word the lattice decoder's prologue reads. It may decide speed
only: whatever it is, a probe's frame count, bytes, descriptors and carry are
the oracle's, the guard bytes around the batch stay, and the device error
word stays 0. Each test makes its own context, so "fresh" is a stream no call
has finished on and no other test's calls touch the slot.

Timings: settled (primer, synchronize, the words asserted, probe), in_flight
(primer, primer, probe queued behind work that keeps the stream busy: the host
plans all of them from the words of before), stale (primer A settled, then
primer B and the probe queued: the host plans from A while the device word
says B)."""
import ctypes as C

import pytest

import history
from test_gpu_parity import carry_list, dev_bytes, frames_list, host
from xynet_amd import _lib
from xynet_amd._lib import DEC_LATTICE, POL_BYTES, POL_DECODER, POL_EPOCH, POL_FSMAX, POL_FSMIN, POL_WORDS

ERR_INVALID = -1  # XYWS_ERR_INVALID (include/xyws.h): the debug readers' answer for a stream without a slot

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MODES = {"normal": 0, "small": _lib.OPT_SMALL_SEG}
# descriptors asked for, from the probe's frame count n
CAPS = {"all": lambda n: n + 2, "none": lambda n: 0, "some": lambda n: int(0.6 * n)}
CASES = ([(h, "settled") for h in history.HISTORIES] + [(h, "in_flight") for h in history.HISTORIES] +
         [(f"{a}>{b}", "stale") for a, b in history.STALE_PAIRS])
# xyws_debug_lattice (see test_gpu_choice._lat_counters): cumulative per slot
BAIL_POL, BAIL_HYP, LOOP_75K, LOOP_120K = 1, 2, 3, 4
LOOP_OF = {264: LOOP_120K, 65550: LOOP_75K}
# histories after which plan_decode launches the lattice decoder first (lattice_preferred)
LATTICE_FIRST = ("fresh", "equal_264_lat", "equal_264_runs", "equal_65550")


@pytest.fixture(scope="module")
def ws():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from xynet_amd import websocket
    return websocket


@pytest.fixture(scope="module")
def ballast():
    """Device work that keeps the stream busy while the host queues calls
    behind it (see Slot.hold)."""
    t = torch.zeros(512 << 20, dtype=torch.uint8, device="cuda")
    yield t
    del t
    torch.cuda.empty_cache()


class Slot:
    """One context of the test's own and the decoders on it."""

    def __init__(self, ws, ballast):
        self.ws, self.ballast = ws, ballast
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.ctx = None
        self.bufs = {}
        self.renew()

    def renew(self):
        """A context no call has run on. The scratch for every batch of the
        matrix is reserved first: an area that grew between a primer and its
        probe would come back zeroed, the device policy word with it."""
        self.close()
        self.ctx = self.ws.Context(0)
        self.ctx.reserve(16 << 20, 1 << 16)
        self.pdec = {}

    def close(self):
        if self.ctx is not None:
            torch.cuda.synchronize()
            self.ctx.close()
            self.ctx = None

    def policy(self):
        """The pinned words of the stream's slot, or None when no call has
        bound one (xyws_debug_policy: XYWS_ERR_INVALID). Synchronizes."""
        out = (C.c_uint64 * POL_WORDS)()
        rc = self.ctx.L.xyws_debug_policy(self.ctx.h, self.stream, out)
        if rc == ERR_INVALID:
            return None
        assert rc == 0, rc
        return list(out)

    def lattice(self):
        out = (C.c_uint64 * 5)()
        rc = self.ctx.L.xyws_debug_lattice(self.ctx.h, self.stream, out)
        if rc == ERR_INVALID:
            return [0] * 5
        assert rc == 0, rc
        return list(out)

    def hold(self):
        """Queue a few passes over 512 MiB: the calls queued next are planned
        before any of them has finished."""
        for _ in range(4):
            self.ballast.add_(1)

    def load(self, primer):
        """The primer's batches on the device (a copy from the host waits for
        the stream: before any hold)."""
        for k, (src, _) in enumerate(primer.calls):
            if (primer.name, k) not in self.bufs:
                self.bufs[(primer.name, k)] = dev_bytes(src)[0]

    def prime(self, primer, settled=False):
        """Queue the primer's calls (settled: each planned from the words the
        one before it left; else no synchronization). Its batches live on the
        device once per test: a decode writes payload bytes only, so a batch
        decoded again has the same frames."""
        if not primer.calls:
            return
        if primer.name not in self.pdec:
            self.pdec[primer.name] = self.ws.frame_decoder(ctx=self.ctx, opts=primer.opts)
        dec = self.pdec[primer.name]
        self.load(primer)
        for k, (src, fresh_carry) in enumerate(primer.calls):
            key = (primer.name, k)
            if fresh_carry:
                dec.reset()
            dec.decode(self.bufs[key], cap=0, count=False)
            if settled:
                torch.cuda.synchronize()

    def settle(self, primer):
        """The primer run to its end, and the words it must have left."""
        if not primer.calls:
            self.renew()
            assert self.policy() is None
            return
        self.prime(primer, settled=True)
        p = self.policy()
        # (the epoch is the finishing decoder's own count of its calls: != 0, not monotonic)
        assert p[POL_EPOCH] != 0, (primer.name, p)
        assert (p[POL_BYTES], p[POL_FSMIN], p[POL_FSMAX], p[POL_DECODER]) == primer.words, (primer.name, p)
        dp = self.lattice()[0]
        assert dp >> 63 and (dp >> 48) & 0x7F == primer.words[3] and dp & ((1 << 48) - 1) == primer.regular, \
            (primer.name, hex(dp))


def check_probe(slot, probe, res, bufs, caps, oracle, what, mids=None):
    """Every piece of a decoded probe against the oracle."""
    exp = probe.expected(oracle)
    off = probe.offset
    for i, (piece, r, (view, whole), cap, (obytes, ofr, ocarry, on)) in enumerate(
            zip(probe.pieces, res, bufs, caps, exp)):
        w = what + (i,)
        assert r.nframes == on, w
        out = host(whole)
        assert out[:off] == b"\xa5" * off and out[off + len(piece):] == b"\xa5" * 32, w
        assert out[off:off + len(piece)] == obytes, w
        assert frames_list(r.frames(), True) == ofr[:min(on, cap)], w
        if mids is not None and i < len(mids):
            assert mids[i] == ocarry, w
    return exp[-1][2]


@pytest.mark.parametrize("capmode", list(CAPS))
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case,timing", CASES)
def test_probes_after_history(ws, oracle, ballast, case, timing, mode, capmode):
    P = history.primers()
    a, b = (case.split(">") + [None])[:2]
    slot = Slot(ws, ballast)
    for name in (a, b):
        if name:
            slot.load(P[name])
    moved = [0] * 5   # the lattice counters' advance over the probes (and the primers queued with them)
    try:
        for probe in history.probes(mode):
            what = (case, timing, mode, capmode, probe.name)
            exp = probe.expected(oracle)
            caps = [CAPS[capmode](e[3]) for e in exp]
            bufs = [dev_bytes(piece, probe.offset) for piece in probe.pieces]
            dec = ws.frame_decoder(ctx=slot.ctx, opts=MODES[mode])
            mids = None
            if timing == "settled":
                slot.settle(P[a])
                if not P[a].calls:
                    dec = ws.frame_decoder(ctx=slot.ctx, opts=MODES[mode])  # (the renewed context)
                l0 = slot.lattice()
                res, mids = [], []
                for (view, _), cap in zip(bufs, caps):
                    res.append(dec.decode(view, cap=cap))
                    mids.append(carry_list(dec.carry()))
            else:
                if timing == "stale":
                    slot.settle(P[a])
                elif not P[a].calls:
                    slot.renew()
                    dec = ws.frame_decoder(ctx=slot.ctx, opts=MODES[mode])
                l0 = slot.lattice()
                torch.cuda.synchronize()
                slot.hold()
                if timing == "stale":
                    slot.prime(P[b])
                else:
                    slot.prime(P[a])
                    slot.prime(P[a])
                res = [dec.decode(view, cap=cap) for (view, _), cap in zip(bufs, caps)]
            torch.cuda.synchronize()
            ocarry = check_probe(slot, probe, res, bufs, caps, oracle, what, mids)
            assert carry_list(dec.carry()) == ocarry, what
            assert slot.ctx.last_device_error() == 0, what
            l1 = slot.lattice()
            for i in range(1, 5):
                moved[i] += l1[i] - l0[i]
            if timing == "settled" and mode == "normal" and a in LATTICE_FIRST:
                # the host sends the probe to the lattice decoder first: gated
                # on a fresh stream and after equal_264_runs (the device word is
                # not the lattice's), ungated after equal_264_lat / equal_65550.
                # On a regular probe its segment loops ran, in the geometry of
                # the probe's own first frame, and it finished the call
                if probe.kind == "regular":
                    assert l1[LOOP_OF[probe.F]] == l0[LOOP_OF[probe.F]] + 1, (what, l0, l1)
                    assert slot.policy()[POL_DECODER] == DEC_LATTICE, what
                # a break at frame 3 passes the prologue's checks (points 1, 2),
                # reaches the loops and ends in the run decoder
                if probe.kind == "break3":
                    assert l1[LOOP_OF[probe.F]] == l0[LOOP_OF[probe.F]] + 1, (what, l0, l1)
                    assert l1[BAIL_HYP] == l0[BAIL_HYP] and l1[BAIL_POL] == l0[BAIL_POL], (what, l0, l1)
                    assert slot.policy()[POL_DECODER] != DEC_LATTICE, what
        print(f"history {case} {timing} {mode} {capmode}: handed over on the policy word {moved[BAIL_POL]}, "
              f"by the checks {moved[BAIL_HYP]}, loops in 75 KiB {moved[LOOP_75K]}, in 120 KiB {moved[LOOP_120K]}")
        # queued behind an irregular call, a lattice call the host still sent
        # (planned from the words of before) was handed whole to the run decoder
        # on the device policy word (na = 2)
        device_history = P[b] if timing == "stale" else P[a]
        if timing != "settled" and device_history.calls and device_history.regular < 128:  # LAT_FMIN
            assert moved[BAIL_POL] >= 1, (case, timing, mode, capmode, moved)
    finally:
        slot.close()

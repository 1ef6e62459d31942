"""Stream histories for xyws_decode_stream: primers and probes.

What a call does with a batch depends on the batch and on what the previous
call on the same (context, stream) slot left behind: the pinned policy words
(POL_*, read by plan_decode on the host) and the device policy word (LW_DPOL,
read by the lattice decoder's prologue). A *primer* is the smallest batch that
leaves one such state; a *probe* is a batch decoded after it. The contract the
probes hold the decoder to: the history decides speed only, never bytes
(xyws_lattice.h, "the hypothesis decides speed only"; xyws_stream.h,
policy_view).

Used by test_gpu_history.py (on the device) and test_history_matrix.py (the
same words and lengths through xyws_debug_plan, no GPU). The adversarial
generators of test_gpu_parity.py live here too (adversarial_stream,
header_like_dense): the old tests import them.
"""
import numpy as np

import streams
import xynet_amd._lib as L

# --------------------------------------------------------------------------- frames
# Frame sizes on the wire with a masked minimal header: 6 + plen for plen < 126,
# 8 + plen up to 65535, 14 + plen above. (132 and 133 bytes cannot be made.)


def quick_frame(rng, b0, plen):
    """A masked frame whose wire payload is random bytes (any bytes are some
    payload under the key: no Python XOR loop)."""
    return streams.header(b0, plen, rng.bytes(4)) + rng.bytes(plen)


def sized_frame(rng, size, b0=0x82):
    """A masked frame of exactly `size` wire bytes."""
    assert 6 <= size <= 131 or 134 <= size <= 65543, size
    return quick_frame(rng, b0, size - 6 if size <= 131 else size - 8)


SMALL_END = 100  # under LAT_FMIN: a lattice call on the batch bails on its first frame


def _mixed_two_sizes(seed, big_size):
    """A batch of mixed frame sizes whose policy words do not depend on where
    the runs are cut. The finisher folds into POL_FSMIN / POL_FSMAX the size of
    the last whole frame of every run that counted one (k_stream_runs:
    fs_note(last_frame_size(L.S)); pol_publish), and which frame a run's chain
    ends on depends on the entry its successor's scan found. So every frame
    is SMALL_END or `big_size` bytes (the words can be nothing else), the first
    256 KiB hold only the small size (run 0 and its successor's entry lie
    inside them in every geometry: 16, 64 or 128 KiB runs, so run 0 ends on a
    small frame), the last 256 KiB only the big one and the batch ends with a
    whole frame (the last run ends on a big frame); a random mix between.
    Every frame has a payload: the size is measured from the start of the last
    frame that had one (last_frame_size's cov_start)."""
    rng = streams.SplitMix(seed)
    out = bytearray()
    while len(out) < 256 << 10:
        out += sized_frame(rng, SMALL_END)
    while len(out) < 512 << 10:
        out += sized_frame(rng, big_size if rng.below(4) == 0 else SMALL_END)
    for _ in range((256 << 10) // big_size + 1):
        out += sized_frame(rng, big_size)
    return bytes(out)


# --------------------------------------------------------------------------- primers
class Primer:
    """calls: the decode calls that leave the state, in order: (bytes, reset the
    carry first). opts: the options of those calls. words: the policy words the
    last call's finisher publishes (None: no call, no slot), without the epoch
    (POL_EPOCH is the finishing decoder's own count of its calls: != 0 after
    any call). Each call is planned from the words the one before it left when
    the primer is run settled; queued without a wait, from older ones.
    regular: the frame size the device policy word then carries (0: mixed
    sizes); under LAT_FMIN the lattice decoder hands the next batch over whole
    (na = 2)."""

    def __init__(self, name, calls, opts, words, regular):
        self.name, self.calls, self.opts, self.words, self.regular = name, calls, opts, words, regular

    def policy(self, epoch=2):
        """The pinned words as xyws_debug_plan takes them."""
        w = [0] * L.POL_WORDS
        if self.words is not None:
            w[L.POL_EPOCH] = epoch
            w[L.POL_BYTES], w[L.POL_FSMIN], w[L.POL_FSMAX], w[L.POL_DECODER] = self.words
        return w


def _equal(seed, plen, n):
    rng = streams.SplitMix(seed)
    return b"".join(quick_frame(rng, 0x82, plen) for _ in range(n))


def _primers():
    p = {}
    # no call at all: the context has no slot for the stream, epoch 0
    p["fresh"] = Primer("fresh", [], 0, None, 0)

    # 1000 frames of 8 + 256 bytes, twice. Whatever went before, the first call
    # ends with FSMIN == FSMAX == 264: by the lattice decoder (its finisher
    # writes {E, bytes, F, F, DEC_LATTICE}, xyws_lattice.h) or, after an
    # irregular call, by the run decoder (every run's last frame is 264 bytes).
    # The second call is then planned from one size >= LAT_FMIN
    # (lattice_preferred), the prologue finds F = 264 and points 1 and 2 on the
    # lattice, every segment holds: the lattice's finisher again.
    b = _equal(0x264, 256, 1000)
    p["equal_264_lat"] = Primer("equal_264_lat", [(b, True), (b, True)], 0,
                                (len(b), 264, 264, L.DEC_LATTICE), 264)
    # the same with XYWS_OPT_NO_LATDEC: want_lat is off, the run decoder's
    # finisher publishes; the second call is planned from one size under
    # WG512_MAX_FRAME (wg512_preferred): 512-thread workgroups, DEC_RUNS512.
    # LW_DPOL then says {264, DEC_RUNS512}: regular, not the lattice's, so the
    # next lattice call keeps its first-segment gate (nogate needs DEC_LATTICE).
    p["equal_264_runs"] = Primer("equal_264_runs", [(b, True), (b, True)], L.OPT_NO_LATDEC,
                                 (len(b), 264, 264, L.DEC_RUNS512), 264)

    # 2000 frames of 6 + 121 = 127 bytes, under LAT_FMIN (128): never the
    # lattice (a fresh stream's lattice call bails on its first frame's size);
    # one size under WG512_MAX_FRAME: DEC_RUNS512 on the second call; the next
    # call's pfs is 127 in every geometry (127 <= 1024 / 4).
    b = _equal(0x127, 121, 2000)
    p["equal_127"] = Primer("equal_127", [(b, True), (b, True)], 0, (len(b), 127, 127, L.DEC_RUNS512), 127)

    # 16 frames of 14 + 65536 bytes: as equal_264_lat; F >= LAT5_MIN_FRAME, so
    # the lattice runs its 75 KiB segments; 65550 > seg / 4 in every geometry:
    # no pfs.
    b = _equal(0x65550, 65536, 16)
    p["equal_65550"] = Primer("equal_65550", [(b, True), (b, True)], 0,
                              (len(b), 65550, 65550, L.DEC_LATTICE), 65550)

    # frames of 100 and 1008 bytes (94 and 1000 B payloads) over 768 KiB (6 runs
    # in the 128 KiB geometry, 48 in the 16 KiB one): see _mixed_two_sizes. The
    # second call is planned from mixed sizes under 2048 on a batch of at most
    # 32 KiB per CU: the 16 KiB geometry, 256 threads, so DEC_RUNS.
    b = _mixed_two_sizes(0x5A11, 1008)
    p["mixed_small"] = Primer("mixed_small", [(b, True), (b, True)], 0, (len(b), SMALL_END, 1008, L.DEC_RUNS), 0)

    # frames of 100 and 20008 bytes (>= BIGSCAN_MIN_FRAME). Planned from FSMAX
    # >= WG512_MAX_FRAME: the default geometry, DEC_RUNS.
    b = _mixed_two_sizes(0xB166, 20008)
    p["mixed_big"] = Primer("mixed_big", [(b, True), (b, True)], 0, (len(b), SMALL_END, 20008, L.DEC_RUNS), 0)

    # A 14-byte header announcing 1 MiB, then 256 KiB of its payload: the second
    # batch lies wholly inside the carried frame. No run counts a frame, so no
    # fs_note: HW_FSMAX stays 0 and pol_publish writes FSMIN = FSMAX = 0 (and
    # the device word's size 0: irregular). With FSMAX == 0 neither geometry
    # choice applies: the default one, DEC_RUNS. (On a fresh stream the lattice
    # kernel goes first and bails: S0.X >= hi.)
    rng = streams.SplitMix(0x0F)
    hdr = streams.header(0x82, 1 << 20, rng.bytes(4))
    body = rng.bytes(256 << 10)
    p["no_frame"] = Primer("no_frame", [(hdr, True), (body, False), (hdr, True), (body, False)], 0,
                           (len(body), 0, 0, L.DEC_RUNS), 0)
    assert all(len(src) <= 4 << 20 for x in p.values() for src, _ in x.calls)
    return p


_PRIMERS = None


def primers():
    global _PRIMERS
    if _PRIMERS is None:
        _PRIMERS = _primers()
    return _PRIMERS


HISTORIES = ["fresh", "equal_264_lat", "equal_264_runs", "equal_127", "equal_65550", "mixed_small", "mixed_big",
             "no_frame"]
# stale: A settled (the host plans from A), B queued behind it (LW_DPOL says B)
STALE_PAIRS = [("equal_264_lat", "mixed_small"), ("mixed_small", "equal_264_lat"),
               ("equal_65550", "mixed_big"), ("mixed_big", "equal_65550")]


# --------------------------------------------------------------------------- moved generators
def header_like_dense(fake, target=3 << 20):
    """Many small frames whose wire payload bytes are themselves chains of
    plausible client headers (test_dense_frames_with_header_like_payloads)."""
    rng = streams.SplitMix(0xDE5E + fake)
    out = bytearray()
    while len(out) < target:
        plen = 120 + rng.below(400)
        key = rng.bytes(4)
        if fake == 0:
            wire = rng.bytes(plen)
        else:
            # fake 7-byte frames (FIN binary, masked, 1-byte payload) or, for
            # fake == 2, fake 126-form frames that jump within the segment
            unit = (bytes([0x82, 0x81]) + rng.bytes(5)) if fake == 1 else \
                (bytes([0x82, 0xFE, 0x00, 0x40]) + rng.bytes(4) + rng.bytes(64))
            off = rng.below(len(unit))
            wire = (rng.bytes(off) + unit * (plen // len(unit) + 2))[:plen]
        out += streams.header(0x82, plen, key, None) + wire
    return bytes(out)


ADVERSARIAL_KINDS = ["stride_fakes", "size_changes", "long_lengths", "segment_ends"]


def adversarial_stream(kind, target):
    """Streams made to mislead the run decoder's stride pass
    (test_stride_pass_adversarial)."""
    rng = streams.SplitMix(0x57D1 + len(kind))
    out = bytearray()
    while len(out) < target:
        if kind == "stride_fakes":
            plen = 100 + rng.below(300)
            # the payload: valid headers of frames of exactly `size` bytes at every
            # offset d, d + size, ... from a random d (fake starts on a shifted lattice)
            fake = streams.header(0x82, plen, rng.bytes(4), None)
            size = len(fake) + plen
            d = 1 + rng.below(size - 1)
            body = bytearray(rng.bytes(plen))
            for o in range(d % size, plen - len(fake), size):
                body[o:o + len(fake)] = fake
            for _ in range(1 + rng.below(40)):
                out += streams.header(0x82, plen, rng.bytes(4), None) + bytes(body)
        elif kind == "size_changes":
            plen = rng.below(600)
            for _ in range(1 + rng.below(6)):
                out += streams.frame(rng, 0x82, plen)
        elif kind == "long_lengths":
            for _ in range(1 + rng.below(20)):
                out += streams.frame(rng, 0x81, 126 + rng.below(2))  # 126 form at the 7-bit edge
            out += streams.frame(rng, 0x82, 65536 + rng.below(3))    # 127 form
            if rng.below(8) == 0:
                out += streams.header(0x82, (1 << 31) + rng.below(5), rng.bytes(4), None)  # runs past the end
                break
        else:  # equal frames whose headers straddle 1 KiB and 128 KiB boundaries
            plen = 1024 - 8 - rng.below(24)
            for _ in range(1 + rng.below(200)):
                out += streams.frame(rng, 0x82, plen)
    return bytes(out)


# --------------------------------------------------------------------------- probes
class Probe:
    """pieces: the batches of one stream, decoded in order with the carry
    chained (one piece: a whole stream). offset: where each lies in its guarded
    device buffer. kind / F: what the path assertions select on."""

    def __init__(self, name, pieces, offset=0, kind="edge", F=0):
        self.name, self.pieces, self.offset, self.kind, self.F = name, pieces, offset, kind, F
        self._oracle = None

    def expected(self, oracle):
        """The oracle's decode of every piece, the carry chained: per piece
        (bytes out, frame list with status, carry list, frame count). Computed
        once and kept."""
        if self._oracle is None:
            from test_gpu_parity import carry_list, frames_list
            res, carry = [], None
            for piece in self.pieces:
                ob = np.frombuffer(piece, np.uint8).copy() if piece else np.zeros(0, np.uint8)
                fr, carry, n = oracle.decode_stream(ob, carry_in=carry, cap=len(piece) // 2 + 2)
                assert n == len(fr)
                res.append((ob.tobytes(), frames_list(fr, True), carry_list(carry), n))
            self._oracle = res
        return self._oracle


SPLIT_NAMES = ["lengths", "tiny_frames", "random_frames_200", "fragments", "trunc_hdr_9", "len_msb",
               "random_bytes_3000"]
# probe bytes by mode: several runs in the geometry the history selects, at
# least 8 segments of up to 128 KiB; the 1 KiB test geometry crosses 200 runs
SIZE = {"normal": 1 << 20, "small": 200000}
REGULAR_F = {264: 256, 65550: 65536}  # frame size: payload length


def regular_batch(F, n, brk=None, seed=0):
    """n frames of F bytes; frame `brk` (if any) is 44 bytes longer, the frames
    after it F bytes again (off the lattice from there on)."""
    rng = streams.SplitMix(0x4E6 + F + seed)
    return b"".join(quick_frame(rng, 0x82, REGULAR_F[F] + (44 if k == brk else 0)) for k in range(n))


def lattice_fakes(pfs, size):
    """A first frame of another size, then frames of `pfs` bytes whose stream
    holds a valid header of a pfs-byte frame exactly on every X0 + k * pfs
    (X0 = 0, the batch's first frame): with the history's pfs, every run's
    lattice entry (find_entry) is plausible and wrong."""
    rng = streams.SplitMix(0xFA4E + pfs)
    plen = pfs - 6 if pfs <= 131 else pfs - 8
    out = bytearray(quick_frame(rng, 0x82, plen + 44))
    while len(out) < size:
        out += quick_frame(rng, 0x82, plen)
    fake = streams.header(0x82, plen, rng.bytes(4))
    assert len(fake) + plen == pfs
    for o in range(pfs, len(out) - len(fake), pfs):
        out[o:o + len(fake)] = fake
    return bytes(out)


_FIXED = []


def _fixed_probes():
    """The probes that are the same in every mode: every edge case whole, and
    the split-with-carry cases cut at golden split points (six of each case's
    list, spread over it: the first two, the quartiles, the last; the full
    lists run in test_stream_split_with_carry)."""
    if _FIXED:
        return _FIXED
    from conftest import load_golden
    case = {}
    for i, name in enumerate(streams.EDGE_CASES):
        case[name] = streams.case_bytes(name)
        _FIXED.append(Probe(name, [case[name]], offset=(0, 5)[i % 2]))
    golden = load_golden("streams.json")["cases"]
    for name in SPLIT_NAMES:
        src, ks = case[name], [s["k"] for s in golden[name]["splits"]]
        for j in sorted({0, 1, len(ks) // 4, len(ks) // 2, 3 * len(ks) // 4, len(ks) - 1}):
            _FIXED.append(Probe(f"{name}@{ks[j]}", [src[:ks[j]], src[ks[j]:]], kind="split"))
    return _FIXED


def _probes(mode):
    size = SIZE[mode]
    out = list(_fixed_probes())
    for F in REGULAR_F:
        n = max(size // F, 5)
        out.append(Probe(f"regular_{F}", [regular_batch(F, n)], kind="regular", F=F))
        # (lattice points 1 and 2 are checked by the prologue: frame 3 is the
        # earliest break that reaches the segment loops)
        for brk in sorted({3, 4, n // 2, n - 1} - {0, 1, 2}):
            for off in (0, 3):
                out.append(Probe(f"break_{F}_at_{brk}_off{off}", [regular_batch(F, n, brk, seed=brk)], offset=off,
                                 kind="break3" if brk == 3 else "break", F=F))
    for pfs in (264, 127):
        out.append(Probe(f"lattice_fakes_{pfs}", [lattice_fakes(pfs, size)], kind="fakes", F=pfs))
    for kind in ADVERSARIAL_KINDS:
        src = adversarial_stream(kind, size)[:size + 4096]   # (a run of frames may overshoot by 200 KiB)
        out.append(Probe(kind, [src], kind="adversarial"))
        out.append(Probe(kind + "_cut", [src[:len(src) - 5]], offset=3, kind="adversarial"))
    for fake in (0, 1, 2):
        out.append(Probe(f"header_like_{fake}", [header_like_dense(fake, size)], kind="adversarial"))
    assert all(len(x.pieces[0]) <= (1 << 20) + 8192 for x in out if x.kind not in ("edge", "split"))
    return out


_PROBES = {}


def probes(mode):
    """The probes of a mode ("normal": no options; "small": XYWS_OPT_SMALL_SEG),
    built once per process (and their oracle decodes kept with them)."""
    if mode not in _PROBES:
        _PROBES[mode] = _probes(mode)
    return _PROBES[mode]

"""The ranges the exact tests of xyws_unmask / xyws_mask_bytes run at
(tests/test_gpu_unmask.py on the device, tests/test_oracle.py for the expected
values), derived from k_unmask_range's own geometry
(xyws_debug_unmask_geometry), not from constants copied here.

T: bytes per tile. G: the most workgroups a launch has (CU count x workgroups
per CU). A range of more than G tiles makes some workgroup walk a chain of
two tiles (the prefetch and the re-claim), more than 2G tiles a chain of
three. A range is placed by its start's misalignment m within a 16-byte line
and ends `tail` bytes past the K-th tile boundary counted from that line's
start (the kernel's tiles start there): n = K T + tail - m bytes.
"""
import ctypes as C

import numpy as np

import streams

SEED = 0x756E6D61736B
PHASES = (0, 1, 2, 3, 5, (1 << 33) + 3)
MI355X_CUS = 256  # (where no device is present: the expected values are checked at that device's sizes)


def geometry():
    """(tile bytes, threads per workgroup, workgroups per CU, scratch slots)."""
    from xynet_amd import _lib
    out = (C.c_uint64 * 4)()
    assert _lib.load().xyws_debug_unmask_geometry(out) == 0
    return tuple(int(x) for x in out)


def cu_count():
    try:
        import torch
        if torch.cuda.is_available():
            return torch.cuda.get_device_properties(0).multi_processor_count
    except ImportError:
        pass
    return MI355X_CUS


def tiles_and_grid():
    """(T, G) on this machine's device."""
    T, _, wpc, _ = geometry()
    return T, cu_count() * wpc


def source(n, seed=SEED):
    """streams.SplitMix(seed).bytes(n) as a uint8 array (the same generator
    vectorized: tens of MiB; no period, so a tile stored from another tile's
    loads differs from the expected bytes)."""
    words = (n + 7) // 8
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.arange(1, words + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    out = z.astype("<u8").view(np.uint8)[:n]
    k = min(n, 4096)
    assert out[:k].tobytes() == streams.SplitMix(seed).bytes(k)
    return out


def key_of(i):
    """Case i's key: four distinct bytes, so every wrong rotation shows."""
    rng = streams.SplitMix(SEED + 1 + i)
    while True:
        key = rng.next() & 0xFFFFFFFF
        if len(set(key.to_bytes(4, "little"))) == 4:
            return key


class Case:
    def __init__(self, i, K, m, tail, T, phase=None):
        self.K, self.m, self.tail = K, m, tail
        self.n = K * T + tail - m
        self.phase = PHASES[i % len(PHASES)] if phase is None else phase
        self.key = key_of(i)

    def __repr__(self):
        return f"Case(K={self.K}, m={self.m}, tail={self.tail}, n={self.n}, phase={self.phase}, key={self.key:#010x})"


def long_cases(T, G):
    """Every (K, m, tail) of the long ranges, the phases in rotation."""
    out = []
    for K in (G + 1, 2 * G + 3):
        for m in (0, 1, 15):
            for tail in (0, 1, 17, T - 1):
                out.append(Case(len(out), K, m, tail, T))
    assert {(c.m + c.phase) % 4 for c in out} == {0, 1, 2, 3}
    return out


def pick(cases, K, m, tail):
    (c,) = [c for c in cases if (c.K, c.m, c.tail) == (K, m, tail)]
    return c


def short_cases(T, G):
    """The short ranges by name: (n, phase, key). slot, slot2: the 64-byte calls
    that bind the scratch slots and come back to them; one, tile1: between two
    long calls on one stream; the last three: xyws_mask_bytes' sizes (the
    third grows the host stage past its floor to a run of more tiles than
    workgroups)."""
    sizes = {"slot": (64, 2), "slot2": (64, 3), "one": (1, 3), "tile1": (T + 1, 1),
             "below": (T - 1, 1), "above": (T + 1, 6), "stage": (G * T + T + 5, (1 << 33) + 3)}
    return {name: (n, phase, key_of(100 + k)) for k, (name, (n, phase)) in enumerate(sizes.items())}


def all_ranges(T, G):
    """Every distinct (n, phase, key) of both tables."""
    seen = {(c.n, c.phase, c.key) for c in long_cases(T, G)}
    seen |= set(short_cases(T, G).values())
    return sorted(seen)


def plain_mask(data, key, phase):
    """data[j] ^ key_le[(phase + j) % 4] for every j, as a new array. The
    index has period 4 in j: it is computed for one block of j and serves
    every block (a block is a multiple of 4 long)."""
    key_le = np.frombuffer(int(key).to_bytes(4, "little"), np.uint8)
    B = 1 << 20
    j = np.arange(B, dtype=np.uint64)
    pat = key_le[(np.uint64(phase) + j) % np.uint64(4)]
    out = data.copy()
    for o in range(0, out.size, B):
        out[o:o + B] ^= pat[:min(B, out.size - o)]
    return out

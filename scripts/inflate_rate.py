"""What inflating a sweep's permessage-deflate messages costs (profiles/inflate_rate.jsonl).

Every connection sends one compressed text message (zlib level 6, raw DEFLATE,
no context takeover, RSV1 on its one masked frame). Cells: 1 024 and 16 384
connections with chat-sized messages of 200-1 000 inflated bytes, and 1 024
connections with 16 KiB messages. Measured per cell:
  (a) inflate_call: xyws_inflate_streams alone on the tables one reassembly wrote;
  (b) sweep_with: recv restore (one device copy, the decode unmasks in place),
      decode, reassemble, inflate;
  (c) sweep_without: the same without the inflate call (the messages stay compressed);
  (d) host_path: what a caller did instead: sweep_without, D2H of the result
      rows, the records and the message slab, zlib on one core for every
      message, H2D of the inflated slab.
The broadcast is not part of the timed sweeps: it runs over the same view
either way. Before anything is timed every connection's inflated bytes are
compared with the host's. The variants are alternated in one process after a
warm-up, each timed by device events around a loop that ends in a synchronise
(the events span the host path's host work too); every cell is repeated and
reports median and range.

--takeover appends rows of another kind to the same file, in the same cells:
every connection's client keeps its context (one zlib.compressobj(6, DEFLATED,
-15) per connection, Z_SYNC_FLUSH, tail stripped) over ROUNDS messages. The
first ROUNDS - 1 build the history on the device; on the last one
xyws_inflate_windows_streams is timed against xyws_inflate_streams over the
same texts compressed one by one, alternated, each call preceded by a copy
that puts its carries back (so every pass inflates the same message against the
same history; in the 16 KiB cell, where the ring is full, a pass overwrites the
oldest 16 KiB it started from, so later passes do the same work over other
bytes: the outputs are compared after the first). The rows also say what a message weighs compressed either way.

usage: inflate_rate.py [--out FILE] [--repeats R] [--takeover]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]
import streams  # noqa: E402
from xynet_amd import _lib, websocket as ws  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflate_rate.jsonl"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--takeover", action="store_true")
args = ap.parse_args()
assert args.repeats >= 5, "the spread needs at least 5 repeats"
assert torch.cuda.is_available(), "inflate_rate.py measures on the GPU: no device, no number"

ctx = ws.Context(0)
L = ctx.L
sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
CAP = MCAP = 2
WORDS = ("the quick brown fox jumps over a lazy dog while we talk about rooms messages sweeps and frames "
         "hello thanks ok sure see you later what time is it there today").split()


def vp(t):
    return C.c_void_p(t.data_ptr())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def zeros(nbytes):
    return torch.zeros(nbytes, dtype=torch.uint8, device="cuda")


def timed(fn, loops):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(loops):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / loops  # us per pass


def summary(v):
    return {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def chat(rng, length):
    out = []
    while sum(len(w) + 1 for w in out) < length:
        out.append(WORDS[rng.next() % len(WORDS)] + ("%d" % (rng.next() % 97) if rng.next() % 5 == 0 else ""))
    return " ".join(out).encode()[:length]


CELLS = ((1024, 200, 1000), (16384, 200, 1000), (1024, 16384, 16384))
ROUNDS = 4


class Side:
    """One variant's sweep tables for n connections: load(payloads) puts a round's frames into the recv image, front()
    decodes and reassembles them, call() inflates them with `fn` over rows with `flags` (and windows)."""

    def __init__(self, n, stride, ocap, fn, flags, windows):
        self.n, self.stride, self.fn = n, stride, fn
        idx = np.arange(n, dtype=np.uint64)
        self.stage, self.recv = zeros(n * stride), zeros(n * stride)
        self.frames, self.counts = zeros(n * CAP * 32), torch.zeros(n, dtype=torch.int64, device="cuda")
        self.dcar, self.mcar, self.icar = zeros(64 * n), zeros(64 * n), zeros(32 * n)
        self.recs, self.vrecs, self.mout, self.iout = zeros(n * MCAP * 40), zeros(n * MCAP * 40), zeros(n * stride), zeros(n * ocap)
        self.mres, self.ires, self.view, self.vres = zeros(32 * n), zeros(32 * n), zeros(64 * n), zeros(32 * n)
        self.win = zeros(n * 32768 if windows else 16)
        self.tab = np.zeros((n, 8), np.uint64)
        self.tab[:, 0], self.tab[:, 2] = self.recv.data_ptr() + stride * idx, self.dcar.data_ptr() + 64 * idx
        self.tab[:, 3], self.tab[:, 4] = self.frames.data_ptr() + 32 * CAP * idx, CAP
        mtab, itab = np.zeros((n, 8), np.uint64), np.zeros((n, 8), np.uint64)
        mtab[:, 0], mtab[:, 1], mtab[:, 2] = self.mout.data_ptr() + stride * idx, stride, self.mcar.data_ptr() + 64 * idx
        mtab[:, 3], mtab[:, 4] = self.recs.data_ptr() + 40 * MCAP * idx, MCAP
        itab[:, 0], itab[:, 1], itab[:, 2], itab[:, 3] = self.iout.data_ptr() + ocap * idx, ocap, self.vrecs.data_ptr() + 40 * MCAP * idx, MCAP
        itab[:, 4], itab[:, 5] = self.icar.data_ptr() + 32 * idx, flags
        if windows:
            itab[:, 6] = self.win.data_ptr() + 32768 * idx
        self.mtab_t, self.itab_t, self.tab_t = dev(mtab), dev(itab), zeros(64 * n)
        self.kept = zeros(32 * n)  # the carries every timed pass starts from

    def load(self, payloads, rng):
        img = np.zeros(self.n * self.stride, np.uint8)
        for i, z in enumerate(payloads):
            key = rng.bytes(4)
            w = streams.header(0xC1, len(z), key) + (np.frombuffer(z, np.uint8) ^ np.resize(np.frombuffer(key, np.uint8), len(z))).tobytes()
            img[self.stride * i:self.stride * i + len(w)], self.tab[i, 1] = np.frombuffer(w, np.uint8), len(w)
        self.stage.copy_(dev(img))
        self.tab_t.copy_(dev(self.tab))

    def front(self):
        self.recv.copy_(self.stage, non_blocking=True)
        _lib.check(L.xyws_decode_streams(ctx.h, vp(self.tab_t), self.n, vp(self.counts), 0, sp))
        _lib.check(L.xyws_reassemble_streams(ctx.h, vp(self.tab_t), vp(self.counts), vp(self.mtab_t), self.n, _lib.REASM_UTF8,
                                             vp(self.mres), sp))

    def call(self):
        self.icar.copy_(self.kept, non_blocking=True)
        _lib.check(getattr(L, self.fn)(ctx.h, vp(self.tab_t), vp(self.mtab_t), vp(self.mres), None, vp(self.itab_t), self.n,
                                       _lib.INF_UTF8, vp(self.view), vp(self.vres), vp(self.ires), sp))


if args.takeover:
    out_rows = []
    for n, lo, hi in CELLS:
        rng = streams.SplitMix(0x7A4E + n + hi)
        texts = [[chat(rng, lo + rng.next() % (hi - lo + 1)) for _ in range(n)] for _ in range(ROUNDS)]
        clients = [zlib.compressobj(6, zlib.DEFLATED, -15) for _ in range(n)]
        kept = [[(c.compress(m) + c.flush(zlib.Z_SYNC_FLUSH))[:-4] for c, m in zip(clients, texts[r])] for r in range(ROUNDS)]
        alone = []
        for m in texts[-1]:
            c = zlib.compressobj(6, zlib.DEFLATED, -15)
            alone.append((c.compress(m) + c.flush(zlib.Z_SYNC_FLUSH))[:-4])
        stride = (max(len(z) for r in kept + [alone] for z in r) + 14 + 15) // 16 * 16
        ocap = (hi + 15) // 16 * 16
        win = Side(n, stride, ocap, "xyws_inflate_windows_streams", _lib.INFC_NEGOTIATED | _lib.INFC_TAKEOVER, True)
        one = Side(n, stride, ocap, "xyws_inflate_streams", _lib.INFC_NEGOTIATED, False)
        for r in range(ROUNDS):  # the history, round by round; the last round's tables stay
            win.load(kept[r], rng)
            win.front()
            win.call()
            if r < ROUNDS - 1:  # (call() starts from `kept`: the carries behind the round before)
                win.kept.copy_(win.icar)
        one.load(alone, rng)
        one.front()
        one.call()
        torch.cuda.synchronize()
        for side in (win, one):  # checks, before anything is timed
            res = side.ires.view(torch.int32).reshape(n, 8).cpu().numpy()
            assert (res[:, 2] == 1).all() and (res[:, 3] == 0).all() and (res[:, 4] == 0).all(), "every message inflated, none bad"
            got = side.iout.cpu().numpy().reshape(n, ocap)
            for i, m in enumerate(texts[-1]):
                assert got[i, :len(m)].tobytes() == m, i
        reached = int(win.ires.view(torch.int32).reshape(n, 8)[:, 5].sum().item())
        modes = {"windows_call": win.call, "plain_call": one.call}
        for fn in modes.values():
            fn()
            fn()
        torch.cuda.synchronize()
        t = {name: [] for name in modes}
        for _ in range(args.repeats):
            for name, fn in modes.items():  # (alternated)
                t[name].append(timed(fn, 20))
        row = {"mode": "takeover", "connections": n, "inflated_bytes_min": lo, "inflated_bytes_max": hi, "rounds": ROUNDS,
               "level": 6, "repeats": args.repeats, "loops": 20, "messages_reaching_history": reached,
               "inflated_bytes_per_message": round(sum(map(len, texts[-1])) / n, 1),
               "compressed_bytes_per_message_takeover": round(sum(map(len, kept[-1])) / n, 1),
               "compressed_bytes_per_message_alone": round(sum(map(len, alone)) / n, 1)}
        for name in modes:
            row[name] = summary(t[name])
        row["windows_over_plain"] = round(row["windows_call"]["median_us"] / row["plain_call"]["median_us"], 3)
        out_rows.append(row)
        print(json.dumps(row), flush=True)
    assert ctx.last_device_error() == 0
    with open(args.out, "a") as f:
        for row in out_rows:
            f.write(json.dumps(row) + "\n")
    sys.exit(0)

rows = []
for n, lo, hi in CELLS:
    rng = streams.SplitMix(0x1F7A + n + hi)
    msgs = [chat(rng, lo + rng.next() % (hi - lo + 1)) for _ in range(n)]
    comp = []
    for m in msgs:
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        comp.append((c.compress(m) + c.flush(zlib.Z_SYNC_FLUSH))[:-4])
    wire = []
    for z in comp:
        key = rng.bytes(4)
        body = np.frombuffer(z, np.uint8) ^ np.resize(np.frombuffer(key, np.uint8), len(z))
        wire.append(streams.header(0xC1, len(z), key) + body.tobytes())
    stride = (max(len(w) for w in wire) + 15) // 16 * 16
    ocap = (hi + 15) // 16 * 16
    img = np.zeros(n * stride, np.uint8)
    for i, w in enumerate(wire):
        img[stride * i:stride * i + len(w)] = np.frombuffer(w, np.uint8)
    stage, recv = dev(img), zeros(n * stride)
    idx = np.arange(n, dtype=np.uint64)
    frames, counts = zeros(n * CAP * 32), torch.zeros(n, dtype=torch.int64, device="cuda")
    dcar, mcar, icar = zeros(64 * n), zeros(64 * n), zeros(32 * n)
    recs, vrecs, mout, iout = zeros(n * MCAP * 40), zeros(n * MCAP * 40), zeros(n * stride), zeros(n * ocap)
    mres, ires, view, vres = zeros(32 * n), zeros(32 * n), zeros(64 * n), zeros(32 * n)
    tab = np.zeros((n, 8), np.uint64)
    tab[:, 0], tab[:, 1], tab[:, 2] = recv.data_ptr() + stride * idx, [len(w) for w in wire], dcar.data_ptr() + 64 * idx
    tab[:, 3], tab[:, 4] = frames.data_ptr() + 32 * CAP * idx, CAP
    mtab = np.zeros((n, 8), np.uint64)
    mtab[:, 0], mtab[:, 1], mtab[:, 2] = mout.data_ptr() + stride * idx, stride, mcar.data_ptr() + 64 * idx
    mtab[:, 3], mtab[:, 4] = recs.data_ptr() + 40 * MCAP * idx, MCAP
    itab = np.zeros((n, 8), np.uint64)
    itab[:, 0], itab[:, 1], itab[:, 2], itab[:, 3] = iout.data_ptr() + ocap * idx, ocap, vrecs.data_ptr() + 40 * MCAP * idx, MCAP
    itab[:, 4], itab[:, 5] = icar.data_ptr() + 32 * idx, _lib.INFC_NEGOTIATED
    tab_t, mtab_t, itab_t = dev(tab), dev(mtab), dev(itab)

    def front():
        recv.copy_(stage, non_blocking=True)
        _lib.check(L.xyws_decode_streams(ctx.h, vp(tab_t), n, vp(counts), 0, sp))
        _lib.check(L.xyws_reassemble_streams(ctx.h, vp(tab_t), vp(counts), vp(mtab_t), n, _lib.REASM_UTF8, vp(mres), sp))

    def inflate_call():
        _lib.check(L.xyws_inflate_streams(ctx.h, vp(tab_t), vp(mtab_t), vp(mres), None, vp(itab_t), n, _lib.INF_UTF8,
                                          vp(view), vp(vres), vp(ires), sp))

    def sweep_with():
        front()
        inflate_call()

    h_rows = torch.zeros(32 * n, dtype=torch.uint8).pin_memory()
    h_recs = torch.zeros(40 * MCAP * n, dtype=torch.uint8).pin_memory()
    h_out = torch.zeros(n * stride, dtype=torch.uint8).pin_memory()
    h_inf = torch.zeros(n * ocap, dtype=torch.uint8).pin_memory()
    hostdev = zeros(n * ocap)

    def host_path():
        front()
        h_rows.copy_(mres, non_blocking=True)
        h_recs.copy_(recs, non_blocking=True)
        h_out.copy_(mout, non_blocking=True)
        torch.cuda.synchronize()
        rec = h_recs.numpy().view(np.uint64).reshape(n, MCAP, 5)
        src, dst = h_out.numpy(), h_inf.numpy()
        for i in range(n):
            off, ln = int(rec[i, 0, 2]), int(rec[i, 0, 3])
            m = zlib.decompressobj(-15).decompress(src[stride * i + off:stride * i + off + ln].tobytes() + b"\x00\x00\xff\xff")
            dst[ocap * i:ocap * i + len(m)] = np.frombuffer(m, np.uint8)
        hostdev.copy_(h_inf, non_blocking=True)

    # ---- checks, before anything is timed
    sweep_with()
    host_path()
    torch.cuda.synchronize()
    res = ires.view(torch.int32).reshape(n, 8).cpu().numpy()
    assert (res[:, 2] == 1).all() and (res[:, 3] == 0).all() and (res[:, 4] == 0).all(), "every message inflated, none bad"
    got, want = iout.cpu().numpy().reshape(n, ocap), hostdev.cpu().numpy().reshape(n, ocap)
    for i in range(n):
        assert got[i, :len(msgs[i])].tobytes() == msgs[i] == want[i, :len(msgs[i])].tobytes(), i
    modes = {"inflate_call": inflate_call, "sweep_with": sweep_with, "sweep_without": front, "host_path": host_path}
    for fn in modes.values():
        fn()
        fn()
    torch.cuda.synchronize()
    loops = {"inflate_call": 20, "sweep_with": 20, "sweep_without": 50, "host_path": 3}
    t = {name: [] for name in modes}
    for _ in range(args.repeats):
        for name, fn in modes.items():  # (alternated: each repeat times every variant)
            t[name].append(timed(fn, loops[name]))
    row = {"connections": n, "inflated_bytes_min": lo, "inflated_bytes_max": hi, "inflated_bytes": sum(map(len, msgs)),
           "compressed_bytes": sum(map(len, comp)), "level": 6, "repeats": args.repeats, "loops": loops}
    for name in modes:
        row[name] = summary(t[name])
    row["inflate_ns_per_connection"] = round(1e3 * row["inflate_call"]["median_us"] / n, 1)
    row["inflate_MBps_out"] = round(row["inflated_bytes"] / row["inflate_call"]["median_us"], 1)
    row["host_over_sweep_with"] = round(row["host_path"]["median_us"] / row["sweep_with"]["median_us"], 2)
    row["sweep_beats_host_beyond_spread"] = row["sweep_with"]["max_us"] < row["host_path"]["min_us"]
    rows.append(row)
    print(json.dumps(row), flush=True)

assert ctx.last_device_error() == 0
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")

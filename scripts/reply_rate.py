"""Answering one sweep of N connections, two ways (profiles/reply_rate.jsonl).

For N in {1, 64, 1024, 16384} connections x {256 B, 4 KiB} per connection of
mixed masked frames (payloads drawn from 0-1000 B and clipped to the room left,
so that every connection's buffer ends at a frame boundary and both ways do the
same work; no close in the data), decoded once by xyws_decode_streams (not
timed), the time of
  (a) one xyws_reply_streams call;
  (b) the loop of xyws_classify_frames + xyws_encode_frames per connection on
      one stream: what a caller did before xyws_reply_streams existed.
Both echo every data frame as FIN | TEXT into the same send slab layout
(len + 13 bytes per connection); their reply bytes are compared once before
anything is timed. The two are alternated in one process after a warm-up, each
timed by device events around a loop that ends in a synchronise; every cell is
repeated and reports median and range.

usage: reply_rate.py [--out FILE] [--repeats R] [--n N,N,...] [--bytes B,B,...]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]
import streams  # noqa: E402
from xynet_amd import _lib, websocket as ws  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reply_rate.jsonl"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--n", default="1,64,1024,16384")
ap.add_argument("--bytes", default="256,4096")
args = ap.parse_args()
assert args.repeats >= 5, "the spread needs at least 5 repeats"
assert torch.cuda.is_available(), "reply_rate.py measures on the GPU: no device, no number"

MAX_PAYLOAD, FLAGS, AMASK = 1 << 20, 0x11, 1 << _lib.ACT_DATA
ctx = ws.Context(0)
L = ctx.L
stream = torch.cuda.current_stream()
sp = C.c_void_p(stream.cuda_stream)


def vp(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


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


def frame_size(plen):
    return (6 if plen < 126 else 8) + plen


def connection(rng, per):
    """Whole masked frames filling exactly `per` bytes; returns (bytes, frames).
    A frame is 6..131 or at least 134 bytes, so the last frame takes the room
    left whenever a drawn frame would leave less than the shortest frame."""
    out, nf = bytearray(), 0
    while len(out) < per:
        room = per - len(out)
        plen = rng.next() % 1001
        if room in (132, 133):
            plen = 0  # (no single frame has this size)
        elif frame_size(plen) + 6 > room:
            plen = room - 6 if room - 6 < 126 else room - 8
        out += streams.header(0x81 if nf & 1 else 0x82, plen, rng.bytes(4)) + rng.bytes(plen)
        nf += 1
    return bytes(out), nf


rows = []
for per in [int(x) for x in args.bytes.split(",")]:
    rng = streams.SplitMix(0x4E91 + per)
    pool = [connection(rng, per) for _ in range(64)]  # 64 different connections, repeated
    assert all(len(b) == per for b, _ in pool), [len(b) for b, _ in pool]
    cap = max(nf for _, nf in pool) + 1
    ocap = per + 13
    for n in [int(x) for x in args.n.split(",")]:
        total = n * per
        host = np.frombuffer(b"".join(pool[i % 64][0] for i in range(min(n, 64))), np.uint8)
        slab = torch.from_numpy(host.copy()).cuda().repeat((n + 63) // 64)[:total].clone()
        frames = torch.empty(n * cap * 32, dtype=torch.uint8, device="cuda")
        counts = torch.zeros(n, dtype=torch.int64, device="cuda")
        verd = torch.zeros(n * cap * 8, dtype=torch.uint8, device="cuda")
        out_a = torch.zeros(n * ocap, dtype=torch.uint8, device="cuda")
        out_b = torch.zeros(n * ocap, dtype=torch.uint8, device="cuda")
        rcs = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
        results = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
        lens_b = torch.zeros(n, dtype=torch.int64, device="cuda")
        idx = np.arange(n, dtype=np.uint64)
        tab = np.zeros((n, 8), np.uint64)
        tab[:, 0] = slab.data_ptr() + per * idx
        tab[:, 1] = per
        tab[:, 3] = frames.data_ptr() + 32 * cap * idx
        tab[:, 4] = cap
        table = torch.from_numpy(tab.view(np.int64).reshape(-1)).cuda()
        rtab = np.zeros((n, 4), np.uint64)
        rtab[:, 0] = out_a.data_ptr() + ocap * idx
        rtab[:, 1] = ocap
        rtab[:, 2] = rcs.data_ptr() + 32 * idx
        rtab[:, 3] = verd.data_ptr() + 8 * cap * idx
        rtable = torch.from_numpy(rtab.view(np.int64).reshape(-1)).cuda()
        # decoded once (fresh carries: every buffer is whole frames), not timed
        _lib.check(L.xyws_decode_streams(ctx.h, vp(table), n, vp(counts), 0, sp))
        torch.cuda.synchronize()
        nframes = int(counts.sum().item())
        assert nframes == sum(pool[i % 64][1] for i in range(n)) and int(counts.max().item()) < cap

        def one_call():
            _lib.check(L.xyws_reply_streams(ctx.h, vp(table), vp(counts), vp(rtable), n, MAX_PAYLOAD, 0, FLAGS, 0, AMASK,
                                            vp(results), sp))

        def loop_of_calls():
            for i in range(n):
                _lib.check(L.xyws_classify_frames(ctx.h, vp(slab, i * per), per, vp(frames, 32 * cap * i), cap,
                                                  vp(counts, 8 * i), MAX_PAYLOAD, 0, vp(verd, 8 * cap * i), None, sp))
                _lib.check(L.xyws_encode_frames(ctx.h, vp(slab, i * per), per, vp(frames, 32 * cap * i), cap,
                                                vp(counts, 8 * i), FLAGS, 0, None, vp(verd, 8 * cap * i), AMASK,
                                                vp(out_b, ocap * i), ocap, None, vp(lens_b, 8 * i), sp))

        modes = {"reply_call": one_call, "loop_of_calls": loop_of_calls}
        for name, fn in modes.items():
            for _ in range(3):  # (warm-up: code objects, scratch)
                fn()
            torch.cuda.synchronize()
        # the same replies, whichever way
        lens_a = results.view(torch.int64).reshape(n, 4)[:, 0]
        assert torch.equal(lens_a, lens_b) and not bool(results.view(torch.int16).reshape(n, 16)[:, 11].any())
        assert torch.equal(out_a, out_b)
        loops = {"reply_call": 200, "loop_of_calls": max(1, min(200, 2000 // n))}
        t = {name: [] for name in modes}
        for _ in range(args.repeats):
            for name, fn in modes.items():  # (alternated: each repeat times both)
                t[name].append(timed(fn, loops[name]))
        row = {"connections": n, "bytes_per_connection": per, "total_bytes": total, "frames": nframes,
               "reply_bytes": int(lens_a.sum().item()), "repeats": args.repeats, "loops": loops}
        for name in modes:
            row[name] = summary(t[name])
        row["reply_call_beats_loop_beyond_spread"] = row["reply_call"]["max_us"] < row["loop_of_calls"]["min_us"]
        row["loop_over_reply_call"] = round(row["loop_of_calls"]["median_us"] / row["reply_call"]["median_us"], 2)
        row["reply_call_GBps"] = round((total + row["reply_bytes"]) / row["reply_call"]["median_us"] / 1e3, 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del slab, frames, counts, verd, out_a, out_b, rcs, results, lens_b, table, rtable
        torch.cuda.empty_cache()

assert ctx.last_device_error() == 0
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")

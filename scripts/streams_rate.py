"""One sweep of N connections, three ways (profiles/streams_rate.jsonl).

For N in {1, 64, 1024, 16384} connections x {256 B, 4 KiB, 64 KiB} per
connection of mixed 0-1000 B masked frames, descriptors on, the time of
  (a) one xyws_decode_streams call (the N carries copied into place first);
  (b) the loop of N xyws_decode_stream calls on one stream: the baseline;
  (c) one xyws_decode_stream of the concatenation: the bandwidth-side ideal.
The connections are consecutive ranges of one continuous stream, so (c) sees
the same frames; each connection's carry-in is the state at its cut (made once
by a chained loop of decodes, not timed), and every timed pass starts from
those same carries. The three are alternated in one process after a warm-up,
each timed by device events around a loop that ends in a synchronise; every
cell is repeated and reports median and range.

usage: streams_rate.py [--out FILE] [--repeats R] [--n N,N,...] [--bytes B,B,...]
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "streams_rate.jsonl"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--n", default="1,64,1024,16384")
ap.add_argument("--bytes", default="256,4096,65536")
args = ap.parse_args()
assert args.repeats >= 5, "the spread needs at least 5 repeats"
assert torch.cuda.is_available(), "streams_rate.py measures on the GPU: no device, no number"

# a pool of whole frames; a slab is the pool repeated (still whole frames back to back)
rng = streams.SplitMix(0x5EE9)
pool, starts = bytearray(), []
while len(pool) < (4 << 20):
    starts.append(len(pool))
    plen = rng.next() % 1001
    pool += streams.header(0x81, plen, rng.bytes(4)) + rng.bytes(plen)  # (any bytes are some masked payload)
P = len(pool)
pool_t = torch.frombuffer(pool, dtype=torch.uint8).cuda()
S2 = np.concatenate([np.array(starts), np.array(starts) + P, [2 * P]])

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


rows = []
for per in [int(x) for x in args.bytes.split(",")]:
    # descriptors for the most frames any range of `per` bytes of the stream holds
    cap = int((np.searchsorted(S2, S2[:len(starts)] + per) - np.arange(len(starts))).max()) + 2
    for n in [int(x) for x in args.n.split(",")]:
        total = n * per
        slab = pool_t.repeat((total + P - 1) // P)[:total].clone()
        frames = torch.empty(n * cap * 32, dtype=torch.uint8, device="cuda")
        counts = torch.zeros(n, dtype=torch.int64, device="cuda")
        cin = torch.zeros((n + 1) * 64, dtype=torch.uint8, device="cuda")
        work = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
        # the state at every cut: connection i decoded from cin[i] into cin[i + 1]
        for i in range(n):
            _lib.check(L.xyws_decode_stream(ctx.h, vp(slab, i * per), per, vp(cin, 64 * i), vp(cin, 64 * i + 64),
                                            None, 0, None, 0, sp))
        tab = np.zeros((n, 8), np.uint64)
        tab[:, 0] = slab.data_ptr() + per * np.arange(n, dtype=np.uint64)
        tab[:, 1] = per
        tab[:, 2] = work.data_ptr() + 64 * np.arange(n, dtype=np.uint64)
        tab[:, 3] = frames.data_ptr() + 32 * cap * np.arange(n, dtype=np.uint64)
        tab[:, 4] = cap
        table = torch.from_numpy(tab.view(np.int64).reshape(-1)).cuda()

        def one_call():
            work.copy_(cin[:n * 64])
            _lib.check(L.xyws_decode_streams(ctx.h, vp(table), n, vp(counts), 0, sp))

        def loop_of_calls():
            for i in range(n):
                _lib.check(L.xyws_decode_stream(ctx.h, vp(slab, i * per), per, vp(cin, 64 * i), vp(work, 64 * i),
                                                vp(frames, 32 * cap * i), cap, vp(counts, 8 * i), 0, sp))

        def concatenation():
            _lib.check(L.xyws_decode_stream(ctx.h, vp(slab), total, vp(cin), vp(work), vp(frames), n * cap,
                                            vp(counts), 0, sp))

        modes = {"streams_call": one_call, "loop_of_calls": loop_of_calls, "concatenation": concatenation}
        # the frames the three find (the same, whichever way)
        found = {}
        for name, fn in modes.items():
            for _ in range(3):  # (warm-up: code objects, scratch, the stream's decoder choice)
                fn()
            torch.cuda.synchronize()
            found[name] = int(counts[:1 if name == "concatenation" else n].sum().item())
        assert len(set(found.values())) == 1, found
        loops = {name: max(1, min(200, int(200000 // (60 * (n if name == "loop_of_calls" else 1)))))
                 for name in modes}
        t = {name: [] for name in modes}
        for _ in range(args.repeats):
            for name, fn in modes.items():  # (alternated: each repeat times all three)
                t[name].append(timed(fn, loops[name]))
        row = {"connections": n, "bytes_per_connection": per, "total_bytes": total, "frames": found["streams_call"],
               "cap_per_connection": cap, "repeats": args.repeats, "loops": loops}
        for name in modes:
            row[name] = summary(t[name])
        row["streams_call_beats_loop_beyond_spread"] = row["streams_call"]["max_us"] < row["loop_of_calls"]["min_us"]
        row["loop_over_streams_call"] = round(row["loop_of_calls"]["median_us"] / row["streams_call"]["median_us"], 2)
        row["streams_call_GBps"] = round(total / row["streams_call"]["median_us"] / 1e3, 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del slab, frames, counts, cin, work, table
        torch.cuda.empty_cache()

assert ctx.last_device_error() == 0
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")

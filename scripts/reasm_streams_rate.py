"""Reassembling one sweep of N connections, two ways (profiles/reasm_streams_rate.jsonl).

For N in {1, 64, 1024, 16384} connections x {256 B, 4 KiB} per connection of
fragmented text messages (three masked fragments each, multi-byte UTF-8 cut by
the fragment boundaries, payloads of 5-40 bytes; a last one-frame message takes
the room left, so that every connection's buffer ends at a message boundary
and every pass does the same work), decoded once by xyws_decode_streams (not
timed), the time of
  (a) one xyws_reassemble_streams call;
  (b) the loop of xyws_reassemble_stream per connection on one stream: what a
      caller did before xyws_reassemble_streams existed.
Both validate UTF-8 and write into the same layouts (len bytes of out, cap + 1
records and a 64-byte carry per connection); their out bytes, records, counts
and carries are compared once before anything is timed. The two are alternated
in one process after a warm-up, each timed by device events around a loop that
ends in a synchronise; every cell is repeated and reports median and range.

usage: reasm_streams_rate.py [--out FILE] [--repeats R] [--n N,N,...] [--bytes B,B,...]
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reasm_streams_rate.jsonl"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--n", default="1,64,1024,16384")
ap.add_argument("--bytes", default="256,4096")
args = ap.parse_args()
assert args.repeats >= 5, "the spread needs at least 5 repeats"
assert torch.cuda.is_available(), "reasm_streams_rate.py measures on the GPU: no device, no number"

ctx = ws.Context(0)
L = ctx.L
stream = torch.cuda.current_stream()
sp = C.c_void_p(stream.cuda_stream)
UNITS = ["é".encode(), "€".encode(), "𝄞".encode(), b"a", b"bc "]


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


def text(rng, nbytes):
    """Valid UTF-8 of exactly nbytes."""
    out = bytearray()
    while len(out) < nbytes:
        u = UNITS[rng.next() % len(UNITS)]
        out += u if len(out) + len(u) <= nbytes else b"a"
    return bytes(out)


def frame(rng, b0, payload):
    key = rng.bytes(4)
    return streams.header(b0, len(payload), key) + streams.masked(payload, key)


def connection(rng, per):
    """Whole fragmented text messages filling exactly `per` bytes; returns
    (bytes, frames, messages)."""
    out, nf, nm = bytearray(), 0, 0
    while True:
        room = per - len(out)
        sizes = [5 + rng.next() % 36 for _ in range(3)]
        left = room - (18 + sum(sizes))
        if left < 6 or left in (132, 133):
            break
        body = text(rng, sum(sizes))  # (the fragments cut it anywhere, inside sequences too)
        a, b = sizes[0], sizes[0] + sizes[1]
        out += frame(rng, 0x01, body[:a]) + frame(rng, 0x00, body[a:b]) + frame(rng, 0x80, body[b:])
        nf += 3
        nm += 1
    room = per - len(out)
    out += frame(rng, 0x81, text(rng, room - 6 if room - 6 < 126 else room - 8))
    return bytes(out), nf + 1, nm + 1


rows = []
for per in [int(x) for x in args.bytes.split(",")]:
    rng = streams.SplitMix(0x4EA5 + per)
    pool = [connection(rng, per) for _ in range(64)]  # 64 different connections, repeated
    assert all(len(b) == per for b, _, _ in pool), [len(b) for b, _, _ in pool]
    cap = max(nf for _, nf, _ in pool) + 1
    mcap = cap + 1
    for n in [int(x) for x in args.n.split(",")]:
        total = n * per
        host = np.frombuffer(b"".join(pool[i % 64][0] for i in range(min(n, 64))), np.uint8)
        slab = torch.from_numpy(host.copy()).cuda().repeat((n + 63) // 64)[:total].clone()
        frames = torch.empty(n * cap * 32, dtype=torch.uint8, device="cuda")
        counts = torch.zeros(n, dtype=torch.int64, device="cuda")
        out_a, out_b = (torch.zeros(total, dtype=torch.uint8, device="cuda") for _ in range(2))
        msgs_a, msgs_b = (torch.zeros(n * mcap * 40, dtype=torch.uint8, device="cuda") for _ in range(2))
        mc_a, mc_b = (torch.zeros(n * 64, dtype=torch.uint8, device="cuda") for _ in range(2))
        results = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
        nm_b = torch.zeros(n, dtype=torch.int64, device="cuda")
        idx = np.arange(n, dtype=np.uint64)
        tab = np.zeros((n, 8), np.uint64)
        tab[:, 0] = slab.data_ptr() + per * idx
        tab[:, 1] = per
        tab[:, 3] = frames.data_ptr() + 32 * cap * idx
        tab[:, 4] = cap
        table = torch.from_numpy(tab.view(np.int64).reshape(-1)).cuda()
        mtab = np.zeros((n, 8), np.uint64)
        mtab[:, 0] = out_a.data_ptr() + per * idx
        mtab[:, 1] = per
        mtab[:, 2] = mc_a.data_ptr() + 64 * idx
        mtab[:, 3] = msgs_a.data_ptr() + 40 * mcap * idx
        mtab[:, 4] = mcap
        mtable = torch.from_numpy(mtab.view(np.int64).reshape(-1)).cuda()
        # decoded once (fresh carries: every buffer is whole frames), not timed
        _lib.check(L.xyws_decode_streams(ctx.h, vp(table), n, vp(counts), 0, sp))
        torch.cuda.synchronize()
        nframes = int(counts.sum().item())
        assert nframes == sum(pool[i % 64][1] for i in range(n)) and int(counts.max().item()) < cap

        def one_call():
            _lib.check(L.xyws_reassemble_streams(ctx.h, vp(table), vp(counts), vp(mtable), n, _lib.REASM_UTF8,
                                                 vp(results), sp))

        def loop_of_calls():
            for i in range(n):
                _lib.check(L.xyws_reassemble_stream(ctx.h, vp(slab, i * per), per, vp(frames, 32 * cap * i), cap,
                                                    vp(counts, 8 * i), _lib.REASM_UTF8, vp(mc_b, 64 * i),
                                                    vp(mc_b, 64 * i), vp(out_b, per * i), per,
                                                    vp(msgs_b, 40 * mcap * i), mcap, vp(nm_b, 8 * i), sp))

        modes = {"streams_call": one_call, "loop_of_calls": loop_of_calls}
        # the same messages, whichever way: one pass each from fresh carries
        for fn in modes.values():
            fn()
        torch.cuda.synchronize()
        res = results.view(torch.int64).reshape(n, 4)
        nmsgs = int(res[:, 1].sum().item())
        assert torch.equal(res[:, 1], nm_b) and nmsgs == sum(pool[i % 64][2] for i in range(n))
        assert not bool((res[:, 2] >> 32).any()), "no truncation, no open message, no invalid UTF-8 in this data"
        assert int((res[:, 2] & 0xFFFFFFFF).sum().item()) == nmsgs  # (every message complete)
        assert torch.equal(out_a, out_b) and torch.equal(mc_a, mc_b)
        ra, rb = msgs_a.reshape(n, mcap, 40), msgs_b.reshape(n, mcap, 40)
        keep = torch.arange(mcap, device="cuda")[None, :] < nm_b[:, None]  # (the stored records of each row)
        assert torch.equal(ra[keep], rb[keep])
        for name, fn in modes.items():
            for _ in range(2):  # (warm-up: code objects, scratch)
                fn()
            torch.cuda.synchronize()
        loops = {"streams_call": 200, "loop_of_calls": max(1, min(200, 2000 // n))}
        t = {name: [] for name in modes}
        for _ in range(args.repeats):
            for name, fn in modes.items():  # (alternated: each repeat times both)
                t[name].append(timed(fn, loops[name]))
        row = {"connections": n, "bytes_per_connection": per, "total_bytes": total, "frames": nframes,
               "messages": nmsgs, "out_bytes": int(res[:, 0].sum().item()), "repeats": args.repeats, "loops": loops}
        for name in modes:
            row[name] = summary(t[name])
        row["streams_call_beats_loop_beyond_spread"] = row["streams_call"]["max_us"] < row["loop_of_calls"]["min_us"]
        row["loop_over_streams_call"] = round(row["loop_of_calls"]["median_us"] / row["streams_call"]["median_us"], 2)
        row["streams_call_GBps"] = round((total + row["out_bytes"]) / row["streams_call"]["median_us"] / 1e3, 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del slab, frames, counts, out_a, out_b, msgs_a, msgs_b, mc_a, mc_b, results, nm_b, table, mtable
        torch.cuda.empty_cache()

assert ctx.last_device_error() == 0
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")

"""Broadcasting one sweep's messages to every room member, three ways (profiles/room_rate.jsonl).

For rooms x members in {1 x 4, 1 x 64, 1 x 1024, 16 x 64, 256 x 64, 1 x 16384}
every connection speaks once: one masked text frame of 40-200 bytes, decoded by
xyws_decode_streams and reassembled by xyws_reassemble_streams once (not timed);
every connection has a 24-byte message head and no reply (base 0). The send
ranges lie back to back in one slab, each as long as its room's wire. The time of
  (a) one xyws_broadcast_streams call: wire build and fan-out;
  (b) what a caller can write once it has a wire: the same call with every
      connection outside the rooms (the wire build and a fan-out that writes
      only rows), then one device-to-device copy per member into its range
      (torch copy_ on views sliced beforehand), all on one stream;
  (c) one device-to-device copy of as many bytes as the fan-out writes: the
      ceiling of this run.
The output slabs of (a) and (b) are compared, and room 0's wire against one
built on the host, before anything is timed. The three are alternated in one
process after a warm-up, each timed by device events around a loop that ends
in a synchronise; every cell is repeated and reports median and range. A cell
whose two slabs do not fit in free device memory is dropped and named.

usage: room_rate.py [--out FILE] [--repeats R] [--cells RxM,RxM,...]
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "room_rate.jsonl"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--cells", default="1x4,1x64,1x1024,16x64,256x64,1x16384")
args = ap.parse_args()
assert args.repeats >= 5, "the spread needs at least 5 repeats"
assert torch.cuda.is_available(), "room_rate.py measures on the GPU: no device, no number"

ctx = ws.Context(0)
L = ctx.L
stream = torch.cuda.current_stream()
sp = C.c_void_p(stream.cuda_stream)
HEAD = 24


def vp(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


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


def hdr(n):
    return bytes([0x81, n]) if n < 126 else bytes([0x81, 126]) + n.to_bytes(2, "big")


rows, dropped = [], []
for cell in args.cells.split(","):
    R, Mb = (int(x) for x in cell.split("x"))
    n = R * Mb
    rng = streams.SplitMix(0xB0CA + n + R)
    lens = [40 + rng.next() % 161 for _ in range(n)]
    msgs = [bytes(0x61 + (q + i) % 26 for q in range(ln)) for i, ln in enumerate(lens)]
    heads = [("[%021d] " % i).encode() for i in range(n)]
    assert all(len(h) == HEAD for h in heads)
    pieces = []
    for m in msgs:
        key = rng.bytes(4)
        pieces.append(streams.header(0x81, len(m), key) + streams.masked(m, key))
    plen = np.asarray([len(p) for p in pieces], np.uint64)
    poff = np.concatenate([[0], np.cumsum(plen)[:-1]]).astype(np.uint64)
    flen = np.asarray([len(hdr(HEAD + ln)) + HEAD + ln for ln in lens], np.uint64)
    wlen = flen.reshape(R, Mb).sum(axis=1)          # each room's wire
    own = np.repeat(wlen, Mb)                       # ... as long as each member's send range
    soff = np.concatenate([[0], np.cumsum(own)[:-1]]).astype(np.uint64)
    out_bytes = int(own.sum())
    free = torch.cuda.mem_get_info()[0]
    if 2 * out_bytes + (1 << 30) > free:
        dropped.append({"cell": cell, "out_bytes": out_bytes, "free_bytes": int(free)})
        print(json.dumps({"dropped": dropped[-1]}), flush=True)
        continue
    recv = dev(np.frombuffer(b"".join(pieces), np.uint8))
    head_t = dev(np.frombuffer(b"".join(heads), np.uint8))
    cap, mcap = 2, 2
    frames = torch.empty(n * cap * 32, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(n, dtype=torch.int64, device="cuda")
    mout = torch.zeros(int(plen.sum()), dtype=torch.uint8, device="cuda")
    recs = torch.zeros(n * mcap * 40, dtype=torch.uint8, device="cuda")
    mres = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    slab_a, slab_b = (torch.zeros(out_bytes, dtype=torch.uint8, device="cuda") for _ in range(2))
    wires = torch.zeros(int(wlen.sum()), dtype=torch.uint8, device="cuda")
    woff = np.concatenate([[0], np.cumsum(wlen)[:-1]]).astype(np.uint64)
    idx = np.arange(n, dtype=np.uint64)
    tab = np.zeros((n, 8), np.uint64)
    tab[:, 0], tab[:, 1] = recv.data_ptr() + poff, plen
    tab[:, 3], tab[:, 4] = frames.data_ptr() + 32 * cap * idx, cap
    mtab = np.zeros((n, 8), np.uint64)
    mtab[:, 0], mtab[:, 1] = mout.data_ptr() + poff, plen
    mtab[:, 3], mtab[:, 4] = recs.data_ptr() + 40 * mcap * idx, mcap
    btab = np.zeros((n, 8), np.uint64)
    btab[:, 0], btab[:, 1] = head_t.data_ptr() + HEAD * idx, HEAD
    btab[:, 2], btab[:, 3] = slab_a.data_ptr() + soff, own
    btab[:, 5] = idx // Mb
    btab_none = btab.copy()
    btab_none[:, 5] = _lib.ROOM_NONE
    members = dev(np.arange(n, dtype=np.uint32))
    rtab = np.zeros((R, 4), np.uint64)
    rtab[:, 0], rtab[:, 1] = members.data_ptr() + 4 * Mb * np.arange(R, dtype=np.uint64), Mb
    rtab[:, 2], rtab[:, 3] = wires.data_ptr() + woff, wlen
    table, mtable, btable, btable_none, rtable = dev(tab), dev(mtab), dev(btab), dev(btab_none), dev(rtab)
    rres = torch.zeros(R * 32, dtype=torch.uint8, device="cuda")
    bres = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    # decoded and reassembled once, not timed
    _lib.check(L.xyws_decode_streams(ctx.h, vp(table), n, vp(counts), 0, sp))
    _lib.check(L.xyws_reassemble_streams(ctx.h, vp(table), vp(counts), vp(mtable), n, _lib.REASM_UTF8, vp(mres), sp))
    torch.cuda.synchronize()
    assert int(counts.sum().item()) == n
    assert int((mres.view(torch.int64).reshape(n, 4)[:, 2] & 0xFFFFFFFF).sum().item()) == n  # (every message complete)
    pairs = [(slab_b[int(soff[i]):int(soff[i] + own[i])], wires[int(woff[i // Mb]):int(woff[i // Mb] + wlen[i // Mb])])
             for i in range(n)]

    def one_call():
        _lib.check(L.xyws_broadcast_streams(ctx.h, vp(mtable), vp(mres), vp(btable), n, vp(rtable), vp(rres), R, 0x11,
                                            0, vp(bres), sp))

    def wire_then_copies():
        _lib.check(L.xyws_broadcast_streams(ctx.h, vp(mtable), vp(mres), vp(btable_none), n, vp(rtable), vp(rres), R,
                                            0x11, 0, vp(bres), sp))
        for dst, src in pairs:
            dst.copy_(src, non_blocking=True)

    def one_copy():
        slab_a.copy_(slab_b, non_blocking=True)

    one_call()
    wire_then_copies()
    torch.cuda.synchronize()
    rr = rres.view(torch.int64).reshape(R, 4).cpu().numpy()
    assert (rr[:, 0] == wlen.astype(np.int64)).all() and (rr[:, 1] == Mb).all() and not (rr[:, 2] >> 32).any()
    want0 = b"".join(hdr(HEAD + lens[i]) + heads[i] + msgs[i] for i in range(Mb))
    assert wires[:int(wlen[0])].cpu().numpy().tobytes() == want0
    equal = bool(torch.equal(slab_a, slab_b))
    assert equal, "the call and the copies wrote different bytes"
    modes = {"broadcast_call": one_call, "wire_then_copies": wire_then_copies, "one_copy": one_copy}
    for fn in modes.values():
        fn()
        fn()
    torch.cuda.synchronize()
    la = max(2, min(200, int(2e10 // out_bytes)))
    loops = {"broadcast_call": la, "wire_then_copies": max(1, min(la, 4000 // n)), "one_copy": la}
    t = {name: [] for name in modes}
    for _ in range(args.repeats):
        for name, fn in modes.items():  # (alternated: each repeat times all three)
            t[name].append(timed(fn, loops[name]))
    row = {"rooms": R, "members": Mb, "connections": n, "wire_bytes_per_room": int(wlen[0]), "out_bytes": out_bytes,
           "outputs_equal": equal, "repeats": args.repeats, "loops": loops}
    for name in modes:
        row[name] = summary(t[name])
    row["call_beats_copies_beyond_spread"] = row["broadcast_call"]["max_us"] < row["wire_then_copies"]["min_us"]
    row["copies_over_call"] = round(row["wire_then_copies"]["median_us"] / row["broadcast_call"]["median_us"], 2)
    row["call_over_one_copy"] = round(row["broadcast_call"]["median_us"] / row["one_copy"]["median_us"], 2)
    row["call_GBps_written"] = round(out_bytes / row["broadcast_call"]["median_us"] / 1e3, 2)
    rows.append(row)
    print(json.dumps(row), flush=True)
    del pairs, recv, head_t, frames, counts, mout, recs, mres, slab_a, slab_b, wires, members
    del table, mtable, btable, btable_none, rtable, rres, bres
    torch.cuda.empty_cache()

assert ctx.last_device_error() == 0
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
    for d in dropped:
        f.write(json.dumps({"dropped": d}) + "\n")

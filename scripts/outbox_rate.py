"""What getting a sweep's send bytes to the host costs (profiles/outbox_rate.jsonl).

Cells: 1 024 and 16 384 connections with a send range of 4 KiB each in one
slab; 1/16, 1/4 or all of them send, 128 B or 2 KiB each. The rows are as a
reply + broadcast sweep leaves them, written here by the host: a reply row
(reply_len 0, status 0) and a broadcast row (send_len) per connection; a silent
connection's send_len is 0. Measured per cell, on the host clock from the first
enqueue to the synchronize after which the host has the bytes:
  (a)  outbox_device: xyws_outbox_streams into device memory, a D2H of the
       summary, a synchronize, then a D2H of pack[0 .. packed_len);
  (a') outbox_pinned: the call into pinned memory (pack, list and summary
       written by the kernels through the device pointer), nothing else;
  (b)  what a caller has without the call: a D2H of the result rows, then
       host_copies: one hipMemcpyAsync per sender, issued from a C loop in the
       library (xyws_debug_outbox_host_fetch), or host_slab: one D2H of the
       whole send slab, capacity and all;
  (c)  floor: one D2H of send_bytes bytes.
call_device and call_pinned are the call alone, by device events: what it adds
to a sweep. Before anything is timed the bytes of (a), (a') and both variants
of (b) are compared. The variants are alternated in one process after a
warm-up; every cell is repeated and reports median and range.

usage: outbox_rate.py [--out FILE] [--repeats R] [--cells N,N,...]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from xynet_amd import _lib, websocket as ws  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outbox_rate.jsonl"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--cells", default="1024,16384")
args = ap.parse_args()
assert args.repeats >= 5, "the spread needs at least 5 repeats"
assert torch.cuda.is_available(), "outbox_rate.py measures on the GPU: no device, no number"

ctx = ws.Context(0)
L = ctx.L
stream = torch.cuda.current_stream()
sp = C.c_void_p(stream.cuda_stream)
OUT_CAP = 4096
dev = torch.device("cuda")


def vp(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


def mapped(t):
    d = C.c_void_p()
    _lib.check(L.xyws_outbox_map(C.c_void_p(t.data_ptr()), C.byref(d)), "xyws_outbox_map")
    return d


def host_timed(fn, loops):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(loops):
        fn()  # (ends in a synchronize)
    return (time.perf_counter() - t0) * 1e6 / loops


def event_timed(fn, loops):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(loops):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / loops


def summary(v):
    return {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


rows = []
for n in (int(x) for x in args.cells.split(",")):
    rng = np.random.default_rng(n)
    slab_h = rng.integers(1, 256, n * OUT_CAP + 64, dtype=np.uint8)
    slab = torch.from_numpy(slab_h).cuda()
    idx = np.arange(n, dtype=np.uint64)
    for every, size in ((16, 128), (16, 2048), (4, 128), (4, 2048), (1, 128), (1, 2048)):
        lens = np.where(idx % every == 0, size, 0).astype(np.uint64)
        senders = int((lens > 0).sum())
        send_bytes = int(lens.sum())
        bres = np.zeros((n, 4), np.uint64)
        bres[:, 0] = lens
        pres = np.zeros((n, 4), np.uint64)
        bres_t, pres_t = torch.from_numpy(bres.view(np.int64)).cuda(), torch.from_numpy(pres.view(np.int64)).cuda()
        tab = np.zeros((n, 8), np.uint64)
        tab[:, 0], tab[:, 1] = slab.data_ptr() + 8 + OUT_CAP * idx, OUT_CAP   # (the ranges abut, 8 off a line)
        tab[:, 3], tab[:, 4] = bres_t.data_ptr() + 32 * idx, pres_t.data_ptr() + 32 * idx
        tab_t = torch.from_numpy(tab.view(np.int64)).cuda()
        need = L.xyws_outbox_scratch_bytes(n)
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        pack_cap = int(((lens + 15) & ~np.uint64(15)).sum())
        d_pack = torch.zeros(pack_cap, dtype=torch.uint8, device=dev)
        d_ent = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
        d_sum = torch.zeros(64, dtype=torch.uint8, device=dev)
        h_pack = torch.zeros(pack_cap, dtype=torch.uint8).pin_memory()      # (a): where the pack is copied to
        h_sum = torch.zeros(64, dtype=torch.uint8).pin_memory()
        p_pack = torch.zeros(pack_cap, dtype=torch.uint8).pin_memory()      # (a'): written by the kernels
        p_ent = torch.zeros(32 * n, dtype=torch.uint8).pin_memory()
        p_sum = torch.zeros(64, dtype=torch.uint8).pin_memory()
        mp_pack, mp_ent, mp_sum = mapped(p_pack), mapped(p_ent), mapped(p_sum)
        b_rows = torch.zeros(n * 4, dtype=torch.int64).pin_memory()         # (b): the result rows on the host
        b_dst = torch.zeros(pack_cap, dtype=torch.uint8).pin_memory()
        b_slab = torch.zeros(n * OUT_CAP + 64, dtype=torch.uint8).pin_memory()
        c_dst = torch.zeros(max(send_bytes, 1), dtype=torch.uint8).pin_memory()
        host_tab = np.ascontiguousarray(tab)

        def call_device():
            _lib.check(L.xyws_outbox_streams(ctx.h, vp(tab_t), n, vp(d_pack), pack_cap, vp(d_ent), vp(d_sum), vp(scratch),
                                             need, sp), "xyws_outbox_streams")

        def call_pinned():
            _lib.check(L.xyws_outbox_streams(ctx.h, vp(tab_t), n, mp_pack, pack_cap, mp_ent, mp_sum, vp(scratch), need, sp),
                       "xyws_outbox_streams")

        def outbox_device():
            call_device()
            h_sum.copy_(d_sum, non_blocking=True)
            stream.synchronize()
            packed = int(h_sum.numpy().view(np.uint64)[2])
            h_pack[:packed].copy_(d_pack[:packed], non_blocking=True)
            stream.synchronize()

        def outbox_pinned():
            call_pinned()
            stream.synchronize()

        def host_lens():
            b_rows.copy_(bres_t.view(-1), non_blocking=True)
            stream.synchronize()
            return np.minimum(b_rows.numpy().view(np.uint64).reshape(n, 4)[:, 0], OUT_CAP)

        def host_copies():
            got = np.ascontiguousarray(host_lens())
            _lib.check(L.xyws_debug_outbox_host_fetch(host_tab.ctypes.data, got.ctypes.data, n, C.c_void_p(b_dst.data_ptr()),
                                                      pack_cap, sp), "xyws_debug_outbox_host_fetch")
            stream.synchronize()

        def host_slab():
            host_lens()
            b_slab.copy_(slab, non_blocking=True)
            stream.synchronize()

        def floor():
            c_dst[:send_bytes].copy_(slab[:send_bytes], non_blocking=True)
            stream.synchronize()

        # ---- checks, before anything is timed: every path's bytes
        outbox_device()
        outbox_pinned()
        host_copies()
        host_slab()
        s = _lib.OutboxSummary.from_buffer_copy(h_sum.numpy().tobytes())
        assert (s.n_entries, s.pack_len, s.packed_len, s.send_bytes, s.n_deferred) == (senders, pack_cap, pack_cap, send_bytes, 0)
        assert p_sum.numpy().tobytes() == h_sum.numpy().tobytes(), "pinned summary"
        assert p_ent.numpy().tobytes() == d_ent.cpu().numpy().tobytes(), "pinned entries"
        want = slab_h[8:8 + n * OUT_CAP].reshape(n, OUT_CAP)[lens > 0, :size].reshape(-1).tobytes()
        for name, t in (("device pack", h_pack), ("pinned pack", p_pack), ("host copies", b_dst)):
            assert t.numpy().tobytes() == want, name
        assert b_slab.numpy().tobytes() == slab_h.tobytes(), "host slab"

        modes = {"outbox_device": outbox_device, "outbox_pinned": outbox_pinned, "host_copies": host_copies,
                 "host_slab": host_slab, "floor": floor}
        calls = {"call_device": call_device, "call_pinned": call_pinned}
        for fn in list(modes.values()) + list(calls.values()):
            fn()
            fn()
        torch.cuda.synchronize()
        loops = {"outbox_device": 20, "outbox_pinned": 20, "host_copies": 20 if senders <= 1024 else 3,
                 "host_slab": 20 if n <= 1024 else 5, "floor": 20, "call_device": 100, "call_pinned": 100}
        t = {name: [] for name in list(modes) + list(calls)}
        for _ in range(args.repeats):  # (alternated: each repeat times every variant)
            for name, fn in modes.items():
                t[name].append(host_timed(fn, loops[name]))
            for name, fn in calls.items():
                t[name].append(event_timed(fn, loops[name]))
        row = {"connections": n, "out_cap": OUT_CAP, "senders": senders, "bytes_each": size, "send_bytes": send_bytes,
               "slab_bytes": n * OUT_CAP, "repeats": args.repeats, "loops": loops}
        for name in t:
            row[name] = summary(t[name])
        best_b = min(row["host_copies"]["median_us"], row["host_slab"]["median_us"])
        row["host_best_us"] = best_b
        row["host_best_over_outbox_device"] = round(best_b / row["outbox_device"]["median_us"], 2)
        row["host_best_over_outbox_pinned"] = round(best_b / row["outbox_pinned"]["median_us"], 2)
        row["outbox_device_over_floor"] = round(row["outbox_device"]["median_us"] / row["floor"]["median_us"], 2)
        row["outbox_pinned_over_floor"] = round(row["outbox_pinned"]["median_us"] / row["floor"]["median_us"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)

assert ctx.last_device_error() == 0
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")

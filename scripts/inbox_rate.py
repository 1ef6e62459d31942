"""What getting a sweep's received bytes to the connections costs (profiles/inbox_rate.jsonl).

Cells: 1 024 and 16 384 open connections with a receive range of 4 KiB each in
one slab; 64, a quarter or all of them receive, 128 B or 2 KiB each, one entry
per receiver. Measured per cell, on the host clock from the first enqueue to the
synchronize after which xyws_decode_streams could start (the bytes lie in the
ranges and the xyws_conn table names them):
  (a)  inbox_block: head, entries and pack laid out as one pinned block, one H2D
       of it, then xyws_inbox_streams over the device copy;
  (a') inbox_pinned: the call reading the same pinned block in place through its
       device pointer, nothing else;
  (b)  what a caller does without the call: the buf and len columns of the n-row
       xyws_conn table written on the host (numpy) and the table uploaded, plus
       host_copies: one hipMemcpyAsync per receiver, issued from a C loop in the
       library (xyws_debug_inbox_host_scatter), or
  (b') host_slab: the same table plus one H2D of the whole receive slab,
       capacity and all.
Filling the block of (a) and the pinned bytes of (b) is not timed: both happen
while the completion queue is drained. call_device and call_pinned are the call
alone, by device events: what it adds to a sweep. Before anything is timed the
receive ranges and the xyws_conn rows of every path are compared. The variants
are alternated in one process after a warm-up; every cell is repeated and
reports median and range.

usage: inbox_rate.py [--out FILE] [--repeats R] [--cells N,N,...]
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inbox_rate.jsonl"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--cells", default="1024,16384")
args = ap.parse_args()
assert args.repeats >= 5, "the spread needs at least 5 repeats"
assert torch.cuda.is_available(), "inbox_rate.py measures on the GPU: no device, no number"

ctx = ws.Context(0)
L = ctx.L
stream = torch.cuda.current_stream()
sp = C.c_void_p(stream.cuda_stream)
RECV_CAP = 4096
dev = torch.device("cuda")
ENT = np.dtype([("conn", "<u4"), ("flags", "<u4"), ("off", "<u8"), ("len", "<u8"), ("at", "<u8")])


def vp(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


def mapped(t):
    d = C.c_void_p()
    _lib.check(L.xyws_outbox_map(C.c_void_p(t.data_ptr()), C.byref(d)), "xyws_outbox_map")
    return d.value


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
    idx = np.arange(n, dtype=np.uint64)
    for receivers, size in ((64, 128), (64, 2048), (n // 4, 128), (n // 4, 2048), (n, 128), (n, 2048)):
        rng = np.random.default_rng(n + receivers + size)
        who = (np.arange(receivers, dtype=np.uint64) * (n // receivers)).astype(np.uint64)
        m, recv_bytes = receivers, receivers * size
        slab = torch.zeros(n * RECV_CAP + 64, dtype=torch.uint8, device=dev)
        bufs = slab.data_ptr() + 8 + RECV_CAP * idx                           # (the ranges abut, 8 off a line)
        carries = np.zeros((n, 4), np.uint64)
        carries[:, 2] = _lib.IB_OPEN
        carries_t = torch.from_numpy(carries.view(np.int64)).cuda()
        conns = np.zeros((n, 8), np.uint64)                                   # the resident xyws_conn table
        conns[:, 0] = bufs
        conns_t = torch.from_numpy(conns.view(np.int64)).cuda()
        iconns = np.zeros((n, 8), np.uint64)
        iconns[:, 0], iconns[:, 1], iconns[:, 2] = bufs, RECV_CAP, carries_t.data_ptr() + 32 * idx
        iconns[:, 3] = conns_t.data_ptr() + 64 * idx
        iconns_t = torch.from_numpy(iconns.view(np.int64)).cuda()
        results_t = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
        summary_t = torch.zeros(64, dtype=torch.uint8, device=dev)
        need = L.xyws_inbox_scratch_bytes(n, m)
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        # the block: head, entries, pack
        block_len = 32 + 32 * m + recv_bytes
        block = torch.zeros(block_len, dtype=torch.uint8).pin_memory()
        bh = block.numpy()
        bh[:32].view(np.uint64)[:2] = [m, recv_bytes]
        e = bh[32:32 + 32 * m].view(ENT)
        e["conn"], e["off"], e["len"], e["at"] = who, np.arange(m, dtype=np.uint64) * size, size, 0
        data = rng.integers(1, 256, recv_bytes, dtype=np.uint8)
        bh[32 + 32 * m:] = data
        d_block = torch.zeros(block_len, dtype=torch.uint8, device=dev)
        m_block = mapped(block)
        # the host paths: the table as the host keeps it, the pinned bytes, the pinned slab image
        b_tab = torch.zeros(n * 8, dtype=torch.int64).pin_memory()
        b_tab.numpy().view(np.uint64).reshape(n, 8)[:, 0] = bufs
        b_tab_t = torch.zeros(n * 8, dtype=torch.int64, device=dev)
        lens = np.zeros(n, np.uint64)
        lens[who.astype(np.int64)] = size
        b_pack = torch.from_numpy(data.copy()).pin_memory()
        dsts = np.ascontiguousarray(bufs[who.astype(np.int64)])
        offs = np.ascontiguousarray(np.arange(m, dtype=np.uint64) * size)
        elens = np.full(m, size, np.uint64)
        b_slab = torch.zeros(n * RECV_CAP + 64, dtype=torch.uint8).pin_memory()
        b_slab.numpy()[8:8 + n * RECV_CAP].reshape(n, RECV_CAP)[who.astype(np.int64), :size] = data.reshape(m, size)

        def call_at(base):
            _lib.check(L.xyws_inbox_streams(ctx.h, vp(iconns_t), n, C.c_void_p(base), C.c_void_p(base + 32), m,
                                            C.c_void_p(base + 32 + 32 * m), recv_bytes, vp(results_t), vp(summary_t),
                                            vp(scratch), need, sp), "xyws_inbox_streams")

        def call_device():
            call_at(d_block.data_ptr())

        def call_pinned():
            call_at(m_block)

        def inbox_block():
            d_block.copy_(block, non_blocking=True)
            call_device()
            stream.synchronize()

        def inbox_pinned():
            call_pinned()
            stream.synchronize()

        def host_table():
            b_tab.numpy().view(np.uint64).reshape(n, 8)[:, 1] = lens
            b_tab_t.copy_(b_tab, non_blocking=True)

        def host_copies():
            host_table()
            _lib.check(L.xyws_debug_inbox_host_scatter(dsts.ctypes.data, offs.ctypes.data, elens.ctypes.data, m,
                                                       C.c_void_p(b_pack.data_ptr()), sp), "xyws_debug_inbox_host_scatter")
            stream.synchronize()

        def host_slab():
            host_table()
            slab.copy_(b_slab, non_blocking=True)
            stream.synchronize()

        # ---- checks, before anything is timed: every path's bytes and rows
        want_slab = b_slab.numpy().tobytes()
        want_rows = np.stack([bufs, lens], axis=1).tobytes()
        for name, fn, tab in (("inbox_block", inbox_block, conns_t), ("inbox_pinned", inbox_pinned, conns_t),
                              ("host_copies", host_copies, b_tab_t), ("host_slab", host_slab, b_tab_t)):
            slab.zero_()
            tab.view(-1, 8)[:, 1] = -1
            fn()
            assert slab.cpu().numpy().tobytes() == want_slab, name
            assert tab.view(-1, 8)[:, :2].contiguous().cpu().numpy().view(np.uint64).tobytes() == want_rows, name
            if name.startswith("inbox"):
                s = _lib.InboxSummary.from_buffer_copy(summary_t.cpu().numpy().tobytes())
                assert (s.n_entries, s.bytes, s.n_conns, s.n_broken, s.n_bad_entries, s.status) == (m, recv_bytes, m, 0, 0, 0)

        modes = {"inbox_block": inbox_block, "inbox_pinned": inbox_pinned, "host_copies": host_copies,
                 "host_slab": host_slab}
        calls = {"call_device": call_device, "call_pinned": call_pinned}
        for fn in list(modes.values()) + list(calls.values()):
            fn()
            fn()
        torch.cuda.synchronize()
        loops = {"inbox_block": 20, "inbox_pinned": 20, "host_copies": 20 if m <= 1024 else 3,
                 "host_slab": 20 if n <= 1024 else 5, "call_device": 100, "call_pinned": 100 if recv_bytes <= 1 << 22 else 20}
        t = {name: [] for name in list(modes) + list(calls)}
        for _ in range(args.repeats):  # (alternated: each repeat times every variant)
            for name, fn in modes.items():
                t[name].append(host_timed(fn, loops[name]))
            for name, fn in calls.items():
                t[name].append(event_timed(fn, loops[name]))
        row = {"connections": n, "recv_cap": RECV_CAP, "receivers": m, "bytes_each": size, "recv_bytes": recv_bytes,
               "block_bytes": block_len, "table_bytes": 64 * n, "slab_bytes": n * RECV_CAP, "repeats": args.repeats,
               "loops": loops}
        for name in t:
            row[name] = summary(t[name])
        best_b = min(row["host_copies"]["median_us"], row["host_slab"]["median_us"])
        row["host_best_us"] = best_b
        row["host_best_over_inbox_block"] = round(best_b / row["inbox_block"]["median_us"], 2)
        row["host_best_over_inbox_pinned"] = round(best_b / row["inbox_pinned"]["median_us"], 2)
        row["host_slab_over_inbox_block"] = round(row["host_slab"]["median_us"] / row["inbox_block"]["median_us"], 2)
        row["host_slab_over_inbox_pinned"] = round(row["host_slab"]["median_us"] / row["inbox_pinned"]["median_us"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)

assert ctx.last_device_error() == 0
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")

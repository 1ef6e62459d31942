"""What keeping unsent send bytes on the device costs (profiles/unsent_rate.jsonl).

Cells: 1 024 and 16 384 connections, each with a buffer [2 KiB pend | 2 KiB out]
in one slab; every connection has 1 KiB of new bytes per sweep (a broadcast
row). None, 1/16 or all of the connections are short by half: in the steady
state such a connection is offered 2 KiB (1 KiB tail, 1 KiB new), takes 1 KiB
and keeps 1 KiB; the carries are set to that state before every step. Measured
per cell on the host clock, from the first enqueue to the synchronize:
  outbox:  xyws_outbox_streams alone on the caller's table, device outputs:
           the parent's cost of ending a sweep;
  unsent:  the host stamps the head and the short rows in pinned memory, then
           xyws_unsent_streams, xyws_unsent_view_streams and
           xyws_outbox_streams on the view;
  host:    the path the calls replace, as far as the library can issue it from
           C: one device-to-host copy per short tail
           (xyws_debug_outbox_host_fetch), a synchronize, the tails prepended in
           a pinned staging buffer by one numpy copy, one upload of the staging
           buffer, then xyws_outbox_streams. The per-connection uploads a real
           caller needs are replaced by one: the figure flatters this path.
The variants are alternated in one process after a warm-up; every cell is
repeated and reports median and range of the per-step time.

usage: unsent_rate.py [--out FILE] [--repeats R] [--steps K] [--cells N,N,...]
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
sys.path[:0] = [ROOT]
from xynet_amd import _lib, websocket as ws  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unsent_rate.jsonl"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--cells", default="1024,16384")
args = ap.parse_args()
assert args.repeats >= 5, "the spread needs at least 5 repeats"
assert torch.cuda.is_available(), "unsent_rate.py measures on the GPU: no device, no number"

ctx = ws.Context(0)
L = ctx.L
sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
PEND = OUT = 2048
NEW = TAIL = 1024


def vp(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def summary(v):
    return {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


rows = []
for n in (int(x) for x in args.cells.split(",")):
    idx = np.arange(n, dtype=np.uint64)
    slab = torch.from_numpy(np.random.default_rng(n).integers(1, 256, n * (PEND + OUT) + 64, dtype=np.uint8)).cuda()
    outs = slab.data_ptr() + 8 + (PEND + OUT) * idx + PEND             # (8 off a line; neighbours abut)
    bres = np.zeros((n, 4), np.uint64)
    bres[:, 0] = NEW
    bres_t = dev64(bres)
    tab = np.zeros((n, 8), np.uint64)
    tab[:, 0], tab[:, 1], tab[:, 3] = outs, OUT, bres_t.data_ptr() + 32 * idx
    tab_t = dev64(tab)
    carries = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    utab = np.zeros((n, 4), np.uint64)
    utab[:, 0], utab[:, 1], utab[:, 2] = outs, PEND, carries.data_ptr() + 32 * idx
    utab_t = dev64(utab)
    view_t, vrows_t = torch.zeros(64 * n, dtype=torch.uint8, device="cuda"), torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    ures_t = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    u_need, o_need = L.xyws_unsent_scratch_bytes(n), L.xyws_outbox_scratch_bytes(n)
    u_scr, o_scr = (torch.empty(b, dtype=torch.uint8, device="cuda") for b in (u_need, o_need))
    pack = torch.zeros(n * (PEND + OUT), dtype=torch.uint8, device="cuda")
    ent, summ = torch.zeros(32 * n, dtype=torch.uint8, device="cuda"), torch.zeros(64, dtype=torch.uint8, device="cuda")
    reports = torch.zeros(n, 2, dtype=torch.int32).pin_memory()        # {sent, sweep}
    head = torch.zeros(4, dtype=torch.int32).pin_memory()
    d = C.c_void_p()
    _lib.check(L.xyws_outbox_map(vp(reports), C.byref(d)), "xyws_outbox_map")
    rep_p = C.c_void_p(d.value)
    _lib.check(L.xyws_outbox_map(vp(head), C.byref(d)), "xyws_outbox_map")
    head_p = C.c_void_p(d.value)
    reports_np, head_np = reports.numpy(), head.numpy()
    stage, front = (torch.zeros(n * TAIL, dtype=torch.uint8).pin_memory() for _ in range(2))
    stage_d = torch.zeros(n * TAIL, dtype=torch.uint8, device="cuda")
    for every in (0, 16, 1):
        short = np.flatnonzero(idx % every == 0) if every else np.zeros(0, np.int64)
        steady = np.zeros((n, 4), np.uint64)                            # pend_len, last_len of the steady state
        steady[:, 1] = NEW
        steady[short, 0], steady[short, 1] = TAIL, TAIL + NEW
        steady_t = dev64(steady).view(torch.uint8).reshape(-1)
        h_tab = np.zeros((n, 8), np.uint64)                             # the tails, as a host table for the C copy loop
        h_tab[:, 0] = outs                                              # S + sent = (out - 1 KiB) + 1 KiB
        h_lens = np.zeros(n, np.uint64)
        h_lens[short] = TAIL
        sweep = [1]

        def outbox(table=tab_t):
            _lib.check(L.xyws_outbox_streams(ctx.h, vp(table), n, vp(pack), pack.numel(), vp(ent), vp(summ), vp(o_scr),
                                             o_need, sp), "xyws_outbox_streams")

        def v_outbox():
            carries.copy_(steady_t)
            outbox()
            torch.cuda.synchronize()

        def v_unsent():
            carries.copy_(steady_t)
            sweep[0] += 1
            head_np[0] = sweep[0]
            reports_np[short, 0], reports_np[short, 1] = TAIL, sweep[0]
            _lib.check(L.xyws_unsent_streams(ctx.h, vp(utab_t), n, rep_p, head_p, vp(ures_t), vp(u_scr), u_need, sp),
                       "xyws_unsent_streams")
            _lib.check(L.xyws_unsent_view_streams(ctx.h, vp(utab_t), vp(tab_t), n, vp(view_t), vp(vrows_t), sp),
                       "xyws_unsent_view_streams")
            outbox(view_t)
            torch.cuda.synchronize()

        def v_host():
            carries.copy_(steady_t)
            _lib.check(L.xyws_debug_outbox_host_fetch(h_tab.ctypes.data, h_lens.ctypes.data, n, vp(stage), stage.numel(), sp),
                       "xyws_debug_outbox_host_fetch")
            torch.cuda.synchronize()
            m = max(TAIL * len(short), 1)
            front.numpy()[:m] = stage.numpy()[:m]                       # (the prepend: one pass over the tails)
            stage_d[:m].copy_(front[:m], non_blocking=True)
            outbox()
            torch.cuda.synchronize()

        variants = dict(outbox=v_outbox, unsent=v_unsent, host=v_host)
        v_unsent()
        res = _lib.read_rows(_lib.UnsentResult, ures_t, n)
        assert sum(r.pend_len for r in res) == TAIL * len(short) and all(r.status in (0, 1) for r in res)
        assert _lib.read_rows(_lib.OutboxSummary, summ, 1)[0].send_bytes == n * NEW + TAIL * len(short)
        times = {k: [] for k in variants}
        for r in range(args.repeats + 1):
            for k, f in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    f()
                if r:  # (the first round is the warm-up)
                    times[k].append((time.perf_counter() - t0) * 1e6 / args.steps)
        row = dict(conns=n, short=len(short), out_bytes=OUT, tail_bytes=TAIL, repeats=args.repeats, steps=args.steps,
                   device=torch.cuda.get_device_name(0), **{k: summary(v) for k, v in times.items()})
        rows.append(row)
        print(json.dumps(row), flush=True)

with open(args.out, "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
ctx.close()

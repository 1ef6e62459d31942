"""What answering the opening handshakes on the device costs (profiles/accept_rate.jsonl).

Cells: 1 024, 4 096 and 16 384 connections (4 096: the join storm of a quarter
of 16 384). Each connection holds the 499-byte browser-shaped request of
tests/accept_cases.py with a random key, in one request slab (stride 512);
the responses go to one send slab (stride 144). Measured per cell:
  (a) accept_call: xyws_accept_streams alone (policy 0, max_request 1024);
  (b) accept_call_rows: the same and one D2H of the result rows, which a
      caller reads to route the accepted connections;
  (c) host_path: what a caller does without the call: one D2H of the request
      slab, xyws_accept_request per connection on one host thread (a C loop in
      the library, xyws_debug_accept_host: the same grammar compiled for the
      host), one H2D of the response slab;
  (d) host_parse: the host loop of (c) alone, timed on the host clock.
Only one SHA-1 placement exists (wave-uniform, with the walk), so there is no
placement pair to compare; --walk tags the rows with the library build that
was measured (the committed kernel's walk is wave-uniform; the rows tagged
lane0 in the profile are a trial build in which lane 0 walked alone).
Before anything is timed a sample of both paths' responses is checked against
hashlib. The variants are alternated in one process after a warm-up, each
timed by device events around a loop that ends in a synchronise (the events
span the host path's host work too: the stream waits for it); every cell is
repeated and reports median and range.

usage: accept_rate.py [--out FILE] [--repeats R] [--cells N,N,...] [--walk TAG] [--append]
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
import accept_cases as AC  # noqa: E402
import accept_model as M  # noqa: E402
from xynet_amd import _lib, websocket as ws  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accept_rate.jsonl"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--cells", default="1024,4096,16384")
ap.add_argument("--walk", default="wave_uniform", help="tag of the library build that is measured")
ap.add_argument("--append", action="store_true")
args = ap.parse_args()
assert args.repeats >= 5, "the spread needs at least 5 repeats"
assert torch.cuda.is_available(), "accept_rate.py measures on the GPU: no device, no number"

ctx = ws.Context(0)
L = ctx.L
sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
REQ, RSTRIDE, OSTRIDE, MAXR, POLICY = 499, 512, 144, 1024, 0


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
for n in (int(x) for x in args.cells.split(",")):
    keys = AC.random_keys(n, seed=0xACC + n)
    img = np.zeros(n * RSTRIDE, np.uint8)
    for i, k in enumerate(keys):
        img[RSTRIDE * i:RSTRIDE * i + REQ] = np.frombuffer(AC.browser(k), np.uint8)
    reqs = torch.from_numpy(img).cuda()
    outs = torch.zeros(n * OSTRIDE, dtype=torch.uint8, device="cuda")
    res = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    idx = np.arange(n, dtype=np.uint64)
    tab = np.zeros((n, 4), np.uint64)
    tab[:, 0], tab[:, 1] = reqs.data_ptr() + RSTRIDE * idx, REQ
    tab[:, 2], tab[:, 3] = outs.data_ptr() + OSTRIDE * idx, OSTRIDE
    tab_t = torch.from_numpy(tab.view(np.int64)).cuda()
    h_res = torch.zeros(n * 32, dtype=torch.uint8).pin_memory()
    h_reqs = torch.zeros(n * RSTRIDE, dtype=torch.uint8).pin_memory()
    h_outs = torch.zeros(n * OSTRIDE, dtype=torch.uint8).pin_memory()
    h_rows = (_lib.AcceptResult * n)()
    d_outs = torch.zeros(n * OSTRIDE, dtype=torch.uint8, device="cuda")

    def accept_call():
        _lib.check(L.xyws_accept_streams(ctx.h, vp(tab_t), n, MAXR, POLICY, vp(res), sp), "xyws_accept_streams")

    def accept_call_rows():
        accept_call()
        h_res.copy_(res, non_blocking=True)
        torch.cuda.synchronize()

    def host_parse():
        _lib.check(L.xyws_debug_accept_host(C.c_void_p(h_reqs.data_ptr()), RSTRIDE, REQ, n, MAXR, POLICY,
                                            C.c_void_p(h_outs.data_ptr()), OSTRIDE, OSTRIDE, h_rows),
                   "xyws_debug_accept_host")

    def host_path():
        h_reqs.copy_(reqs, non_blocking=True)
        torch.cuda.synchronize()
        host_parse()
        d_outs.copy_(h_outs, non_blocking=True)

    # ---- checks, before anything is timed
    accept_call_rows()
    host_path()
    torch.cuda.synchronize()
    got_dev, got_host = outs.cpu().numpy(), d_outs.cpu().numpy()
    rws = h_res.numpy().view(np.uint32).reshape(n, 8)
    assert (rws[:, 0] == M.ACCEPTED).all() and (rws[:, 3] == 129).all(), "every request accepted"
    for i in list(range(0, n, max(1, n // 64)))[:64] + [n - 1]:
        want = M.response_101(keys[i])
        assert got_dev[OSTRIDE * i:OSTRIDE * i + 129].tobytes() == want, ("device response", i)
        assert got_host[OSTRIDE * i:OSTRIDE * i + 129].tobytes() == want, ("host response", i)
        assert bytes(h_rows[i]) == rws[i].tobytes(), ("rows", i)

    modes = {"accept_call": accept_call, "accept_call_rows": accept_call_rows, "host_path": host_path}
    for fn in modes.values():
        fn()
        fn()
    torch.cuda.synchronize()
    loops = {"accept_call": 100, "accept_call_rows": 50, "host_path": 5}
    t = {name: [] for name in modes}
    t["host_parse"] = []
    for _ in range(args.repeats):
        for name, fn in modes.items():  # (alternated: each repeat times every variant)
            t[name].append(timed(fn, loops[name]))
        t0 = time.perf_counter()
        host_parse()
        t["host_parse"].append((time.perf_counter() - t0) * 1e6)
    row = {"connections": n, "request_bytes": REQ, "max_request": MAXR, "policy": POLICY, "req_stride": RSTRIDE,
           "out_stride": OSTRIDE, "walk": args.walk, "repeats": args.repeats, "loops": loops}
    for name in t:
        row[name] = summary(t[name])
    row["accept_call_ns_per_conn"] = round(1e3 * row["accept_call"]["median_us"] / n, 2)
    row["host_parse_ns_per_conn"] = round(1e3 * row["host_parse"]["median_us"] / n, 2)
    row["accepts_per_s_device"] = round(n / row["accept_call"]["median_us"] * 1e6)
    row["accepts_per_s_host_core"] = round(n / row["host_parse"]["median_us"] * 1e6)
    row["host_path_over_call_rows"] = round(row["host_path"]["median_us"] / row["accept_call_rows"]["median_us"], 2)
    row["host_path_over_call_rows_worst"] = round(row["host_path"]["min_us"] / row["accept_call_rows"]["max_us"], 2)
    row["host_parse_over_call"] = round(row["host_parse"]["median_us"] / row["accept_call"]["median_us"], 2)
    row["call_beats_host_core_beyond_spread"] = row["accept_call"]["max_us"] < row["host_parse"]["min_us"]
    rows.append(row)
    print(json.dumps(row), flush=True)

assert ctx.last_device_error() == 0
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a" if args.append else "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")

"""What routing a joiner to its room on the device costs (profiles/route_rate.jsonl).

Cells: 1 024, 4 096 and 16 384 accepted connections. Each holds the 499-byte
browser-shaped request of tests/accept_cases.py with its 12-byte target
replaced by the 24 bytes /rooms/<k>?token=... (511 bytes), in one request slab
(stride 512); the route table has 1 024 exact routes /rooms/<k>
and one prefix route. Every connection joins on accept; the rooms are emptied
on the device before each pass, so every pass does the same work. Measured per
cell:
  (a) route_call: xyws_route_streams alone (policy 0);
  (b) sweep_routed: accept + route + roster, against sweep_preset: accept +
      roster with the rooms already in the roster rows (the sweep as it was
      before this call, from the same library): the added cost per sweep;
  (c) host_route: the host path the call replaces: accept, then D2H of the
      accept rows and the request slab, xyws_route_lookup per connection on one
      host thread (a C loop in the library, xyws_debug_route_host), H2D of the
      room words into the roster rows, then the roster;
  (d) host_lookup: the host loop of (c) alone, on the host clock.
Where the library has the one-thread-per-connection trial kernel
(xyws_debug_route_threads: a trial build; the committed library
has the wave kernel only) it is measured too, as route_threads. Before anything is timed the rooms of both
paths are checked against tests/route_model.py. The variants are alternated in
one process after a warm-up, each timed by device events around a loop that
ends in a synchronise; every cell is repeated and reports median and range.

usage: route_rate.py [--out FILE] [--repeats R] [--cells N,N,...] [--append]
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
import accept_model as AM  # noqa: E402
import route_model as RM  # noqa: E402
from xynet_amd import _lib, websocket as ws  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "route_rate.jsonl"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--cells", default="1024,4096,16384")
ap.add_argument("--append", action="store_true")
args = ap.parse_args()
assert args.repeats >= 5, "the spread needs at least 5 repeats"
assert torch.cuda.is_available(), "route_rate.py measures on the GPU: no device, no number"

ctx = ws.Context(0)
L = ctx.L
sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
TARGET, RSTRIDE, OSTRIDE, MAXR, NR, CAP = 24, 512, 256, 1024, 1024, 64
REQ = len(AC.browser(path=b"")) + TARGET
HAS_THREADS = hasattr(L, "xyws_debug_route_threads")
if HAS_THREADS:
    L.xyws_debug_route_threads.restype = C.c_int
    L.xyws_debug_route_threads.argtypes = [C.c_void_p] * 4 + [C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                                              C.c_uint32, C.c_void_p, C.c_void_p]


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


def target(i, k):
    """/rooms/<k>?token=<hex>, TARGET bytes."""
    t = b"/rooms/%d?token=" % k
    return (t + b"%016x" % (0x9E3779B97F4A7C15 * (i + 1) & 0xFFFFFFFFFFFFFFFF))[:TARGET]


routes = {b"/rooms/%d" % k: k for k in range(NR)}
blob = _lib.route_table(exact=routes, prefix={b"/rooms": 0})
tab_model = RM.table([(k, r, 0) for k, r in routes.items()] + [(b"/rooms", 0, RM.PREFIX)])
blob_t = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()
dev = torch.device("cuda")
rows = []
for n in (int(x) for x in args.cells.split(",")):
    keys = AC.random_keys(n, seed=0xACC + n)
    img = np.zeros(n * RSTRIDE, np.uint8)
    want_room = np.zeros(n, np.uint32)
    for i, k in enumerate(keys):
        t = target(i, (i * 7919) % NR)
        req = AC.browser(k, path=t)
        assert len(req) == REQ <= RSTRIDE and len(t) == TARGET
        img[RSTRIDE * i:RSTRIDE * i + REQ] = np.frombuffer(req, np.uint8)
        if i % max(1, n // 256) == 0 or i == n - 1:
            row = RM.lookup(tab_model, t)
            assert row["status"] == RM.MATCHED and row["room"] == (i * 7919) % NR
        want_room[i] = (i * 7919) % NR
    reqs = torch.from_numpy(img).cuda()
    outs = torch.zeros(n * OSTRIDE, dtype=torch.uint8, device=dev)
    ares = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    rres = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    idx = np.arange(n, dtype=np.uint64)
    atab = np.zeros((n, 4), np.uint64)
    atab[:, 0], atab[:, 1] = reqs.data_ptr() + RSTRIDE * idx, REQ
    atab[:, 2], atab[:, 3] = outs.data_ptr() + OSTRIDE * idx, OSTRIDE
    atab_t = torch.from_numpy(atab.view(np.int64)).cuda()
    rt = np.zeros((n, 2), np.uint32)
    rt[:, 0] = np.arange(n)
    rt_t = torch.from_numpy(rt.view(np.int32)).cuda()
    # the room set: NR rooms of CAP members, every connection joins on accept
    members = torch.zeros(NR * CAP, dtype=torch.int32, device=dev)
    notes = torch.zeros(NR * 4096, dtype=torch.uint8, device=dev)
    rooms, rrooms = _lib.Table(_lib.Room, NR), _lib.Table(_lib.RosterRoom, NR)
    for r in range(NR):
        rooms[r].members = members.data_ptr() + 4 * CAP * r
        rrooms[r].member_cap, rrooms[r].notes, rrooms[r].notes_cap = CAP, notes.data_ptr() + 4096 * r, 4096
    rooms_t, rrooms_t = rooms.upload(dev), rrooms.upload(dev)
    rooms0 = rooms_t.clone()
    bc = np.zeros((n, 16), np.uint32)
    bc[:, _lib.BcastConn.room.offset // 4] = _lib.ROOM_NONE
    bconns_t = torch.from_numpy(bc.view(np.int32)).cuda()
    bconns0 = bconns_t.clone()
    rc = np.zeros((n, 8), np.uint64)
    rc[:, 2], rc[:, 3], rc[:, 6] = outs.data_ptr() + OSTRIDE * idx, OSTRIDE, ares.data_ptr() + 32 * idx
    rc[:, 7] = np.uint64(_lib.ROOM_NONE) | (np.uint64(_lib.RS_JOIN_ON_ACCEPT) << np.uint64(32))
    rconns_t = torch.from_numpy(rc.view(np.int64)).cuda()              # the rooms come from the route call
    rc[:, 7] = want_room.astype(np.uint64) | (np.uint64(_lib.RS_JOIN_ON_ACCEPT) << np.uint64(32))
    rconns_preset_t = torch.from_numpy(rc.view(np.int64)).cuda()       # the rooms preset by the host
    rconns_host_t = rconns_preset_t.clone()
    rconns_host_t.view(torch.int32).view(n, 16)[:, 14] = -1
    room_res = torch.zeros(NR * 32, dtype=torch.uint8, device=dev)
    want = torch.zeros(n, dtype=torch.int32, device=dev)
    ros = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    h_ares = torch.zeros(n * 32, dtype=torch.uint8).pin_memory()
    h_reqs = torch.zeros(n * RSTRIDE, dtype=torch.uint8).pin_memory()
    h_rooms = torch.zeros(n, dtype=torch.int32).pin_memory()

    def reset():
        rooms_t.copy_(rooms0)
        bconns_t.copy_(bconns0)

    def accept_call():
        _lib.check(L.xyws_accept_streams(ctx.h, vp(atab_t), n, MAXR, 0, vp(ares), sp), "xyws_accept_streams")

    def route_call(rconns=rconns_t):
        _lib.check(L.xyws_route_streams(ctx.h, vp(atab_t), vp(ares), vp(rt_t), n, vp(blob_t), len(blob), vp(rconns), n,
                                        _lib.ROOM_NONE, 0, vp(rres), sp), "xyws_route_streams")

    def route_threads():
        _lib.check(L.xyws_debug_route_threads(ctx.h, vp(atab_t), vp(ares), vp(rt_t), n, vp(blob_t), len(blob), vp(rconns_t),
                                              n, _lib.ROOM_NONE, vp(rres), sp), "xyws_debug_route_threads")

    def roster_call(rconns):
        _lib.check(L.xyws_roster_streams(ctx.h, vp(bconns_t), vp(rconns), n, vp(rooms_t), vp(rrooms_t), vp(room_res), NR,
                                         None, 0x11, None, vp(want), vp(ros), sp), "xyws_roster_streams")

    def sweep_routed():
        reset()
        accept_call()
        route_call()
        roster_call(rconns_t)

    def sweep_preset():
        reset()
        accept_call()
        roster_call(rconns_preset_t)

    def host_lookup():
        _lib.check(L.xyws_debug_route_host(blob, len(blob), C.c_void_p(h_reqs.data_ptr()), RSTRIDE,
                                           C.c_void_p(h_ares.data_ptr()), n, _lib.ROOM_NONE,
                                           C.c_void_p(h_rooms.data_ptr())), "xyws_debug_route_host")

    def host_route():
        reset()
        accept_call()
        h_ares.copy_(ares, non_blocking=True)
        h_reqs.copy_(reqs, non_blocking=True)
        torch.cuda.synchronize()
        host_lookup()
        rconns_host_t.view(torch.int32).view(n, 16)[:, 14].copy_(h_rooms, non_blocking=True)
        roster_call(rconns_host_t)

    # ---- checks, before anything is timed: both paths' rooms against the model
    def listed():
        torch.cuda.synchronize()
        counts = rooms_t.cpu().numpy().view(np.uint64).reshape(NR, 4)[:, 1].astype(np.int64)
        m = members.cpu().numpy().reshape(NR, CAP)
        got = np.full(n, -1, np.int64)
        for r in range(NR):
            got[m[r, :counts[r]]] = r
        return got

    accept_call()
    torch.cuda.synchronize()
    assert (ares.cpu().numpy().view(np.uint32).reshape(n, 8)[:, 0] == AM.ACCEPTED).all(), "every request accepted"
    sweep_routed()
    assert (rres.cpu().numpy().view(np.uint32).reshape(n, 8)[:, 1] == want_room).all(), "device rooms"
    assert (rres.cpu().numpy().view(np.uint32).reshape(n, 8)[:, 0] == RM.MATCHED).all()
    assert (listed() == want_room).all(), "device path: the lists"
    host_route()
    assert (listed() == want_room).all() and (h_rooms.numpy().view(np.uint32) == want_room).all(), "host path"
    sweep_preset()
    assert (listed() == want_room).all(), "preset path"
    if HAS_THREADS:
        rres.zero_()
        route_threads()
        torch.cuda.synchronize()
        assert (rres.cpu().numpy().view(np.uint32).reshape(n, 8)[:, 1] == want_room).all(), "trial kernel rooms"

    modes = {"accept_call": accept_call, "route_call": route_call, "sweep_routed": sweep_routed,
             "sweep_preset": sweep_preset, "host_route": host_route}
    if HAS_THREADS:
        modes["route_threads"] = route_threads
    for fn in modes.values():
        fn()
        fn()
    torch.cuda.synchronize()
    loops = {"accept_call": 100, "route_call": 200, "route_threads": 200, "sweep_routed": 50, "sweep_preset": 50,
             "host_route": 5}
    t = {name: [] for name in modes}
    t["host_lookup"] = []
    for _ in range(args.repeats):
        for name, fn in modes.items():  # (alternated: each repeat times every variant)
            t[name].append(timed(fn, loops[name]))
        t0 = time.perf_counter()
        host_lookup()
        t["host_lookup"].append((time.perf_counter() - t0) * 1e6)
    row = {"connections": n, "request_bytes": REQ, "routes": NR + 1, "table_bytes": len(blob), "rooms": NR,
           "repeats": args.repeats, "loops": {k: v for k, v in loops.items() if k in modes}}
    for name in t:
        row[name] = summary(t[name])
    row["route_call_ns_per_conn"] = round(1e3 * row["route_call"]["median_us"] / n, 2)
    row["route_over_accept"] = round(row["route_call"]["median_us"] / row["accept_call"]["median_us"], 3)
    row["sweep_added_us"] = round(row["sweep_routed"]["median_us"] - row["sweep_preset"]["median_us"], 2)
    row["host_route_over_sweep_routed"] = round(row["host_route"]["median_us"] / row["sweep_routed"]["median_us"], 2)
    row["host_lookup_ns_per_conn"] = round(1e3 * row["host_lookup"]["median_us"] / n, 2)
    rows.append(row)
    print(json.dumps(row), flush=True)

assert ctx.last_device_error() == 0
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a" if args.append else "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")

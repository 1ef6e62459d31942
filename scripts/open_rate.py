"""What opening rooms on the device costs (profiles/open_rate.jsonl).

Cells: 1 024, 4 096 and 16 384 accepted joiners, each holding the browser-shaped
request of tests/accept_cases.py with the target /rooms/<name>?token=... in one
request slab (stride 512); the route table has the prefix route /rooms, whose
room is from_room. Three shapes per cell:
  find      every joiner names its own room, all of them in the directory;
  distinct  every joiner names its own room, none of them in the directory;
  one       every joiner names the same new room (the contended chain).
The directory is put back on the device before each pass (find: as one call
left it; distinct, one: empty), so every pass does the same work. Per cell and
shape:
  (a) open_call: xyws_open_streams alone (with the copy that puts the
      directory back, which put_back times alone);
  (b) sweep_open: accept + route + open + roster, against sweep_routed:
      accept + route + roster with the final rooms already in the roster rows
      (the route call then writes its result rows only), from the same library;
  (c) host_open: the host path the call replaces: accept + route, D2H of the
      route rows and the request slab, a Python dict on one host thread, H2D
      of the room words, roster.
Before anything is timed the rooms of the device path and of the host path are
checked against the reference dict. The variants are alternated in one process
after a warm-up, each timed by device events around a loop that ends in a
synchronise; every cell is repeated and reports median and range.

usage: open_rate.py [--out FILE] [--repeats R] [--cells N,N,...] [--shapes find,distinct,one]
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import accept_cases as AC  # noqa: E402
from xynet_amd import _lib, websocket as ws  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "open_rate.jsonl"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--cells", default="1024,4096,16384")
ap.add_argument("--shapes", default="find,distinct,one")
args = ap.parse_args()
assert args.repeats >= 5, "the spread needs at least 5 repeats"
assert torch.cuda.is_available(), "open_rate.py measures on the GPU: no device, no number"

ctx = ws.Context(0)
L = ctx.L
sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
TARGET, RSTRIDE, OSTRIDE, MAXR, FROM, NOTES = 24, 512, 256, 1024, 0, 512
REQ = len(AC.browser(path=b"")) + TARGET
dev = torch.device("cuda")
blob = _lib.route_table(prefix={b"/rooms": FROM})
blob_t = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()


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
    for shape in args.shapes.split(","):
        nr, cap = (2, n) if shape == "one" else (n + 1, 4)
        keys = AC.random_keys(n, seed=0x09E + n)
        img = np.zeros(n * RSTRIDE, np.uint8)
        names, want_room = {}, np.zeros(n, np.uint32)  # the reference dict: rooms in row order
        for i, k in enumerate(keys):
            name = b"/rooms/%d" % (0 if shape == "one" else i)
            t = (name + b"?token=" + b"%016x" % (0x9E3779B97F4A7C15 * (i + 1) & 0xFFFFFFFFFFFFFFFF))[:TARGET]
            req = AC.browser(k, path=t)
            assert len(req) == REQ <= RSTRIDE
            img[RSTRIDE * i:RSTRIDE * i + REQ] = np.frombuffer(req, np.uint8)
            want_room[i] = names.setdefault(name, 1 + len(names))
        reqs = torch.from_numpy(img).cuda()
        outs = torch.zeros(n * OSTRIDE, dtype=torch.uint8, device=dev)
        ares, rres, ros = (torch.zeros(n * 32, dtype=torch.uint8, device=dev) for _ in range(3))
        idx = np.arange(n, dtype=np.uint64)
        atab = np.zeros((n, 4), np.uint64)
        atab[:, 0], atab[:, 1] = reqs.data_ptr() + RSTRIDE * idx, REQ
        atab[:, 2], atab[:, 3] = outs.data_ptr() + OSTRIDE * idx, OSTRIDE
        atab_t = torch.from_numpy(atab.view(np.int64)).cuda()
        rt = np.zeros((n, 2), np.uint32)
        rt[:, 0] = np.arange(n)
        rt_t = torch.from_numpy(rt.view(np.int32)).cuda()
        rt[:, 0] = _lib.ROUTE_NO_ROW
        rt_none_t = torch.from_numpy(rt.view(np.int32)).cuda()
        members = torch.zeros(nr * cap, dtype=torch.int32, device=dev)
        notes = torch.zeros(nr * NOTES, dtype=torch.uint8, device=dev)
        rooms, rrooms = _lib.Table(_lib.Room, nr), _lib.Table(_lib.RosterRoom, nr)
        for r in range(nr):
            rooms[r].members = members.data_ptr() + 4 * cap * r
            rrooms[r].member_cap, rrooms[r].notes, rrooms[r].notes_cap = cap, notes.data_ptr() + NOTES * r, NOTES
        rooms_t, rrooms_t = rooms.upload(dev), rrooms.upload(dev)
        rooms0 = rooms_t.clone()
        bc = np.zeros((n, 16), np.uint32)
        bc[:, _lib.BcastConn.room.offset // 4] = _lib.ROOM_NONE
        bconns_t = torch.from_numpy(bc.view(np.int32)).cuda()
        bconns0 = bconns_t.clone()
        rc = np.zeros((n, 8), np.uint64)
        rc[:, 2], rc[:, 3], rc[:, 6] = outs.data_ptr() + OSTRIDE * idx, OSTRIDE, ares.data_ptr() + 32 * idx
        rc[:, 7] = np.uint64(_lib.ROOM_NONE) | (np.uint64(_lib.RS_JOIN_ON_ACCEPT) << np.uint64(32))
        rconns_t = torch.from_numpy(rc.view(np.int64)).cuda()          # the rooms come from the route and open calls
        rc[:, 7] = want_room.astype(np.uint64) | (np.uint64(_lib.RS_JOIN_ON_ACCEPT) << np.uint64(32))
        rconns_preset_t = torch.from_numpy(rc.view(np.int64)).cuda()   # the final rooms preset by the host
        rconns_host_t = rconns_preset_t.clone()
        rconns_host_t.view(torch.int32).view(n, 16)[:, 14] = -1
        room_res = torch.zeros(nr * 32, dtype=torch.uint8, device=dev)
        want = torch.zeros(n, dtype=torch.int32, device=dev)
        work = torch.zeros(_lib.OPEN_WORK_WORDS * n, dtype=torch.int32, device=dev)
        dblob = _lib.directory_blob(1, n, keys_cap=16 * n)
        dir_t = torch.from_numpy(np.frombuffer(dblob, np.uint8).copy()).cuda()
        dir0 = dir_t.clone()
        h_rres = torch.zeros(n * 32, dtype=torch.uint8).pin_memory()
        h_reqs = torch.zeros(n * RSTRIDE, dtype=torch.uint8).pin_memory()
        h_rooms = torch.zeros(n, dtype=torch.int32).pin_memory()

        def reset():
            rooms_t.copy_(rooms0)
            bconns_t.copy_(bconns0)

        def put_back():
            dir_t.copy_(dir0)

        def accept_call():
            _lib.check(L.xyws_accept_streams(ctx.h, vp(atab_t), n, MAXR, 0, vp(ares), sp), "xyws_accept_streams")

        def route_call(rtc=rt_t, rconns=rconns_t):
            _lib.check(L.xyws_route_streams(ctx.h, vp(atab_t), vp(ares), vp(rtc), n, vp(blob_t), len(blob), vp(rconns), n,
                                            _lib.ROOM_NONE, 0, vp(rres), sp), "xyws_route_streams")

        def open_only():
            _lib.check(L.xyws_open_streams(ctx.h, vp(atab_t), vp(rt_t), n, vp(dir_t), len(dblob), vp(rconns_t), n, FROM,
                                           vp(rres), vp(work), sp), "xyws_open_streams")

        rres0 = None

        def open_call():  # (the route rows and the directory as they were before the call)
            rres.copy_(rres0)
            put_back()
            open_only()

        def copies():
            rres.copy_(rres0)
            put_back()

        def roster_call(rconns):
            _lib.check(L.xyws_roster_streams(ctx.h, vp(bconns_t), vp(rconns), n, vp(rooms_t), vp(rrooms_t), vp(room_res), nr,
                                             None, 0x11, None, vp(want), vp(ros), sp), "xyws_roster_streams")

        def sweep_open():
            reset()
            put_back()
            accept_call()
            route_call()
            open_only()
            roster_call(rconns_t)

        def sweep_routed():
            reset()
            accept_call()
            route_call(rt_none_t)
            roster_call(rconns_preset_t)

        seen = {}

        def host_dict():
            r = h_rres.numpy().view(np.uint32).reshape(n, 8)
            slab, out = h_reqs.numpy(), h_rooms.numpy()
            for i in range(n):
                at = RSTRIDE * i + int(r[i, 3])
                out[i] = seen.setdefault(slab[at:at + int(r[i, 4])].tobytes(), 1 + len(seen))

        def host_open():
            reset()
            seen.clear()
            if shape == "find":
                seen.update(names)
            accept_call()
            route_call()
            h_rres.copy_(rres, non_blocking=True)
            h_reqs.copy_(reqs, non_blocking=True)
            torch.cuda.synchronize()
            host_dict()
            rconns_host_t.view(torch.int32).view(n, 16)[:, 14].copy_(h_rooms, non_blocking=True)
            roster_call(rconns_host_t)

        # ---- checks, before anything is timed: both paths' rooms against the reference dict
        def listed():
            torch.cuda.synchronize()
            counts = rooms_t.cpu().numpy().view(np.uint64).reshape(nr, 4)[:, 1].astype(np.int64)
            m = members.cpu().numpy().reshape(nr, cap)
            got = np.full(n, -1, np.int64)
            for r in range(nr):
                got[m[r, :counts[r]]] = r
            return got

        sweep_open()
        res = rres.cpu().numpy().view(np.uint32).reshape(n, 8)
        assert (res[:, 1] == want_room).all() and (res[:, 0] == 3 | _lib.RT_OPENED).all(), "device rooms"
        assert (listed() == want_room).all(), "device path: the lists"
        assert _lib.directory_names(dir_t.cpu().numpy().tobytes()) == names
        if shape == "find":  # the directory as that call left it
            dir0 = dir_t.clone()
            sweep_open()
            res = rres.cpu().numpy().view(np.uint32).reshape(n, 8)
            assert (res[:, 1] == want_room).all() and (res[:, 0] == 3 | _lib.RT_DIRECTORY).all(), "device rooms, found"
        host_open()
        assert (listed() == want_room).all() and (h_rooms.numpy().view(np.uint32) == want_room).all(), "host path"
        sweep_routed()
        assert (listed() == want_room).all(), "preset path"
        accept_call()
        route_call()
        rres0 = rres.clone()

        modes = {"open_call": open_call, "put_back": copies, "sweep_open": sweep_open, "sweep_routed": sweep_routed,
                 "host_open": host_open}
        for fn in modes.values():
            fn()
            fn()
        torch.cuda.synchronize()
        loops = {"open_call": 100, "put_back": 100, "sweep_open": 30, "sweep_routed": 30, "host_open": 3}
        t = {name: [] for name in modes}
        for _ in range(args.repeats):
            for name, fn in modes.items():  # (alternated: each repeat times every variant)
                t[name].append(timed(fn, loops[name]))
        row = {"joiners": n, "shape": shape, "request_bytes": REQ, "rooms": nr, "directory_bytes": len(dblob),
               "repeats": args.repeats, "loops": loops}
        for name in t:
            row[name] = summary(t[name])
        row["open_alone_us"] = round(row["open_call"]["median_us"] - row["put_back"]["median_us"], 2)
        row["sweep_added_us"] = round(row["sweep_open"]["median_us"] - row["sweep_routed"]["median_us"], 2)
        row["host_open_over_sweep_open"] = round(row["host_open"]["median_us"] / row["sweep_open"]["median_us"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)

assert ctx.last_device_error() == 0
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")

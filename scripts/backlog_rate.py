"""What keeping each room's recent messages on the device costs (profiles/backlog_rate.jsonl).

Cells: 1 024 and 16 384 connections in rooms of 16, and one room of 1 024.
Every connection sends one whole masked text message of 40-200 bytes per
sweep, so every room folds its 10 newest frames each sweep (keep = 10).
Measured per cell:
  (a) backlog_call: xyws_backlog_streams alone on the tables one broadcast
      wrote, no joiner (the carries chain from call to call: every call folds
      again and changes halves);
  (b) six_call: recv restore (one device copy, the decode unmasks in place),
      decode, reassemble, hold, reply, broadcast, backlog, no joiner;
  (c) five_call: the same without the backlog call: the sweep as it was before
      the call existed;
  (d) join_storm: the six-call sweep in which a quarter of the connections
      join (each its own room), against host_path, what a caller did instead:
      the five-call sweep, D2H of every room's wire and row, the last 10
      frames of every room kept on the host (ONE vectorised numpy gather for
      all rooms, no parsing: a lower bound for a deque per room), H2D of the
      backlogs, and one device copy per joiner.
Before anything is timed room 0's log is checked against the last 10 frames
of the host's wire, and a joiner's send bytes of both paths against it. The
variants are alternated in one process after a warm-up, each timed by device
events around a loop that ends in a synchronise (the events span the host
path's host work too: the stream waits for it); every cell is repeated and
reports median and range.

--fold-only times (a) alone on the listed cells and tags the rows with --tag:
the workgroup-size trial of the fold runs it once per library build (XYWS_LIB).

usage: backlog_rate.py [--out FILE] [--repeats R] [--cells N:M,N:M,...] [--fold-only] [--tag T] [--append]
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "backlog_rate.jsonl"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--cells", default="1024:16,16384:16,1024:1024")
ap.add_argument("--fold-only", action="store_true")
ap.add_argument("--tag", default="")
ap.add_argument("--append", action="store_true")
args = ap.parse_args()
assert args.repeats >= 5, "the spread needs at least 5 repeats"
assert torch.cuda.is_available(), "backlog_rate.py measures on the GPU: no device, no number"

ctx = ws.Context(0)
L = ctx.L
stream = torch.cuda.current_stream()
sp = C.c_void_p(stream.cuda_stream)
HEAD, KEEP = 24, 10
FRAME_MAX = 4 + HEAD + 200
LOG_CAP = 2 * KEEP * FRAME_MAX + 30
HOLD_CAP = 2 * 256 + 30
CAP = MCAP = 4


def vp(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def zeros(nbytes):
    return torch.zeros(nbytes, dtype=torch.uint8, device="cuda")


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


def frame(rng, b0, payload):
    key = rng.bytes(4)
    body = np.frombuffer(payload, np.uint8) ^ np.resize(np.frombuffer(key, np.uint8), len(payload))
    return streams.header(b0, len(payload), key) + body.tobytes()


def text(length, salt, base=0x61):
    return (base + (np.arange(length) + salt) % 26).astype(np.uint8).tobytes()


class Variant:
    """One sweep pipeline with carries, tables, result rows, logs and backlog
    carries of its own. join: which connections are flagged XYWS_BL_JOIN."""

    def __init__(self, n, MB, stride, recv, sends, own, soff, heads_t, wires, wlen, woff, members, join=None):
        self.n, R = n, n // MB
        idx = np.arange(n, dtype=np.uint64)
        self.frames, self.counts = zeros(n * CAP * 32), torch.zeros(n, dtype=torch.int64, device="cuda")
        self.dcar, self.mcar, self.rcar, self.hcar = zeros(64 * n), zeros(64 * n), zeros(32 * n), zeros(32 * n)
        self.recs, self.vrecs = zeros(n * MCAP * 40), zeros(n * MCAP * 40)
        self.mres, self.rres, self.bres, self.hres, self.vres, self.jres = (zeros(32 * n) for _ in range(6))
        self.view, self.rrres, self.brres = zeros(64 * n), zeros(32 * R), zeros(32 * R)
        self.AREA = HOLD_CAP + stride
        self.areas = zeros(n * self.AREA)
        self.logs, self.bcar = zeros(R * LOG_CAP), zeros(192 * R)
        tab = np.zeros((n, 8), np.uint64)
        tab[:, 0], tab[:, 2] = recv.data_ptr() + stride * idx, self.dcar.data_ptr() + 64 * idx
        tab[:, 3], tab[:, 4] = self.frames.data_ptr() + 32 * CAP * idx, CAP
        self.tab = tab
        mtab = np.zeros((n, 8), np.uint64)
        mtab[:, 0], mtab[:, 1] = self.areas.data_ptr() + self.AREA * idx + HOLD_CAP, stride
        mtab[:, 2], mtab[:, 3], mtab[:, 4] = self.mcar.data_ptr() + 64 * idx, self.recs.data_ptr() + 40 * MCAP * idx, MCAP
        htab = np.zeros((n, 4), np.uint64)
        htab[:, 0], htab[:, 1] = HOLD_CAP, self.hcar.data_ptr() + 32 * idx
        htab[:, 2], htab[:, 3] = self.vrecs.data_ptr() + 40 * MCAP * idx, MCAP
        rtab = np.zeros((n, 4), np.uint64)
        rtab[:, 0], rtab[:, 1], rtab[:, 2] = sends.data_ptr() + soff, own, self.rcar.data_ptr() + 32 * idx
        btab = np.zeros((n, 8), np.uint64)
        btab[:, 0], btab[:, 1] = heads_t.data_ptr() + HEAD * idx, HEAD
        btab[:, 2], btab[:, 3] = sends.data_ptr() + soff, own
        btab[:, 4], btab[:, 5] = self.rres.data_ptr() + 32 * idx, idx // MB
        roomtab = np.zeros((R, 4), np.uint64)
        ridx = np.arange(R, dtype=np.uint64)
        roomtab[:, 0], roomtab[:, 1] = members.data_ptr() + 4 * MB * ridx, MB
        roomtab[:, 2], roomtab[:, 3] = wires.data_ptr() + woff, wlen
        brtab = np.zeros((R, 4), np.uint64)
        brtab[:, 0], brtab[:, 1] = self.logs.data_ptr() + LOG_CAP * ridx, LOG_CAP
        brtab[:, 2], brtab[:, 3] = self.bcar.data_ptr() + 192 * ridx, KEEP
        jtab = np.zeros((n, 8), np.uint64)
        jtab[:, 0], jtab[:, 1] = sends.data_ptr() + soff, own
        jtab[:, 2], jtab[:, 3] = self.bres.data_ptr() + 32 * idx, self.rres.data_ptr() + 32 * idx
        jtab[:, 4] = idx // MB
        if join is not None:
            jtab[join, 4] |= np.uint64(_lib.BL_JOIN << 32)
        self.mtab_t, self.htab_t, self.rtab_t, self.btab_t, self.roomtab_t, self.brtab_t, self.jtab_t = (
            dev(t) for t in (mtab, htab, rtab, btab, roomtab, brtab, jtab))
        self.R = R

    def table_for(self, lens):
        t = self.tab.copy()
        t[:, 1] = lens
        return dev(t)

    def five(self, recv, stage, ctab):
        """recv restore, decode, reassemble, hold, reply, broadcast on the view."""
        recv.copy_(stage, non_blocking=True)
        _lib.check(L.xyws_decode_streams(ctx.h, vp(ctab), self.n, vp(self.counts), 0, sp))
        _lib.check(L.xyws_reassemble_streams(ctx.h, vp(ctab), vp(self.counts), vp(self.mtab_t), self.n, _lib.REASM_UTF8,
                                             vp(self.mres), sp))
        _lib.check(L.xyws_hold_streams(ctx.h, vp(self.mtab_t), vp(self.mres), vp(self.htab_t), self.n, vp(self.view),
                                       vp(self.vres), vp(self.hres), sp))
        _lib.check(L.xyws_reply_streams(ctx.h, vp(ctab), vp(self.counts), vp(self.rtab_t), self.n, 1 << 20,
                                        _lib.POL_FRAGMENTS, 0, _lib.ENC_FRAME_OPCODE, 1 << _lib.ACT_PING,
                                        vp(self.rres), sp))
        _lib.check(L.xyws_broadcast_streams(ctx.h, vp(self.view), vp(self.vres), vp(self.btab_t), self.n,
                                            vp(self.roomtab_t), vp(self.rrres), self.R, 0x11, 0, vp(self.bres), sp))

    def backlog(self):
        _lib.check(L.xyws_backlog_streams(ctx.h, vp(self.view), vp(self.vres), vp(self.btab_t), self.n,
                                          vp(self.roomtab_t), vp(self.rrres), vp(self.brtab_t), vp(self.brres), self.R,
                                          vp(self.jtab_t), vp(self.jres), sp))


rows = []
for cell in args.cells.split(","):
    n, MB = (int(x) for x in cell.split(":"))
    assert n % MB == 0 and MB >= KEEP
    R = n // MB
    idx = np.arange(n, dtype=np.uint64)
    heads = [("[%021d] " % i).encode() for i in range(n)]
    heads_t = dev(np.frombuffer(b"".join(heads), np.uint8))
    members = dev(np.arange(n, dtype=np.uint32))
    rng = streams.SplitMix(0xB10C + n + MB)
    lens = [40 + rng.next() % 161 for _ in range(n)]
    msgs = [text(ln, i) for i, ln in enumerate(lens)]
    steady = [frame(rng, 0x81, m) for m in msgs]
    stride = (max(len(p) for p in steady) + 15) // 16 * 16
    img = np.zeros(n * stride, np.uint8)
    for i, p in enumerate(steady):
        img[stride * i:stride * i + len(p)] = np.frombuffer(p, np.uint8)
    stage, slens = dev(img), np.asarray([len(p) for p in steady], np.uint64)
    recv = zeros(n * stride)
    flen = np.asarray([len(hdr(HEAD + ln)) + HEAD + ln for ln in lens], np.uint64)
    wlen = flen.reshape(R, MB).sum(axis=1)
    woff = np.concatenate([[0], np.cumsum(wlen)[:-1]]).astype(np.uint64)
    blen = flen.reshape(R, MB)[:, MB - KEEP:].sum(axis=1)  # a room's backlog: its last KEEP frames
    own = np.repeat(wlen + blen, MB)                        # a send range: the wire, then room for the backlog
    soff = np.concatenate([[0], np.cumsum(own)[:-1]]).astype(np.uint64)
    out_bytes = int(np.repeat(wlen, MB).sum())
    sends, wires = zeros(int(own.sum())), zeros(int(wlen.sum()))
    join = np.arange(0, n, 4)
    common = (n, MB, stride, recv, sends, own, soff, heads_t, wires, wlen, woff, members)
    six, five, storm, host = Variant(*common), Variant(*common), Variant(*common, join=join), Variant(*common)
    ctabs = {v: v.table_for(slens) for v in (six, five, storm, host)}

    def six_call():
        six.five(recv, stage, ctabs[six])
        six.backlog()

    def five_call():
        five.five(recv, stage, ctabs[five])

    def join_storm():
        storm.five(recv, stage, ctabs[storm])
        storm.backlog()

    # the host path: pinned landing areas, every room's backlog on the host, the gather that keeps it
    h_wires = torch.zeros(int(wlen.sum()), dtype=torch.uint8).pin_memory()
    h_rr = torch.zeros(32 * R, dtype=torch.uint8).pin_memory()
    boff = np.concatenate([[0], np.cumsum(blen)[:-1]]).astype(np.int64)
    h_bl = torch.zeros(int(blen.sum()), dtype=torch.uint8).pin_memory()
    d_bl = zeros(int(blen.sum()))
    gather = np.concatenate([np.arange(int(woff[r] + wlen[r] - blen[r]), int(woff[r] + wlen[r])) for r in range(R)])
    jdst = [sends[int(soff[i] + wlen[i // MB]):int(soff[i] + wlen[i // MB] + blen[i // MB])] for i in join]
    jsrc = [d_bl[int(boff[i // MB]):int(boff[i // MB] + blen[i // MB])] for i in join]

    def host_path():
        host.five(recv, stage, ctabs[host])
        h_wires.copy_(wires, non_blocking=True)
        h_rr.copy_(host.rrres, non_blocking=True)
        torch.cuda.synchronize()
        np.take(h_wires.numpy(), gather, out=h_bl.numpy())  # the newest KEEP frames of every room
        d_bl.copy_(h_bl, non_blocking=True)
        for dst, src in zip(jdst, jsrc):
            dst.copy_(src, non_blocking=True)

    # ---- checks, before anything is timed
    want0 = b"".join(hdr(HEAD + lens[i]) + heads[i] + msgs[i] for i in range(MB))
    back0 = want0[len(want0) - int(blen[0]):]
    for v, fn in ((six, six_call), (storm, join_storm)):
        fn()
        torch.cuda.synchronize()
        assert wires[:int(wlen[0])].cpu().numpy().tobytes() == want0, "room 0's wire"
        br = v.brres.view(torch.int64).reshape(R, 4).cpu().numpy()
        assert (br[:, 0] == blen.astype(np.int64)).all() and ((br[:, 1] & 0xFFFFFFFF) == KEEP).all(), "backlog rows"
        assert ((br[:, 2] >> 32) == 0).all(), "backlog status"
        car = v.bcar.view(torch.int64).reshape(R, 24).cpu().numpy()
        s0 = int(car[0, 0])
        assert v.logs[s0:s0 + int(blen[0])].cpu().numpy().tobytes() == back0, "room 0's log"
    jr = storm.jres.view(torch.int64).reshape(n, 4).cpu().numpy()
    assert (jr[join, 2] == _lib.BLC_JOINED).all() and (jr[1::4, 2] == 0).all(), "joiners' rows"
    a = int(soff[0] + wlen[0])
    assert sends[a:a + int(blen[0])].cpu().numpy().tobytes() == back0, "a joiner's backlog bytes"
    sends.zero_()
    host_path()
    torch.cuda.synchronize()
    assert sends[a:a + int(blen[0])].cpu().numpy().tobytes() == back0, "the host path's backlog bytes"
    assert sends[int(soff[0]):a].cpu().numpy().tobytes() == want0, "the host path's wire"

    modes = {"backlog_call": six.backlog}
    if not args.fold_only:
        modes.update({"six_call": six_call, "five_call": five_call, "join_storm": join_storm, "host_path": host_path})
    for fn in modes.values():
        fn()
        fn()
    torch.cuda.synchronize()
    la = max(20, min(200, int(4e9 // max(out_bytes, 1))))
    loops = {"six_call": la, "five_call": la, "join_storm": la, "backlog_call": 200, "host_path": max(5, la // 4)}
    t = {name: [] for name in modes}
    for _ in range(args.repeats):
        for name, fn in modes.items():  # (alternated: each repeat times every variant)
            t[name].append(timed(fn, loops[name]))
    row = {"connections": n, "rooms": R, "members": MB, "keep": KEEP, "log_cap": LOG_CAP, "joiners": int(len(join)),
           "recv_bytes": int(slens.sum()), "send_bytes_five_call": out_bytes, "backlog_bytes": int(blen.sum()),
           "repeats": args.repeats, "loops": {k: loops[k] for k in modes}}
    if args.tag:
        row["tag"] = args.tag
    for name in modes:
        row[name] = summary(t[name])
    row["backlog_call_ns_per_room"] = round(1e3 * row["backlog_call"]["median_us"] / R, 2)
    if not args.fold_only:
        row["six_minus_five_us"] = round(row["six_call"]["median_us"] - row["five_call"]["median_us"], 2)
        row["six_over_five"] = round(row["six_call"]["median_us"] / row["five_call"]["median_us"], 3)
        row["host_over_storm"] = round(row["host_path"]["median_us"] / row["join_storm"]["median_us"], 2)
        row["host_over_storm_worst"] = round(row["host_path"]["min_us"] / row["join_storm"]["max_us"], 2)
        row["storm_beats_host_beyond_spread"] = row["join_storm"]["max_us"] < row["host_path"]["min_us"]
    rows.append(row)
    print(json.dumps(row), flush=True)
    del six, five, storm, host, ctabs, stage, recv, sends, wires, h_wires, h_bl, d_bl, jdst, jsrc
    torch.cuda.empty_cache()

assert ctx.last_device_error() == 0
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a" if args.append else "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")

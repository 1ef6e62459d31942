"""What delivering the messages that span sweeps costs (profiles/hold_rate.jsonl).

For 1 024 and 16 384 connections in rooms of 16, two kinds of sweep:
  none  every connection sends one whole masked text message of 40-200 bytes:
        nothing spans, the hold call only writes the view (the cost of the
        extra launch in the common sweep);
  all   every connection's recv bytes are the last fragment (2 KiB) of one
        message and the first fragment (2 KiB) of the next: each sweep carries
        a 2 KiB part in and a 2 KiB part out, and delivers a 4 KiB message per
        connection.
Measured per cell:
  (a) hold_call: xyws_hold_streams alone on the tables one reassembly wrote
      (the hold carries chain from call to call, so every call of `all`
      appends, delivers and begins again);
  (b) five_call: recv restore (one device copy, the decode unmasks in place),
      decode, reassemble, hold, reply, broadcast on the view;
  (c) four_call: the same without the hold call, the broadcast fed the
      reassembly's own table: the sweep as it was before the hold call
      existed (in `all` it delivers nothing);
  (d) host_path (`all` only): what a caller did instead: the four-call sweep,
      D2H of rows, records and message bytes, the append on the host (ONE
      vectorised numpy copy for all connections: a lower bound for a loop of
      per-connection appends), H2D of the assembled messages and their
      records, and a second broadcast of them.
Each variant has decode, message, reply and hold carries of its own and is
primed with the sweep that opens the first message. Before anything is timed
the five-call sweep's room results and room 0's wire are checked against the
host's, and the host path's second broadcast against the five-call wire. The
variants are alternated in one process after a warm-up, each timed by device
events around a loop that ends in a synchronise (the events span the host
path's host work too: the stream waits for it); every cell is repeated and
reports median and range.

usage: hold_rate.py [--out FILE] [--repeats R] [--cells N,N,...]
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hold_rate.jsonl"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--cells", default="1024,16384")
args = ap.parse_args()
assert args.repeats >= 5, "the spread needs at least 5 repeats"
assert torch.cuda.is_available(), "hold_rate.py measures on the GPU: no device, no number"

ctx = ws.Context(0)
L = ctx.L
stream = torch.cuda.current_stream()
sp = C.c_void_p(stream.cuda_stream)
HEAD, MB, PART = 24, 16, 2048
HOLD_CAP = 2 * (2 * PART) + 30
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
    """One sweep pipeline with carries, tables and result rows of its own.
    hold_cap: the bytes in front of every connection's reassembly range (0:
    the layout without a hold)."""

    def __init__(self, n, stride, recv, sends, own, soff, heads_t, wires, wlen, woff, members, hold_cap=HOLD_CAP):
        self.n, R, self.hold_cap = n, n // MB, hold_cap
        idx = np.arange(n, dtype=np.uint64)
        self.frames, self.counts = zeros(n * CAP * 32), torch.zeros(n, dtype=torch.int64, device="cuda")
        self.dcar, self.mcar, self.rcar, self.hcar = zeros(64 * n), zeros(64 * n), zeros(32 * n), zeros(32 * n)
        self.recs, self.vrecs = zeros(n * MCAP * 40), zeros(n * MCAP * 40)
        self.mres, self.rres, self.bres, self.hres, self.vres = (zeros(32 * n) for _ in range(5))
        self.view, self.rrres = zeros(64 * n), zeros(32 * R)
        self.AREA = hold_cap + stride
        self.areas = zeros(n * self.AREA)
        tab = np.zeros((n, 8), np.uint64)
        tab[:, 0], tab[:, 2] = recv.data_ptr() + stride * idx, self.dcar.data_ptr() + 64 * idx
        tab[:, 3], tab[:, 4] = self.frames.data_ptr() + 32 * CAP * idx, CAP
        self.tab = tab
        mtab = np.zeros((n, 8), np.uint64)
        mtab[:, 0], mtab[:, 1] = self.areas.data_ptr() + self.AREA * idx + hold_cap, stride
        mtab[:, 2], mtab[:, 3], mtab[:, 4] = self.mcar.data_ptr() + 64 * idx, self.recs.data_ptr() + 40 * MCAP * idx, MCAP
        htab = np.zeros((n, 4), np.uint64)
        htab[:, 0], htab[:, 1] = hold_cap, self.hcar.data_ptr() + 32 * idx
        htab[:, 2], htab[:, 3] = self.vrecs.data_ptr() + 40 * MCAP * idx, MCAP
        rtab = np.zeros((n, 4), np.uint64)
        rtab[:, 0], rtab[:, 1], rtab[:, 2] = sends.data_ptr() + soff, own, self.rcar.data_ptr() + 32 * idx
        btab = np.zeros((n, 8), np.uint64)
        btab[:, 0], btab[:, 1] = heads_t.data_ptr() + HEAD * idx, HEAD
        btab[:, 2], btab[:, 3] = sends.data_ptr() + soff, own
        btab[:, 4], btab[:, 5] = self.rres.data_ptr() + 32 * idx, idx // MB
        roomtab = np.zeros((R, 4), np.uint64)
        roomtab[:, 0], roomtab[:, 1] = members.data_ptr() + 4 * MB * np.arange(R, dtype=np.uint64), MB
        roomtab[:, 2], roomtab[:, 3] = wires.data_ptr() + woff, wlen
        self.mtab_t, self.htab_t, self.rtab_t, self.btab_t, self.roomtab_t = (dev(t) for t in (mtab, htab, rtab, btab,
                                                                                              roomtab))
        self.R = R

    def table_for(self, lens):
        t = self.tab.copy()
        t[:, 1] = lens
        return dev(t)

    def front(self, recv, stage, ctab):
        """recv restore, decode, reassemble."""
        recv.copy_(stage, non_blocking=True)
        _lib.check(L.xyws_decode_streams(ctx.h, vp(ctab), self.n, vp(self.counts), 0, sp))
        _lib.check(L.xyws_reassemble_streams(ctx.h, vp(ctab), vp(self.counts), vp(self.mtab_t), self.n, _lib.REASM_UTF8,
                                             vp(self.mres), sp))

    def hold(self):
        _lib.check(L.xyws_hold_streams(ctx.h, vp(self.mtab_t), vp(self.mres), vp(self.htab_t), self.n, vp(self.view),
                                       vp(self.vres), vp(self.hres), sp))

    def back(self, ctab, viewed):
        """reply, broadcast (on the view or on the reassembly's own table)."""
        _lib.check(L.xyws_reply_streams(ctx.h, vp(ctab), vp(self.counts), vp(self.rtab_t), self.n, 1 << 20,
                                        _lib.POL_FRAGMENTS, 0, _lib.ENC_FRAME_OPCODE, 1 << _lib.ACT_PING,
                                        vp(self.rres), sp))
        tab, rows = (self.view, self.vres) if viewed else (self.mtab_t, self.mres)
        _lib.check(L.xyws_broadcast_streams(ctx.h, vp(tab), vp(rows), vp(self.btab_t), self.n, vp(self.roomtab_t),
                                            vp(self.rrres), self.R, 0x11, 0, vp(self.bres), sp))


rows = []
for n in (int(x) for x in args.cells.split(",")):
    assert n % MB == 0
    R = n // MB
    idx = np.arange(n, dtype=np.uint64)
    heads = [("[%021d] " % i).encode() for i in range(n)]
    heads_t = dev(np.frombuffer(b"".join(heads), np.uint8))
    members = dev(np.arange(n, dtype=np.uint32))
    for kind in ("none", "all"):
        rng = streams.SplitMix(0x401D + n + len(kind))
        if kind == "none":
            lens = [40 + rng.next() % 161 for _ in range(n)]
            msgs = [text(ln, i) for i, ln in enumerate(lens)]
            steady = [frame(rng, 0x81, m) for m in msgs]
            prime = None
        else:
            lens = [2 * PART] * n
            a = [text(PART, i, 0x41) for i in range(n)]  # the part that goes out (and comes in)
            b = [text(PART, 3 * i) for i in range(n)]  # the part that completes it
            msgs = [x + y for x, y in zip(a, b)]
            steady = [frame(rng, 0x80, y) + frame(rng, 0x01, x) for x, y in zip(a, b)]
            prime = [frame(rng, 0x01, x) for x in a]
        stride = (max(len(p) for p in steady) + 15) // 16 * 16

        def slab(pieces):
            img = np.zeros(n * stride, np.uint8)
            for i, p in enumerate(pieces):
                img[stride * i:stride * i + len(p)] = np.frombuffer(p, np.uint8)
            return dev(img), np.asarray([len(p) for p in pieces], np.uint64)

        stage, slens = slab(steady)
        recv = zeros(n * stride)
        flen = np.asarray([len(hdr(HEAD + ln)) + HEAD + ln for ln in lens], np.uint64)
        wlen = flen.reshape(R, MB).sum(axis=1)
        woff = np.concatenate([[0], np.cumsum(wlen)[:-1]]).astype(np.uint64)
        own = np.repeat(wlen, MB)
        soff = np.concatenate([[0], np.cumsum(own)[:-1]]).astype(np.uint64)
        out_bytes = int(own.sum())
        sends, wires = zeros(out_bytes), zeros(int(wlen.sum()))
        common = (n, stride, recv, sends, own, soff, heads_t, wires, wlen, woff, members)
        five, four, host = Variant(*common), Variant(*common, hold_cap=0), Variant(*common, hold_cap=0)
        ctabs = {v: v.table_for(slens) for v in (five, four, host)}
        if prime is not None:
            pstage, plens = slab(prime)
            for v in (five, four, host):
                pt = v.table_for(plens)
                v.front(recv, pstage, pt)
                if v is five:
                    v.hold()
                v.back(pt, v is five)
            torch.cuda.synchronize()
            st = five.hres.view(torch.int64).reshape(n, 4)[:, 2].cpu().numpy()
            assert (st == _lib.HOLD_ACTIVE).all(), "the priming sweep must leave every connection holding"

        def five_call():
            five.front(recv, stage, ctabs[five])
            five.hold()
            five.back(ctabs[five], True)

        def four_call():
            four.front(recv, stage, ctabs[four])
            four.back(ctabs[four], False)

        # the host path: pinned landing areas, the host's held parts, the assembled messages
        h_rows = torch.zeros(32 * n, dtype=torch.uint8).pin_memory()
        h_recs = torch.zeros(40 * MCAP * n, dtype=torch.uint8).pin_memory()
        h_out = torch.zeros(n * host.AREA, dtype=torch.uint8).pin_memory()
        h_asm = torch.zeros(n * 2 * PART, dtype=torch.uint8).pin_memory()
        held = np.zeros((n, PART), np.uint8)
        if kind == "all":
            for i in range(n):
                held[i] = np.frombuffer(a[i], np.uint8)
            asm = zeros(n * 2 * PART)
            arec = np.zeros((n, 5), np.uint64)
            arec[:, 1], arec[:, 3], arec[:, 4] = 2, 2 * PART, _lib.MSG_COMPLETE | (1 << 32)
            h_arecs = torch.from_numpy(arec.reshape(-1).view(np.uint8).copy()).pin_memory()
            arecs = zeros(40 * n)
            atab = np.zeros((n, 8), np.uint64)
            atab[:, 0], atab[:, 1] = asm.data_ptr() + 2 * PART * idx, 2 * PART
            atab[:, 3], atab[:, 4] = arecs.data_ptr() + 40 * idx, 1
            ares = np.zeros((n, 4), np.uint64)
            ares[:, 0], ares[:, 1], ares[:, 2] = 2 * PART, 1, 1
            atab_t, ares_t = dev(atab), dev(ares)
            btab2 = np.zeros((n, 8), np.uint64)
            btab2[:, 0], btab2[:, 1] = heads_t.data_ptr() + HEAD * idx, HEAD
            btab2[:, 2], btab2[:, 3], btab2[:, 5] = sends.data_ptr() + soff, own, idx // MB
            btab2_t = dev(btab2)

        def host_path():
            host.front(recv, stage, ctabs[host])
            host.back(ctabs[host], False)
            h_rows.copy_(host.mres, non_blocking=True)
            h_recs.copy_(host.recs, non_blocking=True)
            h_out.copy_(host.areas, non_blocking=True)
            torch.cuda.synchronize()
            out = h_out.numpy().reshape(n, host.AREA)
            m = h_asm.numpy().reshape(n, 2 * PART)
            m[:, :PART] = held
            m[:, PART:] = out[:, :PART]              # record 0: CONTINUED | COMPLETE at out_off 0
            held[:] = out[:, PART:2 * PART]          # the last record: open, at out_off PART
            asm.copy_(h_asm, non_blocking=True)
            arecs.copy_(h_arecs, non_blocking=True)
            _lib.check(L.xyws_broadcast_streams(ctx.h, vp(atab_t), vp(ares_t), vp(btab2_t), n, vp(host.roomtab_t),
                                                vp(host.rrres), R, 0x11, 0, vp(host.bres), sp))

        # ---- checks, before anything is timed
        five_call()
        torch.cuda.synchronize()
        rr = five.rrres.view(torch.int64).reshape(R, 4).cpu().numpy()
        assert (rr[:, 0] == wlen.astype(np.int64)).all(), "five-call wire lengths"
        assert ((rr[:, 1] & 0xFFFFFFFF) == MB).all(), "every member's message on the wire"
        want0 = b"".join(hdr(HEAD + lens[i]) + heads[i] + msgs[i] for i in range(MB))
        wire0 = wires[:int(wlen[0])].cpu().numpy().tobytes()
        assert wire0 == want0, "room 0's wire"
        st = five.hres.view(torch.int64).reshape(n, 4)[:, 2].cpu().numpy()
        assert (st == (0 if kind == "none" else _lib.HOLD_DELIVERED | _lib.HOLD_ACTIVE)).all(), "hold results"
        four_call()
        torch.cuda.synchronize()
        rr = four.rrres.view(torch.int64).reshape(R, 4).cpu().numpy()
        assert ((rr[:, 1] & 0xFFFFFFFF) == (MB if kind == "none" else 0)).all(), "the four-call sweep delivers whole messages only"
        modes = {"five_call": five_call, "four_call": four_call, "hold_call": five.hold}
        if kind == "all":
            wires.zero_()
            host_path()
            torch.cuda.synchronize()
            assert wires[:int(wlen[0])].cpu().numpy().tobytes() == want0, "the host path's wire"
            modes["host_path"] = host_path
        for fn in modes.values():
            fn()
            fn()
        torch.cuda.synchronize()
        la = max(20, min(200, int(4e9 // max(out_bytes, 1))))
        loops = {"five_call": la, "four_call": la, "hold_call": 200, "host_path": max(10, la // 4)}
        t = {name: [] for name in modes}
        for _ in range(args.repeats):
            for name, fn in modes.items():  # (alternated: each repeat times every variant)
                t[name].append(timed(fn, loops[name]))
        row = {"connections": n, "kind": kind, "rooms": R, "members": MB, "recv_bytes": int(slens.sum()),
               "send_bytes_five_call": out_bytes, "hold_cap": HOLD_CAP, "repeats": args.repeats,
               "loops": {k: loops[k] for k in modes}}
        for name in modes:
            row[name] = summary(t[name])
        row["hold_call_ns_per_connection"] = round(1e3 * row["hold_call"]["median_us"] / n, 2)
        row["five_minus_four_us"] = round(row["five_call"]["median_us"] - row["four_call"]["median_us"], 2)
        row["five_over_four"] = round(row["five_call"]["median_us"] / row["four_call"]["median_us"], 3)
        if kind == "all":
            row["hold_GBps_copied"] = round(2 * PART * n / row["hold_call"]["median_us"] / 1e3, 2)
            row["host_over_five"] = round(row["host_path"]["median_us"] / row["five_call"]["median_us"], 2)
            row["host_over_five_worst"] = round(row["host_path"]["min_us"] / row["five_call"]["max_us"], 2)
            row["host_over_five_best"] = round(row["host_path"]["max_us"] / row["five_call"]["min_us"], 2)
            row["five_beats_host_beyond_spread"] = row["five_call"]["max_us"] < row["host_path"]["min_us"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del five, four, host, ctabs, stage, recv, sends, wires, h_rows, h_recs, h_out, h_asm
        torch.cuda.empty_cache()

assert ctx.last_device_error() == 0
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")

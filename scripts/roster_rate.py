"""What keeping each room's member list on the device costs (profiles/roster_rate.jsonl).

Cells: 1 024 and 16 384 connections in rooms of 16 (the shapes of
profiles/backlog_rate.jsonl). Every connection sends one whole masked text
message of 40-200 bytes per sweep. Measured per cell, in one process on one
device:
  (a) seven_call: recv restore (one device copy, the decode unmasks in place),
      decode, reassemble, hold, reply, broadcast, roster, backlog, with no
      event, against six_call, the same sweep without the roster call (the
      sweep as it was before the call existed: the same library, on the
      assumption that the six existing calls compile to the same code as in
      the parent commit, whose sources they share unchanged); roster_call is
      the call alone on the tables one broadcast wrote;
  (b) join_storm: the seven-call sweep in which a quarter of the connections
      complete their handshake and join (XYWS_RS_JOIN_ON_ACCEPT, four per
      room), and leave_storm, in which the same quarter closes and leaves
      (XYWS_RS_LEAVE_ON_CLOSE): the two alternate, so the lists return to
      where they began. Against host_join / host_leave, what a caller did
      instead: the six-call sweep, D2H of the accept (or reply) rows, the
      lists rebuilt on the host (vectorised numpy over fixed-size rooms: a
      lower bound for a set per room), the notices composed on the host (one
      numpy fill, all names 21 bytes), H2D of lists and notice bytes, and one
      device copy per recipient.
  (c) the room pass's O(n) joiner scan: the call alone at 1 024 rooms of 1, 4
      and 16 connections, with and without rooms (n_rooms = 0 leaves the events
      and the delivery, but also changes them: every connection is then
      NO_ROOM and the delivery's grid writes rows only). The difference stands
      for the room pass; a line through the three differences gives the part
      that grows with n: the scan's share at 16 384, an estimate from a fit,
      not a counter.
Before anything is timed the lists, a notice wire and a joiner's send bytes
are checked. The variants are alternated in one process after a warm-up, each
timed by device events around a loop that ends in a synchronise; every cell is
repeated and reports median and range.

usage: roster_rate.py [--out FILE] [--repeats R] [--cells N:M,...] [--no-fit]
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roster_rate.jsonl"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--cells", default="1024:16,16384:16")
ap.add_argument("--no-fit", action="store_true")
args = ap.parse_args()
assert args.repeats >= 5, "the spread needs at least 5 repeats"
assert torch.cuda.is_available(), "roster_rate.py measures on the GPU: no device, no number"

ctx = ws.Context(0)
L = ctx.L
stream = torch.cuda.current_stream()
sp = C.c_void_p(stream.cuda_stream)
HEAD, KEEP, NAME = 24, 10, 21
FRAME_MAX = 4 + HEAD + 200
LOG_CAP = 2 * KEEP * FRAME_MAX + 30
HOLD_CAP = 2 * 256 + 30
CAP = MCAP = 4
T_HEAD, T_JOIN, T_LEFT = b"|        SERVER       |:", b" has joined the chat\n", b" has left the chat\n"
WELCOME, FAREWELL = 2 + len(T_HEAD) + NAME + len(T_JOIN), 2 + len(T_HEAD) + NAME + len(T_LEFT)
RESP = 129


def vp(t, off=0):
    return C.c_void_p(t.data_ptr() + off) if t is not None else None


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def zeros(nbytes):
    return torch.zeros(max(nbytes, 1), dtype=torch.uint8, device="cuda")


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
    """One sweep pipeline with carries, tables, result rows, logs, lists and
    notice buffers of its own. present: which connections the lists hold at
    the start; asks: per roster table name the (rows, flags) of the quarter."""

    def __init__(self, n, MB, stride, recv, sends, own, soff, heads_t, names_t, wires, wlen, woff, present, quarter=None):
        self.n, R = n, n // MB
        self.R, self.MB = R, MB
        idx = np.arange(n, dtype=np.uint64)
        ridx = np.arange(R, dtype=np.uint64)
        self.frames, self.counts = zeros(n * CAP * 32), torch.zeros(n, dtype=torch.int64, device="cuda")
        self.dcar, self.mcar, self.rcar, self.hcar = zeros(64 * n), zeros(64 * n), zeros(32 * n), zeros(32 * n)
        self.recs, self.vrecs = zeros(n * MCAP * 40), zeros(n * MCAP * 40)
        self.mres, self.rres, self.bres, self.hres, self.vres, self.jres, self.sres = (zeros(32 * n) for _ in range(7))
        self.view, self.rrres, self.brres, self.srres = zeros(64 * n), zeros(32 * R), zeros(32 * R), zeros(32 * R)
        self.AREA = HOLD_CAP + stride
        self.areas = zeros(n * self.AREA)
        self.logs, self.bcar = zeros(R * LOG_CAP), zeros(192 * R)
        self.NOTES = MB * max(WELCOME, FAREWELL)
        self.notes, self.want = zeros(R * self.NOTES), zeros(4 * n)
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
        # the resident tables: the lists (ascending inside each room), the counts, every connection's room
        lists = np.full((R, MB), 0xFFFFFFFF, np.uint32)
        pres = present.reshape(R, MB)
        counts = pres.sum(axis=1).astype(np.uint64)
        for r in range(R):
            lists[r, :int(counts[r])] = np.nonzero(pres[r])[0] + r * MB
        self.members = dev(lists)
        btab = np.zeros((n, 8), np.uint64)
        btab[:, 0], btab[:, 1] = heads_t.data_ptr() + HEAD * idx, HEAD
        btab[:, 2], btab[:, 3] = sends.data_ptr() + soff, own
        btab[:, 4], btab[:, 5] = self.rres.data_ptr() + 32 * idx, np.where(present, idx // MB, 0xFFFFFFFF)
        roomtab = np.zeros((R, 4), np.uint64)
        roomtab[:, 0], roomtab[:, 1] = self.members.data_ptr() + 4 * MB * ridx, counts
        roomtab[:, 2], roomtab[:, 3] = wires.data_ptr() + woff, wlen
        brtab = np.zeros((R, 4), np.uint64)
        brtab[:, 0], brtab[:, 1] = self.logs.data_ptr() + LOG_CAP * ridx, LOG_CAP
        brtab[:, 2], brtab[:, 3] = self.bcar.data_ptr() + 192 * ridx, KEEP
        # the `seen` rows: the lists as the broadcast read them, which the backlog behind a roster folds
        self.seen_members = zeros(4 * n)
        seentab = roomtab.copy()
        seentab[:, 0], seentab[:, 1] = self.seen_members.data_ptr() + 4 * MB * ridx, 0
        self.seentab_t = dev(seentab)
        rrtab = np.zeros((R, 4), np.uint64)
        rrtab[:, 0], rrtab[:, 1], rrtab[:, 2] = MB, self.notes.data_ptr() + self.NOTES * ridx, self.NOTES
        rrtab[:, 3] = self.seentab_t.data_ptr() + 32 * ridx
        # the backlog's table: behind the roster's rows when there is a roster call, behind the broadcast's else
        jtab = np.zeros((n, 8), np.uint64)
        jtab[:, 0], jtab[:, 1] = sends.data_ptr() + soff, own
        jtab[:, 2], jtab[:, 3] = self.bres.data_ptr() + 32 * idx, self.rres.data_ptr() + 32 * idx
        jtab[:, 4] = 0xFFFFFFFF
        jtab_r = jtab.copy()
        jtab_r[:, 2] = self.sres.data_ptr() + 32 * idx
        # the roster's tables: no event; the quarter joins on accept; the quarter leaves on close
        # (rows that stand for the accept call's and for a closing sweep's reply rows: every fourth connection's)
        acc = np.zeros((n, 8), np.uint32)
        acc[::4, 0], acc[::4, 1], acc[::4, 3] = _lib.ACC_ACCEPTED, 101, RESP
        closed = np.zeros((n, 4), np.uint64)
        closed[:, 1] = np.uint64(_lib.NPOS)
        closed[::4, 2] = np.uint64(_lib.RPL_CLOSED) << np.uint64(48)
        self.acc_t, self.closed_t = dev(acc), dev(closed)
        rc = np.zeros((n, 8), np.uint64)
        rc[:, 0], rc[:, 1] = names_t.data_ptr() + NAME * idx, NAME
        rc[:, 2], rc[:, 3] = sends.data_ptr() + soff, own
        rc[:, 4], rc[:, 5] = self.bres.data_ptr() + 32 * idx, self.rres.data_ptr() + 32 * idx
        rc[:, 7] = 0xFFFFFFFF | (_lib.RS_LEAVE_ON_CLOSE << 32)
        self.rconns = {"idle": dev(rc)}
        if quarter is not None:
            rj, rl = rc.copy(), rc.copy()
            rj[quarter, 4], rj[quarter, 5] = 0, 0
            rj[quarter, 6] = self.acc_t.data_ptr() + 32 * idx[quarter]
            rj[quarter, 7] = (idx[quarter] // MB) | np.uint64(_lib.RS_JOIN_ON_ACCEPT << 32)
            rl[quarter, 5] = self.closed_t.data_ptr() + 32 * idx[quarter]
            self.rconns.update(join=dev(rj), leave=dev(rl))
        self.mtab_t, self.htab_t, self.rtab_t, self.btab_t, self.roomtab_t, self.brtab_t, self.jtab_t, self.jtab_r, \
            self.rrtab_t = (dev(t) for t in (mtab, htab, rtab, btab, roomtab, brtab, jtab, jtab_r, rrtab))

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

    def roster(self, which="idle", n_rooms=None):
        _lib.check(L.xyws_roster_streams(ctx.h, vp(self.btab_t), vp(self.rconns[which]), self.n, vp(self.roomtab_t),
                                         vp(self.rrtab_t), vp(self.srres), self.R if n_rooms is None else n_rooms, None,
                                         0x11, vp(self.jtab_r), vp(self.want), vp(self.sres), sp))

    def backlog(self, after_roster):
        _lib.check(L.xyws_backlog_streams(ctx.h, vp(self.view), vp(self.vres), vp(self.btab_t), self.n,
                                          vp(self.seentab_t if after_roster else self.roomtab_t), vp(self.rrres),
                                          vp(self.brtab_t), vp(self.brres), self.R,
                                          vp(self.jtab_r if after_roster else self.jtab_t), vp(self.jres), sp))


def build(n, MB):
    """The buffers every variant of a cell shares."""
    R = n // MB
    heads = [("[%021d] " % i).encode() for i in range(n)]
    names = [b"%021d" % i for i in range(n)]
    rng = streams.SplitMix(0xB10C + n + MB)
    lens = [40 + rng.next() % 161 for _ in range(n)]
    steady = [frame(rng, 0x81, text(ln, i)) for i, ln in enumerate(lens)]
    stride = (max(len(p) for p in steady) + 15) // 16 * 16
    img = np.zeros(n * stride, np.uint8)
    for i, p in enumerate(steady):
        img[stride * i:stride * i + len(p)] = np.frombuffer(p, np.uint8)
    flen = np.asarray([len(hdr(HEAD + ln)) + HEAD + ln for ln in lens], np.uint64)
    wlen = flen.reshape(R, MB).sum(axis=1)
    woff = np.concatenate([[0], np.cumsum(wlen)[:-1]]).astype(np.uint64)
    blen = flen.reshape(R, MB)[:, max(MB - KEEP, 0):].sum(axis=1)
    own = np.repeat(wlen + blen + np.uint64(RESP + MB * max(WELCOME, FAREWELL)), MB)
    soff = np.concatenate([[0], np.cumsum(own)[:-1]]).astype(np.uint64)
    return dict(R=R, stage=dev(img), slens=np.asarray([len(p) for p in steady], np.uint64), recv=zeros(n * stride),
                stride=stride, wlen=wlen, woff=woff, own=own, soff=soff, sends=zeros(int(own.sum())),
                wires=zeros(int(wlen.sum())), heads_t=dev(np.frombuffer(b"".join(heads), np.uint8)),
                names_t=dev(np.frombuffer(b"".join(names), np.uint8)), names=names,
                out_bytes=int(np.repeat(wlen, MB).sum()))


def variant(b, n, MB, present, quarter=None):
    return Variant(n, MB, b["stride"], b["recv"], b["sends"], b["own"], b["soff"], b["heads_t"], b["names_t"], b["wires"],
                   b["wlen"], b["woff"], present, quarter)


rows = []
for cell in args.cells.split(","):
    n, MB = (int(x) for x in cell.split(":"))
    assert n % MB == 0 and MB % 4 == 0
    b = build(n, MB)
    R, recv, stage, sends = b["R"], b["recv"], b["stage"], b["sends"]
    quarter = np.arange(0, n, 4)
    everyone, rest = np.ones(n, bool), np.ones(n, bool)
    rest[quarter] = False
    six, seven, storm, host = variant(b, n, MB, everyone), variant(b, n, MB, everyone), \
        variant(b, n, MB, rest, quarter), variant(b, n, MB, rest)
    ctabs = {v: v.table_for(b["slens"]) for v in (six, seven, storm, host)}

    def six_call():
        six.five(recv, stage, ctabs[six])
        six.backlog(False)

    def seven_call():
        seven.five(recv, stage, ctabs[seven])
        seven.roster()
        seven.backlog(True)

    def storm_sweep(which):
        storm.five(recv, stage, ctabs[storm])
        storm.roster(which)
        storm.backlog(True)

    # the host path: pinned landing areas; lists, counts, rooms and notices rebuilt on the host
    h_rows = torch.zeros(32 * n, dtype=torch.uint8).pin_memory()
    h_lists = torch.zeros(4 * n, dtype=torch.uint8).pin_memory()
    h_counts = torch.zeros(8 * R, dtype=torch.uint8).pin_memory()
    h_room = torch.zeros(8 * n, dtype=torch.uint8).pin_memory()
    PER = len(quarter) // R  # events per room
    h_notes = torch.zeros(R * PER * WELCOME, dtype=torch.uint8).pin_memory()
    d_notes = zeros(R * PER * WELCOME)
    d_counts, d_room = zeros(8 * R), zeros(8 * n)
    names_np = np.frombuffer(b"".join(b["names"]), np.uint8).reshape(n, NAME)
    host_present = rest.copy()

    def host_sweep(join):
        size = WELCOME if join else FAREWELL
        tail = T_JOIN if join else T_LEFT
        host.five(recv, stage, ctabs[host])
        h_rows.copy_(host.acc_t if join else host.closed_t, non_blocking=True)  # the rows that say who comes or goes
        torch.cuda.synchronize()
        raw = h_rows.numpy()
        if join:
            who = np.nonzero(raw.view(np.uint32).reshape(n, 8)[:, 0] & _lib.ACC_ACCEPTED)[0]
            who = who[~host_present[who]]
        else:
            who = np.nonzero((raw.view(np.uint64).reshape(n, 4)[:, 2] >> np.uint64(48)) & np.uint64(_lib.RPL_CLOSED))[0]
            who = who[host_present[who]]
        host_present[who] = join
        pres = host_present.reshape(R, MB)
        flat = np.nonzero(host_present)[0].astype(np.uint32)
        h_lists.numpy().view(np.uint32)[:len(flat)] = flat
        h_counts.numpy().view(np.uint64)[:] = pres.sum(axis=1)
        h_room.numpy().view(np.uint64)[:] = np.where(host_present, np.arange(n) // MB, 0xFFFFFFFF)
        notes = h_notes.numpy()[:len(who) * size].reshape(len(who), size)
        notes[:, 0], notes[:, 1] = 0x81, size - 2
        notes[:, 2:2 + len(T_HEAD)] = np.frombuffer(T_HEAD, np.uint8)
        notes[:, 2 + len(T_HEAD):2 + len(T_HEAD) + NAME] = names_np[who]
        notes[:, 2 + len(T_HEAD) + NAME:] = np.frombuffer(tail, np.uint8)
        host.members[:4 * len(flat)].copy_(h_lists[:4 * len(flat)], non_blocking=True)
        d_counts.copy_(h_counts, non_blocking=True)
        d_room.copy_(h_room, non_blocking=True)
        d_notes[:len(who) * size].copy_(h_notes[:len(who) * size], non_blocking=True)
        # (packed lists: the rooms' pointers would follow the counts; a strided device copy stands for both columns)
        host.roomtab_t.view(torch.int64).view(R, 4)[:, 1].copy_(d_counts.view(torch.int64))
        host.btab_t.view(torch.int64).view(n, 8)[:, 5].copy_(d_room.view(torch.int64))
        for i in np.nonzero(host_present)[0]:  # one device copy per recipient: its room's notices behind its wire
            r = i // MB
            a = int(b["soff"][i] + b["wlen"][r])
            sends[a:a + PER * size].copy_(d_notes[r * PER * size:(r + 1) * PER * size], non_blocking=True)

    # ---- checks, before anything is timed
    seven_call()
    storm_sweep("join")
    torch.cuda.synchronize()
    sr = seven.srres.view(torch.int32).reshape(R, 8).cpu().numpy()
    assert (sr[:, 0] == 0).all() and (sr[:, 6] == MB).all() and (sr[:, 7] == 0).all(), "no event: the lists stay"
    tr = storm.srres.view(torch.int32).reshape(R, 8).cpu().numpy()
    assert (tr[:, 4] == PER).all() and (tr[:, 6] == MB).all() and (tr[:, 7] == 0).all(), "join storm: rows"
    lists = storm.members.view(torch.int32).reshape(R, MB).cpu().numpy()
    assert (np.sort(lists, axis=1) == np.arange(n).reshape(R, MB)).all(), "join storm: every room is whole"
    hi = hdr(WELCOME - 2) + T_HEAD + b["names"][0] + T_JOIN
    assert storm.notes[:WELCOME].cpu().numpy().tobytes() == hi, "room 0's first welcome"
    a = int(b["soff"][0])
    assert sends[a + RESP:a + RESP + WELCOME].cpu().numpy().tobytes() == hi, "a joiner's welcome behind its 101"
    st = storm.sres.view(torch.int32).reshape(n, 8).cpu().numpy()
    assert (st[quarter, 4] == _lib.RSC_JOINED).all() and (st[1::4, 4] == _lib.RSC_MEMBER).all(), "join storm: statuses"
    storm_sweep("leave")
    torch.cuda.synchronize()
    tr = storm.srres.view(torch.int32).reshape(R, 8).cpu().numpy()
    assert (tr[:, 5] == PER).all() and (tr[:, 6] == MB - PER).all(), "leave storm: rows"
    # (the leavers spoke in this sweep: the fold walks the seen lists, so no room loses its backlog)
    br = storm.brres.view(torch.int32).reshape(R, 8).cpu().numpy()
    assert (br[:, 5] == 0).all() and (br[:, 2] > 0).all(), "leave storm: the backlogs are kept"
    host_sweep(True)
    torch.cuda.synchronize()
    assert host_present.all()
    a = int(b["soff"][1] + b["wlen"][0])
    assert sends[a:a + WELCOME].cpu().numpy().tobytes() == hi, "the host path's welcome"
    host_sweep(False)
    torch.cuda.synchronize()
    assert (host_present == rest).all()

    def storms(loops):
        """join and leave alternate; each is timed by its own events."""
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(loops)]
        for e0, e1, e2 in ev:
            e0.record()
            storm_sweep("join")
            e1.record()
            storm_sweep("leave")
            e2.record()
        torch.cuda.synchronize()
        return (sum(e0.elapsed_time(e1) for e0, e1, _ in ev) * 1e3 / loops,
                sum(e1.elapsed_time(e2) for _, e1, e2 in ev) * 1e3 / loops)

    def hosts(loops):
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(loops)]
        for e0, e1, e2 in ev:
            e0.record()
            host_sweep(True)
            e1.record()
            host_sweep(False)
            e2.record()
        torch.cuda.synchronize()
        return (sum(e0.elapsed_time(e1) for e0, e1, _ in ev) * 1e3 / loops,
                sum(e1.elapsed_time(e2) for _, e1, e2 in ev) * 1e3 / loops)

    modes = {"roster_call": seven.roster, "seven_call": seven_call, "six_call": six_call}
    for fn in modes.values():
        fn()
        fn()
    torch.cuda.synchronize()
    la = max(20, min(200, int(4e9 // max(b["out_bytes"], 1))))
    loops = {"seven_call": la, "six_call": la, "roster_call": 200, "storms": max(10, la // 2), "hosts": 3}
    t = {name: [] for name in list(modes) + ["join_storm", "leave_storm", "host_join", "host_leave"]}
    for _ in range(args.repeats):
        for name, fn in modes.items():  # (alternated: each repeat times every variant)
            t[name].append(timed(fn, loops[name]))
        j, lv = storms(loops["storms"])
        t["join_storm"].append(j)
        t["leave_storm"].append(lv)
        j, lv = hosts(loops["hosts"])
        t["host_join"].append(j)
        t["host_leave"].append(lv)
    row = {"connections": n, "rooms": R, "members": MB, "events_per_storm": int(len(quarter)), "repeats": args.repeats,
           "loops": loops, "send_bytes_six_call": b["out_bytes"]}
    for name in t:
        row[name] = summary(t[name])
    row["seven_minus_six_us"] = round(row["seven_call"]["median_us"] - row["six_call"]["median_us"], 2)
    row["seven_over_six"] = round(row["seven_call"]["median_us"] / row["six_call"]["median_us"], 3)
    row["host_over_join_storm"] = round(row["host_join"]["median_us"] / row["join_storm"]["median_us"], 2)
    row["host_over_leave_storm"] = round(row["host_leave"]["median_us"] / row["leave_storm"]["median_us"], 2)
    row["storms_beat_host_beyond_spread"] = bool(row["join_storm"]["max_us"] < row["host_join"]["min_us"] and
                                                 row["leave_storm"]["max_us"] < row["host_leave"]["min_us"])
    rows.append(row)
    print(json.dumps(row), flush=True)
    del six, seven, storm, host, ctabs, b, recv, stage, sends
    torch.cuda.empty_cache()

if not args.no_fit:  # (c) the joiner scan's share of the room pass at 1 024 rooms
    R, fit = 1024, {}
    for MB in (1, 4, 16):
        n = R * MB
        b = build(n, MB)
        v = variant(b, n, MB, np.ones(n, bool))
        ctab = v.table_for(b["slens"])
        v.five(b["recv"], b["stage"], ctab)
        both, rest_only = (lambda v=v: v.roster()), (lambda v=v: v.roster(n_rooms=0))
        for fn in (both, rest_only):
            fn()
        torch.cuda.synchronize()
        tb, tr = [], []
        for _ in range(args.repeats):
            tb.append(timed(both, 200))
            tr.append(timed(rest_only, 200))
        fit[n] = (summary(tb), summary(tr))
        del v, b, ctab
        torch.cuda.empty_cache()
    xs = np.asarray(sorted(fit), float)
    ys = np.asarray([fit[int(x)][0]["median_us"] - fit[int(x)][1]["median_us"] for x in xs])
    slope, intercept = np.polyfit(xs, ys, 1)
    row = {"fit": "room pass = roster call - the call with n_rooms 0, at 1 024 rooms", "rooms": R,
           "call_us": {str(int(x)): fit[int(x)][0] for x in xs}, "call_without_rooms_us": {str(int(x)): fit[int(x)][1] for x in xs},
           "room_pass_us": {str(int(x)): round(float(y), 2) for x, y in zip(xs, ys)},
           "us_per_1024_connections": round(float(slope) * 1024, 3), "intercept_us": round(float(intercept), 2),
           "scan_share_at_16384": round(float(slope * 16384 / ys[-1]), 3)}
    rows.append(row)
    print(json.dumps(row), flush=True)

assert ctx.last_device_error() == 0
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")

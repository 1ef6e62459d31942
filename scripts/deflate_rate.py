"""What compressing a sweep's broadcast costs and saves (profiles/deflate_rate.jsonl).

Every connection is a member of a room of 16 and speaks once: a whole text
message, laid out as one reassembly wrote it. Cells: 1 024 and 16 384
connections with chat-sized messages of 200-1 000 bytes, 1 024 connections
with 16 KiB messages, and 1 024 connections with JSON-shaped messages.
Measured per cell:
  (a) deflate_call: xyws_deflate_streams alone;
  (b) broadcast_plain: xyws_broadcast_streams, what the parent commit's sweep
      runs at this place;
  (c) broadcast_deflated: xyws_deflate_streams and
      xyws_broadcast_deflated_streams, every member negotiated;
  and, not timed: the bytes a member is sent plain and compressed (its room's
  two wire lengths), and the compressed size against zlib level 6 and zlib
  with Z_FIXED (raw DEFLATE, sync flush, one stream per message).
The calls in front of the broadcast (decode, reassemble, hold, reply) and
behind it (roster, backlog, outbox) are the same either way and are not part
of the timed passes. Before anything is timed every compressed message is
inflated on the host and compared. The variants are alternated in one process
after a warm-up, each timed by device events around a loop that ends in a
synchronise; every cell is repeated and reports median and range.

With --dynamic the cells are measured once more for XYWS_DFO_DYNAMIC and one
row per cell ("option": "dynamic") is appended to the file: the deflate call
with the bit next to the deflate call with opts = 0 on the same build,
alternated; the ratio with the bit next to the same zlib columns; the share of
messages that went out with a dynamic block.

With --takeover the cells are measured once more for
xyws_deflate_windows_streams and one row per cell ("option": "takeover") is
appended: every room takes over and is reset in front of every call (the
previous roster's `joined`), so a message's history is what the room's members
in front of it said in the same sweep, up to 15 messages; the call (text build,
compression, slide) next to xyws_deflate_streams on the same build and next to
the same call over rooms with a null carry (the third instantiation's plain
path), alternated; the ratio next to the same zlib columns; the records that
reached into the history. The difference between the two windows calls is text
build, priming, the second search per piece and the slide together. With
--noprime-lib FILE, a libxyws.so built from the same sources with
-DDFL_WIN_PRIME=0, the same call of that library is timed in the same
alternation ("deflate_call_takeover_noprime": both searches run, nothing is
entered into the table in front of the second), and "priming_net_share" is the
part of the takeover call's median that this leaves out: the priming steps
and what the search then does with the window's positions (longer chains of
candidates, matches extended into the window).

With --takeover-dynamic the takeover cells are measured for
XYWS_DFO_WINDOW_DYNAMIC and one row per cell ("option": "takeover_dynamic") is
appended: the windows call with the bit next to the same call with opts = 0
and next to xyws_deflate_streams with XYWS_DFO_DYNAMIC (no history), on the
same build, alternated; the bytes of all three; the records with a dynamic
block and the records that reached into the history.

usage: deflate_rate.py [--out FILE] [--repeats R] [--dynamic | --takeover [--noprime-lib FILE] | --takeover-dynamic]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]
import streams  # noqa: E402
from xynet_amd import _lib, websocket as ws  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deflate_rate.jsonl"))
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--dynamic", action="store_true")
ap.add_argument("--takeover", action="store_true")
ap.add_argument("--takeover-dynamic", action="store_true")
ap.add_argument("--noprime-lib")
args = ap.parse_args()
TAKE = args.takeover or args.takeover_dynamic  # the windows call is measured, with WOPT
WOPT = _lib.DFO_WINDOW_DYNAMIC if args.takeover_dynamic else 0
assert args.repeats >= 5, "the spread needs at least 5 repeats"
assert torch.cuda.is_available(), "deflate_rate.py measures on the GPU: no device, no number"

ctx = ws.Context(0)
L = ctx.L
sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
NOPRIME = C.CDLL(os.path.abspath(args.noprime_lib)) if args.takeover and args.noprime_lib else None
if NOPRIME:  # (the same sources: the context's layout is the same, so this library takes ctx.h)
    NOPRIME.xyws_deflate_windows_streams.argtypes = L.xyws_deflate_windows_streams.argtypes
    NOPRIME.xyws_deflate_windows_streams.restype = L.xyws_deflate_windows_streams.restype
ROOM = 16
WORDS = ("the quick brown fox jumps over a lazy dog while we talk about rooms messages sweeps and frames "
         "hello thanks ok sure see you later what time is it there today").split()


def vp(t):
    return C.c_void_p(t.data_ptr())


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


def chat(rng, length):
    out = []
    while sum(len(w) + 1 for w in out) < length:
        out.append(WORDS[rng.next() % len(WORDS)] + ("%d" % (rng.next() % 97) if rng.next() % 5 == 0 else ""))
    return " ".join(out).encode()[:length]


def jsonish(rng, length):
    out = b""
    while len(out) < length:
        out += b'{"type":"message","room":"room-%d","user":{"id":%d,"name":"%s"},"text":"%s","ts":%d},' % (
            rng.next() % 64, rng.next() % 100000, WORDS[rng.next() % len(WORDS)].encode(), chat(rng, 20 + rng.next() % 60),
            1700000000 + rng.next() % 100000)
    return out[:length]


def zsize(m, **kw):
    c = zlib.compressobj(6, zlib.DEFLATED, -15, **kw)
    return len(c.compress(m) + c.flush(zlib.Z_SYNC_FLUSH)) - 4


rows = []
for corpus, n, lo, hi in (("chat", 1024, 200, 1000), ("chat", 16384, 200, 1000), ("chat", 1024, 16384, 16384),
                          ("json", 1024, 200, 1000)):
    rng = streams.SplitMix(0xDEF1 + n + hi)
    make = chat if corpus == "chat" else jsonish
    msgs = [make(rng, lo + rng.next() % (hi - lo + 1)) for _ in range(n)]
    stride, nr = (hi + 15) // 16 * 16, n // ROOM
    ocap, wcap = stride + 16, ROOM * (stride + 32)
    img = np.zeros(n * stride, np.uint8)
    recs = np.zeros((n, 5), np.uint64)
    for i, m in enumerate(msgs):
        img[stride * i:stride * i + len(m)] = np.frombuffer(m, np.uint8)
        recs[i] = (0, 1, 0, len(m), _lib.MSG_COMPLETE | (1 << 32))
    mout, recs_t, idx = dev(img), dev(recs), np.arange(n, dtype=np.uint64)
    mres = np.zeros((n, 4), np.uint64)
    mres[:, 0], mres[:, 1], mres[:, 2] = [len(m) for m in msgs], 1, 1
    mtab = np.zeros((n, 8), np.uint64)
    mtab[:, 0], mtab[:, 1], mtab[:, 3], mtab[:, 4] = mout.data_ptr() + stride * idx, stride, recs_t.data_ptr() + 40 * idx, 1
    sends, zout, vrecs = zeros(n * wcap), zeros(n * ocap), zeros(40 * n)
    btab = np.zeros((n, 8), np.uint64)
    btab[:, 2], btab[:, 3], btab[:, 5] = sends.data_ptr() + wcap * idx, wcap, idx // ROOM
    dtab = np.zeros((n, 8), np.uint64)
    dtab[:, 0], dtab[:, 1], dtab[:, 2], dtab[:, 3], dtab[:, 4] = zout.data_ptr() + ocap * idx, ocap, vrecs.data_ptr() + 40 * idx, 1, _lib.DFC_NEGOTIATED
    members, wires, zwires = dev(np.arange(n, dtype=np.uint32)), zeros(nr * wcap), zeros(nr * wcap)
    ridx = np.arange(nr, dtype=np.uint64)
    rtab, ztab = np.zeros((nr, 4), np.uint64), np.zeros((nr, 4), np.uint64)
    for t, w in ((rtab, wires), (ztab, zwires)):
        t[:, 0], t[:, 1], t[:, 2], t[:, 3] = members.data_ptr() + 4 * ROOM * ridx, ROOM, w.data_ptr() + wcap * ridx, wcap
    mres_t, mtab_t, btab_t, dtab_t, rtab_t, ztab_t = (dev(t) for t in (mres, mtab, btab, dtab, rtab, ztab))
    view, vres, vbc, dres, bres, rres, zres = (zeros(s * n) for s in (64, 32, 64, 32, 32, 32, 32))

    def deflate_call(opts=0):
        _lib.check(L.xyws_deflate_streams(ctx.h, vp(mtab_t), vp(mres_t), vp(btab_t), vp(dtab_t), n, opts, vp(view), vp(vres),
                                          vp(vbc), vp(dres), sp))

    def deflate_call_dynamic():
        deflate_call(_lib.DFO_DYNAMIC)

    # --takeover: a text area of 32 KiB + the room's sweep and a carry per room; roster rows that say "joined"
    tcap = 32768 + wcap
    texts, tcarries, drres = zeros(nr * tcap), zeros(32 * nr), zeros(32 * nr)
    drtab, nulltab, joined = np.zeros((nr, 4), np.uint64), np.zeros((nr, 4), np.uint64), np.zeros((nr, 8), np.uint32)
    drtab[:, 0], drtab[:, 1], drtab[:, 2] = texts.data_ptr() + tcap * ridx, tcap, tcarries.data_ptr() + 32 * ridx
    joined[:, 4] = 1
    drtab_t, nulltab_t, joined_t = dev(drtab), dev(nulltab), dev(joined)

    def windows_call(drooms, lib=L, opts=0):
        _lib.check(lib.xyws_deflate_windows_streams(ctx.h, vp(mtab_t), vp(mres_t), vp(btab_t), vp(dtab_t), n, vp(rtab_t), vp(drooms),
                                                  vp(joined_t), nr, opts, vp(view), vp(vres), vp(vbc), vp(dres), vp(drres), sp))

    def deflate_call_takeover():
        windows_call(drtab_t)

    def deflate_call_takeover_dynamic():
        windows_call(drtab_t, opts=_lib.DFO_WINDOW_DYNAMIC)

    def deflate_call_windows_plain():
        windows_call(nulltab_t)

    def deflate_call_takeover_noprime():
        windows_call(drtab_t, NOPRIME)

    def broadcast_plain():
        _lib.check(L.xyws_broadcast_streams(ctx.h, vp(mtab_t), vp(mres_t), vp(btab_t), n, vp(rtab_t), vp(rres), nr, 0x11, 0,
                                            vp(bres), sp))

    def broadcast_deflated():
        deflate_call(_lib.DFO_DYNAMIC if args.dynamic else 0)
        _lib.check(L.xyws_broadcast_deflated_streams(ctx.h, vp(mtab_t), vp(mres_t), vp(btab_t), n, vp(rtab_t), vp(rres), nr,
                                                     0x11, 0, vp(bres), vp(view), vp(vres), vp(vbc), vp(dtab_t), vp(ztab_t),
                                                     vp(zres), sp))

    # ---- checks, before anything is timed
    broadcast_deflated()
    torch.cuda.synchronize()
    res = dres.cpu().numpy().view(np.uint64).reshape(n, 4)
    got, kinds = zout.cpu().numpy().reshape(n, ocap), dres.cpu().numpy().view(np.uint32).reshape(n, 8)
    for i, m in enumerate(msgs):
        z = got[i, :int(res[i, 0])].tobytes()
        assert zlib.decompressobj(-15).decompress(z + b"\x00\x00\xff\xff") == m, i
    plain_len = rres.cpu().numpy().view(np.uint64).reshape(n, 4)[:nr, 0]
    z_len = zres.cpu().numpy().view(np.uint64).reshape(n, 4)[:nr, 0]
    assert (bres.cpu().numpy().view(np.uint64).reshape(n, 4)[:, 1] == np.repeat(z_len, ROOM)).all()
    parents = {}
    for name, fn in (("takeover", deflate_call_takeover), ("dynamic", deflate_call_dynamic)) if args.takeover_dynamic else ():
        fn()
        torch.cuda.synchronize()
        parents["compressed_bytes_" + name] = int(dres.cpu().numpy().view(np.uint64).reshape(n, 4)[:, 0].sum())
    if TAKE:  # every message inflates against what its room said in front of it; the bytes are the takeover's
        windows_call(drtab_t, opts=WOPT)
        torch.cuda.synchronize()
        res = dres.cpu().numpy().view(np.uint64).reshape(n, 4)
        got, kinds = zout.cpu().numpy().reshape(n, ocap), dres.cpu().numpy().view(np.uint32).reshape(n, 8)
        for r in range(nr):
            hist = b""
            for i in range(ROOM * r, ROOM * (r + 1)):
                d = zlib.decompressobj(-15, zdict=hist[-32768:]) if hist else zlib.decompressobj(-15)
                assert d.decompress(got[i, :int(res[i, 0])].tobytes() + b"\x00\x00\xff\xff") == msgs[i], i
                hist += msgs[i]
        room_rows = drres.cpu().numpy().view(np.uint32).reshape(nr, 8)
        assert not (room_rows[:, 4] & ~np.uint32(1)).any()  # (reset, neither cap nor desync)
    modes = {"deflate_call": deflate_call, "broadcast_plain": broadcast_plain, "broadcast_deflated": broadcast_deflated}
    if args.takeover:
        modes = {"deflate_call": deflate_call, "deflate_call_takeover": deflate_call_takeover,
                 "deflate_call_windows_plain": deflate_call_windows_plain}
        if NOPRIME:
            modes["deflate_call_takeover_noprime"] = deflate_call_takeover_noprime
    if args.dynamic:
        modes = {"deflate_call": deflate_call, "deflate_call_dynamic": deflate_call_dynamic}
    if args.takeover_dynamic:
        modes = {"deflate_call": deflate_call, "deflate_call_dynamic": deflate_call_dynamic,
                 "deflate_call_takeover": deflate_call_takeover, "deflate_call_takeover_dynamic": deflate_call_takeover_dynamic}
    for fn in modes.values():
        fn()
        fn()
    torch.cuda.synchronize()
    t = {name: [] for name in modes}
    for _ in range(args.repeats):
        for name, fn in modes.items():  # (alternated: each repeat times every variant)
            t[name].append(timed(fn, 20))
    total = sum(map(len, msgs))
    row = {"corpus": corpus, "connections": n, "room": ROOM, "message_bytes_min": lo, "message_bytes_max": hi,
           "message_bytes": total, "compressed_bytes": int(res[:, 0].sum()), "n_fixed": int(kinds[:, 4].sum()),
           "n_stored": int(kinds[:, 5].sum()), "zlib6_bytes": sum(zsize(m) for m in msgs),
           "zlib_fixed_bytes": sum(zsize(m, strategy=zlib.Z_FIXED) for m in msgs),
           "send_bytes_per_member_plain": round(float(plain_len.mean()), 1),
           "send_bytes_per_member_deflated": round(float(z_len.mean()), 1), "repeats": args.repeats, "loops": 20}
    for name in modes:
        row[name] = summary(t[name])
    row["ratio"] = round(row["compressed_bytes"] / total, 3)
    row["ratio_zlib6"] = round(row["zlib6_bytes"] / total, 3)
    row["ratio_zlib_fixed"] = round(row["zlib_fixed_bytes"] / total, 3)
    row["deflate_MBps_in"] = round(total / row["deflate_call"]["median_us"], 1)
    if args.dynamic:  # (compressed_bytes, ratio and the send bytes are the bit's; Huffman records of either kind: n_deflated)
        row["n_deflated"] = row.pop("n_fixed")
        row.update(option="dynamic", n_dynamic=int(kinds[:, 7].sum()), dynamic_share=round(int(kinds[:, 7].sum()) / n, 3),
                   deflate_dynamic_MBps_in=round(total / row["deflate_call_dynamic"]["median_us"], 1))
    if TAKE:  # (compressed_bytes and ratio are the takeover's; the send bytes are left out: no wire was built)
        one = zlib.compressobj(6, zlib.DEFLATED, -15)
        chained = 0
        for i, m in enumerate(msgs):  # zlib level 6 with its context kept through a room's sweep
            if i % ROOM == 0:
                one = zlib.compressobj(6, zlib.DEFLATED, -15)
            chained += len(one.compress(m) + one.flush(zlib.Z_SYNC_FLUSH)) - 4
        row["n_deflated"] = row.pop("n_fixed")
        for k in ("send_bytes_per_member_plain", "send_bytes_per_member_deflated"):
            row.pop(k)
        row.update(option="takeover", n_history=int(room_rows[:, 3].sum()), ratio_zlib6_chained=round(chained / total, 3),
                   takeover_MBps_in=round(total / row["deflate_call_takeover"]["median_us"], 1))
        if args.takeover_dynamic:  # (compressed_bytes and ratio are the bit's; the two calls it combines beside them)
            took = row["deflate_call_takeover_dynamic"]["median_us"]
            row.update(parents, option="takeover_dynamic", n_dynamic=int(kinds[:, 7].sum()),
                       ratio_takeover=round(parents["compressed_bytes_takeover"] / total, 3),
                       ratio_dynamic=round(parents["compressed_bytes_dynamic"] / total, 3),
                       time_vs_takeover=round(took / row["deflate_call_takeover"]["median_us"], 2),
                       time_vs_dynamic=round(took / row["deflate_call_dynamic"]["median_us"], 2),
                       takeover_dynamic_MBps_in=round(total / took, 1))
        if NOPRIME:
            took = row["deflate_call_takeover"]["median_us"]
            row["priming_net_share"] = round((took - row["deflate_call_takeover_noprime"]["median_us"]) / took, 3)
    rows.append(row)
    print(json.dumps(row), flush=True)

assert ctx.last_device_error() == 0
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a" if args.dynamic or TAKE else "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")

"""Phase split of the run decoder on an echo-sized batch: 0-1000 B masked
text frames (the loopback echo harness's traffic), descriptors on, several
calls on one stream (policy words set), then two calls with XYWS_OPT_STATS.
Prints the per-call HIP-event time and the decoder's counters (cycles per run
at 2.1 GHz) as one JSON line.  usage: small_batch_stats.py [BYTES] [OPTS]"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden")]
import streams  # noqa: E402
from xynet_amd import _lib, websocket as ws  # noqa: E402

size = int(sys.argv[1], 0) if len(sys.argv) > 1 else 4 << 20
xo = int(sys.argv[2], 0) if len(sys.argv) > 2 else 0
rng = streams.SplitMix(0xEC40)
b = bytearray()
while len(b) < size:
    b += streams.frame(rng, 0x81, rng.next() % 1001)
src = bytes(b[:size])
dev = torch.frombuffer(bytearray(src), dtype=torch.uint8).cuda()
dec = ws.frame_decoder(opts=xo)
cap = size // 6 + 2
for _ in range(5):
    dev.copy_(torch.frombuffer(bytearray(src), dtype=torch.uint8))
    r = dec.decode(dev, cap=cap, carry=False)
torch.cuda.synchronize()
s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
s.record()
for _ in range(20):
    r = dec.decode(dev, cap=cap, carry=False)
e.record()
torch.cuda.synchronize()
us = s.elapsed_time(e) / 20 * 1e3
stream = torch.cuda.current_stream()
names = {"ST_RUNS": "runs", "ST_NONE": "runs_without_entry", "ST_BAD": "bad_boundaries", "ST_REPAIR": "repairs",
         "ST_CUT": "cuts", "ST_SPIN": "spins", "ST_SEGS": "dense_passes", "ST_FRAMES": "frames",
         "ST_P_WIN": "scan_segments", "ST_P_CAND": "scan_survivors", "ST_P_UND": "scan_undecided",
         "ST_P_TCOMP": "cyc_scan_filter", "ST_P_TCHECK": "cyc_scan_check", "ST_P_TRES": "cyc_scan_resolve",
         "ST_D_TENT": "cyc_dense_entry", "ST_D_TCHASE": "cyc_dense_chase", "ST_T_PRO": "cyc_prologue",
         "ST_T_MAIN": "cyc_main", "ST_T_WAIT": "cyc_wait", "ST_T_FILL": "cyc_fill", "ST_T_CHASE": "cyc_chase_sync",
         "ST_T_XOR": "cyc_xor", "ST_T_TAIL": "cyc_tail", "ST_T_PF": "cyc_prefetch_issue", "ST_T_CP": "cyc_chase_pass",
         "ST_P_FILL": "cyc_pro_fill", "ST_P_SCAN": "cyc_pro_scan", "ST_P_PUB": "cyc_pro_publish",
         "ST_D_NOENT": "dense_no_entry", "ST_D_CHASE": "dense_chase_fail", "ST_D_MISMATCH": "dense_mismatch",
         "ST_D_OVF": "dense_overflow", "ST_GIVEUP": "giveups", "ST_BRIDGE": "bridges", "ST_STEAL_REQ": "steal_requests",
         "ST_STEAL_ACC": "steals", "ST_STEAL_SEGS": "stolen_segments", "ST_D_TVAL": "cyc_dense_validate",
         "ST_T_ROWS": "cyc_rows", "ST_T_SER": "cyc_serial_chase", "ST_P_LATTICE": "p_lattice", "ST_X_W0": "x41",
         "ST_X_BITS": "x42", "ST_X_SURV": "x43", "ST_T_STRIDE": "cyc_stride_pass"}
out = (C.c_uint64 * _lib.NSTATS)()
for _ in range(2):
    dec.opts = xo | _lib.OPT_STATS
    dec.decode(dev, cap=cap, carry=False)
    dec.ctx.L.xyws_debug_stats(dec.ctx.h, C.c_void_p(stream.cuda_stream), out)
pol = (C.c_uint64 * _lib.POL_WORDS)()
dec.ctx.L.xyws_debug_policy(dec.ctx.h, C.c_void_p(stream.cuda_stream), pol)
st = {label: int(out[getattr(_lib, slot)]) for slot, label in names.items()}
nrun = max(1, st["runs"])
for k in list(st):
    if k.startswith("cyc_"):
        st[k.replace("cyc_", "us_per_run_")] = round(st.pop(k) / nrun / 2100.0, 2)
print(json.dumps({"bytes": size, "opts": xo, "frames": r.nframes, "us_per_call": round(us, 1),
                  "policy": list(pol), "stats": st}))

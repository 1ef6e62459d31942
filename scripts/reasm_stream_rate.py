"""xyws_reassemble against xyws_reassemble_stream, in one run, on the bench's c2
(2^20 x 256 B binary) and c1 (65536 x 4 KiB text) tables: each batch whole
(one call, zero carry) and cut mid-frame into 4 batches (4 calls, each on the
table its own xyws_decode_stream call wrote, the message carry chained). The
non-stream calls on the cut batches compute what xyws_reassemble computes
there (the cut frames clipped and reported): they are in the list as the
time of the same launches without the carry, not as a result.

Per variant: HIP-event time per repetition (all calls of the repetition),
median and min..max over the repetitions after a warm-up; the two entry
points alternate within a repetition. One JSON line per (config, shape) to
profiles/reasm_stream.jsonl (or --out).

Usage: python scripts/reasm_stream_rate.py [--reps 30] [--warmup 5] [--configs c2,c1] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--configs", default="c2,c1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reasm_stream.jsonl"))
    args = ap.parse_args()
    import torch
    import bench
    from xynet_amd import _lib, websocket as ws
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    T = _lib.load_tools()
    ctx = ws.context()
    L, h = ctx.L, ctx.h
    stream = torch.cuda.current_stream()
    sp = C.c_void_p(stream.cuda_stream)
    lines = []
    for cfg in args.configs.split(","):
        buf, info = bench.build_batch(torch, T, cfg, 0, 1)
        size = buf.numel()
        nmax = info["nframes"] + 2
        for shape, cuts in (("whole", []), ("cut4", [size * k // 4 + 37 for k in (1, 2, 3)])):
            # the batches, each decoded in place by its own call (carry chained): views of one buffer
            work = buf.clone()
            dcarry = torch.zeros(64, dtype=torch.uint8, device="cuda")
            pts = [0] + cuts + [size]
            batches = []
            for a, b in zip(pts, pts[1:]):
                part = work[a:b]
                frames_t = torch.empty(nmax * 32, dtype=torch.uint8, device="cuda")
                n_t = torch.zeros(1, dtype=torch.int64, device="cuda")
                cp = C.c_void_p(dcarry.data_ptr())
                assert L.xyws_decode_stream(h, C.c_void_p(part.data_ptr()), part.numel(), cp, cp,
                                            C.c_void_p(frames_t.data_ptr()), nmax, C.c_void_p(n_t.data_ptr()), 0,
                                            sp) == 0
                nf = int(n_t.item())
                plen = int(frames_t[: nf * 32].view(torch.int64).view(-1, 4)[:, 2].sum().item())
                batches.append((part, frames_t, nf, plen))
            # (a stream call also delivers the rest of the frame the previous batch end cut)
            cap = max(part.numel() for part, _, _, _ in batches) + 1
            out = torch.empty(cap, dtype=torch.uint8, device="cuda")
            mcap = max(nf for _, _, nf, _ in batches) + 1
            msgs = torch.zeros(mcap * 40, dtype=torch.uint8, device="cuda")
            cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
            mcarry = torch.zeros(64, dtype=torch.uint8, device="cuda")
            mp = C.c_void_p(mcarry.data_ptr())

            def plain():
                for part, fr, nf, _ in batches:
                    assert L.xyws_reassemble(h, C.c_void_p(part.data_ptr()), part.numel(), C.c_void_p(fr.data_ptr()),
                                             nf, None, _lib.REASM_UTF8, C.c_void_p(out.data_ptr()), cap,
                                             C.c_void_p(msgs.data_ptr()), mcap, C.c_void_p(cnt.data_ptr()), sp) == 0

            def streamed():
                for part, fr, nf, _ in batches:
                    assert L.xyws_reassemble_stream(h, C.c_void_p(part.data_ptr()), part.numel(),
                                                    C.c_void_p(fr.data_ptr()), nf, None, _lib.REASM_UTF8, mp, mp,
                                                    C.c_void_p(out.data_ptr()), cap, C.c_void_p(msgs.data_ptr()),
                                                    mcap, C.c_void_p(cnt.data_ptr()), sp) == 0

            times = {"reassemble": [], "reassemble_stream": []}
            for rep in range(args.warmup + args.reps):
                for name, fn in (("reassemble", plain), ("reassemble_stream", streamed)):
                    mcarry.zero_()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    fn()
                    e1.record(stream)
                    torch.cuda.synchronize()
                    if rep >= args.warmup:
                        times[name].append(e0.elapsed_time(e1))
            ctx.last_device_error()  # (the non-stream calls on cut batches report their clipped frames)
            rec = {"config": cfg, "shape": shape, "calls": len(batches), "frames": sum(b[2] for b in batches),
                   "bytes": size, "reps": args.reps, "unit": "ms per repetition (HIP events, all calls)"}
            for name, ts in times.items():
                rec[name] = {"median": round(statistics.median(ts), 4), "min": round(min(ts), 4),
                             "max": round(max(ts), 4)}
            rec["stream_over_plain"] = round(rec["reassemble_stream"]["median"] / rec["reassemble"]["median"], 3)
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
            del work, batches, out, msgs
        del buf
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

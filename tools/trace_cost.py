#!/usr/bin/env python3
"""What the per-frame and per-block records cost: peaq_batch_run_trace against peaq_batch_run on the same inputs, same
context, same process, timed with HIP events on the calling stream (the batch path joins its own streams back into it).
Runs alternate (plain, trace, plain, ...) so that clock drift hits both alike; medians are reported.

  python tools/trace_cost.py [--pairs 4096] [--seconds 10] [--warmup 2] [--reps 7] [--out profiles/trace_cost.json]

Defaults: BASELINE.json configs[1] (4096 stereo 10 s pairs, basic) and configs[2] (the same, advanced, default FP64
engine).  The record arrays are allocated once, outside the timed region.  Prints one JSON line with both versions,
all samples, the shader clock the device held during each run and the time of each stage's launches (front end, back
end, filter bank: peaq_batch_last_timing), and writes it to --out."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--versions", default="0,1", help="0 = basic, 1 = advanced")
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "trace_cost.json"))
    args = ap.parse_args()
    import torch
    import gstpeaq_amd
    ctx = gstpeaq_amd.Context(0)
    n = int(round(args.seconds * 48000))
    ref, test = gstpeaq_amd.synth_fill(ctx, 1, args.pairs, 2, n)
    nf, nb = gstpeaq_amd.frame_count(n, n), gstpeaq_amd.frame_count(n, n, True)
    results = torch.empty((args.pairs, 16), dtype=torch.float64, device=ref.device)
    d_frames = torch.zeros((args.pairs, nf, 128), dtype=torch.uint8, device=ref.device)
    d_blocks = None
    torch.cuda.synchronize()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        tm = ctx.last_timing()                                   # HIP events around the launches of each stage, summed
        return a.elapsed_time(b), ctx.last_clock_mhz(), tm["frontend_ms"], tm["backend_ms"], tm["fb_ms"], tm["total_ms"]

    record = dict(pairs=args.pairs, seconds=args.seconds, frames_per_pair=nf, blocks_per_pair=nb, warmup=args.warmup,
                  reps=args.reps, versions=[])
    for adv in (int(v) for v in args.versions.split(",")):
        if adv and d_blocks is None:
            d_blocks = torch.zeros((args.pairs, nb, 96), dtype=torch.uint8, device=ref.device)
        plain = lambda: gstpeaq_amd.batch_run(ctx, adv, ref, test, results=results, sync=False)   # noqa: E731
        trace = lambda: gstpeaq_amd.batch_trace(ctx, adv, ref, test, sync=False, d_frames=d_frames,  # noqa: E731
                                                d_blocks=d_blocks if adv else None)
        for _ in range(args.warmup):                             # workspaces, code objects, clocks
            timed(plain), timed(trace)
        tp, tt = [], []
        for _ in range(args.reps):
            tp.append(timed(plain))
            tt.append(timed(trace))
        mp, mt = statistics.median(r[0] for r in tp), statistics.median(r[0] for r in tt)

        # medians.  device_ms: the library's own events around the step's device work (without the binding's host
        # part, which the outer events include); the stages overlap, so they do not add up to it
        def stages(rows):
            return {k: round(statistics.median(r[i] for r in rows), 3)
                    for i, k in ((5, "device_ms"), (2, "frontend_ms"), (3, "backend_ms"), (4, "fb_bank_ms"))}
        record["versions"].append(dict(
            version="advanced" if adv else "basic", batch_run_ms=round(mp, 3), trace_ms=round(mt, 3),
            overhead_pct=round(100 * (mt / mp - 1), 2),
            record_bytes=args.pairs * (nf * 128 + (nb * 96 if adv else 0)),
            batch_run_stages=stages(tp), trace_stages=stages(tt),
            batch_run_ms_all=[round(r[0], 3) for r in tp], trace_ms_all=[round(r[0], 3) for r in tt],
            batch_run_clock_mhz=[round(r[1], 1) for r in tp], trace_clock_mhz=[round(r[1], 1) for r in tt]))
    line = json.dumps(record)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()

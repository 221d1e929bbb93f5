#!/usr/bin/env python3
"""What the filter-bank band summary costs: peaq_batch_run_fb_band_summary against peaq_batch_run on the same inputs,
same context, same process, advanced version, timed with HIP events on the calling stream (the batch path joins its own
streams back into it).  Runs alternate (plain, summary, plain, ...) so that clock drift hits both alike; medians are
reported with every sample.

  python tools/fb_band_summary_cost.py [--pairs 4096] [--seconds 10] [--warmup 2] [--reps 7]
                                       [--out profiles/fb_band_summary_cost.json]

Defaults: BASELINE.json configs[2] (4096 stereo 10 s pairs, advanced).  The summary array (4096 x 2 channels x 7 x 42
doubles = 19 MB) is allocated once, outside the timed region.  Prints one JSON line with all samples, the shader clock
the device held during each run and the time of each stage's launches (front end, FFT back end, filter bank:
peaq_batch_last_timing; the filter-bank back end has no events of its own -- it runs beside the bank's next launch, and
its last launch is the tail of device_ms), and writes it to --out."""
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
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "fb_band_summary_cost.json"))
    args = ap.parse_args()
    import torch
    import gstpeaq_amd
    ctx = gstpeaq_amd.Context(0)
    n = int(round(args.seconds * 48000))
    ref, test = gstpeaq_amd.synth_fill(ctx, 1, args.pairs, 2, n)
    results = torch.empty((args.pairs, 16), dtype=torch.float64, device=ref.device)
    rows = torch.zeros((args.pairs, 2, 7, 42), dtype=torch.float64, device=ref.device)
    torch.cuda.synchronize()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        tm = ctx.last_timing()                                   # HIP events around the launches of each stage, summed
        return (a.elapsed_time(b), ctx.last_clock_mhz(), tm["frontend_ms"], tm["backend_ms"], tm["total_ms"], tm["fb_ms"],
                tm["fb_launches"])

    runs = {"plain": lambda: gstpeaq_amd.batch_run(ctx, 1, ref, test, results=results, sync=False),
            "summary": lambda: gstpeaq_amd.batch_fb_band_summary(ctx, ref, test, d_summary=rows, results=results, sync=False)}
    for _ in range(args.warmup):                                 # workspaces, code objects, clocks
        for fn in runs.values():
            timed(fn)
    samples = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, fn in runs.items():
            samples[k].append(timed(fn))
    med = {k: statistics.median(r[0] for r in v) for k, v in samples.items()}

    # medians.  device_ms: the library's own events around the step's device work (without the binding's host part,
    # which the outer events include); the stages overlap, so they do not add up to it
    def stages(v):
        out = {name: round(statistics.median(r[i] for r in v), 3)
               for i, name in ((4, "device_ms"), (2, "frontend_ms"), (3, "backend_ms"), (5, "fb_ms"))}
        out["fb_launches"] = int(v[0][6])
        out["fb_bank_launch_ms"] = round(out["fb_ms"] / max(out["fb_launches"], 1), 3)
        return out
    record = dict(pairs=args.pairs, seconds=args.seconds, blocks_per_pair=gstpeaq_amd.frame_count(n, n, True),
                  warmup=args.warmup, reps=args.reps, version="advanced",
                  runs={k: dict(ms=round(med[k], 3), overhead_pct=round(100 * (med[k] / med["plain"] - 1), 2),
                                row_bytes=int(rows.numel() * 8) if k == "summary" else 0, stages=stages(v),
                                ms_all=[round(r[0], 3) for r in v], clock_mhz=[round(r[1], 1) for r in v])
                        for k, v in samples.items()})
    line = json.dumps(record)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()

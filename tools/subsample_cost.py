#!/usr/bin/env python3
"""What the sub-sample stage costs beside the step it feeds: (a) one peaq_batch_run step, (b) peaq_batch_refine_delay
over the same batch, (c) peaq_batch_cut_shifted of the test buffer (every pair at q = 77), (d) the same call with every
pair at q = 0, the copy path.  All timed with HIP events on the calling stream, same context, same process,
alternating, two warm-up rounds, medians reported.  The shader clock is the one peaq_batch_last_clock reports for the
steps in between.

  python tools/subsample_cost.py [--pairs 4096] [--seconds 10] [--reps 7] [--out profiles/subsample_cost.json]

Defaults: BASELINE.json configs[1] (4096 stereo 10 s pairs, basic).  Shares of peak: HBM 8.0 TB/s and FP64 vector
78.6 TFLOP/s (spec).  Per pair of n samples and C channels:
  refine: bytes = both signals read once (8 n C), multiply-adds = 33 n (the mono sums' products)
  shifted cut: bytes = the test signal read and written once (8 n C), multiply-adds = 65 n C
Prints one JSON line and, with --out, writes it there."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import gstpeaq_amd
    assert torch.cuda.is_available(), "subsample_cost.py measures on the GPU"
    ctx = gstpeaq_amd.Context(0)
    n = int(round(args.seconds * 48000))
    ref, test = gstpeaq_amd.synth_fill(ctx, 1, args.pairs, args.channels, n)
    results = torch.empty((args.pairs, 16), dtype=torch.float64, device=ref.device)
    out = torch.zeros_like(ref)
    lags = np.full(args.pairs, 37, dtype=np.int32)
    skip = np.full(args.pairs, 37, dtype=np.uint32)
    keep = np.full(args.pairs, n - 37, dtype=np.uint32)
    n_in = np.full(args.pairs, n, dtype=np.uint32)
    q77, q0 = np.full(args.pairs, 77, dtype=np.int32), np.zeros(args.pairs, dtype=np.int32)
    torch.cuda.synchronize()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    step = lambda: gstpeaq_amd.batch_run(ctx, 0, ref, test, results=results, sync=False)                 # noqa: E731
    refine = lambda: gstpeaq_amd.refine_delay(ctx, ref, test, lags)                                      # noqa: E731
    shifted = lambda: gstpeaq_amd.cut_shifted(ctx, test, skip, keep, q77, n_in=n_in, out=out)            # noqa: E731
    copied = lambda: gstpeaq_amd.cut_shifted(ctx, test, skip, keep, q0, n_in=n_in, out=out)              # noqa: E731
    for _ in range(2):                                           # warm-up: workspaces, code objects, tables
        for fn in (step, refine, shifted, copied):
            timed(fn)
    t = {k: [] for k in ("step", "refine", "shifted", "copied")}
    clk = []
    for _ in range(args.reps):
        t["step"].append(timed(step))
        clk.append(ctx.last_clock_mhz())
        t["refine"].append(timed(refine))
        t["shifted"].append(timed(shifted))
        t["copied"].append(timed(copied))
    med = {k: statistics.median(v) for k, v in t.items()}
    nbytes = 8.0 * n * args.channels * args.pairs
    fma_refine = 33.0 * n * args.pairs
    fma_shift = 65.0 * (n - 37) * args.channels * args.pairs
    line = dict(pairs=args.pairs, seconds=args.seconds, channels=args.channels, library=str(gstpeaq_amd.library_path().name),
                shader_clock_mhz=round(statistics.median(clk), 1), batch_run_ms=round(med["step"], 3),
                batch_run_ms_all=[round(x, 3) for x in t["step"]],
                refine=dict(ms=round(med["refine"], 3), all_ms=[round(x, 3) for x in t["refine"]], gbytes=round(nbytes / 1e9, 2),
                            gfma=round(fma_refine / 1e9, 1), hbm_share_of_8TBs=round(nbytes / (med["refine"] * 1e-3) / 8.0e12, 4),
                            fp64_share_of_78_6TF=round(2 * fma_refine / (med["refine"] * 1e-3) / 78.6e12, 4)),
                cut_shifted=dict(ms=round(med["shifted"], 3), all_ms=[round(x, 3) for x in t["shifted"]],
                                 gbytes=round(nbytes / 1e9, 2), gfma=round(fma_shift / 1e9, 1),
                                 hbm_share_of_8TBs=round(nbytes / (med["shifted"] * 1e-3) / 8.0e12, 4),
                                 fp64_share_of_78_6TF=round(2 * fma_shift / (med["shifted"] * 1e-3) / 78.6e12, 4)),
                cut_shifted_q0=dict(ms=round(med["copied"], 3), all_ms=[round(x, 3) for x in t["copied"]],
                                    hbm_share_of_8TBs=round(nbytes / (med["copied"] * 1e-3) / 8.0e12, 4)),
                workspace_bytes=gstpeaq_amd.subdelay_workspace_bytes(args.channels, args.pairs, n),
                refine_plus_shifted_over_step=round((med["refine"] + med["shifted"]) / med["step"], 4))
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()

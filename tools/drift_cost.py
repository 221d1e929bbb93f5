#!/usr/bin/env python3
"""What the drift cut costs beside the shifted cut it generalises: (a) peaq_batch_cut_shifted of the test buffer (every
pair at q = 77), (b) peaq_batch_cut_drift along a flat line (a = 77 / 256, e = 0: the same outputs), (c) along 100 ppm,
(d) along the 1000 ppm cap, (e) with a = e = 0, the copy path.  All timed with HIP events on the calling stream, same
context, same process, alternating, two warm-up rounds, medians and every sample reported.

  python tools/drift_cost.py [--pairs 4096] [--seconds 10] [--reps 7] [--out profiles/drift_cost.json]

Defaults: 4096 stereo 10 s pairs.  Every filtered cut does 65 n C multiply-adds per pair (256 G for the default shape) on
8 n C bytes; shares of peak: HBM 8.0 TB/s and FP64 vector 78.6 TFLOP/s (spec).  The drift cut reads its taps per lane
from the table in device memory where the shifted cut reads one row through scalar loads: that traffic is what (b) - (a)
shows, and (c), (d) what a row that changes along the tile adds.  No ratio is asserted.
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
    assert torch.cuda.is_available(), "drift_cost.py measures on the GPU"
    ctx = gstpeaq_amd.Context(0)
    n = int(round(args.seconds * 48000))
    _, test = gstpeaq_amd.synth_fill(ctx, 1, args.pairs, args.channels, n)
    out = torch.zeros_like(test)
    skip = np.full(args.pairs, 600, dtype=np.uint32)
    keep = np.full(args.pairs, n - 1200, dtype=np.uint32)        # (1000 ppm moves the last output by 480 samples)
    n_in = np.full(args.pairs, n, dtype=np.uint32)
    q77 = np.full(args.pairs, 77, dtype=np.int32)
    full = lambda v: np.full(args.pairs, v, dtype=np.float64)    # noqa: E731
    torch.cuda.synchronize()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    runs = dict(shifted=lambda: gstpeaq_amd.cut_shifted(ctx, test, skip, keep, q77, n_in=n_in, out=out),
                drift_flat=lambda: gstpeaq_amd.cut_drift(ctx, test, skip, keep, full(77 / 256), full(0.0), n_in=n_in, out=out),
                drift_100ppm=lambda: gstpeaq_amd.cut_drift(ctx, test, skip, keep, full(-0.37), full(1e-4), n_in=n_in, out=out),
                drift_1000ppm=lambda: gstpeaq_amd.cut_drift(ctx, test, skip, keep, full(-0.37), full(-1e-3), n_in=n_in, out=out),
                drift_copy=lambda: gstpeaq_amd.cut_drift(ctx, test, skip, keep, full(0.0), full(0.0), n_in=n_in, out=out))
    for _ in range(2):                                           # warm-up: code objects, tables, staging slots
        for fn in runs.values():
            timed(fn)
    t = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, fn in runs.items():
            t[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    nbytes = 8.0 * n * args.channels * args.pairs
    fma = 65.0 * (n - 1200) * args.channels * args.pairs
    line = dict(pairs=args.pairs, seconds=args.seconds, channels=args.channels, library=str(gstpeaq_amd.library_path().name),
                gbytes=round(nbytes / 1e9, 2), gfma=round(fma / 1e9, 1))
    for k in runs:
        line[k] = dict(ms=round(med[k], 3), all_ms=[round(x, 3) for x in t[k]],
                       hbm_share_of_8TBs=round(nbytes / (med[k] * 1e-3) / 8.0e12, 4))
        if k != "drift_copy":
            line[k]["fp64_share_of_78_6TF"] = round(2 * fma / (med[k] * 1e-3) / 78.6e12, 4)
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()

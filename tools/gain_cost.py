#!/usr/bin/env python3
"""What matching level and polarity on the device costs beside the step it feeds: (a) one peaq_batch_run step, (b)
peaq_batch_estimate_delay at max_lag 4096, (c) peaq_batch_measure_gain over the aligned part, (d) peaq_batch_cut of one
buffer, (e) peaq_batch_cut_scaled of one buffer with the measured records.  All timed with HIP events on the calling
stream, same context, same process, alternating, two warm-up rounds, medians of --reps reported, as tools/align_cost.py
does.

  python tools/gain_cost.py [--pairs 4096] [--seconds 10] [--reps 7] [--out profiles/gain_cost.json]

Defaults: BASELINE.json configs[1] (4096 stereo 10 s pairs, basic).  Shares are of HBM's 8.0 TB/s (spec).  Per pair
of n samples kept: measure_gain reads both signals once (8 n channels bytes; the partials, 48 bytes per 4096 samples,
are noise), cut and cut_scaled read and write one (8 n channels bytes).  Prints one JSON line and writes it to --out."""
import argparse
import ctypes as C
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gain_cost.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import gstpeaq_amd
    assert torch.cuda.is_available(), "gain_cost.py measures on the GPU"
    ctx = gstpeaq_amd.Context(0)
    n = int(round(args.seconds * 48000))
    ref, test = gstpeaq_amd.synth_fill(ctx, 1, args.pairs, args.channels, n)
    results = torch.empty((args.pairs, 16), dtype=torch.float64, device=ref.device)
    rec = torch.zeros((args.pairs, 32), dtype=torch.uint8, device=ref.device)
    out = torch.zeros_like(ref)
    lag = 1105
    zero = np.zeros(args.pairs, dtype=np.uint32)
    skip = np.full(args.pairs, lag, dtype=np.uint32)
    keep = np.full(args.pairs, n - lag, dtype=np.uint32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    grec = [None]

    def measure():
        grec[0], _ = gstpeaq_amd.measure_gain(ctx, ref, test, "lsq", zero, skip, keep)

    def estimate():
        rc = ctx.L.peaq_batch_estimate_delay(ctx.h, args.channels, args.pairs, C.c_void_p(ref.data_ptr()),
                                             C.c_void_p(test.data_ptr()), n, None, None, n, 4096,
                                             C.c_void_p(rec.data_ptr()), stream)
        assert rc == 0, ctx.L.peaq_last_error()

    stages = dict(batch_run=lambda: gstpeaq_amd.batch_run(ctx, 0, ref, test, results=results, sync=False),
                  estimate4096=estimate, measure_gain=measure,
                  cut=lambda: gstpeaq_amd.cut(ctx, test, skip, keep, out=out),
                  cut_scaled=lambda: gstpeaq_amd.cut_scaled(ctx, test, skip, keep, grec[0], out=out))
    for _ in range(2):                                           # warm-up: workspaces, code objects
        for fn in stages.values():
            timed(fn)
    t, clk = {k: [] for k in stages}, []
    for _ in range(args.reps):
        for k, fn in stages.items():
            t[k].append(timed(fn))
            if k == "batch_run":
                clk.append(ctx.last_clock_mhz())
    med = {k: statistics.median(v) for k, v in t.items()}
    one = 4 * args.pairs * args.channels * (n - lag)              # bytes of one signal's kept part
    share = lambda nbytes, ms: round(nbytes / (ms * 1e-3) / 8.0e12, 4)   # noqa: E731
    gains = gstpeaq_amd.gain_records(grec[0], args.pairs)["gain"]
    line = dict(pairs=args.pairs, seconds=args.seconds, channels=args.channels, library=str(gstpeaq_amd.library_path().name),
                shader_clock_mhz=round(statistics.median(clk), 1), batch_run_ms=round(med["batch_run"], 3),
                estimate4096_ms=round(med["estimate4096"], 3),
                measure_gain_ms=round(med["measure_gain"], 3), measure_gain_gbytes=round(2 * one / 1e9, 2),
                measure_gain_hbm_share_of_8TBs=share(2 * one, med["measure_gain"]),
                cut_ms=round(med["cut"], 3), cut_gbytes=round(2 * one / 1e9, 2), cut_hbm_share_of_8TBs=share(2 * one, med["cut"]),
                cut_scaled_ms=round(med["cut_scaled"], 3), cut_scaled_hbm_share_of_8TBs=share(2 * one, med["cut_scaled"]),
                cut_scaled_over_cut=round(med["cut_scaled"] / med["cut"], 4),
                estimate4096_measure_cut_cut_scaled_over_step=round(
                    (med["estimate4096"] + med["measure_gain"] + med["cut"] + med["cut_scaled"]) / med["batch_run"], 4),
                workspace_bytes=gstpeaq_amd.gain_workspace_bytes(args.channels, args.pairs, n),
                gain_min_max=[float(gains.min()), float(gains.max())],
                all_ms={k: [round(x, 3) for x in v] for k, v in t.items()})
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What aligning a batch on the device costs beside the step it feeds: (a) one peaq_batch_run step, (b)
peaq_batch_estimate_delay over the same batch at max_lag 1024, 4096 and 16384, (c) peaq_batch_cut of one buffer.  All
timed with HIP events on the calling stream, same context, same process, alternating, two warm-up rounds, medians
reported.  The shader clock is the one peaq_batch_last_clock reports for the steps in between.  PEAQ_AMD_LIB selects
another library for the step (one without the aligner reports the step alone).

  python tools/align_cost.py [--pairs 4096] [--seconds 10] [--reps 7]

Defaults: BASELINE.json configs[1] (4096 stereo 10 s pairs, basic).  Shares of peak: HBM 8.0 TB/s and FP64 vector
78.6 TFLOP/s (spec).  Per pair, with H = 512, NB = ceil(n / H) blocks, S = ceil(max_lag / H), NSEG = 2 S rounded up
to 16, NT = NB + NSEG - 1 transforms, NCH = ceil(NB / 128) chunks:
  bytes = samples read once (8 n channels) + spectra written once (8 KB x (NB + NT)) + spectra read by the products
          (8 KB x (NSEG / 16) x (2 NB + 15 NCH)) + partial sums written and read twice (8 KB x 3 NSEG NCH)
  multiply-adds = transforms (NT + 2 S) x 25 600 (1024-point complex: 5 N log2 N / 2) + products NB x NSEG x 512 x 4.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

LAGS = (1024, 4096, 16384)


def work(n, channels, max_lag):
    """(bytes, multiply-adds) of one pair"""
    nb = max(1, -(-n // 512))
    s = -(-max_lag // 512)
    nseg = -(-2 * s // 16) * 16
    nt, nch = nb + nseg - 1, -(-nb // 128)
    nbytes = 8 * n * channels + 8192 * (nb + nt) + 8192 * (nseg // 16) * (2 * nb + 15 * nch) + 8192 * 3 * nseg * nch
    fma = (nt + 2 * s) * 25600 + nb * nseg * 512 * 4
    return nbytes, fma


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import numpy as np
    import torch
    import gstpeaq_amd
    assert torch.cuda.is_available(), "align_cost.py measures on the GPU"
    ctx = gstpeaq_amd.Context(0)
    n = int(round(args.seconds * 48000))
    ref, test = gstpeaq_amd.synth_fill(ctx, 1, args.pairs, args.channels, n)
    results = torch.empty((args.pairs, 16), dtype=torch.float64, device=ref.device)
    have = hasattr(ctx.L, "peaq_batch_estimate_delay")
    rec = torch.zeros((args.pairs, 32), dtype=torch.uint8, device=ref.device)
    out = torch.zeros_like(ref)
    skip = np.full(args.pairs, 1105, dtype=np.uint32)
    keep = np.full(args.pairs, n - 1105, dtype=np.uint32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    step = lambda: gstpeaq_amd.batch_run(ctx, 0, ref, test, results=results, sync=False)   # noqa: E731

    def estimate(max_lag):
        rc = ctx.L.peaq_batch_estimate_delay(ctx.h, args.channels, args.pairs, C.c_void_p(ref.data_ptr()),
                                             C.c_void_p(test.data_ptr()), n, None, None, n, max_lag,
                                             C.c_void_p(rec.data_ptr()), stream)
        assert rc == 0, ctx.L.peaq_last_error()

    cut = lambda: gstpeaq_amd.cut(ctx, test, skip, keep, out=out)                          # noqa: E731

    for _ in range(2):                                           # warm-up: workspaces, code objects
        timed(step)
        if have:
            for lag in LAGS:
                timed(lambda: estimate(lag))
            timed(cut)
    ts, clk, tc, te = [], [], [], {lag: [] for lag in LAGS}
    for _ in range(args.reps):
        ts.append(timed(step))
        clk.append(ctx.last_clock_mhz())
        if have:
            for lag in LAGS:
                te[lag].append(timed(lambda: estimate(lag)))
            tc.append(timed(cut))
    ms = statistics.median(ts)
    line = dict(pairs=args.pairs, seconds=args.seconds, channels=args.channels, library=str(gstpeaq_amd.library_path().name),
                batch_run_ms=round(ms, 3), shader_clock_mhz=round(statistics.median(clk), 1),
                batch_run_ms_all=[round(x, 3) for x in ts])
    if have:
        mc = statistics.median(tc)
        line["cut_ms"] = round(mc, 3)
        line["cut_gbytes"] = round(2 * 4 * args.pairs * args.channels * (n - 1105) / 1e9, 2)
        line["cut_hbm_share_of_8TBs"] = round(line["cut_gbytes"] * 1e9 / (mc * 1e-3) / 8.0e12, 4)
        line["estimate_ms"] = {}
        for lag in LAGS:
            me = statistics.median(te[lag])
            nbytes, fma = work(n, args.channels, lag)
            line["estimate_ms"][str(lag)] = dict(ms=round(me, 3), gbytes=round(args.pairs * nbytes / 1e9, 1),
                                                 gfma=round(args.pairs * fma / 1e9, 1),
                                                 hbm_share_of_8TBs=round(args.pairs * nbytes / (me * 1e-3) / 8.0e12, 4),
                                                 fp64_share_of_78_6TF=round(2 * args.pairs * fma / (me * 1e-3) / 78.6e12, 4),
                                                 all_ms=[round(x, 3) for x in te[lag]])
        line["workspace_bytes"] = gstpeaq_amd.align_workspace_bytes(args.channels, args.pairs, n, 4096)
        line["estimate4096_plus_cut_over_step"] = round((statistics.median(te[4096]) + mc) / ms, 4)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()

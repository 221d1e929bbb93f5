#!/usr/bin/env python3
"""What the wide delay search costs beside the stages it is made of and the step it feeds: (a) one peaq_batch_run step,
(b) peaq_batch_decimate of one buffer at M = 16 and 64 in both modes, (c) peaq_batch_estimate_delay_wide at max_offset
2^18 and 2^20 with a fine range of 4096, (d) the plain peaq_batch_estimate_delay at 4096 and 16384, (e) peaq_batch_cut of
one buffer.  All timed with HIP events on the calling stream, same context, same process, alternating with the step, two
warm-up rounds, medians reported with all samples.  The wide estimate blocks inside (it reads the coarse records): its
time is what the stream saw from its first launch to its last, host gaps included.

  python tools/wide_cost.py [--pairs 4096] [--seconds 10] [--reps 7] [--out profiles/wide_cost.json]

Defaults: BASELINE.json configs[1] (4096 stereo 10 s pairs, basic).  Shares of peak: HBM 8.0 TB/s (spec).  The decimator
reads every sample once (4 n channels bytes per signal) and writes n / M floats -- and, in envelope mode, n / M doubles
that the centring kernel reads twice; the cut reads and writes 4 n channels bytes.
Prints one JSON line and writes it to --out."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

FACTORS = (16, 64)
MODES = ("waveform", "envelope")
OFFSETS = (1 << 18, 1 << 20)
LAGS = (4096, 16384)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "wide_cost.json"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import gstpeaq_amd
    assert torch.cuda.is_available(), "wide_cost.py measures on the GPU"
    ctx = gstpeaq_amd.Context(0)
    n = int(round(args.seconds * 48000))
    ref, test = gstpeaq_amd.synth_fill(ctx, 1, args.pairs, args.channels, n)
    results = torch.empty((args.pairs, 16), dtype=torch.float64, device=ref.device)
    rec = torch.zeros((args.pairs, 32), dtype=torch.uint8, device=ref.device)
    out = torch.zeros_like(ref)
    dec = {M: torch.zeros((args.pairs, -(-n // M) + (-(-n // M) & 1)), dtype=torch.float32, device=ref.device) for M in FACTORS}
    wide = np.zeros(args.pairs, dtype=gstpeaq_amd.WIDE_DELAY_DTYPE)
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

    def estimate(max_lag):
        rc = ctx.L.peaq_batch_estimate_delay(ctx.h, args.channels, args.pairs, C.c_void_p(ref.data_ptr()),
                                             C.c_void_p(test.data_ptr()), n, None, None, n, max_lag,
                                             C.c_void_p(rec.data_ptr()), stream)
        assert rc == 0, ctx.L.peaq_last_error()

    def estimate_wide(max_offset):
        rc = ctx.L.peaq_batch_estimate_delay_wide(ctx.h, args.channels, args.pairs, C.c_void_p(ref.data_ptr()),
                                                  C.c_void_p(test.data_ptr()), n, None, None, n, max_offset,
                                                  gstpeaq_amd.WIDE_ENVELOPE, 4096,
                                                  wide.ctypes.data_as(C.POINTER(gstpeaq_amd.WideDelay)), stream)
        assert rc == 0, ctx.L.peaq_last_error()

    runs = {"batch_run": lambda: gstpeaq_amd.batch_run(ctx, 0, ref, test, results=results, sync=False),
            "cut": lambda: gstpeaq_amd.cut(ctx, test, skip, keep, out=out)}
    for M in FACTORS:
        for mode in MODES:
            runs["decimate_%d_%s" % (M, mode)] = (lambda M=M, mode=mode: gstpeaq_amd.decimate(ctx, test, M, mode, out=dec[M]))
    for lag in LAGS:
        runs["estimate_%d" % lag] = (lambda lag=lag: estimate(lag))
    for off in OFFSETS:
        runs["estimate_wide_%d" % off] = (lambda off=off: estimate_wide(off))
    others = [k for k in runs if k != "batch_run"]
    for _ in range(2):                                           # warm-up: workspaces, code objects, tap tables
        for k in others:
            timed(runs["batch_run"])
            timed(runs[k])
    t = {k: [] for k in runs}
    for _ in range(args.reps):                                   # alternating with the step
        for k in others:
            t["batch_run"].append(timed(runs["batch_run"]))
            t[k].append(timed(runs[k]))
    med = {k: statistics.median(v) for k, v in t.items()}
    signal_bytes = 4 * args.pairs * args.channels * n
    line = dict(pairs=args.pairs, seconds=args.seconds, channels=args.channels, reps=args.reps,
                library=str(gstpeaq_amd.library_path().name), batch_run_ms=round(med["batch_run"], 3))
    cut_bytes = 2 * 4 * args.pairs * args.channels * (n - 1105)
    line["cut"] = dict(ms=round(med["cut"], 3), gbytes=round(cut_bytes / 1e9, 2),
                       hbm_share_of_8TBs=round(cut_bytes / (med["cut"] * 1e-3) / 8.0e12, 4), all_ms=[round(x, 3) for x in t["cut"]])
    line["decimate"] = {}
    for M in FACTORS:
        for mode in MODES:
            k = "decimate_%d_%s" % (M, mode)
            nbytes = signal_bytes + args.pairs * -(-n // M) * (4 if mode == "waveform" else 4 + 3 * 8)
            line["decimate"]["%d_%s" % (M, mode)] = dict(ms=round(med[k], 3), gbytes=round(nbytes / 1e9, 2),
                                                         hbm_share_of_8TBs=round(nbytes / (med[k] * 1e-3) / 8.0e12, 4),
                                                         share_over_cut_share=round(nbytes / med[k] / (cut_bytes / med["cut"]), 4),
                                                         all_ms=[round(x, 3) for x in t[k]])
    line["estimate"] = {str(lag): dict(ms=round(med["estimate_%d" % lag], 3), all_ms=[round(x, 3) for x in t["estimate_%d" % lag]])
                        for lag in LAGS}
    line["estimate_wide"] = {}
    for off in OFFSETS:
        k = "estimate_wide_%d" % off
        line["estimate_wide"][str(off)] = dict(ms=round(med[k], 3), factor=gstpeaq_amd.wide_factor(off), fine_max_lag=4096,
                                               mode="envelope", over_estimate_16384=round(med[k] / med["estimate_16384"], 4),
                                               all_ms=[round(x, 3) for x in t[k]])
    line["wide_workspace_bytes"] = gstpeaq_amd.wide_workspace_bytes(args.channels, args.pairs, n, 1 << 20)
    text = json.dumps(line)
    print(text, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

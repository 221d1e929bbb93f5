#!/usr/bin/env python3
"""What the track cut costs beside the drift cut it generalises, on the same line in the same run: (a)
peaq_batch_cut_drift along 100 ppm -- the yardstick: this kernel is not the track stage's --, (b) peaq_batch_cut_track
with that line as one segment, (c) as ten equal segments (a knot every `seconds` / 10, two tiles in a thousand meet
one), (d) a zigzag of ten segments at +-1/64, the steepest the cut takes: the phase then changes with every output and
m every 64, so every tap row of the table is touched in every tile, (e) peaq_batch_cut_drift at its own cap of 1000 ppm
for scale.  All timed with HIP events on the calling stream, same context, same process, alternating, two warm-up
rounds, medians and every sample reported.

  python tools/track_cost.py [--pairs 4096] [--seconds 10] [--reps 7] [--out profiles/track_cost.json]

Defaults: 4096 stereo 10 s pairs.  The extra work of the track cut per output is one compare and two selects against
130 tap loads and 130 multiply-adds, so (b) and (c) are expected within about a tenth of (a); the ratios are reported,
none is asserted.  Prints one JSON line and, with --out, writes it there."""
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
    assert torch.cuda.is_available(), "track_cost.py measures on the GPU"
    ctx = gstpeaq_amd.Context(0)
    n = int(round(args.seconds * 48000))
    segs = 10
    window = n // segs
    assert 4096 <= window <= 1 << 20, "seconds: a tenth of the pair is the window"
    _, test = gstpeaq_amd.synth_fill(ctx, 1, args.pairs, args.channels, n)
    out = torch.zeros_like(test)
    margin = window // 64 + window // 128 + 600                  # the zigzag's peak, its last segment running on, the taps
    skip = np.full(args.pairs, margin, dtype=np.uint32)
    keep = np.full(args.pairs, n - 2 * margin, dtype=np.uint32)
    n_in = np.full(args.pairs, n, dtype=np.uint32)
    full = lambda v: np.full(args.pairs, v, dtype=np.float64)    # noqa: E731
    rows = lambda v, k: np.tile(np.asarray(v, np.float64)[None, :k], (args.pairs, 1))   # noqa: E731
    a0, e0 = -0.37, 1e-4
    knots = np.array([(k & 1) * (window / 64) for k in range(segs + 1)])
    zig_e = (knots[1:] - knots[:-1]) / float(window)
    zig_a = knots[:-1] - zig_e * (np.arange(segs) * float(window) + window // 2)
    assert np.abs(zig_e).max() <= 1 / 64
    one, ten = np.ones(args.pairs, np.uint32), np.full(args.pairs, segs, np.uint32)
    torch.cuda.synchronize()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    cut_track = gstpeaq_amd.cut_track
    runs = dict(drift_100ppm=lambda: gstpeaq_amd.cut_drift(ctx, test, skip, keep, full(a0), full(e0), n_in=n_in, out=out),
                track_1_segment=lambda: cut_track(ctx, test, skip, keep, window, one, rows([a0], 1), rows([e0], 1), n_in=n_in, out=out),
                track_10_equal=lambda: cut_track(ctx, test, skip, keep, window, ten, rows([a0] * segs, segs), rows([e0] * segs, segs),
                                                 n_in=n_in, out=out),
                track_zigzag_1_64=lambda: cut_track(ctx, test, skip, keep, window, ten, rows(zig_a, segs), rows(zig_e, segs),
                                                    n_in=n_in, out=out),
                drift_1000ppm=lambda: gstpeaq_amd.cut_drift(ctx, test, skip, keep, full(a0), full(-1e-3), n_in=n_in, out=out))
    for _ in range(2):                                           # warm-up: code objects, tables, staging slots
        for fn in runs.values():
            timed(fn)
    t = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, fn in runs.items():
            t[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    nbytes = 8.0 * n * args.channels * args.pairs
    fma = 65.0 * float(keep[0]) * args.channels * args.pairs
    line = dict(pairs=args.pairs, seconds=args.seconds, channels=args.channels, window=window,
                library=str(gstpeaq_amd.library_path().name), gbytes=round(nbytes / 1e9, 2), gfma=round(fma / 1e9, 1))
    for k in runs:
        line[k] = dict(ms=round(med[k], 3), all_ms=[round(x, 3) for x in t[k]],
                       hbm_share_of_8TBs=round(nbytes / (med[k] * 1e-3) / 8.0e12, 4),
                       fp64_share_of_78_6TF=round(2 * fma / (med[k] * 1e-3) / 78.6e12, 4),
                       ratio_to_drift_100ppm=round(med[k] / med["drift_100ppm"], 4))
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()

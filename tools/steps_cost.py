#!/usr/bin/env python3
"""What the steps stage costs, in one run: (a) peaq_batch_cut_track along a zigzag-free track of ten segments -- the
yardstick: this kernel is not the steps stage's --, (b) peaq_batch_cut_pieces along the same segments as pieces, which is
the same output bit for bit, (c) peaq_batch_cut_pieces with one step of +300 samples per pair in the middle of a tile
(one tile per pair runs two passes), (d) peaq_batch_locate_steps over one candidate of two windows per pair.  All timed
with HIP events on the calling stream, same context, same process, alternating, two warm-up rounds, medians and every
sample reported.

  python tools/steps_cost.py [--pairs 4096] [--seconds 10] [--reps 7] [--out profiles/steps_cost.json]

Defaults: 4096 stereo 10 s pairs.  The extra work of the pieces cut per tile is a binary search over the breakpoints and
the loop's bounds, so (b) is expected within about a tenth of (a); the locator reads two windows of a pair three times
and is expected to be bandwidth-trivial beside the estimate; the ratios are reported, none is asserted.  Prints one JSON
line and, with --out, writes it there."""
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
    assert torch.cuda.is_available(), "steps_cost.py measures on the GPU"
    ctx = gstpeaq_amd.Context(0)
    n = int(round(args.seconds * 48000))
    segs = 10
    window = n // segs
    assert 4096 <= window <= 1 << 20, "seconds: a tenth of the pair is the window"
    ref, test = gstpeaq_amd.synth_fill(ctx, 1, args.pairs, args.channels, n)
    out = torch.zeros_like(test)
    margin = 1000
    skip = np.full(args.pairs, margin, dtype=np.uint32)
    keep = np.full(args.pairs, n - 2 * margin, dtype=np.uint32)
    n_in = np.full(args.pairs, n, dtype=np.uint32)
    rows = lambda v, dtype=np.float64: np.tile(np.asarray(v, dtype)[None, :], (args.pairs, 1))   # noqa: E731
    a0, e0 = -0.37, 1e-4
    starts = [0] + [window // 2 + k * window for k in range(1, segs)]
    ten = np.full(args.pairs, segs, np.uint32)
    at = starts[5] + 1536                                        # the middle of a tile
    step_b = starts[:6] + [at] + starts[6:]
    step_a = [a0] * 6 + [a0 + 300.0] * 5
    eleven = np.full(args.pairs, segs + 1, np.uint32)
    cand = np.zeros(args.pairs, gstpeaq_amd.STEP_CANDIDATE_DTYPE)
    cand["pair"], cand["lo"], cand["hi"], cand["LA"], cand["LB"] = np.arange(args.pairs), 4 * window, 6 * window, 0, 300
    lags = np.zeros(args.pairs, np.int32)
    torch.cuda.synchronize()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    runs = dict(track_10_equal=lambda: gstpeaq_amd.cut_track(ctx, test, skip, keep, window, ten, rows([a0] * segs), rows([e0] * segs),
                                                             n_in=n_in, out=out),
                pieces_10_equal=lambda: gstpeaq_amd.cut_pieces(ctx, test, skip, keep, ten, rows(starts, np.uint32), rows([a0] * segs),
                                                               rows([e0] * segs), n_in=n_in, out=out),
                pieces_one_step=lambda: gstpeaq_amd.cut_pieces(ctx, test, skip, keep, eleven, rows(step_b, np.uint32), rows(step_a),
                                                               rows([e0] * (segs + 1)), n_in=n_in, out=out),
                locate_one_candidate=lambda: gstpeaq_amd.locate_steps(ctx, ref, test, lags, cand))
    for _ in range(2):                                           # warm-up: code objects, tables, staging slots
        for fn in runs.values():
            timed(fn)
    t = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, fn in runs.items():
            t[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    line = dict(pairs=args.pairs, seconds=args.seconds, channels=args.channels, window=window,
                library=str(gstpeaq_amd.library_path().name))
    for k in runs:
        line[k] = dict(ms=round(med[k], 3), all_ms=[round(x, 3) for x in t[k]],
                       ratio_to_track_10_equal=round(med[k] / med["track_10_equal"], 4))
    line["locate_one_candidate"]["note"] = "includes the binding's read-back of the records"
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()

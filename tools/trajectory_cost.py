#!/usr/bin/env python3
"""What readings through each pair cost: peaq_batch_run_trajectory against peaq_batch_run on the same inputs, same
context, same process, timed with HIP events on the calling stream (the batch path joins its own streams back into it).
Runs alternate (plain, trajectory, plain, ...) so that clock drift hits both alike; medians are reported.

  python tools/trajectory_cost.py [--pairs 4096] [--seconds 10] [--interval 48000] [--reps 5]

Defaults: BASELINE.json configs[1] (4096 stereo 10 s pairs, basic) and configs[2] (the same, advanced, default FP64
engine), one reading per second.  Prints one JSON line per version."""
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
    ap.add_argument("--interval", type=int, default=48000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--versions", default="0,1", help="0 = basic, 1 = advanced")
    args = ap.parse_args()
    import torch
    import gstpeaq_amd
    ctx = gstpeaq_amd.Context(0)
    n = int(round(args.seconds * 48000))
    ref, test = gstpeaq_amd.synth_fill(ctx, 1, args.pairs, 2, n)
    n_points = -(-n // args.interval)
    results = torch.empty((args.pairs, 16), dtype=torch.float64, device=ref.device)
    torch.cuda.synchronize()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for adv in (int(v) for v in args.versions.split(",")):
        plain = lambda: gstpeaq_amd.batch_run(ctx, adv, ref, test, results=results, sync=False)   # noqa: E731
        traj = lambda: gstpeaq_amd.batch_trajectory(ctx, adv, ref, test, args.interval, n_points, sync=False)  # noqa: E731
        timed(plain), timed(traj)                                # warm-up: workspaces, code objects
        tp, tt = [], []
        for _ in range(args.reps):
            tp.append(timed(plain))
            tt.append(timed(traj))
        mp, mt = statistics.median(tp), statistics.median(tt)
        print(json.dumps(dict(version="advanced" if adv else "basic", pairs=args.pairs, seconds=args.seconds,
                              interval=args.interval, n_points=n_points, batch_run_ms=round(mp, 3),
                              trajectory_ms=round(mt, 3), overhead_pct=round(100 * (mt / mp - 1), 2),
                              batch_run_ms_all=[round(x, 3) for x in tp], trajectory_ms_all=[round(x, 3) for x in tt])),
              flush=True)


if __name__ == "__main__":
    main()

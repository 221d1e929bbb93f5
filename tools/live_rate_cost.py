#!/usr/bin/env python3
"""What live rate conversion costs on the broker's workload (BASELINE.json configs[5]: 1024 concurrent stereo sessions of
10 s, fed in 4096-sample buffers by feeder threads while the broker's tick thread batches what became ready).

Per version (basic, advanced) three configurations, and, with --parent DIR (a built checkout of the parent commit), that
tree's tools/bench_broker.py on the shape of the first:
  off           48 kHz streams, no rates set: what the parent runs.  The median must lie inside the parent's own
                minimum-to-maximum spread.
  preconverted  streams of 10 s at 44.1 kHz converted beforehand (resample, outside the timed part) and pushed at 48 kHz:
                what a host-side converter in front of every push would hand over, its own cost not counted
  rated         the same streams pushed as they are into a broker with rates (44100, 44100)
Every run is a process of its own; the trees and configurations alternate, --reps rounds of all of them, so that the spread
of each is known before a difference is read.  Reported per run: wall time, frame pairs per second, the broker's tick times
(mean / p99 / max of the host and the device part, from peaq_broker_stats).

The range kernel's own time is measured by a run of its own (--one kernel): one launch over 2 x `sessions` stereo segments
-- both pads of every session, as a tick with rates on both pads enqueues per path in two launches of `sessions` -- of
1, 2, 4 and 8 frames a window, the C entry called with segment records built once, timed with events around 20 launches
after 3 of warm-up (the entry's host checks run beside the device and are shorter than the kernel); beside it the same outputs through
peaq_batch_resample (the tiled kernel), whole signals, for the price of lane = output against lane = period.  The overlap
a window converts again is 1024 of its (frames + 1) 1024 outputs.

One JSON object on the last line; --out FILE keeps it.

    python tools/live_rate_cost.py --parent ../parent_checkout --out profiles/live_rate_cost.json"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import threading
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

CONFIGS = ("off", "preconverted", "rated")
RATE = 44100


def one(args):
    """one run in this process: -> the JSON line"""
    import numpy as np
    import torch
    import gstpeaq_amd
    import synth_np
    ctx = gstpeaq_amd.Context(0)
    rated = args.one == "rated"
    n = int(args.seconds * (48000 if args.one == "off" else RATE))
    pairs = [synth_np.pair(1 + i, 2, n) for i in range(16)]      # reused round-robin (the host generator is slow)
    if args.one == "preconverted":
        def conv(x):
            y, m = gstpeaq_amd.resample(ctx, torch.from_numpy(np.ascontiguousarray(x[None])).cuda(), RATE)
            return y[0, :int(m[0])].cpu().numpy().copy()
        pairs = [(conv(r), conv(t)) for r, t in pairs]
        n = len(pairs[0][0])
    b = gstpeaq_amd.Broker(ctx, 2, args.sessions, advanced=args.advanced, rates=(RATE, RATE) if rated else None)
    sids = [b.open() for _ in range(args.sessions)]
    b.start(args.period_us)
    results = [None] * args.sessions

    def feeder(w):
        mine = range(w, args.sessions, args.feeders)
        for pos in range(0, n, args.buffer):
            for i in mine:
                ref, test = pairs[i % 16]
                b.push(sids[i], 0, ref[pos:pos + args.buffer])
                b.push(sids[i], 1, test[pos:pos + args.buffer])
        for i in mine:
            b.flush(sids[i])
        for i in mine:
            results[i] = b.results(sids[i])

    t0 = time.perf_counter()
    threads = [threading.Thread(target=feeder, args=(w,)) for w in range(args.feeders)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    dt = time.perf_counter() - t0
    frames = sum(r["frames"] for r in results)
    line = dict(tree="this", config=args.one, advanced=bool(args.advanced), sessions=args.sessions, seconds=args.seconds,
                buffer=args.buffer, wall_s=dt, frame_pairs_per_s=frames / dt, frames=frames,
                odg_mean=float(np.mean([r["odg"] for r in results])))
    line.update(b.stats())
    b.stop()
    b.close()
    print(json.dumps(line))


def kernel(args):
    """the range kernel alone, and the tiled kernel over the same outputs"""
    import numpy as np
    import torch
    import gstpeaq_amd
    ctx = gstpeaq_amd.Context(0)
    S = 2 * args.sessions
    out = {}

    def timed(call):
        for _ in range(3):
            call()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            call()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / 20

    for frames in (1, 2, 4, 8):
        count = (frames + 1) * 1024
        first = 160 * 1000 + 37
        lo, hi = gstpeaq_amd.live_rate_span(RATE, first, count)
        x = torch.rand((S, hi - lo, 2), device="cuda") - 0.5
        y = torch.zeros((S, count, 2), device="cuda")
        # (the C entry itself with the segment records built once: Python's part of a call is not the kernel's time)
        import ctypes as C
        arr = (gstpeaq_amd.RateSegment * S)(*[gstpeaq_amd.RateSegment(first, lo, gstpeaq_amd.RATE_OPEN, count, hi - lo)] * S)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        call_args = (ctx.h, 2, RATE, S, arr, C.c_void_p(x.data_ptr()), hi - lo, C.c_void_p(y.data_ptr()), count, stream)
        assert ctx.L.peaq_batch_resample_range(*call_args) == 0
        us_range = timed(lambda: ctx.L.peaq_batch_resample_range(*call_args))
        n_in = int(np.ceil(count * RATE / 48000.)) + 2
        xw = torch.rand((S, n_in, 2), device="cuda") - 0.5
        yw = torch.zeros((S, gstpeaq_amd.resampled_length(n_in, RATE) + 2, 2), device="cuda")
        us_tile = timed(lambda: gstpeaq_amd.resample(ctx, xw, RATE, out=yw))
        out["%d_frames" % frames] = dict(segments=S, outputs_per_segment=count, range_us=us_range, tile_us=us_tile,
                                         range_ns_per_output=1e3 * us_range / (S * count),
                                         converted_again_share=1024. / count)
    print(json.dumps(dict(config="kernel", rate=RATE, channels=2, **out)))


def child(cmd, cwd, env=None):
    r = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode:
        raise SystemExit("%s failed (%d):\n%s" % (" ".join(cmd), r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def spread(values):
    return dict(median=statistics.median(values), min=min(values), max=max(values), all=values)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sessions", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--buffer", type=int, default=4096)
    ap.add_argument("--feeders", type=int, default=8)
    ap.add_argument("--period-us", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--versions", default="basic,advanced")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its bench_broker.py alternates with this tree")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", choices=CONFIGS + ("kernel",), default=None, help="(internal) one run of this configuration")
    ap.add_argument("--advanced", action="store_true", help="(with --one)")
    args = ap.parse_args()
    if args.one == "kernel":
        return kernel(args)
    if args.one:
        return one(args)
    shape = ["--sessions", str(args.sessions), "--seconds", str(args.seconds), "--buffer", str(args.buffer),
             "--feeders", str(args.feeders), "--period-us", str(args.period_us)]
    me = [sys.executable, str(Path(__file__).resolve())]
    runs, report = {}, dict(sessions=args.sessions, seconds=args.seconds, buffer=args.buffer, reps=args.reps, rate=RATE, runs={})
    for version in args.versions.split(","):
        adv = ["--advanced"] if version == "advanced" else []
        order = (["parent"] if args.parent else []) + list(CONFIGS)
        for rep in range(args.reps):
            # (the order turns by one every round: whichever run comes first after another kind of load reads differently)
            for config in order[rep % len(order):] + order[:rep % len(order)]:
                if config == "parent":
                    env = {k: v for k, v in os.environ.items() if k != "PEAQ_AMD_LIB"}
                    line = child([sys.executable, "tools/bench_broker.py"] + shape + adv, cwd=args.parent, env=env)
                else:
                    line = child(me + ["--one", config] + shape + adv, cwd=str(ROOT))
                runs.setdefault((version, config), []).append(line)
    report["kernel"] = child(me + ["--one", "kernel", "--sessions", str(args.sessions)], cwd=str(ROOT))
    for (version, config), lines in runs.items():
        entry = dict(wall_s=spread([x["wall_s"] for x in lines]),
                     frame_pairs_per_s=spread([x["frame_pairs_per_s"] for x in lines]))
        for key in ("tick_host_us_mean", "tick_host_us_p99", "tick_device_us_mean", "tick_device_us_p99",
                    "tick_device_us_max", "latency_us_p99", "launches"):
            entry[key] = spread([x[key] for x in lines])
        if "odg_mean" in lines[0]:
            entry["odg_mean"] = lines[0]["odg_mean"]
        report["runs"]["%s/%s" % (version, config)] = entry
    for version in args.versions.split(","):
        r = report["runs"]
        base, off = r.get("%s/parent" % version), r["%s/off" % version]
        if base:
            off["wall_over_parent_pct"] = 100. * (off["wall_s"]["median"] / base["wall_s"]["median"] - 1.)
            off["inside_parent_spread"] = base["wall_s"]["min"] <= off["wall_s"]["median"] <= base["wall_s"]["max"]
        pre, rated = r["%s/preconverted" % version], r["%s/rated" % version]
        rated["wall_over_preconverted_pct"] = 100. * (rated["wall_s"]["median"] / pre["wall_s"]["median"] - 1.)
        rated["tick_device_over_preconverted_pct"] = 100. * (rated["tick_device_us_mean"]["median"] /
                                                             pre["tick_device_us_mean"]["median"] - 1.)
        rated["tick_host_over_preconverted_pct"] = 100. * (rated["tick_host_us_mean"]["median"] /
                                                           pre["tick_host_us_mean"]["median"] - 1.)
    text = json.dumps(report)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()

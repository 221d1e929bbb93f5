#!/usr/bin/env python3
"""What the live meter costs on the broker's workload (BASELINE.json configs[5]: 1024 concurrent stereo sessions of 10 s,
fed in 4096-sample buffers by feeder threads while the broker's tick thread batches what became ready).

Per version (basic, advanced) three configurations -- meter off, a window of 3 s every 1 s, a window of 1 s every 0.1 s
-- and, with --parent DIR (a built checkout of the parent commit), that tree's tools/bench_broker.py on the same shape.
Every run is a process of its own; the trees and configurations alternate, --reps rounds of all of them, so that the
spread of each is known before a difference is read.  Reported per run: wall time, frame pairs per second, the broker's
tick times (mean / p99 / max of the host and the device part, from peaq_broker_stats) and, with the meter on, the time
of one meter_read of every session after the flush and the readings it returned.  One JSON object on the last line;
--out FILE keeps it.

    python tools/meter_cost.py --parent ../parent_checkout --out profiles/meter_cost.json"""
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

GEOMETRIES = {"off": None, "3s_1s": (3.0, 1.0), "1s_0.1s": (1.0, 0.1)}


def one(args):
    """one run in this process: -> the JSON line"""
    import numpy as np
    import gstpeaq_amd
    import synth_np
    ctx = gstpeaq_amd.Context(0)
    n = int(args.seconds * 48000)
    pairs = [synth_np.pair(1 + i, 2, n) for i in range(16)]      # reused round-robin (the host generator is slow)
    b = gstpeaq_amd.Broker(ctx, 2, args.sessions, advanced=args.advanced)
    geometry = GEOMETRIES[args.one]
    if geometry:
        window, hop = (gstpeaq_amd.meter_frames(s) for s in geometry)
        b.set_meter(window, hop, depth=args.depth)
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
                buffer=args.buffer, wall_s=dt, frame_pairs_per_s=frames / dt,
                odg_mean=float(np.mean([r["odg"] for r in results])))
    if geometry:
        t0 = time.perf_counter()
        got = [b.meter_read(sid) for sid in sids]
        line.update(meter_read_all_s=time.perf_counter() - t0, window_frames=window, hop_frames=hop, depth=args.depth,
                    readings=sum(len(rows) for rows, _ in got), dropped=sum(d for _, d in got),
                    expected_per_session=len(gstpeaq_amd.meter_windows(n, n, window, hop)))
    line.update(b.stats())
    b.stop()
    b.close()
    print(json.dumps(line))


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
    ap.add_argument("--depth", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--versions", default="basic,advanced")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its bench_broker.py alternates with this tree")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", choices=sorted(GEOMETRIES), default=None, help="(internal) one run of this configuration")
    ap.add_argument("--advanced", action="store_true", help="(with --one)")
    args = ap.parse_args()
    if args.one:
        return one(args)
    shape = ["--sessions", str(args.sessions), "--seconds", str(args.seconds), "--buffer", str(args.buffer),
             "--feeders", str(args.feeders), "--period-us", str(args.period_us)]
    runs = {}
    for version in args.versions.split(","):
        adv = ["--advanced"] if version == "advanced" else []
        order = (["parent"] if args.parent else []) + list(GEOMETRIES)
        for rep in range(args.reps):
            # (the order turns by one every round: whichever run comes first after another kind of load reads differently)
            for config in order[rep % len(order):] + order[:rep % len(order)]:
                if config == "parent":
                    env = {k: v for k, v in os.environ.items() if k != "PEAQ_AMD_LIB"}
                    line = child([sys.executable, "tools/bench_broker.py"] + shape + adv, cwd=args.parent, env=env)
                else:
                    line = child([sys.executable, str(Path(__file__).resolve()), "--one", config, "--depth", str(args.depth)]
                                 + shape + adv, cwd=str(ROOT))
                runs.setdefault((version, config), []).append(line)
    report = dict(sessions=args.sessions, seconds=args.seconds, buffer=args.buffer, reps=args.reps, runs={})
    for (version, config), lines in runs.items():
        entry = dict(wall_s=spread([x["wall_s"] for x in lines]),
                     frame_pairs_per_s=spread([x["frame_pairs_per_s"] for x in lines]))
        for key in ("tick_host_us_mean", "tick_host_us_p99", "tick_device_us_mean", "tick_device_us_p99",
                    "tick_device_us_max", "latency_us_p99"):
            entry[key] = spread([x[key] for x in lines])
        if "meter_read_all_s" in lines[0]:
            entry["meter_read_all_s"] = spread([x["meter_read_all_s"] for x in lines])
            for key in ("window_frames", "hop_frames", "depth", "readings", "dropped", "expected_per_session"):
                entry[key] = lines[0][key]
        report["runs"]["%s/%s" % (version, config)] = entry
    for version in args.versions.split(","):
        base = report["runs"].get("%s/parent" % version)
        for config in GEOMETRIES:
            e = report["runs"]["%s/%s" % (version, config)]
            if base:
                e["wall_over_parent_pct"] = 100. * (e["wall_s"]["median"] / base["wall_s"]["median"] - 1.)
                if config == "off":
                    e["inside_parent_spread"] = base["wall_s"]["min"] <= e["wall_s"]["median"] <= base["wall_s"]["max"]
    text = json.dumps(report)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()

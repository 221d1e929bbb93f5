#!/usr/bin/env python3
"""What the band meter costs on the broker's workload (1024 concurrent stereo sessions of 10 s, fed in 4096-sample
buffers by feeder threads while the broker's tick thread batches what became ready), in the pattern of
tools/meter_cost.py.

Per version (basic, advanced) a meter of 3 s every 1 s with the band rows off and on and, with --parent DIR (a built
checkout of the parent commit), that tree's tools/meter_cost.py on the same shape and geometry -- the meter as it was
before the band rows existed.  Every run is a process of its own; the trees and configurations alternate, --reps rounds
of all of them with the order turned by one each round.  Reported per run: wall time, frame pairs per second, the
broker's tick times (mean / p99 / max of the host and the device part, from peaq_broker_stats) -- the tick's mean device
time is the figure to read, the wall time of these one-second runs scatters by 10 .. 40 % --, the time of one read of
every session after the flush, and with bands on the bytes of rows it returned.  One JSON object on the last line;
--out FILE keeps it.

    python tools/meter_bands_cost.py --parent ../parent_checkout --out profiles/meter_bands_cost.json"""
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

WINDOW_S, HOP_S = 3.0, 1.0
CONFIGS = ("off", "on")


def one(args):
    """one run in this process: -> the JSON line"""
    import numpy as np
    import gstpeaq_amd
    import synth_np
    ctx = gstpeaq_amd.Context(0)
    n = int(args.seconds * 48000)
    pairs = [synth_np.pair(1 + i, 2, n) for i in range(16)]      # reused round-robin (the host generator is slow)
    bands = args.one == "on"
    b = gstpeaq_amd.Broker(ctx, 2, args.sessions, advanced=args.advanced)
    window, hop = gstpeaq_amd.meter_frames(WINDOW_S), gstpeaq_amd.meter_frames(HOP_S)
    b.set_meter(window, hop, depth=args.depth, bands=bands)
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
    t0 = time.perf_counter()
    got = [b.meter_read(sid, bands=bands) for sid in sids]
    line = dict(tree="this", config=args.one, advanced=bool(args.advanced), sessions=args.sessions, seconds=args.seconds,
                buffer=args.buffer, wall_s=dt, frame_pairs_per_s=frames / dt,
                odg_mean=float(np.mean([r["odg"] for r in results])), meter_read_all_s=time.perf_counter() - t0,
                window_frames=window, hop_frames=hop, depth=args.depth, readings=sum(len(rows) for rows, _ in got),
                dropped=sum(d for _, d in got),
                row_bytes=sum(r["bands"].nbytes for rows, _ in got for r in rows) if bands else 0,
                workspace_bytes_per_session=gstpeaq_amd.meter_bands_workspace(window, hop, args.depth, args.advanced, 2)
                if bands else 0)
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
    ap.add_argument("--parent", default=None,
                    help="a built checkout of the parent commit: its meter_cost.py (3 s every 1 s) alternates with this tree")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", choices=CONFIGS, default=None, help="(internal) one run of this configuration")
    ap.add_argument("--advanced", action="store_true", help="(with --one)")
    args = ap.parse_args()
    if args.one:
        return one(args)
    shape = ["--sessions", str(args.sessions), "--seconds", str(args.seconds), "--buffer", str(args.buffer),
             "--feeders", str(args.feeders), "--period-us", str(args.period_us), "--depth", str(args.depth)]
    runs = {}
    for version in args.versions.split(","):
        adv = ["--advanced"] if version == "advanced" else []
        order = (["parent"] if args.parent else []) + list(CONFIGS)
        for rep in range(args.reps):
            # (the order turns by one every round: whichever run comes first after another kind of load reads differently)
            for config in order[rep % len(order):] + order[:rep % len(order)]:
                if config == "parent":
                    env = {k: v for k, v in os.environ.items() if k != "PEAQ_AMD_LIB"}
                    line = child([sys.executable, "tools/meter_cost.py", "--one", "3s_1s"] + shape + adv, cwd=args.parent,
                                 env=env)
                else:
                    line = child([sys.executable, str(Path(__file__).resolve()), "--one", config] + shape + adv,
                                 cwd=str(ROOT))
                runs.setdefault((version, config), []).append(line)
    report = dict(sessions=args.sessions, seconds=args.seconds, buffer=args.buffer, reps=args.reps, window_s=WINDOW_S,
                  hop_s=HOP_S, depth=args.depth, runs={})
    for (version, config), lines in runs.items():
        entry = dict(wall_s=spread([x["wall_s"] for x in lines]),
                     frame_pairs_per_s=spread([x["frame_pairs_per_s"] for x in lines]),
                     meter_read_all_s=spread([x["meter_read_all_s"] for x in lines]))
        for key in ("tick_host_us_mean", "tick_host_us_p99", "tick_device_us_mean", "tick_device_us_p99",
                    "tick_device_us_max", "latency_us_p99"):
            entry[key] = spread([x[key] for x in lines])
        for key in ("window_frames", "hop_frames", "readings", "dropped", "row_bytes", "workspace_bytes_per_session"):
            if key in lines[0]:
                entry[key] = lines[0][key]
        report["runs"]["%s/%s" % (version, config)] = entry
    for version in args.versions.split(","):
        base = report["runs"].get("%s/parent" % version)
        for config in CONFIGS:
            e = report["runs"]["%s/%s" % (version, config)]
            if base:
                e["wall_over_parent_pct"] = 100. * (e["wall_s"]["median"] / base["wall_s"]["median"] - 1.)
                e["tick_device_over_parent_pct"] = 100. * (e["tick_device_us_mean"]["median"] /
                                                           base["tick_device_us_mean"]["median"] - 1.)
    text = json.dumps(report)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()

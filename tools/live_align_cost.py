#!/usr/bin/env python3
"""What live alignment costs on the broker's workload (BASELINE.json configs[5]: 1024 concurrent stereo sessions of 10 s,
fed in 4096-sample buffers by feeder threads while the broker's tick thread batches what became ready).

Per version (basic, advanced) two configurations -- alignment off, and the delay watch with windows of one second (47
frames) -- and, with --parent DIR (a built checkout of the parent commit), that tree's tools/bench_broker.py on the same
shape.  Every run is a process of its own; the trees and configurations alternate, --reps rounds of all of them, so that
the spread of each is known before a difference is read: with the facility off the median must lie inside the parent's
own minimum-to-maximum spread.  Reported per run: wall time, frame pairs per second, the broker's tick times (mean / p99 /
max of the host and the device part, from peaq_broker_stats) and, with the watch on, the windows read after the flush.

The acquisition's price is latency, not throughput, and is counted in ticks by a run of its own with manual ticks
(--one acquire): n sessions whose probes are complete at the same moment, ticks until each has run its first frame, with
and without acquisition.

One JSON object on the last line; --out FILE keeps it.

    python tools/live_align_cost.py --parent ../parent_checkout --out profiles/live_align_cost.json"""
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

CONFIGS = {"off": None, "watch_1s": 1.0}


def one(args):
    """one run in this process: -> the JSON line"""
    import numpy as np
    import gstpeaq_amd
    import synth_np
    ctx = gstpeaq_amd.Context(0)
    n = int(args.seconds * 48000)
    pairs = [synth_np.pair(1 + i, 2, n) for i in range(16)]      # reused round-robin (the host generator is slow)
    b = gstpeaq_amd.Broker(ctx, 2, args.sessions, advanced=args.advanced)
    seconds = CONFIGS[args.one]
    if seconds:
        window = gstpeaq_amd.meter_frames(seconds)
        b.set_align(0, watch=window)
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
    if seconds:
        t0 = time.perf_counter()
        got = [b.watch_read(sid) for sid in sids]
        whole = (n - 2048) // 1024 + 1
        line.update(watch_read_all_s=time.perf_counter() - t0, watch_frames=window,
                    last_index_ok=all(w is not None and w["index"] == whole // window - 1 for w in got),
                    offsets=sorted({w["offset"] for w in got if w is not None}))
    line.update(b.stats())
    b.stop()
    b.close()
    print(json.dumps(line))


def acquire(args):
    """ticks from "the probe is complete" to "the first frame has run", per session, with and without acquisition"""
    import gstpeaq_amd
    import synth_np
    ctx = gstpeaq_amd.Context(0)
    probe = 48000 + 2 * 256
    ref, test = synth_np.pair(3, 2, probe + 8192)
    out = {}
    for label, max_lag in (("off", 0), ("acquire", 256)):
        b = gstpeaq_amd.Broker(ctx, 2, args.acquire_sessions, advanced=args.advanced)
        b.set_align(max_lag, watch=1)                       # (windows of one frame: the watch's index counts frames run)
        sids = [b.open() for _ in range(args.acquire_sessions)]
        for pos in range(0, probe - 4096, 4096):            # all but the probe's last buffer, worked off as it comes
            for sid in sids:
                b.push(sid, 0, ref[pos:pos + 4096])
                b.push(sid, 1, test[pos:pos + 4096])
            b.tick()
        before = {sid: b.watch_read(sid) for sid in sids}
        for sid in sids:
            b.push(sid, 0, ref[pos + 4096:probe])
            b.push(sid, 1, test[pos + 4096:probe])
        ticks, first = 0, {}
        while len(first) < len(sids) and ticks < 64:
            b.tick()
            ticks += 1
            for sid in sids:
                w = b.watch_read(sid)
                moved = w is not None and (before[sid] is None or w["index"] > before[sid]["index"])
                if sid not in first and moved:
                    first[sid] = ticks
        out[label] = dict(ticks_to_first_frame=sorted(first.values()), sessions=len(sids))
        b.close()
    print(json.dumps(dict(config="acquire", advanced=bool(args.advanced), **out)))


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
    ap.add_argument("--acquire-sessions", type=int, default=20)
    ap.add_argument("--versions", default="basic,advanced")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its bench_broker.py alternates with this tree")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", choices=sorted(CONFIGS) + ["acquire"], default=None, help="(internal) one run of this configuration")
    ap.add_argument("--advanced", action="store_true", help="(with --one)")
    args = ap.parse_args()
    if args.one == "acquire":
        return acquire(args)
    if args.one:
        return one(args)
    shape = ["--sessions", str(args.sessions), "--seconds", str(args.seconds), "--buffer", str(args.buffer),
             "--feeders", str(args.feeders), "--period-us", str(args.period_us)]
    me = [sys.executable, str(Path(__file__).resolve())]
    runs, report = {}, dict(sessions=args.sessions, seconds=args.seconds, buffer=args.buffer, reps=args.reps, runs={}, acquire={})
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
        report["acquire"][version] = child(me + ["--one", "acquire", "--acquire-sessions", str(args.acquire_sessions)] + adv,
                                           cwd=str(ROOT))
    for (version, config), lines in runs.items():
        entry = dict(wall_s=spread([x["wall_s"] for x in lines]),
                     frame_pairs_per_s=spread([x["frame_pairs_per_s"] for x in lines]))
        for key in ("tick_host_us_mean", "tick_host_us_p99", "tick_device_us_mean", "tick_device_us_p99",
                    "tick_device_us_max", "latency_us_p99"):
            entry[key] = spread([x[key] for x in lines])
        if "watch_read_all_s" in lines[0]:
            entry["watch_read_all_s"] = spread([x["watch_read_all_s"] for x in lines])
            for key in ("watch_frames", "last_index_ok", "offsets"):
                entry[key] = lines[0][key]
        report["runs"]["%s/%s" % (version, config)] = entry
    for version in args.versions.split(","):
        base = report["runs"].get("%s/parent" % version)
        for config in CONFIGS:
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

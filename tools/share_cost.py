#!/usr/bin/env python3
"""What sharing references saves a host-fed corpus.  One process, one context, alternating, two warm-up
rounds, medians of --reps samples (all samples are kept in the line):

  (a) --pairs stereo S16 pairs of --seconds in pageable memory, in two layouts -- --refs references with pairs / refs
      tests each (tests of a reference next to each other), and one reference per test -- each through
      peaq_batch_run_host_refs and through peaq_batch_run_host on the same pairs written out: wall time, frame-pairs/s,
      raw bytes packed;
  (b) peaq_batch_gather alone over --gather-outputs outputs, eight per row and one per row, and peaq_batch_cut over as
      many pairs (HIP events): bytes read plus bytes written over the time, as a share of 8 TB/s;
  (c) the shader clock the batch driver measured in the last host-fed run of a round.

  python tools/share_cost.py [--pairs 4096] [--refs 512] [--seconds 10] [--reps 7] [--out profiles/share_cost.json]

Defaults: BASELINE.json configs[1] (4096 stereo 10 s pairs, basic).  Prints one JSON line."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--refs", type=int, default=512)
    ap.add_argument("--distinct", type=int, default=512, help="different signals in host memory; the lists cycle through them")
    ap.add_argument("--gather-outputs", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import gstpeaq_amd
    from gstpeaq_amd import capi
    assert torch.cuda.is_available(), "share_cost.py measures on the GPU"
    assert args.pairs % args.refs == 0 and args.distinct <= args.pairs
    k_tests = args.pairs // args.refs
    ctx = gstpeaq_amd.Context(0)
    n = int(round(args.seconds * 48000))
    ref, test = gstpeaq_amd.synth_fill(ctx, 1, args.distinct, 2, n)

    def s16(x):
        return torch.clamp(torch.round(x.double() * 32768.), -32768., 32767.).to(torch.int16).cpu().numpy()

    h_ref, h_test = s16(ref), s16(test)                  # pageable
    signal_bytes = n * 2 * 2

    # layout -> (refs, tests, ref_index): a reference's tests next to each other
    layouts = {}
    for name, n_refs in (("shared", args.refs), ("one_each", args.pairs)):
        per = args.pairs // n_refs
        layouts[name] = ([h_ref[r % args.distinct] for r in range(n_refs)], [h_test[t % args.distinct] for t in range(args.pairs)],
                         [t // per for t in range(args.pairs)])

    def run(name, shared_entry):
        refs, tests, index = layouts[name]
        t0 = time.perf_counter()
        if shared_entry:
            rows, _ = capi._run_host_refs_rows(ctx, 0, refs, tests, index, "s16", 2, 48000, None, 0, 92.0)
        else:
            rows, _ = capi._run_host_rows(ctx, 0, [(refs[r], t) for r, t in zip(index, tests)], "s16", 2, 48000, None, 0, 92.0)
        dt = time.perf_counter() - t0
        return dict(wall_s=dt, frame_pairs_per_s=float(rows[:, 14].sum()) / dt), rows

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    go = min(args.gather_outputs, args.distinct)
    g_out = torch.zeros((go, n, 2), dtype=torch.float32, device=ref.device)
    zeros, whole = np.zeros(go, np.uint32), np.full(go, n, np.uint32)
    gathers = {"eight_per_row": np.arange(go, dtype=np.uint32) // 8, "one_per_row": np.arange(go, dtype=np.uint32)}
    device_ops = {k: (lambda src=src: gstpeaq_amd.gather(ctx, ref[:int(src.max()) + 1], src, zeros, whole, out=g_out))
                  for k, src in gathers.items()}
    device_ops["cut"] = lambda: gstpeaq_amd.cut(ctx, test[:go], zeros, whole, out=g_out)

    variants = [(name, entry) for name in layouts for entry in (True, False)]
    fed = {v: [] for v in variants}
    dev_ms = {k: [] for k in device_ops}
    clk, same = [], True
    for rep in range(2 + args.reps):                     # two warm-up rounds: workspaces, staging sets, code objects
        rows = {}
        for v in variants if rep % 2 == 0 else variants[::-1]:
            sample, rows[v] = run(*v)
            if rep >= 2:
                fed[v].append(sample)
        for name in layouts:
            same = same and rows[(name, True)].tobytes() == rows[(name, False)].tobytes()
        if rep >= 2:
            clk.append(ctx.last_clock_mhz())
        for k, fn in device_ops.items():
            ms = timed(fn)
            if rep >= 2:
                dev_ms[k].append(ms)

    def summary(samples):
        out = {k: round(statistics.median(s[k] for s in samples), 4 if k == "wall_s" else 1) for k in samples[0]}
        out["frame_pairs_per_s_all"] = [round(s["frame_pairs_per_s"]) for s in samples]
        return out

    line = dict(pairs=args.pairs, refs=args.refs, tests_per_ref=k_tests, distinct=args.distinct, seconds=args.seconds, channels=2,
                format="s16", reps=args.reps, shader_clock_mhz=round(statistics.median(clk), 1), results_identical=bool(same))
    for name, n_refs in (("shared", args.refs), ("one_each", args.pairs)):
        a, b = summary(fed[(name, True)]), summary(fed[(name, False)])
        spread = (max(b["frame_pairs_per_s_all"]) - min(b["frame_pairs_per_s_all"])) / b["frame_pairs_per_s"]
        line[name] = dict(refs=n_refs, run_host_refs=a, run_host=b,
                          raw_gbytes_refs=round((n_refs + args.pairs) * signal_bytes / 1e9, 2),
                          raw_gbytes_pairs=round(2 * args.pairs * signal_bytes / 1e9, 2),
                          byte_ratio=round(2 * args.pairs / (n_refs + args.pairs), 3),
                          refs_over_pairs=round(a["frame_pairs_per_s"] / b["frame_pairs_per_s"], 3),
                          run_host_spread=round(spread, 3))
    line["workspace_bytes"] = dict(
        run_host_refs_shared=gstpeaq_amd.feed_refs_workspace_bytes(gstpeaq_amd.make_feed("s16", 2), 0, args.refs, args.pairs, n),
        run_host=gstpeaq_amd.feed_workspace_bytes(gstpeaq_amd.make_feed("s16", 2), 0, args.pairs, n))
    out_bytes = go * n * 2 * 4
    line["device"] = {}
    for k, ms in dev_ms.items():
        med = statistics.median(ms)
        rows_read = int(gathers[k].max()) + 1 if k in gathers else go
        line["device"][k] = dict(outputs=go, rows=rows_read, ms=round(med, 3), ms_all=[round(x, 3) for x in ms],
                                 gbytes_copied=round(2 * out_bytes / 1e9, 2),
                                 copied_share_of_8TBs=round(2 * out_bytes / (med * 1e-3) / HBM, 4),
                                 hbm_gbytes=round((out_bytes + rows_read * n * 2 * 4) / 1e9, 2))
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

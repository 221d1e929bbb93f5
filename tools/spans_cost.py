#!/usr/bin/env python3
"""What the scores of time spans cost in the advanced version: peaq_batch_run_adv_spans against peaq_batch_run and
peaq_batch_run_trace (advanced = 1) on the same inputs, same process, timed with HIP events on the calling stream (the
batch path joins its own streams back into it).  Four runs alternate (plain, trace, spans 5 s / 1 s hop, spans 1 s /
0.5 s hop, plain, ...) so that clock drift hits all alike; medians are reported with every sample and the samples'
spread.

  python tools/spans_cost.py [--pairs 4096] [--seconds 10] [--warmup 2] [--reps 7] [--parent-lib PATH]
                             [--no-cold-start] [--out profiles/spans_cost.json]

Defaults: BASELINE.json configs[2] (4096 stereo 10 s pairs, advanced version, default engine).  --parent-lib: another
build of the library (the parent commit's libpeaq_amd.so), loaded beside this one with a context of its own, runs the
plain call; without it this build's peaq_batch_run does.  The output arrays are allocated once, outside the timed
region.

The trace run is the feed of the replay (both back ends in their trace instantiations, into arrays of the caller's): a
spans run over the trace run is the replay's own share, the trace run over the plain run the feed's.

The cold-start alternative is measured once, for the 5 s / 1 s case: the same sliding spans scored as pairs of their
own -- pair_stride views into the same buffers through peaq_batch_run, one call per span, both front ends run again for
each.  Prints one JSON line with all samples, the shader clock the device held during each run and the time of each
stage's launches (peaq_batch_last_timing), and writes it to --out."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from windows_cost import context_of                    # noqa: E402  (another build of the library beside this one)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--no-cold-start", action="store_true")
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "spans_cost.json"))
    args = ap.parse_args()
    import torch
    import gstpeaq_amd
    ctx = gstpeaq_amd.Context(0)
    plain_ctx = context_of(args.parent_lib) if args.parent_lib else ctx
    n = int(round(args.seconds * 48000))
    # One spare pair behind the last: a row of the batch entries is pair_stride samples that the kernels may read (the
    # high-pass walk of the filter-bank path fetches the chunk behind the one it works on, bounded by the row, not by
    # the pair's length), and the cold-start views below begin inside their pairs -- the last pair's row then reaches
    # into the spare one instead of past the end of the allocation.
    ref, test = (t[:args.pairs] for t in gstpeaq_amd.synth_fill(ctx, 1, args.pairs + 1, 2, n))
    nf, nb = gstpeaq_amd.frame_count(n, n), gstpeaq_amd.frame_count(n, n, True)
    results = torch.empty((args.pairs, 16), dtype=torch.float64, device=ref.device)
    d_frames = torch.zeros((args.pairs, nf, 128), dtype=torch.uint8, device=ref.device)
    d_blocks = torch.zeros((args.pairs, nb, 96), dtype=torch.uint8, device=ref.device)
    shapes = {"spans_5s_1s": gstpeaq_amd.sliding_windows(n, 5 * 48000, 48000),
              "spans_1s_0.5s": gstpeaq_amd.sliding_windows(n, 48000, 24000)}
    d_spans = {k: torch.empty((args.pairs, len(w), 16), dtype=torch.float64, device=ref.device) for k, w in shapes.items()}
    torch.cuda.synchronize()
    record = dict(pairs=args.pairs, seconds=args.seconds, frames_per_pair=nf, blocks_per_pair=nb, warmup=args.warmup,
                  reps=args.reps, plain_library="parent" if args.parent_lib else "this build",
                  n_spans={k: len(w) for k, w in shapes.items()},
                  workspace_bytes={k: int(ctx.L.peaq_batch_adv_spans_workspace_bytes(2, args.pairs, n, len(w))) -
                                   int(ctx.L.peaq_batch_workspace_bytes(1, 2, args.pairs, n)) for k, w in shapes.items()})

    def timed(fn, c):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        tm = c.last_timing()                                     # HIP events around the launches of each stage, summed
        return (a.elapsed_time(b), c.last_clock_mhz(), tm["frontend_ms"], tm["backend_ms"], tm["fb_ms"], tm["total_ms"],
                tm["backend_launches"], tm["fb_launches"])

    runs = {"plain": (lambda: gstpeaq_amd.batch_run(plain_ctx, 1, ref, test, results=results, sync=False), plain_ctx),
            "trace": (lambda: gstpeaq_amd.batch_trace(ctx, 1, ref, test, d_frames=d_frames, d_blocks=d_blocks, sync=False),
                      ctx)}
    for k, w in shapes.items():
        runs[k] = (lambda k=k, w=w: gstpeaq_amd.batch_adv_spans(ctx, ref, test, w, d_spans=d_spans[k], results=results,
                                                                 sync=False), ctx)
    for _ in range(args.warmup):                                 # workspaces, code objects, clocks
        for fn, c in runs.values():
            timed(fn, c)
    samples = {k: [] for k in runs}
    for _ in range(args.reps):
        for k, (fn, c) in runs.items():
            samples[k].append(timed(fn, c))
    med = {k: statistics.median(r[0] for r in v) for k, v in samples.items()}

    def stages(v):
        out = {name: round(statistics.median(r[i] for r in v), 3)
               for i, name in ((5, "device_ms"), (2, "frontend_ms"), (3, "backend_ms"), (4, "fb_bank_ms"))}
        out["backend_launches"], out["fb_launches"] = int(v[0][6]), int(v[0][7])
        return out
    record["runs"] = {
        k: dict(ms=round(med[k], 3), mean_ms=round(statistics.mean(r[0] for r in v), 3),
                min_ms=round(min(r[0] for r in v), 3), max_ms=round(max(r[0] for r in v), 3),
                stdev_ms=round(statistics.stdev(r[0] for r in v), 3) if len(v) > 1 else 0.,
                overhead_pct=round(100 * (med[k] / med["plain"] - 1), 2),
                over_trace_pct=round(100 * (med[k] / med["trace"] - 1), 2), stages=stages(v),
                ms_all=[round(r[0], 3) for r in v], clock_mhz=[round(r[1], 1) for r in v])
        for k, v in samples.items()}

    if not args.no_cold_start:
        # every span as a pair of its own: a view that starts at the span's first sample, as long as the span
        w = shapes["spans_5s_1s"]
        stride = ref.shape[1]
        cold = torch.empty((len(w), args.pairs, 16), dtype=torch.float64, device=ref.device)

        def cold_start():
            for i, (start, length) in enumerate(w.tolist()):
                off = start * 2 * 4                              # stereo float32
                gstpeaq_amd.capi._check(ctx.L.peaq_batch_run(
                    ctx.h, 1, 2, 92.0, args.pairs, C.c_void_p(ref.data_ptr() + off), C.c_void_p(test.data_ptr() + off),
                    stride, None, None, length, C.c_void_p(cold[i].data_ptr()), None))
        timed(cold_start, ctx)                                   # (the shorter pairs' workspaces and launch shapes)
        ms = timed(cold_start, ctx)[0]
        record["cold_start_5s_1s"] = dict(ms=round(ms, 3), calls=len(w),
                                          spans_run_over_cold_start=round(med["spans_5s_1s"] / ms, 4),
                                          cold_start_over_spans_run=round(ms / med["spans_5s_1s"], 2))
    line = json.dumps(record)
    print(line, flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What feeding a corpus from host memory costs.  One process, one session, alternating, two warm-up
rounds, medians of --reps samples (all samples are kept in the line):

  (a) peaq_batch_run_host over --pairs host pairs (--distinct different ones, listed pairs / distinct times; pageable
      memory) for F32, S16 and S24: wall time, frame-pairs/s, H2D GB/s (raw bytes of both signals over the wall time);
      S16 also with PEAQ_AMD_FEED_THREADS=1, which tells host packing from PCIe;
  (b) the loop of tools/bench_pcie.py: pinned F32 chunks of 512 pairs, double buffered, copy stream beside batch_run;
  (c) the resident batch_run step over --pairs pairs (HIP events);
  (d) peaq_batch_decode_pcm alone per format and peaq_batch_cut over --decode-pairs pairs (HIP events): bytes read plus
      bytes written over the time, as a share of 8 TB/s.

  python tools/feed_cost.py [--pairs 4096] [--distinct 512] [--seconds 10] [--reps 7] [--out profiles/feed_cost.json]

Defaults: BASELINE.json configs[1] (4096 stereo 10 s pairs, basic).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

FORMATS = ("f32", "s16", "s24")
ALL_FORMATS = ("u8", "s16", "s24", "s32", "f32", "f64")
HBM = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=512)
    ap.add_argument("--decode-pairs", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import gstpeaq_amd
    from gstpeaq_amd import capi
    assert torch.cuda.is_available(), "feed_cost.py measures on the GPU"
    assert args.pairs % args.distinct == 0
    dev = torch.device("cuda", 0)
    ctx = gstpeaq_amd.Context(0)
    n = int(round(args.seconds * 48000))
    ref, test = gstpeaq_amd.synth_fill(ctx, 1, args.pairs, 2, n)
    results = torch.empty((args.pairs, 16), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()

    # ---- the host corpus: the first `distinct` pairs in each format, pageable ----
    def host_copy(x, fmt):
        x = x[:args.distinct]
        if fmt == "f32":
            return x.cpu().numpy()
        bits = 16 if fmt == "s16" else 24
        v = torch.clamp(torch.round(x.double() * 2. ** (bits - 1)), -2. ** (bits - 1), 2. ** (bits - 1) - 1).to(torch.int32)
        if fmt == "s16":
            return v.to(torch.int16).cpu().numpy()
        return torch.stack([v & 255, (v >> 8) & 255, (v >> 16) & 255], dim=-1).to(torch.uint8).cpu().numpy()

    corpus = {}
    for fmt in FORMATS:
        r, t = host_copy(ref, fmt), host_copy(test, fmt)
        listed = [(r[p % args.distinct], t[p % args.distinct]) for p in range(args.pairs)]
        corpus[fmt] = (listed, 2 * args.pairs * n * 2 * gstpeaq_amd.pcm_sample_bytes(fmt))

    def host_fed(fmt, threads=None):
        if threads is None:
            os.environ.pop("PEAQ_AMD_FEED_THREADS", None)
        else:
            os.environ["PEAQ_AMD_FEED_THREADS"] = str(threads)
        listed, nbytes = corpus[fmt]
        t0 = time.perf_counter()
        rows, _ = capi._run_host_rows(ctx, 0, listed, fmt, 2, 48000, None, 0, 92.0)
        dt = time.perf_counter() - t0
        os.environ.pop("PEAQ_AMD_FEED_THREADS", None)
        return dict(wall_s=dt, frame_pairs_per_s=float(rows[:, 14].sum()) / dt, h2d_GBps=nbytes / dt / 1e9)

    # ---- (b) the loop of tools/bench_pcie.py ----
    chunk = min(512, args.pairs)
    ref_h = torch.empty(ref[:chunk].shape, dtype=ref.dtype, pin_memory=True).copy_(ref[:chunk])
    test_h = torch.empty(ref[:chunk].shape, dtype=ref.dtype, pin_memory=True).copy_(test[:chunk])
    bufs = [(torch.empty_like(ref[:chunk]), torch.empty_like(ref[:chunk])) for _ in range(2)]
    res2 = [torch.empty((chunk, 16), dtype=torch.float64, device=dev) for _ in range(2)]
    copy_s, comp_s = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    copied = [torch.cuda.Event() for _ in range(2)]
    done = [torch.cuda.Event() for _ in range(2)]
    n_chunks = args.pairs // chunk

    def pinned_loop():
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i in range(n_chunks):
            b = i & 1
            with torch.cuda.stream(copy_s):
                if i >= 2:
                    copy_s.wait_event(done[b])
                bufs[b][0].copy_(ref_h, non_blocking=True)
                bufs[b][1].copy_(test_h, non_blocking=True)
                copied[b].record(copy_s)
            with torch.cuda.stream(comp_s):
                comp_s.wait_event(copied[b])
                gstpeaq_amd.batch_run(ctx, 0, bufs[b][0], bufs[b][1], results=res2[b], sync=False, stream=comp_s)
                done[b].record(comp_s)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        frames = float(res2[0][:, 14].sum().item()) * n_chunks
        return dict(wall_s=dt, frame_pairs_per_s=frames / dt, h2d_GBps=2 * ref_h.numel() * 4 * n_chunks / dt / 1e9)

    # ---- (c), (d): HIP events on the current stream ----
    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    step = lambda: gstpeaq_amd.batch_run(ctx, 0, ref, test, results=results, sync=False)   # noqa: E731
    dp = min(args.decode_pairs, args.pairs)
    raws = {fmt: torch.randint(0, 256, (dp, n * 2 * gstpeaq_amd.pcm_sample_bytes(fmt)), dtype=torch.uint8, device=dev)
            for fmt in ALL_FORMATS}
    dec_out = torch.zeros((dp, n, 2), dtype=torch.float32, device=dev)
    cut_out = torch.zeros((dp, n, 2), dtype=torch.float32, device=dev)
    skip = np.full(dp, 1105, dtype=np.uint32)
    keep = np.full(dp, n - 1105, dtype=np.uint32)
    decode = {fmt: (lambda fmt=fmt: gstpeaq_amd.decode_pcm(ctx, raws[fmt], fmt, 2, out=dec_out)) for fmt in ALL_FORMATS}
    cut = lambda: gstpeaq_amd.cut(ctx, test[:dp], skip, keep, out=cut_out)                 # noqa: E731

    fed = {fmt: [] for fmt in FORMATS}
    fed_1 = []
    loop, ts, clk, tc = [], [], [], []
    td = {fmt: [] for fmt in ALL_FORMATS}
    for rep in range(2 + args.reps):                             # two warm-up rounds: workspaces, staging sets, code objects
        keepit = rep >= 2
        for fmt in FORMATS:
            v = host_fed(fmt)
            if keepit:
                fed[fmt].append(v)
        v = host_fed("s16", threads=1)
        if keepit:
            fed_1.append(v)
        v = pinned_loop()
        if keepit:
            loop.append(v)
        v = timed(step)
        if keepit:
            ts.append(v)
            clk.append(ctx.last_clock_mhz())
        for fmt in ALL_FORMATS:
            v = timed(decode[fmt])
            if keepit:
                td[fmt].append(v)
        v = timed(cut)
        if keepit:
            tc.append(v)

    def summary(samples):
        out = {k: round(statistics.median(s[k] for s in samples), 4 if k == "wall_s" else 1) for k in samples[0]}
        out["frame_pairs_per_s_all"] = [round(s["frame_pairs_per_s"]) for s in samples]
        return out

    frames = float(results[:, 14].sum().item())
    ms = statistics.median(ts)
    feed = gstpeaq_amd.make_feed("s16", 2)
    line = dict(pairs=args.pairs, distinct=args.distinct, seconds=args.seconds, channels=2, reps=args.reps,
                feed_threads_default=8, shader_clock_mhz=round(statistics.median(clk), 1),
                host_fed={fmt: summary(fed[fmt]) for fmt in FORMATS}, host_fed_s16_one_thread=summary(fed_1),
                pinned_f32_loop=summary(loop),
                resident_step=dict(ms=round(ms, 3), frame_pairs_per_s=round(frames / (ms * 1e-3)), ms_all=[round(x, 3) for x in ts]),
                feed_workspace_bytes_s16=gstpeaq_amd.feed_workspace_bytes(feed, 0, args.pairs, n))
    f32 = line["host_fed"]["f32"]["frame_pairs_per_s"]
    line["s16_over_f32"] = round(line["host_fed"]["s16"]["frame_pairs_per_s"] / f32, 3)
    line["s24_over_f32"] = round(line["host_fed"]["s24"]["frame_pairs_per_s"] / f32, 3)
    line["f32_over_pinned_loop"] = round(f32 / line["pinned_f32_loop"]["frame_pairs_per_s"], 3)
    mc = statistics.median(tc)
    cut_bytes = 2 * 4 * dp * 2 * (n - 1105)
    line["cut"] = dict(pairs=dp, ms=round(mc, 3), gbytes=round(cut_bytes / 1e9, 2), hbm_share_of_8TBs=round(cut_bytes / (mc * 1e-3) / HBM, 4))
    line["decode"] = {}
    for fmt in ALL_FORMATS:
        md = statistics.median(td[fmt])
        nbytes = dp * n * 2 * (gstpeaq_amd.pcm_sample_bytes(fmt) + 4)
        line["decode"][fmt] = dict(pairs=dp, ms=round(md, 3), gbytes=round(nbytes / 1e9, 2),
                                   hbm_share_of_8TBs=round(nbytes / (md * 1e-3) / HBM, 4),
                                   bytes_per_s_over_cut=round(nbytes / md / (cut_bytes / mc), 3), ms_all=[round(x, 3) for x in td[fmt]])
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()

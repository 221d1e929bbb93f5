#!/usr/bin/env python3
"""What scoring a batch that is not sampled at 48 kHz costs: (a) one peaq_batch_run step, (b) peaq_batch_resample of the
reference AND the test buffer of the same batch from `--rate`, (c) the CLI's host converter (resample_to_48k through
PEAQ_AMD_CLI_DUMP, one core) on one pair, scaled to the batch.  (a) and (b) are timed with HIP events on the calling
stream, same context, same process, alternating, medians reported; (b) is one window around both calls.  The shader
clock is the one peaq_batch_last_clock reports for the steps in between.

  python tools/resample_cost.py [--pairs 4096] [--seconds 10] [--rate 44100] [--reps 7]

Defaults: BASELINE.json configs[1] (4096 stereo 10 s pairs, basic).  Shares of peak: HBM 8.0 TB/s and FP64 vector
78.6 TFLOP/s (spec), bytes = every input sample read once + every output sample written once, multiply-adds = output
samples x 2K (the tiled kernel also evaluates `zero_taps` zero-valued taps per output, not counted).  Prints one
JSON line."""
import argparse
import json
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def cli_convert_seconds(rate, seconds, channels):
    """wall time of the CLI reading, converting and dumping one pair (both files), minus the same at 48 kHz"""
    import numpy as np
    import synth_np
    cli = ROOT / "gstpeaq_amd" / "cli" / "peaq"
    if not cli.exists():
        return None
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for r in (rate, 48000):
            ref, test = synth_np.pair(1, channels, int(round(seconds * r)))
            for name, x in (("r", ref), ("t", test)):
                body = x.astype("<f4").tobytes()
                fmt = struct.pack("<HHIIHH", 3, channels, r, r * channels * 4, channels * 4, 32)
                chunks = b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(body)) + body
                (Path(d) / f"{name}{r}.wav").write_bytes(b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks)
            env = dict(os.environ, PEAQ_AMD_CLI_DUMP=str(Path(d) / "dump"))
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                subprocess.run([str(cli), str(Path(d) / f"r{r}.wav"), str(Path(d) / f"t{r}.wav")], check=True,
                               capture_output=True, env=env)
                ts.append(time.perf_counter() - t0)
            out[r] = min(ts)
    return max(out[rate] - out[48000], 0.)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import numpy as np
    import torch
    import gstpeaq_amd
    assert torch.cuda.is_available(), "resample_cost.py measures on the GPU"
    ctx = gstpeaq_amd.Context(0)
    n48 = int(round(args.seconds * 48000))
    n_in = int(round(args.seconds * args.rate))
    ref, test = gstpeaq_amd.synth_fill(ctx, 1, args.pairs, args.channels, n48)
    # the batch at --rate: the same kind of material (seeded pairs), its first n_in samples declared to run at --rate
    src_ref, src_test = ref[:, :n_in].contiguous(), test[:, :n_in].contiguous()
    n_out = gstpeaq_amd.resampled_length(n_in, args.rate)
    stride = n_out + (n_out & 1)
    out_ref = torch.zeros((args.pairs, stride, args.channels), dtype=torch.float32, device=ref.device)
    out_test = torch.zeros_like(out_ref)
    results = torch.empty((args.pairs, 16), dtype=torch.float64, device=ref.device)
    torch.cuda.synchronize()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    step = lambda: gstpeaq_amd.batch_run(ctx, 0, ref, test, results=results, sync=False)   # noqa: E731

    def conv():
        gstpeaq_amd.resample(ctx, src_ref, args.rate, out=out_ref)
        gstpeaq_amd.resample(ctx, src_test, args.rate, out=out_test)

    lens = np.full(args.pairs, n_in, dtype=np.uint32)

    def conv_lengths():                                          # the same with per-pair length arrays (what rate= passes)
        gstpeaq_amd.resample(ctx, src_ref, args.rate, lens, out=out_ref)
        gstpeaq_amd.resample(ctx, src_test, args.rate, lens, out=out_test)

    for _ in range(2):                                           # warm-up: workspaces, code objects, tap tables
        timed(step), timed(conv), timed(conv_lengths)
    ts, tc, tl, clk = [], [], [], []
    for _ in range(args.reps):
        ts.append(timed(step))
        clk.append(ctx.last_clock_mhz())
        tc.append(timed(conv))
        tl.append(timed(conv_lengths))
    ms, mc, ml = statistics.median(ts), statistics.median(tc), statistics.median(tl)
    plan = gstpeaq_amd.resample_plan(args.rate)
    g = np.gcd(48000, args.rate)
    half = 32.15 if args.rate < 48000 else 4. * np.ceil(64. * args.rate / 48000. / 8.)
    taps = 2 * (int(np.ceil(half)) + 1)
    samples_out = 2 * args.pairs * args.channels * n_out
    samples_in = 2 * args.pairs * args.channels * n_in
    fma = samples_out * taps
    nbytes = 4 * (samples_in + samples_out)
    cpu_pair = cli_convert_seconds(args.rate, args.seconds, args.channels)
    print(json.dumps(dict(pairs=args.pairs, seconds=args.seconds, rate=args.rate, channels=args.channels,
                          L=int(48000 // g), M=int(args.rate // g), taps=taps,
                          kernel="tile" if plan["tiled"] else "any", zero_taps=plan["zero_taps"],
                          lds_bytes=plan["lds_bytes"],
                          batch_run_ms=round(ms, 3), resample_both_ms=round(mc, 3),
                          resample_both_with_lengths_ms=round(ml, 3),
                          resample_over_step=round(mc / ms, 4), shader_clock_mhz=round(statistics.median(clk), 1),
                          gbytes=round(nbytes / 1e9, 2), gfma=round(fma / 1e9, 1),
                          hbm_share_of_8TBs=round(nbytes / (mc * 1e-3) / 8.0e12, 4),
                          fp64_share_of_78_6TF=round(2 * fma / (mc * 1e-3) / 78.6e12, 4),
                          cpu_one_pair_s=None if cpu_pair is None else round(cpu_pair, 3),
                          cpu_batch_s_one_core=None if cpu_pair is None else round(cpu_pair * args.pairs, 1),
                          batch_run_ms_all=[round(x, 3) for x in ts], resample_both_ms_all=[round(x, 3) for x in tc])),
          flush=True)


if __name__ == "__main__":
    main()

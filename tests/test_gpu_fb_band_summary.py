"""Band summaries of the filter-bank path (peaq_batch_run_fb_band_summary, include/peaq_amd.h): the 40-band terms behind
RmsModDiff, RmsNoiseLoudAsym and AvgLinDist reduced over each pair's counted blocks on the device.  Pinned here against
the device's own filter-bank band traces and block trace of the same inputs reduced in numpy
(tests/test_fb_band_summary_host.py::summarise_fb), against the CPU oracle, against the results of the same call (the
header's identities), across the launch seam of the filter-bank path, for what the call leaves untouched, and through
the host entry and the CLI.  Needs an MI355X (`-m gpu`).

Inputs: the four pairs of tests/test_fb_band_summary_host.py, mono and stereo, as one ragged batch -- plain, ragged,
gapped (blocks below the data boundary at the start, in the middle and at the end: what fails if the tentative logic is
wrong) and all-silent.

Sums against the device's traces: rows 0, 1 and 6, every count and the sum of W add the same terms in the same order and
are held bit for bit; rows 2 .. 5 and the sum of W^2 multiply before they add, which the device may fuse: 1e-12 relative,
the bound tests/test_gpu_band_summary.py holds its fused rows to (at most 3 roundings per block on non-negative terms,
1000 blocks at the most here: 3000 x 2^-53 = 3.4e-13).  Measured on the first run on an MI355X: every row
but MODDIFF_SQ bit for bit on all pairs, MODDIFF_SQ and the sum of W^2 within 7.9e-16; the term rows against the recipe
at most 2.6e-13 (MODDIFF_WSUM), 2.7e-13 (MODDIFF_SQ), 2.4e-13 (NOISELOUD_SQ), 2.1e-12 (MISSING_SQ) and 5.0e-10
(LINDIST_SUM); the identities within 4.4e-16 in both FIR modes."""
import subprocess

import numpy as np
import pytest

import gst_env
from test_conformance_runner import write_wav
from test_fb_band_summary_host import (GAPPED, NB, PLANES, R, ROW, ROWS, SILENT, VIEWS, all_pairs, counted_range,
                                       counts_of, flags_of, movs_of, oracle_inputs, summarise_fb)
from test_gpu_fb_bands import TERM_BOUND, deviation, recipe
from test_gpu_trajectory import to_device

pytestmark = pytest.mark.gpu

SENTINEL = -777.25                                   # what the tests put into the summary array before a run
ABOVE = 1
EXACT = (0, 1, 6)                                    # rows held bit for bit; the others to 1e-12
INPUTS = ["unsm_ref", "unsm_test", "exc_ref", "exc_test"]


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback in the product)")
    import gpu_common
    return gpu_common


_RUNS, _TRACES = {}, {}


def run(gpu, channels, swap=1):
    """the four pairs as one ragged batch -> (batch_fb_band_summary's dict, the whole summary array as numpy
    [pairs + 1, channels, 7, 42]); the array is one pair longer than the batch and full of SENTINEL first.  One run per
    argument set and FIR mode, shared by the tests"""
    import gstpeaq_amd
    import torch
    key = (gpu.mode(), channels, swap)
    if key not in _RUNS:
        ref, test, n_ref, n_test = to_device(all_pairs(channels))
        whole = torch.full((5, channels, R, ROW), SENTINEL, dtype=torch.float64, device="cuda")
        ctx = gpu.ctx()
        try:
            if not swap:
                ctx.set_settings(swap_mod_patts_for_noise_loudness_movs=0)
            out = gstpeaq_amd.batch_fb_band_summary(ctx, ref, test, n_ref, n_test, d_summary=whole)
        finally:
            ctx.set_settings()
        _RUNS[key] = (out, whole.cpu().numpy())
    return _RUNS[key]


def device_traces(gpu, channels):
    """the filter-bank band traces (all planes) and the block trace of the same batch: (dict plane name -> [pairs,
    blocks, channels, 40], the block records [pairs][blocks]); computed once per FIR mode, shared, never changed"""
    import gstpeaq_amd
    key = (gpu.mode(), channels)
    if key not in _TRACES:
        ref, test, n_ref, n_test = to_device(all_pairs(channels))
        ctx = gpu.ctx()
        bands = gstpeaq_amd.batch_fb_bands(ctx, ref, test, 0x1FFF, n_ref, n_test)
        trace = gstpeaq_amd.batch_trace(ctx, 1, ref, test, n_ref, n_test)
        _TRACES[key] = ({k: bands[k] for k in PLANES + INPUTS[:2]}, trace["blocks"])
    return _TRACES[key]


def rel(got, want):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(want != 0., np.abs(got - want) / np.abs(want), np.abs(got))


def check_against_traces(label, got, planes, blocks, channels):
    """one pair's rows [channels, 7, 42] against summarise_fb() of its device traces; -> the largest relative deviation
    of the fused rows"""
    flags = blocks["flags"]
    want = summarise_fb(planes, flags, blocks["ch"][:, :channels, :])
    worst = 0.
    for k in range(R):
        dev = float(np.max(rel(got[:, k], want[:, k])))
        print(f"fb-band-summary-measure {label} {ROWS[k]}: max rel dev {dev:.3e}, bit for bit: "
              f"{got[:, k].tobytes() == want[:, k].tobytes()}")
        if k in EXACT:
            assert got[:, k].tobytes() == want[:, k].tobytes(), (label, ROWS[k])
        else:
            np.testing.assert_allclose(got[:, k], want[:, k], rtol=1e-12, atol=0, err_msg=f"{label} {ROWS[k]}")
            worst = max(worst, dev)
    assert np.array_equal(got[:, (0, 1, 2, 4, 5, 6), NB], want[:, (0, 1, 2, 4, 5, 6), NB]), label   # n, m and sum W
    assert not got[:, :, NB + 1].any(), label
    return worst


# ---- 1: against the device's own traces ------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
def test_rows_are_the_device_s_traces_reduced_over_the_counted_blocks(gpu, channels):
    """(on the default engine, whose filter bank gives two runs the same bits: the summary and its traces are runs of
    their own, and the reduced-precision bank's sums meet in LDS atomics in the order the waves arrive, peaq_fb.hip)"""
    out, whole = run(gpu, channels)
    planes, blocks = device_traces(gpu, channels)
    assert out["rows"].shape == (4, channels, R, ROW)
    worst = 0.
    for p, nblk in enumerate(counts_of(channels)):
        bl = blocks[p][:nblk]
        assert np.array_equal(bl["flags"], flags_of(channels, p)), p           # (the device's flags are the CPU's restatement)
        worst = max(worst, check_against_traces(f"mode={gpu.mode()} channels={channels} pair={p}", out["rows"][p],
                                                {k: v[p, :nblk] for k, v in planes.items()}, bl, channels))
    print(f"fb-band-summary-measure mode={gpu.mode()} channels={channels}: fused rows within {worst:.3e}")
    assert [int(c) for c in out["counted"][:, 0]] == [201, 197, 180, 0]
    assert not out["rows"][SILENT].any() and all(np.isnan(out[v][SILENT]).all() for v in VIEWS)
    assert out["rows"][GAPPED][0, 4, NB] > 0
    assert (whole[4] == SENTINEL).all()


# ---- 2: against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
def test_rows_match_the_oracle_and_the_recipe_on_the_device_s_inputs(gpu, channels, fir_mode):
    """the excitation means against the oracle's block records at the FIR mode's per-block tolerance (a mean of
    non-negative values inherits its terms' relative bound); the term rows against summarise_fb() of the recipe fed with
    the device's own input planes, at the per-plane bounds of tests/test_gpu_fb_bands.py"""
    from gstpeaq_amd.capi import _fb_band_summary_views
    out, _ = run(gpu, channels)
    planes, _ = device_traces(gpu, channels)
    for p, nblk in enumerate(counts_of(channels)[:SILENT]):
        flags = flags_of(channels, p)
        inp = oracle_inputs(channels, p)
        zeros = np.zeros_like(inp["exc_ref"])
        want = _fb_band_summary_views(summarise_fb(dict(exc_ref=inp["exc_ref"], exc_test=inp["exc_test"],
                                                        **{k: zeros for k in PLANES[2:]}), flags))
        for name in ("exc_ref_mean", "exc_test_mean"):
            np.testing.assert_allclose(out[name][p], want[name], rtol=gpu.tol("blocks"), atol=0, err_msg=f"pair {p} {name}")
        assert np.array_equal(out["counted"][p], want["counted"]), p
        dev_in = {k: planes[k][p, :nblk] for k in INPUTS}
        with np.errstate(divide="ignore", invalid="ignore"):                   # (silent stretches: blocks that are not read)
            rec = recipe(dev_in)
        term = summarise_fb(dict(exc_ref=dev_in["exc_ref"], exc_test=dev_in["exc_test"], **{k: rec[k] for k in PLANES[2:]}),
                            flags)
        for k, plane in ((2, "moddiff"), (3, "moddiff"), (4, "noiseloud"), (5, "missing"), (6, "lindist")):
            dev = float(np.max(deviation(out["rows"][p][:, k, :NB], term[:, k, :NB])))
            print(f"fb-band-summary-measure mode={gpu.mode()} channels={channels} pair={p} {ROWS[k]} against the recipe: "
                  f"max deviation {dev:.3e}")
            assert dev <= TERM_BOUND[plane], (p, ROWS[k], dev)


# ---- 3: identities with the results of the same call -----------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
def test_identities_with_the_results_of_the_same_call(gpu, channels, fir_mode):
    out, _ = run(gpu, channels)
    _, blocks = device_traces(gpu, channels)
    for p, nblk in enumerate(counts_of(channels)):
        rows, movs = out["rows"][p], out["results"][p]["movs"]
        got = movs_of(rows)
        if p == SILENT:
            assert np.isnan(got).all() and np.isnan([movs[0], movs[1], movs[4]]).all()
            continue
        dev = [g / w - 1. for g, w in zip(got, (movs[0], movs[1], movs[4]))]
        print(f"fb-band-summary-measure mode={gpu.mode()} channels={channels} pair={p} identities: RmsModDiff {dev[0]:+.3e}, "
              f"RmsNoiseLoudAsym {dev[1]:+.3e}, AvgLinDist {dev[2]:+.3e}")
        assert max(abs(x) for x in dev) <= 1e-10, (p, got, movs)
        if gpu.mode() != "default":                      # (the block trace is another run: see test 1)
            continue
        # sum_b row2 is the sum over the counted MOD_OPEN blocks of W D, from the block trace
        bl = blocks[p][:nblk]
        a, b = counted_range(bl["flags"])
        sel = np.arange(max(a, 125), b + 1)
        wd = (bl["ch"][sel, :channels, 1] * bl["ch"][sel, :channels, 0]).sum(axis=0) * np.sqrt(40.) / 100.
        np.testing.assert_allclose(rows[:, 2, :NB].sum(axis=-1), wd, rtol=1e-10, atol=0, err_msg=f"pair {p}")
        np.testing.assert_allclose(out["moddiff"][p].sum(axis=-1) * out["rows"][p][:, 2, NB], wd, rtol=1e-10)


# ---- 4: the results --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("swap", [1, 0])
@pytest.mark.parametrize("channels", [1, 2])
def test_results_are_batch_run_s_bytes(gpu, channels, swap):
    """(two runs: on the default engine, see test 1)"""
    import gstpeaq_amd
    import torch
    out, _ = run(gpu, channels, swap)
    ref, test, n_ref, n_test = to_device(all_pairs(channels))
    ctx = gpu.ctx()
    try:
        if not swap:
            ctx.set_settings(swap_mod_patts_for_noise_loudness_movs=0)
        plain = gstpeaq_amd.batch_run(ctx, 1, ref, test, n_ref, n_test, sync=False)
    finally:
        ctx.set_settings()
    torch.cuda.synchronize()
    assert plain.cpu().numpy().tobytes() == out["d_results"].cpu().numpy().tobytes()
    if not swap:                                         # the switch reaches MISSING and LINDIST and nothing else
        dflt, _ = run(gpu, channels, 1)
        assert out["rows"][:, :, :5].tobytes() == dflt["rows"][:, :, :5].tobytes()
        assert not np.array_equal(out["rows"][:3, :, 5], dflt["rows"][:3, :, 5])
        assert not np.array_equal(out["rows"][:3, :, 6], dflt["rows"][:3, :, 6])


# ---- 5: launch seam --------------------------------------------------------------------------------------------------
def test_rows_across_the_launch_seam(gpu):
    """four stereo pairs of 192 000 samples: 1000 blocks, two launches of the filter-bank path at 840 blocks each.  Pair
    0 is untouched; pair 1 is silent until block 845, so its first counted block lies behind the seam (kInit handed
    over); pair 2 is silent over blocks 830 .. 850, a tentative run across the seam that is taken back; pair 3 is
    silent from block 835 on, tentative across the seam and restored at the end"""
    import gstpeaq_amd
    import torch
    ctx = gpu.ctx()
    n = 192000
    ref, test = gstpeaq_amd.synth_fill(ctx, 700, 4, 2, n)
    for p, (a, b) in {1: (0, 845 * 192), 2: (830 * 192, 851 * 192), 3: (835 * 192, n)}.items():
        ref[p, a:b] = 0
        test[p, a:b] = 0
    assert gstpeaq_amd.frame_count(n, n, True) == 1000
    out = gstpeaq_amd.batch_fb_band_summary(ctx, ref, test)
    assert ctx.last_timing()["fb_launches"] == 2, ctx.last_timing()
    plain = gstpeaq_amd.batch_run(ctx, 1, ref, test, sync=False)
    torch.cuda.synchronize()
    assert plain.cpu().numpy().tobytes() == out["d_results"].cpu().numpy().tobytes()
    bands = gstpeaq_amd.batch_fb_bands(ctx, ref, test, PLANES)
    blocks = gstpeaq_amd.batch_trace(ctx, 1, ref, test)["blocks"]
    spans, worst = [], 0.
    for p in range(4):
        bl = blocks[p][:1000]
        spans.append(counted_range(bl["flags"]))
        worst = max(worst, check_against_traces(f"seam pair={p}", out["rows"][p], {k: bands[k][p] for k in PLANES}, bl, 2))
        assert int(out["counted"][p, 0]) == spans[-1][1] - spans[-1][0] + 1 == int(out["counted"][p, 1]), (p, spans)
    print(f"fb-band-summary-measure launch seam: counted blocks {spans}, fused rows within {worst:.3e}")
    assert spans[0] == (0, 999) and spans[2] == (0, 999), spans
    assert spans[1][0] >= 845 and spans[1][1] == 999, spans
    assert spans[3][0] == 0 and 830 <= spans[3][1] < 840, spans
    below = np.flatnonzero((blocks[2][:1000]["flags"] & ABOVE) == 0)
    assert {839, 840} <= set(below.tolist()) and below.min() >= 829 and below.max() <= 851, below


# ---- 6: what the call leaves alone -----------------------------------------------------------------------------------
def test_nothing_leaks_into_a_later_run_and_a_summary_is_the_same_run_to_run(gpu):
    """the same call twice gives the same bytes; a batch_run and a batch_band_summary after it on the same context give
    what they give on a fresh context (the FFT summary shares the context's saved copy with this one)"""
    import gstpeaq_amd
    import torch
    ref, test, n_ref, n_test = to_device(all_pairs(2))
    ctx = gpu.ctx()
    fresh_ctx = gstpeaq_amd.Context(0)
    f_run = gstpeaq_amd.batch_run(fresh_ctx, 1, ref, test, n_ref, n_test, sync=False)
    f_sum = gstpeaq_amd.batch_band_summary(fresh_ctx, 1, ref, test, n_ref, n_test, sync=False)
    f_sum0 = gstpeaq_amd.batch_band_summary(fresh_ctx, 0, ref, test, n_ref, n_test, sync=False)
    first = gstpeaq_amd.batch_fb_band_summary(ctx, ref, test, n_ref, n_test, sync=False)
    after = gstpeaq_amd.batch_run(ctx, 1, ref, test, n_ref, n_test, sync=False)
    again = gstpeaq_amd.batch_fb_band_summary(ctx, ref, test, n_ref, n_test, sync=False)
    summ = gstpeaq_amd.batch_band_summary(ctx, 1, ref, test, n_ref, n_test, sync=False)
    gstpeaq_amd.batch_fb_band_summary(ctx, ref, test, n_ref, n_test, sync=False)
    summ0 = gstpeaq_amd.batch_band_summary(ctx, 0, ref, test, n_ref, n_test, sync=False)
    torch.cuda.synchronize()
    assert first["d_results"].cpu().numpy().tobytes() == f_run.cpu().numpy().tobytes()
    assert after.cpu().numpy().tobytes() == f_run.cpu().numpy().tobytes()
    for k in ("d_summary", "d_results"):
        assert first[k].cpu().numpy().tobytes() == again[k].cpu().numpy().tobytes(), k
        assert summ[k].cpu().numpy().tobytes() == f_sum[k].cpu().numpy().tobytes(), k
        assert summ0[k].cpu().numpy().tobytes() == f_sum0[k].cpu().numpy().tobytes(), k
    fresh_ctx.close()


# ---- 7: host entry and CLI -------------------------------------------------------------------------------------------
def test_host_memory_entry_equals_the_batch_entry(gpu):
    import gstpeaq_amd
    r, t = all_pairs(2)[GAPPED]
    host = gstpeaq_amd.run_pair_fb_band_summary(gpu.ctx(), r, t)
    every, _ = run(gpu, 2)
    assert host["rows"].shape == (2, R, ROW) and host["rows"].tobytes() == every["rows"][GAPPED].tobytes()
    for name in VIEWS + ["counted"]:
        assert np.array_equal(host[name], every[name][GAPPED], equal_nan=True), name
    for key in ("movs", "di", "odg", "totalsnr", "frames", "fb_blocks"):
        np.testing.assert_array_equal(host["result"][key], every["results"][GAPPED][key])


def test_host_memory_entry_with_rate_and_align_equals_the_batch_entry(gpu):
    """the gapped pair taken as 44.1 kHz material, the test signal 200 samples late: conversion and alignment happen on
    the device in both entries"""
    import gstpeaq_amd
    import torch
    r, t = all_pairs(2)[GAPPED]
    t = np.concatenate([np.zeros((200, 2), dtype=np.float32), t])[:len(r)]
    host = gstpeaq_amd.run_pair_fb_band_summary(gpu.ctx(), r, t, rate=44100, align=1024)
    d_ref, d_test = torch.from_numpy(r[None]).cuda(), torch.from_numpy(t[None]).cuda()
    batch = gstpeaq_amd.batch_fb_band_summary(gpu.ctx(), d_ref, d_test, rate=44100, align=1024)
    assert host["rows"].tobytes() == batch["rows"][0].tobytes() and host["rows"][0, 0, NB] > 150
    assert abs(host["delay"]["lag"] - round(200 * 48000 / 44100)) <= 1
    np.testing.assert_array_equal(host["result"]["movs"], batch["results"][0]["movs"])


def test_cli_fb_band_summary(gpu, tmp_path):
    """`peaq --advanced --fb-band-summary=FILE`: the CSV parses back to the doubles of run_pair_fb_band_summary (%.17g),
    one line per (channel, band) with the band's centre frequency, the seven rows' values and their denominators; the
    printed lines are those printed without the flag"""
    import gstpeaq_amd
    r, t = all_pairs(2)[GAPPED]
    write_wav(tmp_path / "ref.wav", r, bits=32, fmt_float=True)
    write_wav(tmp_path / "test.wav", t, bits=32, fmt_float=True)
    csv = tmp_path / "summary.csv"
    plain = subprocess.run([str(gst_env.CLI), "--advanced", tmp_path / "ref.wav", tmp_path / "test.wav"],
                           capture_output=True, text=True, timeout=300)
    out = subprocess.run([str(gst_env.CLI), "--advanced", f"--fb-band-summary={csv}", tmp_path / "ref.wav",
                          tmp_path / "test.wav"], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and out.returncode == 0, (plain.stderr, out.stderr, out.stdout)
    assert out.stdout == plain.stdout and "Objective Difference Grade" in out.stdout
    exp = gstpeaq_amd.run_pair_fb_band_summary(gpu.ctx(), r, t)
    lines = csv.read_text().strip().splitlines()
    assert lines[0].split(",") == ["channel", "band", "fc"] + ROWS + ["counted", "modwt_sum", "modwt_sq_sum", "loud_blocks"]
    rows = [ln.split(",") for ln in lines[1:]]
    assert len(rows) == 2 * NB
    it = iter(rows)
    for c in range(2):
        for b in range(NB):
            row = next(it)
            assert (int(row[0]), int(row[1])) == (c, b) and float(row[2]) == exp["fc"][b]
            got = np.array([float(v) for v in row[3:]])
            want = [exp["rows"][c, k, b] for k in range(R)] + [exp["rows"][c, k, NB] for k in (0, 2, 3, 4)]
            assert got.tobytes() == np.array(want).tobytes(), (c, b)

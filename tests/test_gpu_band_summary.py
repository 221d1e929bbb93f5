"""Band summaries (peaq_batch_run_band_summary, include/peaq_amd.h): the FFT path's per-band values reduced over each
pair's counted frames on the device.  Pinned here against the device's own band traces of the same inputs reduced in
numpy (tests/test_band_summary_host.py::summarise with the frame trace's flags), against the CPU oracle's planes, against
the results of the same call (the header's identities), across the batch path's launch boundaries, for what the call
leaves untouched, and through the host entry and the CLI.  Needs an MI355X (`-m gpu`).

Inputs: the five pairs of tests/test_band_summary_host.py, mono and stereo -- the three pairs of tests/test_gpu_bands.py,
the gapped pair (frames below the data boundary at the start, in the middle and at the end: what fails if the tentative
logic is wrong) and the all-silent pair.

Sums against the device's traces: the same terms in the same order, so rows 0, 3, 4 and 7 are expected bit for bit (the
test prints whether they are); asserted to 1e-12 relative -- at most 2 roundings per frame on non-negative terms, fewer
than 64 frames, 128 x 2^-53 = 1.4e-14.  Measured on the first passing run on an MI355X: rows 0, 3, 4 and 7
bit for bit, rows 1 and 2 and every count too, both versions, all pairs; rows 5 and 6 within 3.4e-16 (the device fuses the
product of the weight and the term into the sum), the sums of the weights exact."""
import subprocess

import numpy as np
import pytest

import gst_env
import oracle_lib as orc
from test_band_summary_host import (DISTURBED, GAPPED, ROWS, SILENT, all_pairs, counts_of, flags_of, movs_of,
                                    oracle_planes, summarise)
from test_conformance_runner import write_wav
from test_gpu_pattern_bands import TERM_BOUND, deviation
from test_gpu_trajectory import to_device
from test_pattern_bands_host import recipe

pytestmark = pytest.mark.gpu

SENTINEL = -777.25                                   # what the tests put into the summary array before a run
ABOVE = 1
NB = {0: 109, 1: 55}
SUMS, COUNTS = (0, 3, 4, 7), (0, 1, 2, 3, 4, 7)      # rows expected bit for bit; rows whose denominator is a count


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback in the product)")
    import gpu_common
    return gpu_common


_RUNS, _TRACES = {}, {}


def run(gpu, advanced, channels):
    """the five pairs as one ragged batch -> (batch_band_summary's dict, the whole summary array as numpy
    [pairs + 1, channels, R, row]); the array is one pair longer than the batch and full of SENTINEL first.  One run per
    argument set, shared by the tests"""
    import gstpeaq_amd
    import torch
    key = (gpu.mode(), advanced, channels)
    if key not in _RUNS:
        ref, test, n_ref, n_test = to_device(all_pairs(channels))
        whole = torch.full((6, channels, 4 if advanced else 8, NB[advanced] + 1), SENTINEL, dtype=torch.float64, device="cuda")
        out = gstpeaq_amd.batch_band_summary(gpu.ctx(), advanced, ref, test, n_ref, n_test, d_summary=whole)
        _RUNS[key] = (out, whole.cpu().numpy())
    return _RUNS[key]


def device_traces(gpu, advanced, channels):
    """the band traces, the pattern-band traces (basic version) and the frame trace of the same batch: (dict plane name
    -> [pairs, frames, channels, nb], the frame records [pairs][frames]); computed once, shared, never changed"""
    import gstpeaq_amd
    key = (gpu.mode(), advanced, channels)
    if key not in _TRACES:
        ref, test, n_ref, n_test = to_device(all_pairs(channels))
        ctx = gpu.ctx()
        names = ("nmr", "exc_ref") if advanced else ("nmr", "exc_ref", "exc_test")
        bands = gstpeaq_amd.batch_bands(ctx, advanced, ref, test, names, n_ref, n_test)
        planes = {k: bands[k] for k in names}
        if not advanced:
            pat = gstpeaq_amd.batch_pattern_bands(ctx, ref, test, ("moddiff1", "moddiff2", "modwt", "noiseloud", "unsm_ref",
                                                                   "unsm_test"), n_ref, n_test)
            planes.update({k: pat[k] for k in ("moddiff1", "moddiff2", "modwt", "noiseloud", "unsm_ref", "unsm_test")})
        trace = gstpeaq_amd.batch_trace(ctx, advanced, ref, test, n_ref, n_test)
        _TRACES[key] = (planes, trace["frames"])
    return _TRACES[key]


def rel(got, want):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(want != 0., np.abs(got - want) / np.abs(want), np.abs(got))


# ---- 1: against the device's own band traces -----------------------------------------------------------------------
@pytest.mark.parametrize("advanced", [0, 1])
@pytest.mark.parametrize("channels", [1, 2])
def test_rows_are_the_device_s_band_traces_reduced_over_the_counted_frames(gpu, channels, advanced):
    out, whole = run(gpu, advanced, channels)
    planes, frames = device_traces(gpu, advanced, channels)
    nb = NB[advanced]
    assert out["rows"].shape == (5, channels, 4 if advanced else 8, nb + 1)
    exact = {k: True for k in SUMS if k < out["rows"].shape[2]}
    for p, nf in enumerate(counts_of(channels)):
        fr = frames[p][:nf]
        flags = fr["flags"]
        if p < SILENT:                                   # (the device's flags are the CPU's restatement)
            assert np.array_equal(flags & ABOVE, flags_of(channels, p) & ABOVE), p
        r = planes["nmr"][p, :nf]
        assert not (np.abs(r / DISTURBED - 1.) <= 1e-12).any(), p              # no ratio sits on the threshold
        weight = None if advanced else fr["ch"][:, :channels, 2]
        want = summarise({k: v[p, :nf] for k, v in planes.items() if not k.startswith("unsm")}, flags, weight)
        got = out["rows"][p]
        for k in range(got.shape[1]):
            worst = float(np.max(rel(got[:, k], want[:, k])))
            same = got[:, k].tobytes() == want[:, k].tobytes()
            print(f"band-summary-measure advanced={advanced} channels={channels} pair={p} {ROWS[k]}: max rel dev "
                  f"{worst:.3e}, bit for bit: {same}")
            if k in exact:
                exact[k] &= same
            if k == 2:
                assert np.array_equal(got[:, k], want[:, k]), (p, ROWS[k])
            else:
                np.testing.assert_allclose(got[:, k, :nb], want[:, k, :nb], rtol=1e-12, atol=0, err_msg=f"pair {p} {ROWS[k]}")
            if k in COUNTS:
                assert np.array_equal(got[:, k, nb], want[:, k, nb]), (p, ROWS[k])
            else:
                np.testing.assert_allclose(got[:, k, nb], want[:, k, nb], rtol=1e-12, atol=0, err_msg=f"pair {p} sum of W")
    print(f"band-summary-measure advanced={advanced} channels={channels} rows bit for bit over all pairs: "
          f"{ {ROWS[k]: v for k, v in exact.items()} }")
    counted = out["counted"]
    assert counted.shape == (5, channels) and [int(c) for c in counted[:, 0]] == [31, 31, 30, 37, 0]
    assert (whole[5] == SENTINEL).all()


# ---- 2: against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
def test_means_match_the_oracle_s_planes(gpu, channels):
    """the excitation means to 1e-9 and the noise-to-mask means to 1e-6 relative against summarise() on the oracle's
    planes with the CPU's flags (a time mean of non-negative values inherits its terms' relative bound); the term rows
    against summarise() on the recipe fed with the device's own unsmeared planes, at the per-plane bounds of
    tests/test_gpu_pattern_bands.py"""
    from gstpeaq_amd.capi import _band_summary_views
    out, _ = run(gpu, 0, channels)
    planes, _ = device_traces(gpu, 0, channels)
    for p, nf in enumerate(counts_of(channels)[:SILENT]):
        flags = flags_of(channels, p)
        want = _band_summary_views(summarise(oracle_planes(channels, p), flags), 109)
        for name, rtol in (("exc_ref_mean", 1e-9), ("exc_test_mean", 1e-9), ("nmr_mean", 1e-6), ("nmr_max", 1e-6)):
            np.testing.assert_allclose(out[name][p], want[name], rtol=rtol, atol=0, err_msg=f"pair {p} {name}")
        assert np.array_equal(out["counted"][p], want["counted"]), p
        rec = recipe({k: planes[k][p, :nf] for k in ("unsm_ref", "unsm_test")})
        rec["nmr"] = planes["nmr"][p, :nf]
        term = _band_summary_views(summarise(rec, flags), 109)
        for name, plane in (("moddiff1", "moddiff1"), ("moddiff2", "moddiff2"), ("noiseloud_mean", "noiseloud")):
            dev = float(np.max(deviation(out[name][p], term[name])))
            print(f"band-summary-measure channels={channels} pair={p} {name}: max deviation {dev:.3e}")
            assert dev <= TERM_BOUND[plane], (p, name, dev)


@pytest.mark.parametrize("channels", [1, 2])
def test_advanced_means_match_the_oracle_s_planes(gpu, channels):
    from gstpeaq_amd.capi import _band_summary_views
    out, _ = run(gpu, 1, channels)
    for p, (ref, test) in enumerate(all_pairs(channels)[:SILENT]):
        nf = counts_of(channels)[p]
        rec, tab = orc.frontend_records(55, ref, test, nf), orc.tables(55)
        sm, er = np.zeros((channels, 55)), np.zeros((nf, channels, 55))
        for f in range(nf):                              # fftearmodel.c:496-504
            sm = tab["ear_tc"] * sm + (1 - tab["ear_tc"]) * rec[f, :, 0:55]
            er[f] = np.maximum(sm, rec[f, :, 0:55])
        nmr = rec[:, :, 448:448 + 55] * tab["mask_diff"] / er
        want = _band_summary_views(summarise(dict(nmr=nmr, exc_ref=er), flags_of(channels, p)), 55)
        np.testing.assert_allclose(out["exc_ref_mean"][p], want["exc_ref_mean"], rtol=1e-9, atol=0, err_msg=f"pair {p}")
        for name in ("nmr_mean", "nmr_max"):
            np.testing.assert_allclose(out[name][p], want[name], rtol=1e-6, atol=0, err_msg=f"pair {p} {name}")
        assert np.array_equal(out["counted"][p], want["counted"]), p


# ---- 3: identities with the results of the same call -------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
def test_identities_with_the_results_of_the_same_call(gpu, channels):
    """TotalNMR, AvgModDiff1 and AvgModDiff2 from the rows at the host test's tolerances; the RelDistFrames inequality
    (summed over the channels: the MOV is their mean); d_results are peaq_batch_run's bytes; the silent pair reads zeros,
    its named views NaN like its MOVs"""
    import gstpeaq_amd
    import torch
    out, _ = run(gpu, 0, channels)
    ref, test, n_ref, n_test = to_device(all_pairs(channels))
    plain = gstpeaq_amd.batch_run(gpu.ctx(), 0, ref, test, n_ref, n_test, sync=False)
    torch.cuda.synchronize()
    assert plain.cpu().numpy().tobytes() == out["d_results"].cpu().numpy().tobytes()
    for p in range(5):
        rows, movs = out["rows"][p], out["results"][p]["movs"]
        nmr, md1, md2 = movs_of(rows)
        if p == SILENT:
            assert not rows.any() and np.isnan([nmr, md1, md2]).all() and np.isnan([movs[2], movs[6], movs[7]]).all()
            for name in ("nmr_mean", "nmr_max", "nmr_disturbed", "exc_ref_mean", "exc_test_mean", "moddiff1", "moddiff2",
                         "noiseloud_mean"):
                assert np.isnan(out[name][p]).all(), name
            continue
        assert abs(nmr - movs[2]) <= 1e-9, (p, nmr, movs[2])
        assert abs(md1 / movs[6] - 1.) <= 1e-10 and abs(md2 / movs[7] - 1.) <= 1e-10, (p, md1, md2, movs)
        n = rows[0, 2, 109]
        disturbed = movs[10] * n * channels              # disturbed counted frames, summed over the channels
        assert rows[:, 2, :109].max(axis=-1).sum() <= disturbed + 1e-6 <= rows[:, 2, :109].sum() + 2e-6, (p, disturbed)
        np.testing.assert_allclose(out["moddiff1"][p].sum(axis=-1).mean(), movs[6], rtol=1e-10)


@pytest.mark.parametrize("channels", [1, 2])
def test_advanced_results_are_batch_run_s_and_the_row_sum_is_the_trace_s(gpu, channels):
    """sum_b row0 / nb is the sum over the counted frames of the frame trace's ch[c][1]"""
    import gstpeaq_amd
    import torch
    out, _ = run(gpu, 1, channels)
    _, frames = device_traces(gpu, 1, channels)
    ref, test, n_ref, n_test = to_device(all_pairs(channels))
    plain = gstpeaq_amd.batch_run(gpu.ctx(), 1, ref, test, n_ref, n_test, sync=False)
    torch.cuda.synchronize()
    assert plain.cpu().numpy().tobytes() == out["d_results"].cpu().numpy().tobytes()
    for p, nf in enumerate(counts_of(channels)):
        fr = frames[p][:nf]
        above = np.flatnonzero(fr["flags"] & ABOVE)
        want = fr["ch"][above[0]:above[-1] + 1, :channels, 1].sum(axis=0) if above.size else np.zeros(channels)
        np.testing.assert_allclose(out["rows"][p][:, 0, :55].sum(axis=-1) / 55, want, rtol=1e-12, atol=0, err_msg=f"pair {p}")


# ---- 4: launch boundaries ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("advanced", [0, 1])
def test_rows_across_launch_boundaries(gpu, advanced):
    """256 stereo pairs of 5 s, the shape the band-trace tests cross launches with: 234 frames in 4 back-end launches of
    64.  Four pairs are silenced in stretches that straddle a seam: one starts below the boundary until frame 66, one
    has an interior gap over frames 60 .. 70, one ends below it from frame 185 on (a tentative run handed from launch to
    launch and never taken back), one has all three.  Their summaries are bit for bit those of a batch of their own,
    whose frames are one launch; the results are peaq_batch_run's bytes"""
    import gstpeaq_amd
    import torch
    ctx = gpu.ctx()
    n, pairs = 240000, 256
    ref, test = gstpeaq_amd.synth_fill(ctx, 700, pairs, 2, n)
    lead, gap, tail = (0, 67 * 1024), (59 * 1024, 72 * 1024), (185 * 1024, n)
    own = {0: [], 37: [lead], 64: [gap], 127: [tail], 200: [lead, (100 * 1024, 130 * 1024), tail]}
    for p, cuts in own.items():
        for a, b in cuts:
            ref[p, a:b] = 0
            test[p, a:b] = 0
    assert gstpeaq_amd.frame_count(n, n) == 234
    out = gstpeaq_amd.batch_band_summary(ctx, advanced, ref, test, sync=False)
    tm = ctx.last_timing()
    assert tm["frontend_launches"] == 4 and tm["backend_launches"] == 4, tm
    whole = gstpeaq_amd.batch_run(ctx, advanced, ref, test, sync=False)
    torch.cuda.synchronize()
    assert whole.cpu().numpy().tobytes() == out["d_results"].cpu().numpy().tobytes()
    idx = list(own)
    sub = gstpeaq_amd.batch_band_summary(ctx, advanced, ref[idx].contiguous(), test[idx].contiguous())
    assert ctx.last_timing()["frontend_launches"] == 1
    big = out["d_summary"].cpu().numpy()
    assert sub["rows"].tobytes() == big[idx].tobytes()
    assert sub["d_results"].cpu().numpy().tobytes() == out["d_results"][idx].cpu().numpy().tobytes()
    # what the cuts were made for, on the frame trace of the five pairs: the counted range starts behind the first seam,
    # a run of frames below the boundary lies across a seam inside it, or it ends before the last seam
    frames = gstpeaq_amd.batch_trace(ctx, advanced, ref[idx].contiguous(), test[idx].contiguous())["frames"]
    spans = []
    for i in range(len(idx)):
        above = np.flatnonzero(frames[i]["flags"][:234] & ABOVE)
        spans.append((int(above[0]), int(above[-1])))
        assert int(sub["counted"][i, 0]) == spans[-1][1] - spans[-1][0] + 1 == int(sub["counted"][i, 1]), (i, spans)
        below = np.flatnonzero((frames[i]["flags"][spans[-1][0]:spans[-1][1] + 1] & ABOVE) == 0) + spans[-1][0]
        if idx[i] == 64:
            assert {63, 64} <= set(below.tolist()), below
    print(f"band-summary-measure advanced={advanced} launch boundaries: counted frames {spans}")
    assert spans[1][0] > 64 and spans[4][0] > 64 and spans[3][1] < 191 and spans[4][1] < 191, spans
    assert spans[0][0] < 64 and spans[0][1] > 192 and spans[2][0] < 64 and spans[2][1] > 192, spans


# ---- 5: what the call leaves alone -----------------------------------------------------------------------------------------
def test_nothing_leaks_into_a_later_run_and_a_summary_is_the_same_run_to_run(gpu):
    """a batch_run, a batch_trace and a batch_bands after a summary run on the same context return the bytes they return
    on a fresh context; the summary is bit-identical run to run (memory behind the batch: asserted in test 1)"""
    import gstpeaq_amd
    import torch
    ref, test, n_ref, n_test = to_device(all_pairs(2))
    ctx = gpu.ctx()
    fresh_ctx = gstpeaq_amd.Context(0)
    f_run = gstpeaq_amd.batch_run(fresh_ctx, 0, ref, test, n_ref, n_test, sync=False)
    f_trace = gstpeaq_amd.batch_trace(fresh_ctx, 0, ref, test, n_ref, n_test, sync=False)
    f_bands = gstpeaq_amd.batch_bands(fresh_ctx, 0, ref, test, 31, n_ref, n_test, sync=False)
    first = gstpeaq_amd.batch_band_summary(ctx, 0, ref, test, n_ref, n_test, sync=False)
    after = gstpeaq_amd.batch_run(ctx, 0, ref, test, n_ref, n_test, sync=False)
    again = gstpeaq_amd.batch_band_summary(ctx, 0, ref, test, n_ref, n_test, sync=False)
    trace = gstpeaq_amd.batch_trace(ctx, 0, ref, test, n_ref, n_test, sync=False)
    gstpeaq_amd.batch_band_summary(ctx, 0, ref, test, n_ref, n_test, sync=False)
    bands = gstpeaq_amd.batch_bands(ctx, 0, ref, test, 31, n_ref, n_test, sync=False)
    torch.cuda.synchronize()
    assert first["d_results"].cpu().numpy().tobytes() == f_run.cpu().numpy().tobytes()
    assert after.cpu().numpy().tobytes() == f_run.cpu().numpy().tobytes()
    for k in ("d_summary", "d_results"):
        assert first[k].cpu().numpy().tobytes() == again[k].cpu().numpy().tobytes(), k
    for k in ("d_bands", "d_results"):
        assert bands[k].cpu().numpy().tobytes() == f_bands[k].cpu().numpy().tobytes(), k
    for k in ("d_frames", "d_results"):
        assert trace[k].cpu().numpy().tobytes() == f_trace[k].cpu().numpy().tobytes(), k
    fresh_ctx.close()


# ---- 6: host entry and CLI -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("advanced", [0, 1])
def test_host_memory_entry_equals_the_batch_entry(gpu, advanced):
    import gstpeaq_amd
    r, t = all_pairs(2)[GAPPED]
    host = gstpeaq_amd.run_pair_band_summary(gpu.ctx(), advanced, r, t)
    every, _ = run(gpu, advanced, 2)
    assert host["rows"].tobytes() == every["rows"][GAPPED].tobytes()
    for name in ("nmr_mean", "nmr_max", "nmr_disturbed", "exc_ref_mean"):
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
    host = gstpeaq_amd.run_pair_band_summary(gpu.ctx(), 0, r, t, rate=44100, align=1024)
    d_ref, d_test = torch.from_numpy(r[None]).cuda(), torch.from_numpy(t[None]).cuda()
    batch = gstpeaq_amd.batch_band_summary(gpu.ctx(), 0, d_ref, d_test, rate=44100, align=1024)
    assert host["rows"].tobytes() == batch["rows"][0].tobytes() and host["rows"][0, 0, 109] > 30
    assert abs(host["delay"]["lag"] - round(200 * 48000 / 44100)) <= 1
    np.testing.assert_array_equal(host["result"]["movs"], batch["results"][0]["movs"])


@pytest.mark.parametrize("advanced", [0, 1])
def test_cli_band_summary(gpu, advanced, tmp_path):
    """`peaq --band-summary=FILE`: the CSV parses back to the doubles of run_pair_band_summary (%.17g), one line per
    (channel, band) with the band's centre frequency, the rows' values and their denominators; the printed lines are
    those printed without the flag"""
    import gstpeaq_amd
    r, t = all_pairs(2)[GAPPED]
    write_wav(tmp_path / "ref.wav", r, bits=32, fmt_float=True)
    write_wav(tmp_path / "test.wav", t, bits=32, fmt_float=True)
    csv = tmp_path / "summary.csv"
    flags = ["--advanced"] if advanced else []
    plain = subprocess.run([str(gst_env.CLI), *flags, tmp_path / "ref.wav", tmp_path / "test.wav"],
                           capture_output=True, text=True, timeout=300)
    out = subprocess.run([str(gst_env.CLI), *flags, f"--band-summary={csv}", tmp_path / "ref.wav", tmp_path / "test.wav"],
                         capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and out.returncode == 0, (plain.stderr, out.stderr, out.stdout)
    assert out.stdout == plain.stdout and "Objective Difference Grade" in out.stdout
    exp = gstpeaq_amd.run_pair_band_summary(gpu.ctx(), advanced, r, t)
    nb, names = NB[advanced], ROWS[:4 if advanced else 8]
    lines = csv.read_text().strip().splitlines()
    dens = ["counted"] if advanced else ["counted", "modwt_sum", "loud_frames"]
    assert lines[0].split(",") == ["channel", "band", "fc"] + names + dens
    rows = [ln.split(",") for ln in lines[1:]]
    assert len(rows) == 2 * nb
    it = iter(rows)
    for c in range(2):
        for b in range(nb):
            row = next(it)
            assert (int(row[0]), int(row[1])) == (c, b) and float(row[2]) == exp["fc"][b]
            got = np.array([float(v) for v in row[3:]])
            want = [exp["rows"][c, k, b] for k in range(len(names))] + [exp["rows"][c, 0, nb]]
            if not advanced:
                want += [exp["rows"][c, 5, nb], exp["rows"][c, 7, nb]]
            assert got.tobytes() == np.array(want).tobytes(), (c, b)

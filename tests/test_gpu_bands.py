"""Band traces (peaq_batch_run_bands, include/peaq_amd.h): the FFT path's values per frame, channel and critical band of
every pair of a batch, before accumulation -- pinned here against values computed in numpy from the CPU oracle's
front-end records and tables, against the frame trace of the same inputs (identities on device values only), for their
layout under every plane mask, across the batch path's launch boundaries, for the results of the same call, and through
the host entry and the CLI.  Needs an MI355X (`-m gpu`).

Inputs: a reference of a tone plus noise, 2048 + 29 x 1024 + 300 samples (frame 24, where the gates of gstpeaq.c:871
open, is passed, and a flush frame exists), and three test signals: the reference plus white noise at 1e-2, at 1.5e-4
and -- 700 samples shorter, a ragged pair -- at 1e-3.  The middle one is that quiet so that the frame's detection
probability lies strictly between 0.01 and 0.99 in most of its frames (asserted on the oracle's trace below): the
identity with p_detect is then not checked at saturation only.

DETECT and STEPS against numpy: e = 10 log10 (exc_ref) - 10 log10 (exc_test) is a difference of two logarithms of 30 ..
80 dB, so the planes are held relative only where |e| >= 0.01 dB and to 1e-12 absolute elsewhere.  The relative bound
DETECT_STEPS_RTOL is, per plane, ten times the largest deviation measured on the first run on an MI355X (DESIGN.md 20
has the figures), below the project's ceiling of 1e-6 for cancellation-limited values."""
import subprocess

import numpy as np
import pytest

import gst_env
import oracle_lib as orc
from fe_stage_cases import planes_from_records       # (the arithmetic: shared with tests/test_gpu_fe_stage_batches.py)
from test_conformance_runner import write_wav
from test_gpu_trajectory import to_device

pytestmark = pytest.mark.gpu

N = 2048 + 29 * 1024 + 300
NAMES = ["nmr", "exc_ref", "exc_test", "detect", "steps"]     # in the order of the bits, which is the order of the slots
BITS = dict(zip(NAMES, (1, 2, 4, 8, 16)))
SENTINEL = -777.25                                   # what the tests put into the row arrays before a run
# measured on the first run on an MI355X, largest relative deviation from the numpy values over the bands with
# |e| >= 0.01 dB, both channel counts, all three pairs: DETECT 3.751e-11 (28 881 values), STEPS 3.609e-14 (19 564
# values that are not exactly 0) -> ten times that, each plane its own
DETECT_STEPS_RTOL = dict(detect=3.8e-10, steps=3.7e-13)
assert max(DETECT_STEPS_RTOL.values()) <= 1e-6       # the ceiling: a larger measured value is a finding, not a tolerance


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback in the product)")
    import gpu_common
    return gpu_common


_PAIRS, _EXPECTED, _RUNS = {}, {}, {}


def pairs_of(channels):
    """[(ref, test)] x 3: noise at 1e-2, at 1.5e-4, and the ragged pair at 1e-3 whose test signal is 700 samples shorter"""
    if channels not in _PAIRS:
        rng = np.random.default_rng(5)
        t = np.arange(N)[:, None] / 48000.
        f = np.array([1000., 3150.])[:channels][None, :]
        ref = (0.05 * np.sin(2 * np.pi * f * t) + 0.00025 * rng.standard_normal((N, channels))).astype(np.float32)
        tests = [(ref + np.float32(s) * rng.standard_normal((N, channels)).astype(np.float32)).astype(np.float32)
                 for s in (1e-2, 1.5e-4, 1e-3)]
        tests[2] = np.ascontiguousarray(tests[2][:N - 700])
        _PAIRS[channels] = [(ref, x) for x in tests]
    return _PAIRS[channels]


def expected(bands, channels, p):
    """the planes of pair p in numpy from the oracle's front-end records (unsmeared excitations at 0 and 112, noise at
    448) and tables: dict name -> [frames, channels, bands], with `noise` and (109 bands) `e_db`; computed once, shared,
    never changed"""
    key = (bands, channels, p)
    if key in _EXPECTED:
        return _EXPECTED[key]
    ref, test = pairs_of(channels)[p]
    nf = orc.count_frames(len(ref), len(test))
    out = planes_from_records(bands, orc.frontend_records(bands, ref, test, nf), orc.tables(bands))
    _EXPECTED[key] = out
    return out


def counts_of(channels):
    return [orc.count_frames(len(r), len(t)) for r, t in pairs_of(channels)]


def filled(n_pairs, stride, channels, n_planes, row):
    """a row array one pair longer than the batch, full of SENTINEL; -> (the whole array, the batch's part)"""
    import torch
    whole = torch.full((n_pairs + 1, stride, channels, n_planes, row), SENTINEL, dtype=torch.float64, device="cuda")
    return whole, whole[:n_pairs]


def run(gpu, advanced, channels, mask, uniform=False):
    """the three pairs (uniform: the two of equal length, without per-pair lengths) as one batch with the planes of
    `mask` -> (batch_bands' dict, the whole row array as numpy [pairs + 1, stride, channels, n_planes, row]); the array
    is one frame longer than the longest pair needs, one pair longer than the batch, and full of SENTINEL first.  One
    run per argument set, shared by the tests"""
    import gstpeaq_amd
    key = (gpu.mode(), advanced, channels, mask, uniform)
    if key not in _RUNS:
        pairs = pairs_of(channels)[:2] if uniform else pairs_of(channels)
        ref, test, n_ref, n_test = to_device(pairs)
        assert ref.shape[1] == N
        whole, part = filled(len(pairs), max(counts_of(channels)) + 1, channels, bin(mask).count("1"), 56 if advanced else 110)
        out = gstpeaq_amd.batch_bands(gpu.ctx(), advanced, ref, test, mask, None if uniform else n_ref,
                                      None if uniform else n_test, d_bands=part)
        _RUNS[key] = (out, whole.cpu().numpy())
    return _RUNS[key]


def names_of(mask):
    return [n for n in NAMES if mask & BITS[n]]


# ---- 1: against the oracle -------------------------------------------------------------------------------------------
def test_the_quiet_pair_s_detection_probability_is_not_saturated():
    """on the oracle's trace: strictly between 0.01 and 0.99 in more than half of the frames, mono and stereo"""
    for channels in (1, 2):
        ref, test = pairs_of(channels)[1]
        nf = orc.count_frames(len(ref), len(test))
        p = orc.mov_trace(ref, test, nf)["p_detect"][:, 0]
        assert nf == 31 and np.count_nonzero((p > 0.01) & (p < 0.99)) > nf // 2, p


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("advanced", [0, 1])
def test_planes_match_numpy_on_the_oracle_s_records(gpu, advanced, channels):
    """every plane the version has, all frames of the three pairs: the excitations at 1e-9 relative (the project's
    tolerance for patterns), NMR at 1e-6 relative and 1e-12 absolute (what tests/test_gpu_trace.py holds nmr_mean and
    nmr_max to), DETECT and STEPS at DETECT_STEPS_RTOL where |e| >= 0.01 dB and 1e-12 absolute elsewhere"""
    bands, mask = (55, 3) if advanced else (109, 31)
    out, _ = run(gpu, advanced, channels, mask)
    assert sorted(k for k in out if k in NAMES) == sorted(names_of(mask))
    assert np.array_equal(out["counts"], counts_of(channels))
    t = orc.tables(bands)
    np.testing.assert_allclose(out["fc"], t["fc"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(out["mask_diff"], t["mask_diff"], rtol=1e-12, atol=0)
    worst = dict(detect=0., steps=0.)
    for p, nf in enumerate(counts_of(channels)):
        exp = expected(bands, channels, p)
        for name in names_of(mask):
            got, want = out[name][p, :nf], exp[name]
            assert got.shape == want.shape == (nf, channels, bands)
            if name in ("exc_ref", "exc_test"):
                np.testing.assert_allclose(got, want, rtol=1e-9, atol=0, err_msg=f"pair {p} {name}")
            elif name == "nmr":
                np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-12, err_msg=f"pair {p} {name}")
            else:
                # (STEPS is exactly 0 while |e| < 1 dB: those bands go with "elsewhere")
                big = (np.abs(exp["e_db"]) >= 0.01) & (want != 0.)
                dev = np.abs(got - want)
                rel = float(np.max(dev[big] / np.abs(want[big])))
                worst[name] = max(worst[name], rel)
                print(f"bands-measure channels={channels} pair={p} {name}: max rel dev {rel:.3e} over {np.count_nonzero(big)} "
                      f"values with |e| >= 0.01 dB, max abs dev elsewhere {float(np.max(dev[~big], initial=0.)):.3e}")
                assert big.any()
                assert (dev[~big] <= 1e-12).all(), (p, name, float(np.max(dev[~big], initial=0.)))
    if not advanced:
        print(f"bands-measure channels={channels} worst: detect {worst['detect']:.3e} steps {worst['steps']:.3e}")
        assert worst["detect"] <= DETECT_STEPS_RTOL["detect"] and worst["steps"] <= DETECT_STEPS_RTOL["steps"], worst


# ---- 2: identities with the frame trace, device values only ---------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("advanced", [0, 1])
def test_identities_with_the_frame_trace(gpu, advanced, channels):
    import gstpeaq_amd
    bands, mask = (55, 3) if advanced else (109, 31)
    out, _ = run(gpu, advanced, channels, mask)
    ref, test, n_ref, n_test = to_device(pairs_of(channels))
    trace = gstpeaq_amd.batch_trace(gpu.ctx(), advanced, ref, test, n_ref, n_test)
    for p, nf in enumerate(counts_of(channels)):
        fr = trace["frames"][p][:nf]
        nmr = out["nmr"][p, :nf]
        mean_k = 1 if advanced else 4
        # the sum has 109 (55) positive terms in another order
        np.testing.assert_allclose(nmr.mean(axis=-1), fr["ch"][:, :channels, mean_k], rtol=1e-12, atol=0, err_msg=f"pair {p}")
        # the noise plane of the oracle's records back from the two device planes
        noise = nmr * out["exc_ref"][p, :nf] / out["mask_diff"]
        np.testing.assert_allclose(noise, expected(bands, channels, p)["noise"], rtol=1e-6, atol=0, err_msg=f"pair {p}")
        if advanced:
            continue
        assert np.array_equal(nmr.max(axis=-1), fr["ch"][:, :channels, 5]), p      # a maximum rounds nothing
        steps = out["steps"][p, :nf].max(axis=1).sum(axis=-1)
        np.testing.assert_allclose(steps, fr["steps"], rtol=1e-12, atol=0, err_msg=f"pair {p}")
        p_detect = 1. - np.exp2(-out["detect"][p, :nf].max(axis=1).sum(axis=-1))
        np.testing.assert_allclose(p_detect, fr["p_detect"], rtol=0, atol=1e-9, err_msg=f"pair {p}")
        if p == 1:                                   # ... and not at saturation only
            assert np.count_nonzero((fr["p_detect"] > 0.01) & (fr["p_detect"] < 0.99)) > nf // 2


# ---- 3: layout ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("advanced", [0, 1])
def test_every_plane_mask_writes_the_same_values_at_its_slot_ranks(gpu, advanced, channels):
    """all 31 masks (advanced: the 3) against the run with every plane: the same bits at the slot that is the rank of
    the plane's bit; the pad entry of every written row is 0; rows past each pair's count and the array behind the
    last pair still hold the sentinel"""
    bands, full = (55, 3) if advanced else (109, 31)
    every, _ = run(gpu, advanced, channels, full)
    cnt = counts_of(channels)
    for mask in range(1, full + 1):
        out, whole = run(gpu, advanced, channels, mask)
        names = names_of(mask)
        assert whole.shape == (4, max(cnt) + 1, channels, len(names), bands + 1)
        assert (whole[3] == SENTINEL).all(), mask
        for p, nf in enumerate(cnt):
            assert (whole[p, nf:] == SENTINEL).all(), (mask, p)
            assert (whole[p, :nf, :, :, bands] == 0.).all(), (mask, p)
            assert not (whole[p, :nf, :, :, :bands] == SENTINEL).any(), (mask, p)
            for k, name in enumerate(names):
                assert whole[p, :nf, :, k, :bands].tobytes() == every[name][p, :nf].tobytes(), (mask, p, name)
                assert np.array_equal(out[name][p, :nf], every[name][p, :nf], equal_nan=True)
        assert out["d_results"].cpu().numpy().tobytes() == every["d_results"].cpu().numpy().tobytes(), mask


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("advanced", [0, 1])
def test_uniform_length_equals_per_pair_lengths(gpu, advanced, channels):
    """the two pairs of equal length without n_ref / n_test (n_uniform) give the rows they give with them"""
    bands, full = (55, 3) if advanced else (109, 31)
    every, _ = run(gpu, advanced, channels, full)
    out, whole = run(gpu, advanced, channels, full, uniform=True)
    assert np.array_equal(out["counts"], [31, 31]) and (whole[2] == SENTINEL).all() and (whole[:2, 31:] == SENTINEL).all()
    for name in names_of(full):
        assert out[name][:, :31].tobytes() == every[name][:2, :31].tobytes(), name
    assert out["d_results"].cpu().numpy().tobytes() == every["d_results"][:2].cpu().numpy().tobytes()


# ---- 4: launch boundaries ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("advanced", [0, 1])
def test_rows_across_launch_boundaries(gpu, advanced):
    """256 stereo pairs of 5 s, as tests/test_gpu_trace.py::test_records_across_launch_boundaries chooses them: 234 frames
    in 4 front-end launches.  No row of the batch keeps the sentinel, the results are peaq_batch_run's bytes, and four
    pairs' rows are bit for bit those of a batch of their own (whose frames are one launch)"""
    import gstpeaq_amd
    import torch
    ctx = gpu.ctx()
    n, pairs = 240000, 256
    mask, names, row = (3, ["nmr", "exc_ref"], 56) if advanced else (1 | 8, ["nmr", "detect"], 110)
    ref, test = gstpeaq_amd.synth_fill(ctx, 700, pairs, 2, n)
    nf = gstpeaq_amd.frame_count(n, n)
    assert nf == 234
    d_bands = torch.full((pairs, nf, 2, 2, row), SENTINEL, dtype=torch.float64, device="cuda")
    out = gstpeaq_amd.batch_bands(ctx, advanced, ref, test, names, sync=False, d_bands=d_bands)
    tm = ctx.last_timing()
    assert tm["frontend_launches"] == 4 and tm["backend_launches"] == 4, tm
    torch.cuda.synchronize()
    assert not bool((d_bands == SENTINEL).any()) and bool((d_bands[..., row - 1] == 0).all())
    whole = gstpeaq_amd.batch_run(ctx, advanced, ref, test, sync=False)
    torch.cuda.synchronize()
    assert whole.cpu().numpy().tobytes() == out["d_results"].cpu().numpy().tobytes()
    own = [0, 37, 64, 127]
    sub = gstpeaq_amd.batch_bands(ctx, advanced, ref[own].contiguous(), test[own].contiguous(), mask, sync=False)
    assert ctx.last_timing()["frontend_launches"] == 1
    torch.cuda.synchronize()
    assert sub["d_bands"].shape == (4, nf, 2, 2, row)
    assert sub["d_bands"].cpu().numpy().tobytes() == d_bands[own].cpu().numpy().tobytes()
    assert sub["d_results"].cpu().numpy().tobytes() == out["d_results"][own].cpu().numpy().tobytes()


# ---- 5: results and leakage ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("advanced", [0, 1])
def test_results_are_batch_run_s_and_nothing_leaks_into_a_later_batch(gpu, advanced):
    """d_results of a band run are peaq_batch_run's bytes; a batch_run after a band run on the same context returns
    the bytes it returns on a fresh context; a band run is bit-identical run to run"""
    import gstpeaq_amd
    import torch
    mask = 3 if advanced else 31
    ref, test, n_ref, n_test = to_device(pairs_of(2))
    ctx = gpu.ctx()
    first = gstpeaq_amd.batch_bands(ctx, advanced, ref, test, mask, n_ref, n_test, sync=False)
    after = gstpeaq_amd.batch_run(ctx, advanced, ref, test, n_ref, n_test, sync=False)
    again = gstpeaq_amd.batch_bands(ctx, advanced, ref, test, mask, n_ref, n_test, sync=False)
    fresh_ctx = gstpeaq_amd.Context(0)
    fresh = gstpeaq_amd.batch_run(fresh_ctx, advanced, ref, test, n_ref, n_test, sync=False)
    torch.cuda.synchronize()
    assert after.cpu().numpy().tobytes() == fresh.cpu().numpy().tobytes()
    assert after.cpu().numpy().tobytes() == first["d_results"].cpu().numpy().tobytes()
    for k in ("d_bands", "d_results"):
        assert first[k].cpu().numpy().tobytes() == again[k].cpu().numpy().tobytes(), k
    fresh_ctx.close()


def test_results_follow_the_fir_mode_in_the_advanced_version(gpu, fir_mode):
    """the FIR mode is irrelevant to the rows (the FFT path does not pass through the filter bank) and still applies to
    d_results: in either mode they are peaq_batch_run's bytes on the same context"""
    import gstpeaq_amd
    import torch
    ref, test, n_ref, n_test = to_device(pairs_of(2))
    out = gstpeaq_amd.batch_bands(gpu.ctx(), 1, ref, test, 3, n_ref, n_test, sync=False)
    plain = gstpeaq_amd.batch_run(gpu.ctx(), 1, ref, test, n_ref, n_test, sync=False)
    torch.cuda.synchronize()
    assert out["d_results"].cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()
    import gpu_common
    default = gstpeaq_amd.batch_bands(gpu_common.ctx("default"), 1, ref, test, 3, n_ref, n_test, sync=False)
    torch.cuda.synchronize()
    assert out["d_bands"].cpu().numpy().tobytes() == default["d_bands"].cpu().numpy().tobytes()


# ---- 6: host entry and CLI -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("advanced", [0, 1])
def test_host_memory_entry_equals_the_batch_entry(gpu, advanced):
    import gstpeaq_amd
    mask = 3 if advanced else 31
    r, t = pairs_of(2)[2]
    host = gstpeaq_amd.run_pair_bands(gpu.ctx(), advanced, r, t, mask)
    every, _ = run(gpu, advanced, 2, mask)
    nf = counts_of(2)[2]
    for name in names_of(mask):
        assert host[name].shape == (nf, 2, 55 if advanced else 109)
        assert host[name].tobytes() == every[name][2, :nf].tobytes(), name
    for key in ("movs", "di", "odg", "totalsnr", "frames", "fb_blocks"):
        np.testing.assert_array_equal(host["result"][key], every["results"][2][key])
    whole = gstpeaq_amd.run_pair(gpu.ctx(), advanced, r, t)
    np.testing.assert_array_equal(host["result"]["movs"], whole["movs"])


@pytest.mark.parametrize("advanced,planes", [(0, None), (0, "steps,nmr,exc_test"), (1, "exc_ref,nmr")])
def test_cli_bands(gpu, advanced, planes, tmp_path):
    """`peaq --bands=FILE[:PLANES]`: the CSV rows parse back to the doubles of run_pair_bands (%.17g), one line per
    (frame, channel, plane) in the order of the slots, the header carries the centre frequencies, the printed lines are
    those printed without --bands; the default plane is nmr"""
    import gstpeaq_amd
    r, t = pairs_of(2)[2]
    write_wav(tmp_path / "ref.wav", r, bits=32, fmt_float=True)
    write_wav(tmp_path / "test.wav", t, bits=32, fmt_float=True)
    flags = ["--advanced"] if advanced else []
    csv = tmp_path / "bands.csv"
    plain = subprocess.run([str(gst_env.CLI), *flags, tmp_path / "ref.wav", tmp_path / "test.wav"],
                           capture_output=True, text=True, timeout=300)
    out = subprocess.run([str(gst_env.CLI), *flags, f"--bands={csv}" + (f":{planes}" if planes else ""),
                          tmp_path / "ref.wav", tmp_path / "test.wav"], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and out.returncode == 0, (plain.stderr, out.stderr, out.stdout)
    assert out.stdout == plain.stdout and "Objective Difference Grade" in out.stdout
    names = [n for n in NAMES if n in (planes.split(",") if planes else ["nmr"])]
    exp = gstpeaq_amd.run_pair_bands(gpu.ctx(), advanced, r, t, names)
    bands, nf = (55 if advanced else 109), counts_of(2)[2]
    lines = csv.read_text().strip().splitlines()
    header = lines[0].split(",")
    assert header[:3] == ["frame", "channel", "plane"] and len(header) == 3 + bands
    assert np.array([float(v) for v in header[3:]]).tobytes() == exp["fc"].tobytes()
    rows = [ln.split(",") for ln in lines[1:]]
    assert len(rows) == nf * 2 * len(names) and all(len(row) == 3 + bands for row in rows)
    it = iter(rows)
    for f in range(nf):
        for c in range(2):
            for name in names:
                row = next(it)
                assert (int(row[0]), int(row[1]), row[2]) == (f, c, name)
                assert np.array([float(v) for v in row[3:]]).tobytes() == exp[name][f, c].tobytes(), row[:3]

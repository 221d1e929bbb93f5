"""Delay estimation and cutting on the device (peaq_batch_estimate_delay, peaq_batch_cut, peaq_run_pair_aligned;
Python estimate_delay / cut / align / align=; the CLI's --align) on the MI355X.

Yardstick for the correlation: numpy in FP64 -- np.fft over the zero-padded whole signals (np.correlate for the short
hand-made cases) --, an independent method.  The header's bound on c[d] is 1e-9 norm; the yardstick's own error is
some 1e-15 norm.  Before a lag is compared the case's margin (|c[lag]| - runner_up) / norm is required to be at least
1e-3 in the yardstick, six orders above the bound, so the arg-max cannot hang on rounding; no case may miss it.
Everything after the estimate -- cut, and the engine behind it -- is compared bit for bit."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import gpu_common
import gst_env
import synth_np

pytestmark = pytest.mark.gpu

N = 96000
DELAYS = (0, 1, 511, 512, 513, 1105, 2048, 4095, 4096)
BOUND = 1e-9
MARGIN = 1e-3


def ctx():
    return gpu_common.ctx("default")


def write_wav(path, x, rate=48000):
    """x [n, channels] as a 32-bit float RIFF/WAVE file (a copy of its own: no other test file is needed)"""
    x = np.asarray(x)
    ch = x.shape[1]
    body = x.astype("<f4").tobytes()
    fmt = struct.pack("<HHIIHH", 3, ch, rate, rate * ch * 4, ch * 4, 32)
    chunks = b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(body)) + body
    Path(path).write_bytes(b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks)


def run_cli(*args):
    return subprocess.run([str(gst_env.CLI), *map(str, args)], capture_output=True, text=True, timeout=300)


def printed(out):
    lines = out.stdout.strip().splitlines()
    assert lines[-2].startswith("Objective Difference Grade: ") and lines[-1].startswith("Distortion Index: "), out.stdout
    return lines[-2].split()[-1], lines[-1].split()[-1]


def mono(x):
    return x.astype(np.float64).sum(axis=1)


def correlation(ref, test, max_lag):
    """c[d], d = -max_lag .. max_lag, of the mono sums (FP64, FFT over the zero-padded whole signals), and norm"""
    r, t = mono(ref), mono(test)
    norm = float(np.sqrt(np.dot(r, r) * np.dot(t, t)))
    if len(r) == 0 or len(t) == 0:
        return np.zeros(2 * max_lag + 1), norm
    size = 1 << int(np.ceil(np.log2(len(r) + len(t) + 2 * max_lag + 2)))
    c = np.fft.irfft(np.conj(np.fft.rfft(r, size)) * np.fft.rfft(t, size), size)
    return np.concatenate([c[size - max_lag:], c[:max_lag + 1]]), norm


def pick(c, max_lag):
    """(lag, peak, runner_up) by the header's rule: largest |c|, ties to the smaller |d|, then to the positive one"""
    d = np.arange(-max_lag, max_lag + 1)
    order = np.lexsort((d < 0, np.abs(d), -np.abs(c)))
    lag = int(d[order[0]])
    return lag, float(c[order[0]]), float(np.abs(c[order[1]]))


def expected(ref, test, max_lag):
    c, norm = correlation(ref, test, max_lag)
    if norm == 0.:
        return dict(lag=0, peak=0., runner_up=0., norm=0., margin=None)
    lag, peak, second = pick(c, max_lag)
    return dict(lag=lag, peak=peak, runner_up=second, norm=norm, margin=(abs(peak) - second) / norm)


def shifted(test, d):
    """the test signal late by d samples (zeros in front) or, d < 0, early by -d (its first samples dropped)"""
    if d >= 0:
        return np.concatenate([np.zeros((d, test.shape[1]), np.float32), test])
    return test[-d:]


def batch(pairs):
    """[(ref, test)] of any lengths -> (ref tensor, test tensor, n_ref, n_test) with one stride"""
    import torch
    ch = pairs[0][0].shape[1]
    stride = max(max(len(r), len(t)) for r, t in pairs)
    stride = max(stride + (stride & 1), 2)
    a = np.zeros((2, len(pairs), stride, ch), np.float32)
    for p, (r, t) in enumerate(pairs):
        a[0, p, :len(r)], a[1, p, :len(t)] = r, t
    d = torch.from_numpy(a).cuda()
    return d[0], d[1], np.array([len(r) for r, _ in pairs], np.uint32), np.array([len(t) for _, t in pairs], np.uint32)


def estimate(pairs, max_lag):
    import gstpeaq_amd
    ref, test, n_ref, n_test = batch(pairs)
    return gstpeaq_amd.estimate_delay(ctx(), ref, test, max_lag, n_ref, n_test)


def check(pairs, max_lag, got, what):
    worst = 0.
    for p, (r, t) in enumerate(pairs):
        exp = expected(r, t, max_lag)
        assert exp["margin"] is not None and exp["margin"] >= MARGIN, (what, p, exp)     # no case may be dropped
        assert int(got["lag"][p]) == exp["lag"], (what, p, int(got["lag"][p]), exp)
        for k in ("peak", "runner_up", "norm"):
            err = abs(float(got[k][p]) - exp[k]) / exp["norm"]
            worst = max(worst, err)
            assert err <= BOUND, (what, p, k, float(got[k][p]), exp)
    return worst


# ---- 1. the lag is exact -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("sign", [1, -1], ids=["late", "early"])
def test_lag_of_delayed_and_advanced_pairs_is_exact(channels, sign):
    src = [synth_np.pair(seed, channels, N) for seed in range(1, 25)]
    worst = 0.
    for d in DELAYS:
        pairs = [(r, shifted(t, sign * d)) for r, t in src]
        got = estimate(pairs, 4096)
        worst = max(worst, check(pairs, 4096, got, (channels, sign * d)))
    print(f"channels {channels} sign {sign}: largest error of peak / runner_up / norm {worst:.3e} norm (bound {BOUND:g})")


def test_lag_beyond_4096_with_the_widest_range():
    pairs = [(r, shifted(t, d)) for (r, t), d in zip([synth_np.pair(s, 2, N) for s in (3, 4)], (9000, -9000))]
    r, t = synth_np.pair(5, 1, N)
    got = estimate(pairs, 16384)
    check(pairs, 16384, got, "stereo 9000")
    assert [int(v) for v in got["lag"]] == [9000, -9000]
    got = estimate([(r, shifted(t, 9000))], 16384)
    check([(r, shifted(t, 9000))], 16384, got, "mono 9000")
    assert int(got["lag"][0]) == 9000


def test_polarity_inverted_test_signal_aligns_with_a_negative_peak():
    r, t = synth_np.pair(6, 2, N)
    pairs = [(r, shifted(-t, 777))]
    got = estimate(pairs, 4096)
    check(pairs, 4096, got, "inverted")
    assert int(got["lag"][0]) == 777 and float(got["peak"][0]) < 0.


def test_ragged_lengths_through_the_length_arrays():
    src = [synth_np.pair(seed, 2, N) for seed in (7, 8, 9, 10)]
    pairs = [(src[0][0][:70000], shifted(src[0][1], 300)),           # n_ref < n_test
             (src[1][0], shifted(src[1][1], 2000)[:50001]),          # n_ref > n_test
             (src[2][0][:4097], shifted(src[2][1], -100)[:5000]),    # short
             (src[3][0], shifted(src[3][1], -4000))]
    got = estimate(pairs, 4096)
    check(pairs, 4096, got, "ragged")
    assert [int(v) for v in got["lag"]] == [300, 2000, -100, -4000]


def test_record_of_a_pair_does_not_depend_on_its_batch():
    src = [synth_np.pair(seed, 2, N) for seed in (11, 12, 13)]
    pairs = [(r, shifted(t, 100 * (i + 1))) for i, (r, t) in enumerate(src)]
    together = estimate(pairs, 4096)
    alone = estimate(pairs[1:2], 4096)
    for k in together:
        assert together[k][1:2].tobytes() == alone[k].tobytes(), k


# ---- 2. cases that must come out as defined ----------------------------------------------------------------------
def test_tie_goes_to_the_smaller_then_the_positive_lag():
    n, k = 6000, 700
    ref = np.zeros((n, 1), np.float32)
    ref[3000] = 1.
    test = np.zeros((n, 1), np.float32)
    test[3000 - k] = test[3000 + k] = 1.                   # c[+k] = c[-k] = 1
    c = np.correlate(mono(test), mono(ref), "full")[n - 1 - 4096: n + 4096]
    assert c[4096 + k] == 1. and c[4096 - k] == 1. and pick(c, 4096)[0] == k
    test2 = test.copy()
    test2[3000 + 300] = test2[3000 - 300] = -1.            # |c| ties at four lags: the smaller |d|, positive
    got = estimate([(ref, test), (ref, test2)], 4096)
    assert [int(v) for v in got["lag"]] == [k, 300]
    assert abs(got["peak"][0] - 1.) <= BOUND * got["norm"][0] and abs(got["runner_up"][0] - 1.) <= BOUND * got["norm"][0]
    assert abs(got["peak"][1] + 1.) <= BOUND * got["norm"][1]


def test_zero_and_empty_signals_give_lag_zero():
    r, t = synth_np.pair(14, 2, 20000)
    z = np.zeros_like(r)
    e = np.zeros((0, 2), np.float32)
    got = estimate([(r, z), (z, t), (z, z), (r, e), (e, t), (r, t)], 4096)
    for p in range(5):
        assert int(got["lag"][p]) == 0 and got["peak"][p] == 0. and got["runner_up"][p] == 0., (p, got)
    assert int(got["lag"][5]) == expected(r, t, 4096)["lag"]
    import gstpeaq_amd
    import torch
    empty = torch.zeros((1, 2, 2), dtype=torch.float32, device="cuda")
    got = gstpeaq_amd.estimate_delay(ctx(), empty, empty, 4096, [0], [0])
    assert int(got["lag"][0]) == 0 and got["peak"][0] == 0.


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan], ids=["inf", "-inf", "nan"])
def test_non_finite_samples_give_the_defined_record(bad):
    """a float file can carry an Inf or a NaN: no estimate, lag 0, peak 0, norm NaN -- for that pair only"""
    r, t = synth_np.pair(15, 2, 20000)
    late = shifted(t, 250)
    r_bad, t_bad, t_bad2 = r.copy(), late.copy(), late.copy()
    r_bad[7000, 1] = bad
    t_bad[0, 0] = bad                                       # in the zeros in front
    t_bad2[len(late) - 1, 1] = bad
    pairs = [(r_bad, late), (r, t_bad), (r, t_bad2), (r_bad, t_bad), (r, late)]
    for max_lag in (4096, 16384):
        got = estimate(pairs, max_lag)
        for p in range(4):
            assert int(got["lag"][p]) == 0 and got["peak"][p] == 0. and got["runner_up"][p] == 0., (p, got)
            assert np.isnan(got["norm"][p]), (p, got)
        check(pairs[4:], max_lag, {k: v[4:] for k, v in got.items()}, "the finite pair beside them")
        assert int(got["lag"][4]) == 250


def test_batch_larger_than_one_scratch_group():
    """80 ragged ten-second pairs at max_lag 4096 need 1.33 GB of scratch: the estimator takes them in two groups
    (64 + 16).  Every lag is checked, the second group's records and some of the first against the yardstick."""
    import gstpeaq_amd
    n_pairs, n = 80, 480000
    assert gstpeaq_amd.align_workspace_bytes(1, n_pairs, n, 4096) == 1 << 30
    assert gstpeaq_amd.align_workspace_bytes(1, 1, n, 4096) * n_pairs > 1 << 30
    assert (1 << 30) // gstpeaq_amd.align_workspace_bytes(1, 1, n, 4096) == 64
    ref, test = gstpeaq_amd.synth_fill(ctx(), 200, n_pairs, 1, n)
    import torch
    torch.cuda.synchronize()
    ref, test = ref.cpu().numpy(), test.cpu().numpy()
    delays = [((37 * p) % 4001) * (1 if p % 3 else -1) for p in range(n_pairs)]
    pairs = []
    for p in range(n_pairs):
        r = ref[p][:n - 1000 * (p % 7)]                       # ragged on both sides
        t = shifted(test[p], delays[p])[:n - 777 * (p % 5)]
        pairs.append((r, t))
    got = estimate(pairs, 4096)
    assert [int(v) for v in got["lag"]] == delays
    picked = [0, 1, 63] + list(range(64, 80))
    check([pairs[p] for p in picked], 4096, {k: v[picked] for k, v in got.items()}, "two groups")
    again = estimate(pairs[64:], 4096)                        # the second group's pairs as a batch of their own
    for k in got:
        assert got[k][64:].tobytes() == again[k].tobytes(), k


# ---- 3. cut is exact ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
def test_cut_against_numpy_slicing_bit_for_bit(channels):
    import gstpeaq_amd
    import torch
    rng = np.random.default_rng(5)
    n_pairs, stride = 7, 5003
    x = rng.standard_normal((n_pairs, stride, channels)).astype(np.float32)
    skip = np.array([0, 1, 2, 3, 1000, 4999, 17], np.uint32)
    keep = np.array([5003, 5002, 0, 1, 4003, 4, 1234], np.uint32)
    d = torch.from_numpy(x).cuda()
    y = gstpeaq_amd.cut(ctx(), d, skip, keep)
    torch.cuda.synchronize()
    y = y.cpu().numpy()
    assert y.shape == (n_pairs, 5004, channels)
    for p in range(n_pairs):
        assert y[p, :keep[p]].tobytes() == x[p, skip[p]:skip[p] + keep[p]].tobytes(), p
        assert not y[p, keep[p]:].any(), p
    # a wider destination with an odd stride: the tail past n_keep keeps its sentinel
    out = torch.full((n_pairs, 6001, channels), -7.5, dtype=torch.float32, device="cuda")
    gstpeaq_amd.cut(ctx(), d, skip, keep, out=out)
    torch.cuda.synchronize()
    y = out.cpu().numpy()
    for p in range(n_pairs):
        assert y[p, :keep[p]].tobytes() == x[p, skip[p]:skip[p] + keep[p]].tobytes(), p
        assert (y[p, keep[p]:] == -7.5).all(), p
    with pytest.raises(gstpeaq_amd.PeaqError):
        gstpeaq_amd.cut(ctx(), d, [0] * 6 + [4000], [0] * 6 + [1004])          # passes the stride
    with pytest.raises(gstpeaq_amd.PeaqError):
        gstpeaq_amd.cut(ctx(), d, skip, keep, out=torch.zeros((n_pairs, 5002, channels), device="cuda"))
    # d_out must not overlap d_in: the buffer itself, and a buffer that starts inside it
    with pytest.raises(gstpeaq_amd.PeaqError, match="overlaps"):
        gstpeaq_amd.cut(ctx(), d, skip, np.minimum(keep, 3), out=d)
    big = torch.zeros((2 * n_pairs, stride, channels), dtype=torch.float32, device="cuda")
    with pytest.raises(gstpeaq_amd.PeaqError, match="overlaps"):
        gstpeaq_amd.cut(ctx(), big[:n_pairs], skip, keep, out=big[n_pairs - 1:2 * n_pairs - 1])
    gstpeaq_amd.cut(ctx(), big[:n_pairs], skip, keep, out=big[n_pairs:])          # side by side is fine
    torch.cuda.synchronize()


# ---- 4. end to end, bit for bit ----------------------------------------------------------------------------------
def same_result(a, b):
    return all(np.array([a[k]]).tobytes() == np.array([b[k]]).tobytes() for k in ("di", "odg", "totalsnr")) and \
        a["frames"] == b["frames"] and a["fb_blocks"] == b["fb_blocks"] and a["movs"].tobytes() == b["movs"].tobytes()


E2E_N = 48000
E2E_DELAYS = (1105, -640, 4096, 1)


def e2e_pairs(channels):
    return [(r, shifted(t, d)) for (r, t), d in zip([synth_np.pair(s, channels, E2E_N) for s in (21, 22, 23, 24)], E2E_DELAYS)]


def host_sliced(pairs, lags):
    import gstpeaq_amd
    out = []
    for (r, t), lag in zip(pairs, lags):
        sr, st, n = gstpeaq_amd.aligned_lengths(lag, len(r), len(t))
        assert (sr, st, n) == (max(-lag, 0), max(lag, 0), min(len(r) - max(-lag, 0), len(t) - max(lag, 0)))
        out.append((r[sr:sr + n], t[st:st + n]))
    return out


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("advanced", [0, 1], ids=["basic", "advanced"])
def test_align_keyword_equals_the_host_sliced_run(advanced, channels):
    import gstpeaq_amd
    pairs = e2e_pairs(channels)
    ref, test, n_ref, n_test = batch(pairs)
    got = gstpeaq_amd.batch_run(ctx(), advanced, ref, test, n_ref, n_test, align=4096)
    sliced = host_sliced(pairs, E2E_DELAYS)
    exp = gstpeaq_amd.batch_run(ctx(), advanced, *batch(sliced))
    plain = gstpeaq_amd.batch_run(ctx(), advanced, ref, test, n_ref, n_test)
    for p in range(len(pairs)):
        assert same_result(got[p], exp[p]), (p, got[p], exp[p])
    # the delay matters: as they are the pairs read far worse
    gaps = [abs(plain[p]["odg"] - got[p]["odg"]) for p in range(len(pairs))]
    print("ODG aligned", [g["odg"] for g in got], "as they are", [g["odg"] for g in plain])
    assert max(gaps) > 0.5, gaps
    # a zero-prepended pair reads what the original pair cut to the common length reads
    r, t = synth_np.pair(21, channels, E2E_N)
    orig = gstpeaq_amd.batch_run(ctx(), advanced, *batch([(r[:len(sliced[0][0])], t[:len(sliced[0][0])])]))
    assert same_result(got[0], orig[0]), (got[0], orig[0])
    # trajectories and the one-pair path
    pts, res = gstpeaq_amd.batch_trajectory(ctx(), advanced, ref, test, 9600, 5, n_ref, n_test, align=4096)
    epts, eres = gstpeaq_amd.batch_trajectory(ctx(), advanced, *batch(sliced)[:2], 9600, 5, *batch(sliced)[2:])
    for p in range(len(pairs)):
        assert same_result(res[p], eres[p]) and same_result(res[p], exp[p]), p
        for k in range(5):
            assert same_result(pts[p][k], epts[p][k]), (p, k, pts[p][k], epts[p][k])   # (bytes: NaN readings too)
    for p in range(len(pairs)):
        one = gstpeaq_amd.run_pair(ctx(), advanced, pairs[p][0], pairs[p][1], align=4096)
        assert one["delay"]["lag"] == E2E_DELAYS[p]
        assert same_result(one, exp[p]), (p, one, exp[p])


def test_align_after_rate_conversion_equals_resample_then_align():
    import gstpeaq_amd
    import torch
    pairs = [(r, shifted(t, d)) for (r, t), d in zip([synth_np.pair(s, 2, 44100) for s in (25, 26)], (900, -333))]
    ref, test, n_ref, n_test = batch(pairs)
    got = gstpeaq_amd.batch_run(ctx(), 0, ref, test, n_ref, n_test, rate=44100, align=4096)
    longest = max(gstpeaq_amd.resampled_length(int(v), 44100) for v in list(n_ref) + list(n_test))
    r48, t48 = (torch.zeros((2, longest + (longest & 1), 2), dtype=torch.float32, device="cuda") for _ in (0, 1))
    _, o_ref = gstpeaq_amd.resample(ctx(), ref, 44100, n_ref, out=r48)
    _, o_test = gstpeaq_amd.resample(ctx(), test, 44100, n_test, out=t48)
    torch.cuda.synchronize()
    exp = gstpeaq_amd.batch_run(ctx(), 0, r48, t48, o_ref, o_test, align=4096)
    for p in range(2):
        assert same_result(got[p], exp[p]), (p, got[p], exp[p])
    one = gstpeaq_amd.run_pair(ctx(), 0, pairs[0][0], pairs[0][1], rate=44100, align=4096)
    assert same_result(one, exp[0]), (one, exp[0])
    assert abs(one["delay"]["lag"] - 900 * 48000 / 44100) <= 1.5


# ---- 5. determinism -----------------------------------------------------------------------------------------------
def test_two_runs_over_a_64_pair_batch_give_identical_records():
    import gstpeaq_amd
    ref, test = gstpeaq_amd.synth_fill(ctx(), 100, 64, 2, 48000)
    test = torch_roll(test, 321)
    a = gstpeaq_amd.estimate_delay(ctx(), ref, test, 4096)
    b = gstpeaq_amd.estimate_delay(ctx(), ref, test, 4096)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (a["lag"] == 321).all(), a["lag"]


def torch_roll(x, d):
    import torch
    y = torch.zeros_like(x)
    y[:, d:] = x[:, :x.shape[1] - d]
    return y.contiguous()


# ---- 6. the CLI ---------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not gst_env.CLI.exists(), reason="gstpeaq_amd/cli/peaq not built")
def test_cli_align_prints_the_delay_and_the_aligned_grade(tmp_path):
    import gstpeaq_amd
    r, t = synth_np.pair(31, 2, 60000)
    late = shifted(t, 1105)
    write_wav(tmp_path / "ref.wav", r)
    write_wav(tmp_path / "test.wav", t)
    write_wav(tmp_path / "late.wav", late)
    exp = gstpeaq_amd.batch_run(ctx(), 0, *batch(host_sliced([(r, late)], [1105])))[0]
    rec = expected(r, late, 4096)
    out = run_cli("--align", tmp_path / "ref.wav", tmp_path / "late.wav")
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 3 and lines[0] == "Delay: 1105 samples (correlation %.3f)" % (rec["peak"] / rec["norm"]), out.stdout
    assert printed(out) == ("%.3f" % exp["odg"], "%.3f" % exp["di"])
    out = run_cli("--align=2000", "--advanced", tmp_path / "ref.wav", tmp_path / "late.wav")
    assert out.returncode == 0 and out.stdout.startswith("Delay: 1105 samples"), out.stdout + out.stderr
    # without the option nothing changes: the two usual lines, for the pair as it is
    plain = gstpeaq_amd.run_pair(ctx(), 0, r, t)
    out = run_cli(tmp_path / "ref.wav", tmp_path / "test.wav")
    assert out.stdout == "Objective Difference Grade: %.3f\nDistortion Index: %.3f\n" % (plain["odg"], plain["di"])
    assert run_cli("--align=0", tmp_path / "ref.wav", tmp_path / "late.wav").returncode == 1
    assert run_cli("--align=16385", tmp_path / "ref.wav", tmp_path / "late.wav").returncode == 1

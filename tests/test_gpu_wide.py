"""The wide delay search on the MI355X (peaq_batch_decimate, peaq_batch_estimate_delay_wide, peaq_run_pair_wide; Python
decimate / estimate_delay_wide / wide=; the CLI's --align-wide).

Yardstick for the decimator: the header's definition restated with numpy in FP64 on the library's own taps.  Tolerance
per output v: 2^-23 |v| + 1e-12 A, A = sum |h| max |u|: one FP32 rounding, and at most 1025 + 4096 FP64 roundings of
1.1e-16 relative to A (the filter's chain and the mean's sum, whose order the definition leaves open).
The wide estimate is DEFINED as a composition of public stages and is held to it bit for bit; that it finds real
offsets is shown on seeded signals after a numpy model of the coarse stage has shown that the inputs allow it."""
import ctypes as C
import functools
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import gpu_common
import gst_env

pytestmark = pytest.mark.gpu

NONE, RANGE, EDGE = 1, 2, 4


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


def bits(a):
    """an array's bits, so that NaNs compare"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same_record(got, want):
    for k in ("lag", "coarse_lag", "factor", "flags"):
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    for stage in ("fine", "coarse"):
        for k in ("lag", "peak", "runner_up", "norm"):
            assert np.array_equal(bits(got[stage][k]), bits(want[stage][k])), (stage, k, got[stage][k], want[stage][k])


def batch(signals, extra=0, fill=0.):
    """[n_i, channels] arrays -> (CUDA tensor [n_pairs, stride, channels], lengths); samples past a length hold `fill`"""
    import torch
    n = np.array([len(s) for s in signals], dtype=np.uint32)
    stride = max(int(n.max()) + extra, 2)
    stride += 0 if extra else stride & 1
    x = np.full((len(signals), stride, signals[0].shape[1]), fill, dtype=np.float32)
    for p, s in enumerate(signals):
        x[p, :len(s)] = s
    return torch.from_numpy(x).cuda(), n


# ---- the definition, restated -----------------------------------------------------------------------------------------
def decimate_np(x, M, mode, h):
    """y (FP64, before the rounding to FP32) and A of one signal x [n, channels]"""
    s = x[:, 0].astype(np.float64)
    if x.shape[1] == 2:
        s = s + x[:, 1].astype(np.float64)
    u = np.abs(s) if mode == "envelope" else s
    n_dec = -(-len(u) // M)
    padded = np.zeros(n_dec * M + 16 * M + 1)
    padded[8 * M:8 * M + len(u)] = u
    y = np.lib.stride_tricks.sliding_window_view(padded, 16 * M + 1)[::M][:n_dec] @ h
    if mode == "envelope":
        y = y - y.mean()
    return y, np.abs(h).sum() * (np.abs(u).max() if len(u) else 0.)


def coarse_model(ref, test, M, mode, h, reach):
    """(lag in decimated samples, peak / norm) of the coarse stage, restated: numpy decimation, FP64 correlation by FFT"""
    r = decimate_np(ref, M, mode, h)[0].astype(np.float32).astype(np.float64)
    t = decimate_np(test, M, mode, h)[0].astype(np.float32).astype(np.float64)
    size = 1 << int(np.ceil(np.log2(len(r) + len(t))))
    c = np.fft.irfft(np.conj(np.fft.rfft(r, size)) * np.fft.rfft(t, size), size)
    c = np.concatenate([c[size - reach:], c[:reach + 1]])          # d = -reach .. reach
    norm = np.sqrt(np.dot(r, r) * np.dot(t, t))
    d = int(np.argmax(np.abs(c)))
    return d - reach, (c[d] / norm if norm > 0 else 0.), norm


LENGTHS = lambda M, CH: (1, M - 1, M, M + 1, 8 * M, 16 * M + 1, (CH - 1) * M, CH * M - (M - 1), CH * M + 1,   # noqa: E731
                         2 * CH * M + 1, 1000 * M + 5, 4096 * M - 3)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("mode", ["waveform", "envelope"])
@pytest.mark.parametrize("M", [2, 16, 64])
def test_decimator_against_the_numpy_restatement(M, mode, channels):
    import torch
    import gstpeaq_amd
    CH = gstpeaq_amd.WIDE_CHUNK
    h = gstpeaq_amd.wide_taps(M)
    rng = np.random.default_rng(1000 * M + 10 * channels + (mode == "envelope"))
    signals = [rng.standard_normal((n, channels)).astype(np.float32) for n in LENGTHS(M, CH)]
    # an odd in_stride longer than every pair (rows on and off 16 bytes); NaNs behind every pair's end: reading them shows
    x, n = batch(signals, extra=38, fill=np.nan)
    assert x.shape[1] % 2 == 1 and x.shape[1] > n.max()
    n_dec_max = -(-int(n.max()) // M)
    assert n_dec_max <= 4096
    out = torch.full((len(signals), n_dec_max + 5), 7.5, dtype=torch.float32, device="cuda")
    y, n_dec = gstpeaq_amd.decimate(ctx(), x, M, mode, n=n, out=out)
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    assert sorted({CH - 1, CH, CH + 1, 2 * CH + 1} - set(n_dec.tolist())) == []
    for p, s in enumerate(signals):
        want, A = decimate_np(s, M, mode, h)
        assert n_dec[p] == len(want) == -(-len(s) // M)
        v = got[p, :n_dec[p]].astype(np.float64)
        assert np.isfinite(v).all(), (p, len(s))
        err = np.abs(v - want)
        bound = 2. ** -23 * np.abs(want) + 1e-12 * A
        worst = int(np.argmax(err - bound))
        print("M %d %s ch %d n %d: max err %.3e (bound there %.3e)" % (M, mode, channels, len(s), err[worst], bound[worst]))
        assert (err <= bound).all(), (p, len(s), worst, v[worst], want[worst], bound[worst])
        assert (got[p, n_dec[p]:] == 7.5).all(), (p, len(s))            # entries past n_dec are left as they were


def test_decimator_uniform_length_and_default_output():
    import torch
    import gstpeaq_amd
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3, 5000, 2)).astype(np.float32)
    h = gstpeaq_amd.wide_taps(8)
    y, n_dec = gstpeaq_amd.decimate(ctx(), torch.from_numpy(x).cuda(), 8, "envelope")
    torch.cuda.synchronize()
    assert y.shape == (3, 626) and n_dec.tolist() == [625] * 3
    for p in range(3):
        want, A = decimate_np(x[p], 8, "envelope", h)
        assert (np.abs(y[p, :625].cpu().numpy() - want) <= 2. ** -23 * np.abs(want) + 1e-12 * A).all()
        assert y[p, 625] == 0


# ---- the estimate is the composition ----------------------------------------------------------------------------------
def offset_pair(base, D, d, n_ref, n_test):
    """test[n + d] = ref[n]: both are stretches of base, which reaches D samples before ref's start"""
    return base[D:D + n_ref].copy(), base[D - d:D - d + n_test].copy()


@functools.lru_cache(maxsize=None)
def composition_inputs():
    rng = np.random.default_rng(77)
    offsets = (5000, -5000, 20000, -20000, 40000, -33000, 16384, 0)
    pairs = []
    for p, d in enumerate(offsets):
        base = rng.standard_normal((144000 + 2 * 40000, 2)).astype(np.float32)
        pairs.append(offset_pair(base, 40000, d, 144000 - 1000 * p, 144000 - 777 * (7 - p)))
    ref, n_ref = batch([r for r, _ in pairs])
    test, n_test = batch([t for _, t in pairs])
    if ref.shape[1] < test.shape[1]:
        ref, _ = batch([r for r, _ in pairs], extra=test.shape[1] - int(n_ref.max()))
    elif test.shape[1] < ref.shape[1]:
        test, _ = batch([t for _, t in pairs], extra=ref.shape[1] - int(n_test.max()))
    return ref, test, n_ref, n_test, offsets


def composed(ref, test, n_ref, n_test, max_offset, mode, max_lag):
    """the header's six steps through the Python stages"""
    import torch
    import gstpeaq_amd as g
    c = ctx()
    M = g.wide_factor(max_offset)
    reach = -(-max_offset // M)
    stride = max(-(-int(max(n_ref.max(), n_test.max())) // M), 2)
    dec = [torch.zeros((len(n_ref), stride + (stride & 1)), dtype=torch.float32, device="cuda") for _ in (0, 1)]
    _, nd_ref = g.decimate(c, ref, M, mode, n=n_ref, out=dec[0])
    _, nd_test = g.decimate(c, test, M, mode, n=n_test, out=dec[1])
    coarse = g.estimate_delay(c, dec[0].unsqueeze(-1), dec[1].unsqueeze(-1), reach, nd_ref, nd_test)
    none = ~(coarse["norm"] > 0)
    coarse_lag = np.where(none, 0, coarse["lag"] * M).astype(np.int32)
    cuts = np.array([g.aligned_lengths(int(coarse_lag[p]), int(n_ref[p]), int(n_test[p])) for p in range(len(n_ref))],
                    dtype=np.uint32).reshape(len(n_ref), 3)
    common = np.ascontiguousarray(cuts[:, 2])
    fine = g.estimate_delay(c, g.cut(c, ref, cuts[:, 0], common), g.cut(c, test, cuts[:, 1], common), max_lag, common, common)
    flags = np.where(none, NONE, np.where(np.abs(coarse["lag"]) == reach, RANGE, 0)) | np.where(np.abs(fine["lag"]) == max_lag, EDGE, 0)
    return dict(lag=(coarse_lag + fine["lag"]).astype(np.int32), coarse_lag=coarse_lag,
                factor=np.full(len(n_ref), M, dtype=np.uint32), flags=flags.astype(np.uint32), fine=fine, coarse=coarse)


@pytest.mark.parametrize("mode", ["waveform", "envelope"])
def test_the_wide_estimate_is_the_composition(mode):
    import gstpeaq_amd
    ref, test, n_ref, n_test, offsets = composition_inputs()
    got = gstpeaq_amd.estimate_delay_wide(ctx(), ref, test, 50000, mode, 4096, n_ref, n_test)
    want = composed(ref, test, n_ref, n_test, 50000, mode, 4096)
    assert (got["factor"] == 4).all()
    same_record(got, want)
    if mode == "waveform":                              # white noise: the waveform search finds every offset
        assert got["lag"].tolist() == list(offsets) and (got["flags"] == 0).all(), (got["lag"], got["flags"])


def test_a_record_depends_neither_on_its_batch_nor_on_the_run():
    import gstpeaq_amd
    ref, test, n_ref, n_test, _ = composition_inputs()
    whole = gstpeaq_amd.estimate_delay_wide(ctx(), ref, test, 50000, "envelope", 4096, n_ref, n_test)
    again = gstpeaq_amd.estimate_delay_wide(ctx(), ref, test, 50000, "envelope", 4096, n_ref, n_test)
    same_record(again, whole)
    for p in (3, 7):
        alone = gstpeaq_amd.estimate_delay_wide(ctx(), ref[p:p + 1].contiguous(), test[p:p + 1].contiguous(), 50000, "envelope",
                                                4096, n_ref[p:p + 1], n_test[p:p + 1])
        one = {k: (v[p:p + 1] if not isinstance(v, dict) else {kk: vv[p:p + 1] for kk, vv in v.items()}) for k, v in whole.items()}
        same_record(alone, one)


# ---- it finds what the plain search cannot ----------------------------------------------------------------------------
N10 = 480000
REACH = 300037
FOUND_OFFSETS = (20000, -20000, 157323, -157323, 300037, -300037, 157323)   # the last one: high-passed at 2 kHz


def modulated(rng, n, highpass=None):
    """stereo noise up to 15 kHz (full-band noise has no bandwidth for the model to measure: its bandwidth MOVs are NaN)
    under one slow random envelope (a value every 10 ms, interpolated): nothing periodic"""
    m = -(-n // 32768) * 32768                          # (a length the FFT is quick at)
    spec = np.fft.rfft(rng.standard_normal((m, 2)), axis=0)
    spec[int(15000. * m / 48000.):] = 0
    if highpass:
        spec[:int(highpass * m / 48000.)] = 0
    carrier = np.fft.irfft(spec, m, axis=0)[:n]
    knots = rng.uniform(-1., 1., n // 480 + 2)
    env = 1. + 0.9 * np.interp(np.arange(n) / 480., np.arange(len(knots)), knots)
    return (0.1 * carrier * env[:, None]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def found_inputs():
    rng = np.random.default_rng(2024)
    pairs = []
    for p, d in enumerate(FOUND_OFFSETS):
        base = modulated(rng, N10 + 2 * REACH, highpass=2000. if p == 6 else None)
        r, t = offset_pair(base, REACH, d, N10, N10)
        t = t + (0.1 * np.sqrt(np.mean(t.astype(np.float64) ** 2)) * rng.standard_normal(t.shape)).astype(np.float32)   # 20 dB down
        if p == 2:
            t = -t                                      # polarity-inverted
        pairs.append((r, t))
    return pairs


def test_it_finds_what_the_plain_search_cannot():
    import gstpeaq_amd
    pairs = found_inputs()
    max_offset, max_lag = 400000, 4096
    M = gstpeaq_amd.wide_factor(max_offset)
    assert M == 32
    h = gstpeaq_amd.wide_taps(M)
    # the inputs allow it: the numpy model of the coarse stage lands within half the fine range
    for (r, t), d in zip(pairs, FOUND_OFFSETS):
        lag, corr, _ = coarse_model(r, t, M, "envelope", h, -(-max_offset // M))
        print("offset %d: the model's coarse lag %d (%+d), correlation %.3f" % (d, lag * M, lag * M - d, corr))
        assert abs(lag * M - d) < max_lag // 2, (d, lag * M)
    ref, _ = batch([r for r, _ in pairs])
    test, _ = batch([t for _, t in pairs])
    got = gstpeaq_amd.estimate_delay_wide(ctx(), ref, test, max_offset, "envelope", max_lag)
    print("lags", got["lag"], "coarse", got["coarse_lag"], "flags", got["flags"])
    assert got["lag"].tolist() == list(FOUND_OFFSETS), got
    assert (got["flags"] == 0).all() and (got["factor"] == M).all(), got
    assert (np.abs(got["coarse_lag"] - np.array(FOUND_OFFSETS)) < max_lag // 2).all()
    assert got["fine"]["peak"][2] < 0 and (np.delete(got["fine"]["peak"], 2) > 0).all()   # the sign shows in the peak
    plain = gstpeaq_amd.estimate_delay(ctx(), ref, test, 16384)["lag"]
    assert (plain != np.array(FOUND_OFFSETS)).all(), plain


# ---- flags ------------------------------------------------------------------------------------------------------------
def test_flags_for_silence_a_nan_and_an_offset_out_of_range():
    import gstpeaq_amd
    rng = np.random.default_rng(31)
    n, max_offset, max_lag = 144000, 32768, 4096
    M = gstpeaq_amd.wide_factor(max_offset)
    reach = -(-max_offset // M)
    assert (M, reach) == (2, 16384)
    h = gstpeaq_amd.wide_taps(M)
    beyond = max_offset + 2            # one decimated sample past the range: the peak's flank makes the edge the largest
    base = modulated(rng, n + 2 * beyond)
    r0, t0 = offset_pair(base, beyond, 1000, n, n)
    silent = np.zeros_like(t0)
    with_nan = t0.copy()
    with_nan[70001, 1] = np.nan
    r2, t2 = offset_pair(base, beyond, beyond, n, n)
    pairs = [(r0, silent), (r0, with_nan), (r2, t2), (r0, t0)]
    # the numpy model says the same: no norm, a NaN norm, the largest correlation at the edge of the range, and a plain case
    model = [coarse_model(r, t, M, "envelope", h, reach) for r, t in pairs]
    assert model[0][2] == 0 and np.isnan(model[1][2]) and model[2][0] == reach and model[3][0] * M in range(990, 1011), model
    ref, _ = batch([r for r, _ in pairs])
    test, _ = batch([t for _, t in pairs])
    got = gstpeaq_amd.estimate_delay_wide(ctx(), ref, test, max_offset, "envelope", max_lag)
    plain = gstpeaq_amd.estimate_delay(ctx(), ref, test, max_lag)
    print(got)
    assert got["flags"][0] == NONE and got["coarse"]["norm"][0] == 0 and got["coarse_lag"][0] == 0
    assert got["lag"][0] == plain["lag"][0] == 0
    assert got["flags"][1] & NONE and np.isnan(got["coarse"]["norm"][1]) and got["coarse_lag"][1] == 0
    assert got["lag"][1] == plain["lag"][1]
    assert got["flags"][2] == RANGE and got["coarse"]["lag"][2] == reach and got["coarse_lag"][2] == max_offset
    assert got["lag"][2] == beyond and got["fine"]["lag"][2] == 2
    assert got["flags"][3] == 0 and got["lag"][3] == 1000


# ---- end to end -------------------------------------------------------------------------------------------------------
def hand_cut(r, t, d):
    return (r[:len(r) - d], t[d:]) if d >= 0 else (r[-d:], t[:len(t) + d])


def same_result(got, want):
    assert np.array_equal(bits(got["movs"]), bits(want["movs"])), (got, want)
    assert np.isfinite(want["odg"]) and np.isfinite(want["di"]), want
    assert got["di"] == want["di"] and got["odg"] == want["odg"] and got["frames"] == want["frames"], (got, want)


@pytest.mark.parametrize("advanced", [0, 1])
def test_batch_run_with_wide_scores_the_pairs_cut_by_hand(advanced):
    import gstpeaq_amd
    pairs = [found_inputs()[p] for p in (4, 5)]
    offsets = [FOUND_OFFSETS[p] for p in (4, 5)]
    ref, _ = batch([r for r, _ in pairs])
    test, _ = batch([t for _, t in pairs])
    got = gstpeaq_amd.batch_run(ctx(), advanced, ref, test, align=4096, wide=400000)
    assert gstpeaq_amd.align.last_wide["lag"].tolist() == offsets
    cut = [hand_cut(r, t, d) for (r, t), d in zip(pairs, offsets)]
    cref, n_cut = batch([r for r, _ in cut])
    ctest, _ = batch([t for _, t in cut])
    want = gstpeaq_amd.batch_run(ctx(), advanced, cref, ctest, n_cut, n_cut)
    for g, w in zip(got, want):
        same_result(g, w)


def test_run_pair_with_wide_is_peaq_run_pair_wide_and_the_cli_prints_it(tmp_path):
    import gstpeaq_amd
    c = ctx()
    r, t = found_inputs()[4]
    d = FOUND_OFFSETS[4]
    got = gstpeaq_amd.run_pair(c, 0, r, t, align=4096, wide=400000)
    assert got["delay"]["lag"] == d and got["wide"]["flags"] == 0 and got["wide"]["factor"] == 32, got
    same_result(got, gstpeaq_amd.run_pair(c, 0, *hand_cut(r, t, d)))
    rec, out = gstpeaq_amd.WideDelay(), np.zeros(16)
    fp = C.POINTER(C.c_float)
    assert c.L.peaq_run_pair_wide(c.h, 0, 2, 92., 48000, 400000, gstpeaq_amd.WIDE_ENVELOPE, 4096, r.ctypes.data_as(fp), len(r),
                                  t.ctypes.data_as(fp), len(t), C.byref(rec), out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert rec.lag == d and rec.coarse_lag == got["wide"]["coarse_lag"] and rec.fine.peak == got["wide"]["fine"]["peak"]
    assert np.array_equal(out[:11], got["movs"]) and out[12] == got["odg"] and out[11] == got["di"]
    write_wav(tmp_path / "ref.wav", r)
    write_wav(tmp_path / "late.wav", t)
    run = run_cli("--align-wide=8", tmp_path / "ref.wav", tmp_path / "late.wav")
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 4, run.stdout
    assert lines[0] == "Delay: %d samples (correlation %.3f)" % (d, rec.fine.peak / rec.fine.norm), run.stdout
    assert lines[1].startswith("Wide: coarse %d samples, factor 32, envelope" % rec.coarse_lag), run.stdout
    assert lines[2] == "Objective Difference Grade: %.3f" % got["odg"] and lines[3] == "Distortion Index: %.3f" % got["di"]

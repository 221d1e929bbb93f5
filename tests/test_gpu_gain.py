"""Level and polarity matching on the device against FP64 numpy (include/peaq_amd.h, "level and polarity matching on
the device"): the sums against math.fsum within the header's bound, the gain within 1 ulp of the numpy
expression on the record's own sums, exact cases, flags, cut_scaled bit for bit, independence of the batch,
determinism, and the keyword paths bit for bit against the stage's own entry points called one by one."""
import math
import re
from pathlib import Path

import numpy as np
import pytest

import gpu_common
import synth_np

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CHUNK = int(re.search(r"^#define\s+PEAQ_GAIN_CHUNK\s+(\d+)", (ROOT / "include" / "peaq_amd.h").read_text(), flags=re.M).group(1))
LENGTHS = (0, 1, 2, 3, 5, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7)
BOUND = 1e-12                    # |S - exact| <= BOUND * sum |term| (the header's)
SILENT, NONFINITE, ZERO, RANGE = 1, 2, 4, 8


def ctx():
    return gpu_common.ctx("default")


def cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def same_result(a, b):
    return all(np.array([a[k]]).tobytes() == np.array([b[k]]).tobytes() for k in ("di", "odg", "totalsnr")) and \
        a["frames"] == b["frames"] and a["fb_blocks"] == b["fb_blocks"] and a["movs"].tobytes() == b["movs"].tobytes()


def measure(ref, test, mode, **kw):
    import gstpeaq_amd
    _, read = gstpeaq_amd.measure_gain(ctx(), cuda(ref), cuda(test), mode, **kw)
    return read()


def ulp_apart(a, b):
    return a == b or (np.isfinite(a) and np.isfinite(b) and abs(a - b) <= np.spacing(abs(b)))


def expected_gain(mode, srr, stt, srt):
    srr, stt, srt = np.float64(srr), np.float64(stt), np.float64(srt)
    if mode == "lsq":
        return srt / stt
    if mode == "rms":
        return np.copysign(np.sqrt(srr / stt), -1.0 if srt < 0 else 1.0)
    return np.float64(-1.0 if srt < 0 else 1.0)


# ---- 1. the sums ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
def test_sums_against_fsum_for_every_phase_pair_and_length(channels):
    """one call: a pair per (skip_ref % 4, skip_test % 4, length); the two buffers have different strides, so the pair
    bases walk through the phases too"""
    rng = np.random.default_rng(11 + channels)
    cases = [(sr, st, n) for sr in range(4) for st in range(4) for n in LENGTHS]
    longest = max(LENGTHS)
    ref = rng.standard_normal((len(cases), longest + 9, channels)).astype(np.float32)
    test = rng.standard_normal((len(cases), longest + 14, channels)).astype(np.float32)
    skip_ref = np.array([4 * (i % 2) + c[0] for i, c in enumerate(cases)], np.uint32)
    skip_test = np.array([4 * (i % 3) + c[1] for i, c in enumerate(cases)], np.uint32)
    n = np.array([c[2] for c in cases], np.uint32)
    rec = measure(ref, test, "lsq", skip_ref=skip_ref, skip_test=skip_test, n=n, per_channel=True, max_gain_db=120.0)
    assert (rec["n"] == n).all()
    worst = 0.0
    for p, (sr, st, k) in enumerate(cases):
        r = ref[p, skip_ref[p]:skip_ref[p] + k].astype(np.float64)
        t = test[p, skip_test[p]:skip_test[p] + k].astype(np.float64)
        for c in range(channels):
            for name, terms in (("srr", r[:, c] * r[:, c]), ("stt", t[:, c] * t[:, c]), ("srt", r[:, c] * t[:, c])):
                exact, scale = math.fsum(terms), math.fsum(np.abs(terms))
                got = rec[name][p, c]
                assert abs(got - exact) <= BOUND * scale, (p, sr, st, k, c, name, got, exact)
                if scale:
                    worst = max(worst, abs(got - exact) / scale)
        if channels == 1:
            assert rec["srr"][p, 1] == 0 and rec["stt"][p, 1] == 0 and rec["srt"][p, 1] == 0, p
    print("channels", channels, "worst |S - exact| / sum |term|:", worst)


# ---- 2. the gain ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_channel", [False, True], ids=["joint", "per_channel"])
@pytest.mark.parametrize("mode", ["lsq", "rms", "polarity"])
def test_gain_is_the_numpy_expression_on_the_records_own_sums(mode, per_channel):
    rng = np.random.default_rng(3)
    for channels in (1, 2):
        ref = rng.standard_normal((6, 3001, channels)).astype(np.float32)
        scale = np.array([0.31, -0.7, 1.9, -2.3, 0.05, 11.0], np.float32)[:, None, None]
        test = (ref * scale + 0.1 * rng.standard_normal(ref.shape)).astype(np.float32)
        if channels == 2:
            test[:, :, 1] *= np.float32(-0.45)           # the channels differ, in sign too
        rec = measure(ref, test, mode, per_channel=per_channel)
        assert not rec["flags"].any(), rec["flags"]
        for p in range(6):
            if per_channel and channels == 2:
                for c in range(2):
                    exp = expected_gain(mode, rec["srr"][p, c], rec["stt"][p, c], rec["srt"][p, c])
                    assert ulp_apart(rec["gain"][p, c], exp), (p, c, rec["gain"][p, c], exp)
                assert rec["gain"][p, 0] != rec["gain"][p, 1]
            else:
                exp = expected_gain(mode, rec["srr"][p, 0] + rec["srr"][p, 1], rec["stt"][p, 0] + rec["stt"][p, 1],
                                    rec["srt"][p, 0] + rec["srt"][p, 1])
                assert ulp_apart(rec["gain"][p, 0], exp), (p, rec["gain"][p, 0], exp)
                assert rec["gain"][p, 1].tobytes() == rec["gain"][p, 0].tobytes(), p


@pytest.mark.parametrize("channels", [1, 2])
def test_exact_cases_bit_for_bit(channels):
    rng = np.random.default_rng(4)
    ref = rng.standard_normal((1, 2 * CHUNK + 77, channels)).astype(np.float32)
    for k in (-3, 1):
        test = (ref * np.float32(2.0 ** k)).astype(np.float32)
        for mode in ("lsq", "rms"):
            for pc in (False, True):
                rec = measure(ref, test, mode, per_channel=pc)
                assert (rec["gain"] == 2.0 ** -k).all() and not rec["flags"].any(), (k, mode, pc, rec["gain"])
    y = (ref + 0.2 * rng.standard_normal(ref.shape)).astype(np.float32)
    rec = measure(ref, -y, "polarity")
    assert (rec["gain"] == -1.0).all() and not rec["flags"].any(), rec["gain"]
    rec = measure(ref, y, "polarity", per_channel=True)
    assert (rec["gain"] == 1.0).all() and not rec["flags"].any(), rec["gain"]


# ---- 3. the flags --------------------------------------------------------------------------------------------------
def test_flags_keep_the_gain_at_one_and_report_the_finite_sums():
    rng = np.random.default_rng(5)
    ref = rng.standard_normal((1, 500, 2)).astype(np.float32)
    srr = [math.fsum(ref[0, :, c].astype(np.float64) ** 2) for c in range(2)]
    # silence
    rec = measure(ref, np.zeros_like(ref), "lsq")
    assert (rec["flags"] == SILENT).all() and (rec["gain"] == 1.0).all(), rec
    assert (rec["stt"] == 0).all() and (rec["srt"] == 0).all() and np.allclose(rec["srr"][0], srr, rtol=1e-12)
    rec = measure(ref, ref, "rms", n=[0])
    assert (rec["flags"] == SILENT).all() and (rec["gain"] == 1.0).all() and rec["n"][0] == 0
    # a NaN or an Inf sample, in channel 1: per channel only that one is flagged, jointly both
    for bad in (np.nan, np.inf, -np.inf):
        test = ref.copy()
        test[0, 123, 1] = bad
        rec = measure(ref, test, "lsq", per_channel=True)
        assert rec["flags"][0].tolist() == [0, NONFINITE] and rec["gain"][0].tolist() == [1.0, 1.0], (bad, rec)
        assert rec["stt"][0, 0] == rec["srr"][0, 0] and np.isclose(rec["srr"][0, 1], srr[1], rtol=1e-12), (bad, rec)
        rec = measure(ref, test, "rms")
        assert (rec["flags"] == NONFINITE).all() and (rec["gain"] == 1.0).all(), (bad, rec)
        assert np.isclose(rec["stt"][0, 0], srr[0], rtol=1e-12)
    # a reference orthogonal to the test signal under LSQ
    r = np.zeros((1, 40, 1), np.float32)
    t = np.zeros((1, 40, 1), np.float32)
    r[0, :2, 0] = [1, 1]
    t[0, :2, 0] = [1, -1]
    rec = measure(r, t, "lsq")
    assert (rec["flags"] == ZERO).all() and (rec["gain"] == 1.0).all() and rec["srt"][0, 0] == 0 and rec["srr"][0, 0] == 2 \
        and rec["stt"][0, 0] == 2, rec
    assert not measure(r, t, "rms")["flags"].any() and not measure(r, t, "polarity")["flags"].any()
    # out of range
    test = (ref * np.float32(1e-4)).astype(np.float32)
    rec = measure(ref, test, "lsq", max_gain_db=40.0)
    assert (rec["flags"] == RANGE).all() and (rec["gain"] == 1.0).all() and (rec["stt"][0] > 0).all(), rec
    rec = measure(ref, test, "lsq", max_gain_db=100.0)
    assert not rec["flags"].any() and np.allclose(rec["gain"], 1e4, rtol=1e-6), rec
    rec = measure(test, ref, "rms", max_gain_db=40.0)      # ... and the other way round
    assert (rec["flags"] == RANGE).all() and (rec["gain"] == 1.0).all(), rec


# ---- 4. cut_scaled -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
def test_cut_scaled_against_numpy_bit_for_bit(channels):
    import gstpeaq_amd
    import torch
    rng = np.random.default_rng(5)
    n_pairs, stride = 7, 5003
    x = rng.standard_normal((n_pairs, stride, channels)).astype(np.float32)
    skip = np.array([0, 1, 2, 3, 1000, 4999, 17], np.uint32)
    keep = np.array([5003, 5002, 0, 1, 4003, 4, 1234], np.uint32)
    ref = (x * np.linspace(0.3, 2.2, n_pairs, dtype=np.float32)[:, None, None]).astype(np.float32)
    if channels == 2:
        ref[:, :, 1] *= np.float32(-1.7)
    d = cuda(x)
    for pc in (False, True):
        rec, read = gstpeaq_amd.measure_gain(ctx(), cuda(ref), d, "lsq", per_channel=pc)
        g = read()["gain"]
        assert (g != 1.0).all() and (not pc or channels == 1 or (g[:, 0] != g[:, 1]).all()), g
        for out in (None, torch.full((n_pairs, 6001, channels), -7.5, dtype=torch.float32, device="cuda")):
            y = gstpeaq_amd.cut_scaled(ctx(), d, skip, keep, rec, out=out)
            torch.cuda.synchronize()
            y = y.cpu().numpy()
            for p in range(n_pairs):
                exp = (x[p, skip[p]:skip[p] + keep[p]].astype(np.float64) * g[p, :channels]).astype(np.float32)
                assert y[p, :keep[p]].tobytes() == exp.tobytes(), (pc, p)
                assert (y[p, keep[p]:] == (0.0 if out is None else -7.5)).all(), (pc, p)   # poisoned: untouched past n_keep
    with pytest.raises(gstpeaq_amd.PeaqError, match="overlaps"):
        gstpeaq_amd.cut_scaled(ctx(), d, skip, np.minimum(keep, 3), rec, out=d)


@pytest.mark.parametrize("channels", [1, 2])
def test_cut_scaled_with_gains_of_one_is_cut_nan_payloads_included(channels):
    import gstpeaq_amd
    import torch
    rng = np.random.default_rng(6)
    x = rng.standard_normal((5, 1031, channels)).astype(np.float32)
    bits = x.view(np.uint32)
    bits[0, 7, 0] = 0x7FC12345                             # quiet NaNs with payloads, a signalling one, -0, a denormal
    bits[1, 3, channels - 1] = 0xFFA00001
    bits[2, 1000, 0] = 0x7F812345
    bits[3, 5, 0] = 0x80000000
    bits[4, 6, 0] = 0x00000001
    skip = np.array([0, 1, 2, 3, 5], np.uint32)
    keep = np.array([1031, 1030, 1029, 1028, 1001], np.uint32)
    d = cuda(x)
    rec, read = gstpeaq_amd.measure_gain(ctx(), d, d, None)           # OFF: sums only, gain 1.0
    assert (read()["gain"] == 1.0).all()
    a = gstpeaq_amd.cut(ctx(), d, skip, keep)
    b = gstpeaq_amd.cut_scaled(ctx(), d, skip, keep, rec)
    torch.cuda.synchronize()
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    for p in range(5):
        assert b[p, :keep[p]].cpu().numpy().tobytes() == x[p, skip[p]:skip[p] + keep[p]].tobytes(), p
    if channels == 2:
        # one channel at 1.0 (its bits moved), the other scaled: a hand-made record
        g = np.zeros(5, gstpeaq_amd.GAIN_DTYPE)
        g["gain"] = [1.0, -0.375]
        y = gstpeaq_amd.cut_scaled(ctx(), d, skip, keep, cuda(g.view(np.uint8).reshape(5, 80)))
        torch.cuda.synchronize()
        y = y.cpu().numpy()
        for p in range(5):
            src = x[p, skip[p]:skip[p] + keep[p]]
            assert y[p, :keep[p], 0].tobytes() == src[:, 0].tobytes(), p
            exp = (src[:, 1].astype(np.float64) * -0.375).astype(np.float32)
            ok = ~np.isnan(exp)
            assert y[p, :keep[p], 1][ok].tobytes() == exp[ok].tobytes() and np.isnan(y[p, :keep[p], 1][~ok]).all(), p


# ---- 5. independence and determinism ---------------------------------------------------------------------------------
def test_record_of_a_pair_does_not_depend_on_its_batch_and_runs_repeat():
    import gstpeaq_amd
    rng = np.random.default_rng(8)
    n_pairs, stride = 64, 2 * CHUNK + 301
    ref = rng.standard_normal((n_pairs, stride, 2)).astype(np.float32)
    test = (0.6 * ref + 0.1 * rng.standard_normal(ref.shape)).astype(np.float32)
    skip_ref = rng.integers(0, 40, n_pairs).astype(np.uint32)
    skip_test = rng.integers(0, 40, n_pairs).astype(np.uint32)
    n = rng.integers(1, stride - 40, n_pairs).astype(np.uint32)
    n[17] = stride - 40
    d_ref, d_test = cuda(ref), cuda(test)
    runs = []
    for _ in (0, 1):
        _, read = gstpeaq_amd.measure_gain(ctx(), d_ref, d_test, "rms", skip_ref, skip_test, n, per_channel=True)
        runs.append(read())
    for k in runs[0]:
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), k
    for p in (0, 17, 63):                                  # alone, in buffers of its own (another base, another phase)
        r = ref[p:p + 1, skip_ref[p]:skip_ref[p] + n[p]]
        t = test[p:p + 1, skip_test[p]:skip_test[p] + n[p]]
        alone = measure(np.concatenate([np.zeros((1, 3, 2), np.float32), r], axis=1), t, "rms", skip_ref=[3], n=[n[p]],
                        per_channel=True)
        for k in alone:
            assert alone[k][0].tobytes() == runs[0][k][p].tobytes(), (p, k, alone[k][0], runs[0][k][p])


# ---- 6. the keyword paths, bit for bit -------------------------------------------------------------------------------
E2E_N = 48000


def quantised(x, bits=10):
    return (np.round(x.astype(np.float64) * 2 ** bits) / 2 ** bits).astype(np.float32)


def late(x, d):
    return np.concatenate([np.zeros((d, x.shape[1]), np.float32), x])


def batch(pairs):
    ch = pairs[0][0].shape[1]
    stride = max(max(len(r), len(t)) for r, t in pairs)
    stride += stride & 1
    a = np.zeros((2, len(pairs), stride, ch), np.float32)
    for p, (r, t) in enumerate(pairs):
        a[0, p, :len(r)], a[1, p, :len(t)] = r, t
    return cuda(a[0]), cuda(a[1]), np.array([len(r) for r, _ in pairs], np.uint32), np.array([len(t) for _, t in pairs], np.uint32)


def by_hand(ref, test, n_ref, n_test, max_lag, mode, **kw):
    """estimate_delay, measure_gain, cut and cut_scaled one by one -> (ref', test', n, records)"""
    import gstpeaq_amd
    lags = gstpeaq_amd.estimate_delay(ctx(), ref, test, max_lag, n_ref, n_test)["lag"] if max_lag else np.zeros(len(n_ref), int)
    cuts = np.array([gstpeaq_amd.aligned_lengths(int(lags[p]), int(n_ref[p]), int(n_test[p])) for p in range(len(n_ref))], np.uint32)
    rec, read = gstpeaq_amd.measure_gain(ctx(), ref, test, mode, cuts[:, 0], cuts[:, 1], cuts[:, 2], **kw)
    r = gstpeaq_amd.cut(ctx(), ref, cuts[:, 0], cuts[:, 2])
    t = gstpeaq_amd.cut_scaled(ctx(), test, cuts[:, 1], cuts[:, 2], rec)
    return r, t, np.ascontiguousarray(cuts[:, 2]), read(), lags


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("advanced", [0, 1], ids=["basic", "advanced"])
def test_keywords_equal_the_stages_called_one_by_one(advanced, channels):
    import gstpeaq_amd
    x, y = synth_np.pair(41, channels, E2E_N)
    pairs = [(x, late((quantised(x) * np.float32(0.3)).astype(np.float32), 37))]
    ref, test, n_ref, n_test = batch(pairs)
    r, t, n, rec, lags = by_hand(ref, test, n_ref, n_test, 64, "lsq")
    assert lags[0] == 37 and abs(rec["gain"][0, 0] - 1 / 0.3) < 0.05 and not rec["flags"].any(), (lags, rec)
    exp = gstpeaq_amd.batch_run(ctx(), advanced, r, t, n, n)
    got = gstpeaq_amd.batch_run(ctx(), advanced, ref, test, n_ref, n_test, align=64, gain="lsq")
    assert same_result(got[0], exp[0]), (got[0], exp[0])
    one = gstpeaq_amd.run_pair(ctx(), advanced, *pairs[0], align=64, gain="lsq")
    assert same_result(one, exp[0]) and one["delay"]["lag"] == 37, (one, exp[0])
    for k in ("gain", "srr", "stt", "srt", "flags"):
        assert np.array(one["gain"][k], dtype=rec[k].dtype).tobytes() == rec[k][0].tobytes(), (k, one["gain"], rec)
    # exact: -0.25 y, late, with the polarity alone undone is (x, 0.25 y) aligned
    q = (y * np.float32(0.25)).astype(np.float32)
    got = gstpeaq_amd.batch_run(ctx(), advanced, *batch([(x, late(-q, 37))]), align=64, gain="polarity")
    exp = gstpeaq_amd.batch_run(ctx(), advanced, *batch([(x, late(q, 37))]), align=64)
    assert same_result(got[0], exp[0]), (got[0], exp[0])
    # exact: 0.5 x under LSQ is (x, x); and matching helps a pair that is only quieter
    same = gstpeaq_amd.batch_run(ctx(), advanced, *batch([(x, x)]))
    got = gstpeaq_amd.batch_run(ctx(), advanced, *batch([(x, (x * np.float32(0.5)).astype(np.float32))]), gain="lsq")
    assert same_result(got[0], same[0]), (got[0], same[0])
    quiet = batch([(x, (x * np.float32(0.3)).astype(np.float32))])
    matched = gstpeaq_amd.batch_run(ctx(), advanced, *quiet, gain="lsq")[0]
    plain = gstpeaq_amd.batch_run(ctx(), advanced, *quiet)[0]
    print("ODG matched", matched["odg"], "unmatched", plain["odg"])
    assert matched["odg"] > plain["odg"], (matched, plain)
    # gain=None is what it was
    a = gstpeaq_amd.batch_run(ctx(), advanced, ref, test, n_ref, n_test, align=64)
    b = gstpeaq_amd.batch_run(ctx(), advanced, ref, test, n_ref, n_test, align=64, gain=None)
    assert same_result(a[0], b[0])


def test_trajectory_and_trace_keywords_equal_the_plain_calls_on_matched_buffers():
    import gstpeaq_amd
    x, _ = synth_np.pair(42, 2, E2E_N)
    ref, test, n_ref, n_test = batch([(x, late((quantised(x) * np.float32(-0.4)).astype(np.float32), 21))])
    r, t, n, rec, _ = by_hand(ref, test, n_ref, n_test, 64, "rms", per_channel=True)
    for advanced in (0, 1):
        pts, res = gstpeaq_amd.batch_trajectory(ctx(), advanced, ref, test, 9600, 5, n_ref, n_test, align=64, gain="rms",
                                                gain_per_channel=True)
        epts, eres = gstpeaq_amd.batch_trajectory(ctx(), advanced, r, t, 9600, 5, n, n)
        assert same_result(res[0], eres[0]) and all(same_result(pts[0][k], epts[0][k]) for k in range(5))
        got = gstpeaq_amd.batch_trace(ctx(), advanced, ref, test, n_ref, n_test, align=64, gain="rms", gain_per_channel=True)
        exp = gstpeaq_amd.batch_trace(ctx(), advanced, r, t, n, n)
        assert same_result(got["results"][0], exp["results"][0]) and same_result(got["results"][0], eres[0])
        assert got["frames"].tobytes() == exp["frames"].tobytes()
        if advanced:
            assert got["blocks"].tobytes() == exp["blocks"].tobytes()


def test_gain_after_rate_conversion_equals_resample_then_align_then_match():
    import gstpeaq_amd
    import torch
    x, _ = synth_np.pair(43, 2, 44100)
    pairs = [(x, late((quantised(x) * np.float32(0.45)).astype(np.float32), 30))]
    ref, test, n_ref, n_test = batch(pairs)
    got = gstpeaq_amd.batch_run(ctx(), 0, ref, test, n_ref, n_test, rate=44100, align=64, gain="lsq")
    longest = max(gstpeaq_amd.resampled_length(int(v), 44100) for v in list(n_ref) + list(n_test))
    r48, t48 = (torch.zeros((1, longest + (longest & 1), 2), dtype=torch.float32, device="cuda") for _ in (0, 1))
    _, o_ref = gstpeaq_amd.resample(ctx(), ref, 44100, n_ref, out=r48)
    _, o_test = gstpeaq_amd.resample(ctx(), test, 44100, n_test, out=t48)
    r, t, n, rec, _ = by_hand(r48, t48, o_ref, o_test, 64, "lsq")
    exp = gstpeaq_amd.batch_run(ctx(), 0, r, t, n, n)
    assert same_result(got[0], exp[0]), (got[0], exp[0])
    one = gstpeaq_amd.run_pair(ctx(), 0, *pairs[0], rate=44100, align=64, gain="lsq")
    assert same_result(one, exp[0]), (one, exp[0])


# ---- 7. the feed -----------------------------------------------------------------------------------------------------
def test_feed_with_gain_equals_batch_run_on_the_decoded_tensors():
    import gstpeaq_amd
    rng = np.random.default_rng(9)
    refs, tests, index = [], [], []
    for r in range(2):
        x, y = synth_np.pair(50 + r, 2, 24000 + 1000 * r)
        refs.append(np.round(x * 32767 * 0.5).astype("<i2"))
        for k, (g, d) in enumerate(((0.5, 11), (-0.3, 0), (1.7, 40))):
            t = late((y if k else x) * np.float32(g * 0.5), d) + 1e-3 * rng.standard_normal((len(x) + d, 2)).astype(np.float32)
            tests.append(np.round(np.clip(t, -1, 1) * 32767).astype("<i2"))
            index.append(r)
    decoded = [(refs[index[t]].astype(np.float32) / np.float32(32768), tests[t].astype(np.float32) / np.float32(32768))
               for t in range(len(tests))]
    ref, test, n_ref, n_test = batch(decoded)
    for advanced in (0, 1):
        exp = gstpeaq_amd.batch_run(ctx(), advanced, ref, test, n_ref, n_test, align=64, gain="rms")
        *_, rec, lags = by_hand(ref, test, n_ref, n_test, 64, "rms")
        for chunk_pairs in (0, 2):
            res, delays, gains = gstpeaq_amd.run_host_refs(ctx(), advanced, refs, tests, index, "s16", 2, align=64, gain="rms",
                                                           chunk_pairs=chunk_pairs)
            for t in range(len(tests)):
                assert same_result(res[t], exp[t]), (advanced, chunk_pairs, t, res[t], exp[t])
            assert (delays["lag"] == lags).all()
            for k in rec:
                assert gains[k].tobytes() == rec[k].tobytes(), (chunk_pairs, k, gains[k], rec[k])
        # plain pairs: one test per reference
        res2, _, gains2 = gstpeaq_amd.run_host(ctx(), advanced, [(refs[index[t]], tests[t]) for t in range(len(tests))], "s16", 2,
                                               align=64, gain="rms")
        assert all(same_result(res2[t], exp[t]) for t in range(len(tests))) and gains2["gain"].tobytes() == rec["gain"].tobytes()
        # without alignment: skips of 0 and the shorter length
        res3, gains3 = gstpeaq_amd.run_host_refs(ctx(), advanced, refs, tests, index, "s16", 2, gain="lsq", gain_per_channel=True)
        exp3 = gstpeaq_amd.batch_run(ctx(), advanced, ref, test, n_ref, n_test, gain="lsq", gain_per_channel=True)
        assert all(same_result(res3[t], exp3[t]) for t in range(len(tests)))
        # gain=None is the shared feed as it stands, and so is PEAQ_GAIN_OFF through the new entry point
        a, da = gstpeaq_amd.run_host_refs(ctx(), advanced, refs, tests, index, "s16", 2, align=64)
        b, db = gstpeaq_amd.run_host_refs(ctx(), advanced, refs, tests, index, "s16", 2, align=64, gain=None)
        c, dc, gc = gstpeaq_amd.run_host_refs(ctx(), advanced, refs, tests, index, "s16", 2, align=64, gain="off")
        assert all(same_result(a[t], b[t]) and same_result(a[t], c[t]) for t in range(len(tests)))
        assert (da["lag"] == dc["lag"]).all() and not gc["gain"].any()


# ---- 8. the CLI ------------------------------------------------------------------------------------------------------
def write_wav(path, x, rate=48000):
    """x [n, channels] as a 32-bit float RIFF/WAVE file"""
    import struct
    x = np.asarray(x)
    ch = x.shape[1]
    body = x.astype("<f4").tobytes()
    fmt = struct.pack("<HHIIHH", 3, ch, rate, rate * ch * 4, ch * 4, 32)
    chunks = b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(body)) + body
    Path(path).write_bytes(b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks)


def run_cli(*args):
    import subprocess
    import gst_env
    return subprocess.run([str(gst_env.CLI), *map(str, args)], capture_output=True, text=True, timeout=300)


def cli_built():
    import gst_env
    return gst_env.CLI.exists()


@pytest.mark.skipif(not cli_built(), reason="gstpeaq_amd/cli/peaq not built")
def test_cli_match_gain_prints_the_gain_and_the_matched_grade(tmp_path):
    x, _ = synth_np.pair(44, 2, E2E_N)
    half = late((x * np.float32(0.5)).astype(np.float32), 37)       # test = 0.5 x, late: the matched factor is exactly 2
    write_wav(tmp_path / "ref.wav", x)
    write_wav(tmp_path / "full.wav", late(x, 37))
    write_wav(tmp_path / "half.wav", half)
    write_wav(tmp_path / "inv.wav", -half)
    full = run_cli("--align=64", tmp_path / "ref.wav", tmp_path / "full.wav")
    assert full.returncode == 0, full.stdout + full.stderr
    out = run_cli("--align=64", "--match-gain=rms", tmp_path / "ref.wav", tmp_path / "half.wav")
    assert out.returncode == 0, out.stdout + out.stderr
    lines, grade = out.stdout.strip().splitlines(), full.stdout.strip().splitlines()
    assert len(lines) == 4 and lines[0] == grade[0] and lines[0].startswith("Delay: 37 samples"), out.stdout
    assert lines[1].startswith("Gain: ") and "+6.02 dB" in lines[1] and "inverted" not in lines[1], out.stdout
    assert lines[2:] == grade[1:], (out.stdout, full.stdout)          # (a factor of exactly 2: the unscaled pair's buffers)
    out = run_cli("--align=64", "--match-gain", "--gain-per-channel", "--advanced", tmp_path / "ref.wav", tmp_path / "inv.wav")
    assert out.returncode == 0 and out.stdout.count("inverted") == 2, out.stdout + out.stderr
    # --list: one gain per pair
    (tmp_path / "list.txt").write_text("%s\t%s\n%s\t%s\n" % (tmp_path / "ref.wav", tmp_path / "half.wav", tmp_path / "ref.wav",
                                                           tmp_path / "inv.wav"))
    out = run_cli("--list=%s" % (tmp_path / "list.txt"), "--align=64", "--match-gain=rms")
    assert out.returncode == 0, out.stdout + out.stderr
    rows = out.stdout.strip().splitlines()
    assert len(rows) == 2 and all(r.count("Gain: ") == 1 and "+6.02 dB" in r for r in rows), out.stdout
    assert "inverted" not in rows[0] and "inverted" in rows[1], out.stdout
    assert rows[0].split("\t")[2:4] == [grade[1].split()[-1], grade[2].split()[-1]], out.stdout
    # without the option the output is what it was; with --interval or --trace the option is refused
    plain = run_cli("--align=64", tmp_path / "ref.wav", tmp_path / "half.wav")
    assert plain.returncode == 0 and "Gain" not in plain.stdout and len(plain.stdout.strip().splitlines()) == 3
    assert run_cli("--match-gain", "--interval=0.5", tmp_path / "ref.wav", tmp_path / "half.wav").returncode == 1
    assert run_cli("--match-gain", "--trace=%s" % (tmp_path / "t.csv"), tmp_path / "ref.wav", tmp_path / "half.wav").returncode == 1
    assert run_cli("--match-gain=loud", tmp_path / "ref.wav", tmp_path / "half.wav").returncode == 1
    assert run_cli("--match-gain", "--max-gain=0", tmp_path / "ref.wav", tmp_path / "half.wav").returncode == 1

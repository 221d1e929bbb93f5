"""The sub-sample stage on the device against FP64 numpy (include/peaq_amd.h, "sub-sample delay on the device";
DESIGN.md 16): cut_shifted against the numpy sum, refine_delay against math.fsum and the numpy arg-max, flags,
independence of the batch, determinism, the keyword paths bit for bit against the stage's entry points called one by
one, and what the stage is for: a pair delayed by a non-integer amount scores as the undelayed one does.

Tolerance of cut_shifted, as tests/test_gpu_resample.py states it for the converter: both sides round an FP64 sum of 65
products to FP32 once (one FP32 ulp, 2^-23 |y|); the two sums differ by summation rounding and by the device fusing
multiply and add, bounded by 65 x 2^-53 x sum|h| x max|x|.  sum|h| is largest for the half-sample row, 4.17 (read from
the table below and asserted), so the bound is 65 x 1.11e-16 x 4.17 max|x| = 3.0e-14 max|x|, rounded up to 1e-13 max|x|."""
import math
import subprocess

import numpy as np
import pytest

import gpu_common

pytestmark = pytest.mark.gpu

R, K, STEPS = 16, 32, 256
NONE, EDGE = 1, 2
TILE = 1024                      # outputs per workgroup of frac_cut_kernel
SUM_BOUND = 1e-13                # x max|x|: see above
CK_BOUND = 1e-12                 # |c_k - exact| <= CK_BOUND * sum |term| (the header's)


def ctx():
    return gpu_common.ctx("default")


def cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def tables():
    import gstpeaq_amd
    if not hasattr(tables, "t"):
        tables.t = gstpeaq_amd.subsample_tables()
    return tables.t


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def same_result(a, b):
    return all(np.array([a[k]]).tobytes() == np.array([b[k]]).tobytes() for k in ("di", "odg", "totalsnr")) and \
        a["frames"] == b["frames"] and a["fb_blocks"] == b["fb_blocks"] and a["movs"].tobytes() == b["movs"].tobytes()


def shifted_model(x, n_in, skip, n_keep, q):
    """the header's sum in FP64, taps o = -32 .. 32 in order; x: [n, channels] float32"""
    h = tables()[1][q + STEPS // 2]
    z = np.zeros((K, x.shape[1]))
    pad = np.vstack([z, x[:n_in].astype(np.float64), z, np.zeros((skip + n_keep, x.shape[1]))])
    out = np.zeros((n_keep, x.shape[1]))
    for o in range(-K, K + 1):
        out += h[o + K] * pad[K + skip + o:K + skip + o + n_keep]
    return out


# ---- 1. cut_shifted -------------------------------------------------------------------------------------------------
KEEPS = (1, 31, 33, 4095, 4096, 4097, 2 * TILE + 5)      # the last spans three tiles
SKIPS = (0, 1, 2, 3, 31, 33)
QS = (-128, -1, 1, 77, 127)


@pytest.mark.parametrize("channels", [1, 2])
def test_cut_shifted_against_the_numpy_sum(channels):
    """one call: a pair per (n_keep, skip, n_in = skip + n_keep or 40 more), q mixed within the call, an odd in_stride;
    every sample compared, the sentinel behind n_keep kept"""
    import gstpeaq_amd
    h_abs = np.abs(tables()[1]).sum(axis=1).max()
    assert h_abs < 4.2 and 65 * 2.0 ** -53 * h_abs <= SUM_BOUND, h_abs
    rng = np.random.default_rng(40 + channels)
    cases = [(keep, skip, extra) for keep in KEEPS for skip in SKIPS for extra in (0, 40)]
    cases.append((0, 33, 40))                           # nothing kept, beside the long pairs: the sentinel stays
    qs = np.array([QS[i % len(QS)] for i in range(len(cases))], np.int32)
    in_stride = max(KEEPS) + max(SKIPS) + 40 + 1
    in_stride += 1 - (in_stride & 1)                    # odd
    assert in_stride & 1
    x = rng.standard_normal((len(cases), in_stride, channels)).astype(np.float32)
    skip = np.array([c[1] for c in cases], np.uint32)
    keep = np.array([c[0] for c in cases], np.uint32)
    n_in = np.array([c[0] + c[1] + c[2] for c in cases], np.uint32)
    import torch
    sentinel = np.float32(-77.25)
    out = torch.full((len(cases), max(KEEPS) + 3, channels), float(sentinel), dtype=torch.float32, device="cuda")
    gstpeaq_amd.cut_shifted(ctx(), cuda(x), skip, keep, qs, n_in=n_in, out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    worst = 0.0
    for p, (k, s, extra) in enumerate(cases):
        if k == 0:
            assert (got[p] == sentinel).all(), (p, s)
            continue
        want = shifted_model(x[p], int(n_in[p]), s, k, int(qs[p]))
        tol = 2.0 ** -23 * np.abs(want) + SUM_BOUND * np.abs(x[p]).max() + 1.5e-45
        err = np.abs(got[p, :k].astype(np.float64) - want)
        assert (err <= tol).all(), (p, k, s, extra, int(qs[p]), float((err / tol).max()), int(np.argmax((err / tol).max(axis=1))))
        worst = max(worst, float((err / tol).max()))
        assert (got[p, k:] == sentinel).all(), (p, k, s)
    print("channels", channels, "worst error / tolerance:", worst)


@pytest.mark.parametrize("channels", [1, 2])
def test_q_zero_is_bit_for_bit_cut_with_nan_payloads(channels):
    import gstpeaq_amd
    import torch
    rng = np.random.default_rng(50 + channels)
    cases = [(keep, skip) for keep in KEEPS for skip in SKIPS]
    in_stride = max(KEEPS) + max(SKIPS) + 1
    in_stride += 1 - (in_stride & 1)
    bits = rng.integers(0, 2 ** 32, size=(len(cases), in_stride, channels), dtype=np.uint32)
    bits[:, ::7] = 0x7FC12345                           # quiet NaNs with a payload
    bits[:, 3::11] = 0xFF800001                         # signalling, negative
    x = bits.view(np.float32)
    skip = np.array([c[1] for c in cases], np.uint32)
    keep = np.array([c[0] for c in cases], np.uint32)
    outs = [torch.full((len(cases), max(KEEPS) + 3, channels), -3.5, dtype=torch.float32, device="cuda") for _ in (0, 1)]
    gstpeaq_amd.cut(ctx(), cuda(x), skip, keep, out=outs[0])
    gstpeaq_amd.cut_shifted(ctx(), cuda(x), skip, keep, np.zeros(len(cases), np.int32), n_in=skip + keep, out=outs[1])
    torch.cuda.synchronize()
    a, b = outs[0].cpu().numpy(), outs[1].cpu().numpy()
    assert same_bits(a, b)
    for p, (k, s) in enumerate(cases):
        assert same_bits(b[p, :k], x[p, s:s + k]), (p, k, s)


# ---- 2. refine_delay ------------------------------------------------------------------------------------------------
def noise(kind, n, channels, seed):
    """band-limited (20 kHz) white or pink noise, FP64 [n, channels], rms 0.1"""
    rng = np.random.default_rng(seed)
    X = np.fft.rfft(rng.standard_normal((n, channels)), axis=0)
    f = np.fft.rfftfreq(n, 1 / 48000.0)
    if kind == "pink":
        X = X / np.sqrt(np.maximum(f, 20.0))[:, None]
    X[f > 20000.0] = 0
    y = np.fft.irfft(X, n, axis=0)
    return 0.1 * y / np.std(y)


def delayed(x, d):
    """x delayed by d samples (FFT phase rotation, zero-padded so that nothing wraps into the signal)"""
    n = len(x)
    N = 1 << int(np.ceil(np.log2(n + 4096)))
    X = np.fft.rfft(x, N, axis=0)
    f = np.arange(X.shape[0])[:, None] / N
    return np.fft.irfft(X * np.exp(-2j * np.pi * f * d), N, axis=0)[:n]


def model(ref, test, lag):
    """the header's estimate on the FP32 samples: (c [33] by math.fsum, sum |term| [33], v [256], q, margin)"""
    r = ref.astype(np.float64).sum(axis=1)
    t = test.astype(np.float64).sum(axis=1)
    c, scale = np.zeros(2 * R + 1), np.zeros(2 * R + 1)
    for k in range(-R, R + 1):
        d = lag + k
        lo, hi = max(0, -d), min(len(r), len(t) - d)
        if hi > lo:
            terms = r[lo:hi] * t[lo + d:hi + d]
            c[k + R], scale[k + R] = math.fsum(terms), math.fsum(np.abs(terms))
    s = -1.0 if c[R] < 0 else 1.0
    v = np.zeros(STEPS)
    for k in range(2 * R + 1):                          # k = -16 .. 16 in order, product and sum rounded apart
        v = v + c[k] * tables()[0][:, k]
    v = s * v
    order = np.argsort(v)
    return c, scale, v, int(order[-1]) - STEPS // 2, float(v[order[-1]] - v[order[-2]])


REFINE_CASES = [(kind, n, ch, q0, False, False) for kind in ("white", "pink") for n in (4097, 48000) for ch in (1, 2)
                for q0 in (-128, -115, 0, 32, 77, 127)]
REFINE_CASES += [("white", 48000, 2, 32, True, False), ("pink", 4097, 1, 77, True, False),      # inverted
                 ("white", 48000, 2, -115, False, True), ("pink", 4097, 1, 32, False, True)]    # the reference is late


@pytest.fixture(scope="module")
def refine_runs():
    """every case made once, the device run per (length, channels) in one batch, the numpy model beside it"""
    import gstpeaq_amd
    made = {}
    for i, (kind, n, ch, q0, inverted, negative) in enumerate(REFINE_CASES):
        ref = noise(kind, n, ch, 100 + i)
        d = 37 + q0 / STEPS
        if negative:                                    # lag -37: delay the reference instead, by 37 - q0 / 256
            ref, test, lag = delayed(ref, 37 - q0 / STEPS), ref, -37
        else:
            test, lag = delayed(ref, d), 37
        if inverted:
            test = -test
        made[i] = (ref.astype(np.float32), test.astype(np.float32), lag)
    got = {}
    for n in (4097, 48000):
        for ch in (1, 2):
            idx = [i for i, c in enumerate(REFINE_CASES) if c[1] == n and c[2] == ch]
            ref = np.stack([made[i][0] for i in idx])
            test = np.stack([made[i][1] for i in idx])
            lags = np.array([made[i][2] for i in idx], np.int32)
            rec = gstpeaq_amd.refine_delay(ctx(), cuda(ref), cuda(test), lags)
            # c_k of a pair is c_0 of the same pair at the lag lag + k: one more batch gives every sum
            ks = np.arange(-R, R + 1)
            every = gstpeaq_amd.refine_delay(ctx(), cuda(np.repeat(ref, len(ks), axis=0)), cuda(np.repeat(test, len(ks), axis=0)),
                                             (lags[:, None] + ks[None, :]).reshape(-1).astype(np.int32))
            for j, i in enumerate(idx):
                got[i] = ({k: rec[k][j] for k in rec}, every["c0"][j * len(ks):(j + 1) * len(ks)])
    return made, got


@pytest.mark.parametrize("case", range(len(REFINE_CASES)), ids=lambda i: "%s-%d-%dch-q%d%s%s" % (REFINE_CASES[i][:4] + (
    "-inv" if REFINE_CASES[i][4] else "", "-neg" if REFINE_CASES[i][5] else "")))
def test_refine_delay_against_numpy(refine_runs, case):
    made, got = refine_runs
    kind, n, ch, q0, inverted, negative = REFINE_CASES[case]
    ref, test, lag = made[case]
    rec, ck = got[case]
    c, scale, v, q, margin = model(ref, test, lag)
    print(REFINE_CASES[case], "numpy q", q, "device q", int(rec["q"]), "margin / max|c|", margin / np.abs(c).max())
    assert margin > 1e-9 * np.abs(c).max(), (q, margin)   # the model's own arg-max is far from a tie
    assert (np.abs(ck - c) <= CK_BOUND * scale).all(), (np.abs(ck - c) / scale).max()
    assert int(rec["q"]) == q and rec["lag"] == lag and rec["frac"] == q / STEPS
    assert rec["c0"] == ck[R]
    assert abs(rec["peak"] - v[q + STEPS // 2] * (-1.0 if c[R] < 0 else 1.0)) <= 1e-11 * np.abs(c).max()
    assert (rec["c0"] < 0) == inverted and (rec["peak"] < 0) == inverted
    assert int(rec["flags"]) == (EDGE if q in (-128, 127) else 0)
    if n == 48000:
        assert abs(q - q0) <= 1, (q, q0)
    if q0 in (-128, 127):
        assert int(rec["flags"]) == EDGE


def test_silent_empty_and_nan_pairs_are_flagged():
    import gstpeaq_amd
    rng = np.random.default_rng(7)
    n = 5000
    ref = rng.standard_normal((6, n, 2)).astype(np.float32)
    test = ref.copy()
    test[0] = 0                                         # every c_k is 0
    ref[1] = 0
    test[2, 2500, 1] = np.nan                           # a sum is not finite
    ref[3, 4999, 0] = np.inf
    n_ref = np.array([n, n, n, n, n, 0], np.uint32)
    n_test = np.array([n, n, n, n, 100, n], np.uint32)
    lags = np.array([0, 3, 0, -2, 100, 0], np.int32)    # pair 4: the lag reaches the test signal's length
    rec = gstpeaq_amd.refine_delay(ctx(), cuda(ref), cuda(test), lags, n_ref, n_test)
    assert (rec["flags"] == NONE).all(), rec["flags"]
    assert (rec["q"] == 0).all() and (rec["peak"] == 0).all() and (rec["frac"] == 0).all()
    assert (rec["lag"] == lags).all()
    far = gstpeaq_amd.refine_delay(ctx(), cuda(ref[:2]), cuda(ref[:2]), np.array([-n, 2 ** 31 - 1], np.int32))
    assert (far["flags"] == NONE).all() and (far["q"] == 0).all()


def test_record_is_the_same_alone_in_a_batch_and_on_a_second_run():
    import gstpeaq_amd
    pairs = []
    for i, (n, q0) in enumerate([(4097, 77), (48000, -115), (9000, 32), (48000, 127), (4097, -1), (20000, 5), (4096, 0), (33, 0)]):
        ref = noise("pink" if i & 1 else "white", n, 2, 300 + i)
        pairs.append((ref.astype(np.float32), delayed(ref, 37 + q0 / STEPS).astype(np.float32)))
    longest = max(len(r) for r, _ in pairs)
    ref = np.zeros((8, longest + 1, 2), np.float32)
    test = np.zeros_like(ref)
    for p, (r, t) in enumerate(pairs):
        ref[p, :len(r)], test[p, :len(t)] = r, t
    n = np.array([len(r) for r, _ in pairs], np.uint32)
    lags = np.array([37, 37, 37, 37, 37, 37, 37, 20], np.int32)
    batch = gstpeaq_amd.refine_delay(ctx(), cuda(ref), cuda(test), lags, n, n)
    again = gstpeaq_amd.refine_delay(ctx(), cuda(ref), cuda(test), lags, n, n)
    for k in batch:
        assert batch[k].tobytes() == again[k].tobytes(), k
    for p, (r, t) in enumerate(pairs):
        alone = gstpeaq_amd.refine_delay(ctx(), cuda(r[None]), cuda(t[None]), lags[p:p + 1])
        for k in batch:
            assert alone[k][0].tobytes() == batch[k][p].tobytes(), (p, k, alone[k][0], batch[k][p])


# ---- 3. the keywords equal the stages called one by one ---------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus():
    """four stereo pairs of about 1 s: delays 37.5, 12.25, 0 and -20.75 samples, the second at half the level"""
    rows = []
    for i, (d, g) in enumerate([(37.5, 1.0), (12.25, 0.5), (0.0, 1.0), (-20.75, 1.0)]):
        ref = noise("pink", 48000 + 100 * i, 2, 500 + i)
        rng = np.random.default_rng(600 + i)
        if d >= 0:
            r, t = ref, delayed(ref, d)
        else:
            r, t = delayed(ref, -d), ref
        rows.append((r.astype(np.float32), (g * t + 1e-4 * rng.standard_normal(t.shape)).astype(np.float32)))
    longest = max(len(r) for r, _ in rows)
    ref = np.zeros((len(rows), longest, 2), np.float32)
    test = np.zeros_like(ref)
    for p, (r, t) in enumerate(rows):
        ref[p, :len(r)], test[p, :len(t)] = r, t
    n = np.array([len(r) for r, _ in rows], np.uint32)
    return rows, ref, test, n


@pytest.mark.parametrize("advanced", [0, 1], ids=["basic", "advanced"])
@pytest.mark.parametrize("gain", [None, "lsq"])
def test_batch_keyword_is_the_stages_one_by_one(corpus, advanced, gain):
    import gstpeaq_amd
    rows, ref, test, n = corpus
    d_ref, d_test = cuda(ref), cuda(test)
    kw = {} if gain is None else dict(gain=gain)
    got = gstpeaq_amd.batch_run(ctx(), advanced, d_ref, d_test, n, n, align=4096, subsample=True, **kw)
    lags = gstpeaq_amd.estimate_delay(ctx(), d_ref, d_test, 4096, n, n)["lag"]
    sub = gstpeaq_amd.refine_delay(ctx(), d_ref, d_test, lags, n, n)
    assert list(lags) == [38, 12, 0, -21] or list(lags) == [37, 12, 0, -21], lags
    cuts = np.array([gstpeaq_amd.aligned_lengths(int(lags[p]), int(n[p]), int(n[p])) for p in range(len(n))], np.uint32)
    a = gstpeaq_amd.cut(ctx(), d_ref, cuts[:, 0], cuts[:, 2])
    b = gstpeaq_amd.cut_shifted(ctx(), d_test, cuts[:, 1], cuts[:, 2], sub["q"], n_in=n)
    if gain is not None:
        rec, read = gstpeaq_amd.measure_gain(ctx(), a, b, gain, n=cuts[:, 2])
        b = gstpeaq_amd.cut_scaled(ctx(), b, np.zeros(len(n), np.uint32), cuts[:, 2], rec)
    want = gstpeaq_amd.batch_run(ctx(), advanced, a, b, cuts[:, 2], cuts[:, 2])
    for p in range(len(n)):
        assert same_result(got[p], want[p]), (p, got[p], want[p])
    last = gstpeaq_amd.align.last_subdelay
    assert (last["q"] == sub["q"]).all() and (last["lag"] == lags).all()
    # the other batch entry points take the keyword through the same path
    pts, res = gstpeaq_amd.batch_trajectory(ctx(), advanced, d_ref, d_test, 24000, 2, n, n, align=4096, subsample=True, **kw)
    tr = gstpeaq_amd.batch_trace(ctx(), advanced, d_ref, d_test, n, n, align=4096, subsample=True, **kw)
    for p in range(len(n)):
        assert same_result(res[p], want[p]) and same_result(tr["results"][p], want[p]), p


@pytest.mark.parametrize("advanced", [0, 1], ids=["basic", "advanced"])
def test_subsample_false_is_todays_result(corpus, advanced):
    import gstpeaq_amd
    rows, ref, test, n = corpus
    d_ref, d_test = cuda(ref), cuda(test)
    for kw in (dict(), dict(align=4096), dict(align=4096, gain="lsq"), dict(gain="rms")):
        a = gstpeaq_amd.batch_run(ctx(), advanced, d_ref, d_test, n, n, **kw)
        b = gstpeaq_amd.batch_run(ctx(), advanced, d_ref, d_test, n, n, subsample=False, **kw)
        assert all(same_result(x, y) for x, y in zip(a, b)), kw
    with pytest.raises(gstpeaq_amd.PeaqError, match="requires align="):
        gstpeaq_amd.batch_run(ctx(), advanced, d_ref, d_test, n, n, subsample=True)


@pytest.mark.parametrize("gain", [None, "lsq"])
def test_run_pair_and_the_cli_agree_with_the_batch_keyword(corpus, gain, tmp_path):
    import gstpeaq_amd
    import gst_env
    rows, ref, test, n = corpus
    kw = {} if gain is None else dict(gain=gain)
    want = gstpeaq_amd.batch_run(ctx(), 0, cuda(ref), cuda(test), n, n, align=4096, subsample=True, **kw)
    sub = gstpeaq_amd.align.last_subdelay
    for p, (r, t) in enumerate(rows[:2]):
        got = gstpeaq_amd.run_pair(ctx(), 0, r, t, align=4096, subsample=True, **kw)
        assert same_result(got, want[p]), (p, got, want[p])
        assert got["subdelay"]["q"] == sub["q"][p] and got["subdelay"]["lag"] == sub["lag"][p]
        assert got["subdelay"]["peak"] == sub["peak"][p] and got["subdelay"]["flags"] == sub["flags"][p]
    if gain is None and gst_env.CLI.exists():
        # 32-bit float files hand the CLI the samples as they are
        r, t = rows[0]
        write_wav(tmp_path / "r.wav", r)
        write_wav(tmp_path / "t.wav", t)
        run = subprocess.run([str(gst_env.CLI), "--align-subsample=4096", str(tmp_path / "r.wav"), str(tmp_path / "t.wav")],
                             capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stdout + run.stderr
        lines = run.stdout.strip().splitlines()
        assert lines[0].startswith("Delay: %d %+.4f samples" % (sub["lag"][0], sub["frac"][0])), run.stdout
        assert lines[1] == "Objective Difference Grade: %.3f" % want[0]["odg"], run.stdout
        assert lines[2] == "Distortion Index: %.3f" % want[0]["di"], run.stdout
        (tmp_path / "list.txt").write_text("%s\t%s\n" % (tmp_path / "r.wav", tmp_path / "t.wav"))
        refused = subprocess.run([str(gst_env.CLI), "--align-subsample", "--list=%s" % (tmp_path / "list.txt")],
                                 capture_output=True, text=True, timeout=300)
        assert refused.returncode == 1 and "host-fed path does not take it yet" in refused.stderr, refused.stderr


def write_wav(path, x, rate=48000):
    """x [n, channels] as a 32-bit float RIFF/WAVE file"""
    import struct
    from pathlib import Path
    x = np.asarray(x)
    ch = x.shape[1]
    body = x.astype("<f4").tobytes()
    fmt = struct.pack("<HHIIHH", 3, ch, rate, rate * ch * 4, ch * 4, 32)
    chunks = b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(body)) + body
    Path(path).write_bytes(b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks)


# ---- 4. it does what it is for -----------------------------------------------------------------------------------------
PURPOSE_DELAY, PURPOSE_SNR_DB = 37.5, 80.0
# ODGs of the CPU oracle (tests/oracle_lib.py, advanced version) for purpose_pair(): undelayed, integer-aligned (lag 38),
# corrected by the numpy model of this file (model: q = -128; shifted_model)
PURPOSE_ORACLE = (0.195, -0.456, 0.195)


def purpose_pair():
    """stereo, 2 s: 200 clicks of 0.5 on digital silence; the test signal late by 37.5 samples, hiss 80 dB below the
    reference's rms.  (ref, test, undelayed): undelayed is the reference with the same hiss and no delay"""
    rng = np.random.default_rng(4)
    ref = np.zeros((96000, 2))
    ref[rng.integers(100, 96000 - 100, 200)] = 0.5
    hiss = ref.std() * 10 ** (-PURPOSE_SNR_DB / 20) * np.random.default_rng(9).standard_normal(ref.shape)
    return ref.astype(np.float32), (delayed(ref, PURPOSE_DELAY) + hiss).astype(np.float32), (ref + hiss).astype(np.float32)


def test_a_half_sample_delay_scores_as_the_undelayed_pair():
    """The oracle's three ODGs for the pair are PURPOSE_ORACLE: 0.195 undelayed, -0.456 integer-aligned, 0.195 corrected by
    the numpy model; the integer-aligned pair lies 0.65 below the undelayed one.  Chosen on the CPU with the oracle:
    PEAQ compares magnitude spectra of 2048-sample frames (FFT ear model) and envelopes (filter bank), which half a
    sample of delay hardly changes in a dense signal -- band-limited white or pink noise, tones and square waves lose
    0.00 to 0.06 ODG in either version -- but a click spread over its neighbours by the residue shows against silence in
    the advanced version's filter bank (clicks on a floor 74 dB down: 0.10; on silence, this pair: 0.65)."""
    import gstpeaq_amd
    und_odg, int_odg, fix_odg = PURPOSE_ORACLE
    assert int_odg <= und_odg - 0.5, PURPOSE_ORACLE
    ref, test, undelayed = purpose_pair()
    odg_und = gstpeaq_amd.run_pair(ctx(), 1, ref, undelayed)["odg"]
    odg_int = gstpeaq_amd.run_pair(ctx(), 1, ref, test, align=4096)["odg"]
    got = gstpeaq_amd.run_pair(ctx(), 1, ref, test, align=4096, subsample=True)
    print("device ODG: undelayed", odg_und, "integer", odg_int, "subsample", got["odg"], got["delay"], got["subdelay"])
    assert got["odg"] > odg_int
    assert abs(got["odg"] - odg_und) < abs(odg_int - odg_und)


def test_the_lsq_gain_is_unbiased_after_the_shift():
    """test = 0.5 x the reference delayed by 37.5 samples: measured after the shift the gain is 2 within 1 %; measured on
    the integer-aligned signals it is low by sinc (0.5) averaged over the spectrum, which the numpy model shows first"""
    import gstpeaq_amd
    ref = noise("white", 48000, 2, 21)
    test = (0.5 * delayed(ref, PURPOSE_DELAY)).astype(np.float32)
    ref = ref.astype(np.float32)
    with_shift = gstpeaq_amd.run_pair(ctx(), 0, ref, test, align=4096, gain="lsq", subsample=True)
    assert abs(with_shift["gain"]["gain"][0] - 2.0) < 0.02, with_shift["gain"]
    without = gstpeaq_amd.run_pair(ctx(), 0, ref, test, align=4096, gain="lsq")
    lag = without["delay"]["lag"]
    r, t = ref.astype(np.float64), test.astype(np.float64)
    m = len(r) - lag
    numpy_gain = (r[:m] * t[lag:lag + m]).sum() / (t[lag:lag + m] ** 2).sum()
    print("gain after the shift", with_shift["gain"]["gain"], "without", without["gain"]["gain"], "numpy", numpy_gain)
    if abs(numpy_gain - 2.0) > 0.2:
        assert abs(without["gain"]["gain"][0] - 2.0) > 0.2, without["gain"]



"""Scores of time windows inside each pair (peaq_batch_run_windows, include/peaq_amd.h): a window's
reading is the read-out of accumulators that start fresh before the window's first frame and are given what the pair's
own accumulators are given in the window's frames -- a view into the running stream.  Pinned here
  * bit for bit against the trajectory's points (windows {0, L < m}) and the end result (windows {0, L >= m}),
  * for windows in mid-stream against a NumPy restatement of the accumulator rules (movaccum.c: add, tentative / saved,
    read-out) fed the run's own per-frame values -- batch_trace's records and debug_frontend's scalars --, a model that
    is first held against the shipped path on the whole pair,
  * across the batch path's launch boundaries, for the one-pair entry, for leakage into a later batch, and for the CLI.
Needs an MI355X (`-m gpu`).

Tolerance of the model comparison: model and device do the same FP64 operations in the same order and differ by at most
one rounding per accumulated term (the device fuses multiply-adds) plus a few at the read-out (sqrt, log10, the fast
division in the NMR).  All accumulated terms are non-negative; with under 120 frames per window that is below
120 * 2^-52, about 3e-14 relative: the MOVs are held to rtol = 1e-13, DI and ODG (through the network) to 1e-10."""
import math
import subprocess

import numpy as np
import pytest

import cases as case_defs
import gst_env
from test_conformance_runner import write_wav

pytestmark = pytest.mark.gpu

CASE_NAMES = ("gap1_mono", "gap3_stereo", "synth_quiet_60dB", "synth_quiet_36dB", "synth_s0_stereo",
              "synth_ragged_test_short")
MOV_RTOL, DI_ATOL = 1e-13, 1e-10
ABOVE, MOD_OPEN, LOUD_OPEN = 1, 2, 4
# the front end's scalars in debug_frontend's record (PEAQ_DEBUG_RECORD_DOUBLES = 576: five band vectors of 112, then)
S_BW_REF, S_BW_TEST, S_EHS, S_FLAGS_REF, S_FLAGS_TEST, S_SIG_E, S_NOISE_E = range(560, 567)
(BW_REF, BW_TEST, NMR, WINMOD, ADB, EHS, AVGMOD1, AVGMOD2, NOISELOUD, MFPD, RELDIST) = range(11)
AVG, AVG_LOG, RMS, AVG_WINDOW, FILTERED_MAX, ADB_MODE = range(6)
MODE = {NMR: AVG_LOG, WINMOD: AVG_WINDOW, ADB: ADB_MODE, NOISELOUD: RMS, MFPD: FILTERED_MAX}


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback in the product)")
    import gpu_common
    return gpu_common


def cases():
    by_name = {c["name"]: c for c in case_defs.e2e_cases() if c["advanced"] == 0}
    return [by_name[n] for n in CASE_NAMES]


def F(a):
    return (a - 2048) // 1024 + 1 if a >= 2048 else 0


def window_frames(n_ref, n_test, start, length):
    """the rule of include/peaq_amd.h, restated"""
    import gstpeaq_amd
    n, m, total = min(n_ref, n_test), max(n_ref, n_test), gstpeaq_amd.frame_count(n_ref, n_test)
    e = start + length
    first = total if start >= m else F(min(start, n))
    end = total if e >= m else F(min(e, n))
    return first, end - first


def to_device(inputs):
    import torch
    ch = inputs[0][0].shape[1]
    stride = max(max(len(r), len(t)) for r, t in inputs)
    stride += stride & 1
    ref = np.zeros((len(inputs), stride, ch), dtype=np.float32)
    test = np.zeros_like(ref)
    n_ref = np.array([len(r) for r, _ in inputs], dtype=np.uint32)
    n_test = np.array([len(t) for _, t in inputs], dtype=np.uint32)
    for i, (r, t) in enumerate(inputs):
        ref[i, :len(r)] = r
        test[i, :len(t)] = t
    return torch.from_numpy(ref).cuda(), torch.from_numpy(test).cuda(), n_ref, n_test


_PAIR = {}


def pair_data(gpu, case):
    """one pair's inputs on the device, its plain result, its trace and its front-end scalars: made once per case"""
    import gstpeaq_amd
    import torch
    name = case["name"]
    if name not in _PAIR:
        r, t = case_defs.make_inputs(case)
        ref, test, n_ref, n_test = to_device([(r, t)])
        ctx = gpu.ctx()
        plain = gstpeaq_amd.batch_run(ctx, 0, ref, test, n_ref, n_test, sync=False)
        torch.cuda.synchronize()
        trace = gstpeaq_amd.batch_trace(ctx, 0, ref, test, n_ref, n_test)
        total = int(trace["n_frames"][0])
        assert total == gstpeaq_amd.frame_count(len(r), len(t))
        fe = gstpeaq_amd.debug_frontend(ctx, 109, torch.from_numpy(r).cuda(), torch.from_numpy(t).cuda(), total)
        _PAIR[name] = dict(r=r, t=t, ref=ref, test=test, n_ref=n_ref, n_test=n_test, plain_bytes=plain.cpu().numpy().tobytes(),
                           plain=gstpeaq_amd.capi._result_dict(plain.cpu().numpy()[0], False),
                           frames=trace["frames"][0][:total], scalars=fe[:, :, 560:567], total=total)
    return _PAIR[name]


# ---- the model: movaccum.c's rules on Python floats ---------------------------------------------------------------
class Acc:
    def __init__(self, mode):
        self.mode, self.status = mode, "init"
        self.num = self.den = self.num2 = self.mx = self.filt = 0.
        self.past = [math.nan] * 3
        self.saved = (0., 0., 0., 0.)

    def set_tentative(self, tentative):            # movaccum.c:317-362
        if tentative:
            if self.status == "normal":
                self.saved = (self.num, self.den, self.num2, self.mx)
                self.status = "tentative"
        else:
            self.status = "normal"

    def add(self, v, w):                           # movaccum.c:368-425
        if self.status == "init":
            return
        if self.mode == RMS:
            w *= w
            self.num += w * v * v
            self.den += w
        elif self.mode in (AVG, AVG_LOG, ADB_MODE):
            self.num += w * v
            self.den += w
        elif self.mode == AVG_WINDOW:
            sq = math.sqrt(v) if v >= 0 else math.nan
            if not math.isnan(self.past[0]):
                ws = (((sq + self.past[0]) + self.past[1]) + self.past[2]) / 4.
                ws *= ws
                ws *= ws
                self.num += ws
                self.den += 1.
            self.past = [self.past[1], self.past[2], sq]
        else:
            self.filt = 0.9 * self.filt + 0.1 * v
            if self.filt > self.mx:
                self.mx = self.filt

    def value(self):                               # movaccum.c:448-477, one channel's term
        num, den, num2, mx = self.saved if self.status == "tentative" else (self.num, self.den, self.num2, self.mx)
        div = lambda a, b: a / b if b != 0 else (math.nan if a == 0 or math.isnan(a) else math.copysign(math.inf, a))
        if self.mode == AVG:
            return div(num, den)
        if self.mode == AVG_LOG:
            q = div(num, den)
            return 10. * math.log10(q) if q > 0 else (-math.inf if q == 0 else math.nan)
        if self.mode in (AVG_WINDOW, RMS):
            q = div(num, den)
            return math.sqrt(q) if q >= 0 else math.nan
        if self.mode == FILTERED_MAX:
            return mx
        return (-0.5 if num == 0. else math.log10(num / den)) if den > 0 else 0.


# nn.c:187-216 (basic version, the tables of BS.1387)
AMIN = [393.916656, 361.965332, -24.045116, 1.110661, -0.206623, 0.074318, 1.113683, 0.950345, 0.029985, 0.000101, 0.]
AMAX = [921, 881.131226, 16.212030, 107.137772, 2.886017, 13.933351, 63.257874, 1145.018555, 14.819740, 1., 1.]
WX = [[-0.502657, 0.436333, 1.219602], [4.307481, 3.246017, 1.123743], [4.984241, -2.211189, -0.192096],
      [0.051056, -1.762424, 4.331315], [2.321580, 1.789971, -0.754560], [-5.303901, -3.452257, -10.814982],
      [2.730991, -6.111805, 1.519223], [0.624950, -1.331523, -5.955151], [3.102889, 0.871260, -5.922878],
      [-1.051468, -0.939882, -0.142913], [-1.804679, -0.503610, -0.620456]]
WXB, WY = [-2.518254, 0.654841, -2.207228], [-3.817048, 4.107138, 4.629582]


def sigmoid(x):
    try:
        return 1. / (1. + math.exp(-x))
    except OverflowError:
        return 0.


def network(movs):
    x = list(WXB)
    for i in range(11):
        m = (movs[i] - AMIN[i]) / (AMAX[i] - AMIN[i])
        for j in range(3):
            x[j] += WX[i][j] * m
    di = -0.307594
    for j in range(3):
        di += WY[j] * sigmoid(x[j])
    return di, -3.98 + (0.22 - -3.98) * sigmoid(di)


def model(frames, scalars, channels, first, count):
    """the reading of frames [first, first + count): the routing of peaq_backend_fft.inc:362-502 into fresh accumulators"""
    accs = [[Acc(MODE.get(i, AVG)) for i in range(11)] for _ in range(channels)]
    sig = noise = 0.
    for f in range(first, first + count):
        tr, sc = frames[f], scalars[f]
        flags = int(tr["flags"])
        energy = any((int(sc[c][S_FLAGS_REF - 560]) | int(sc[c][S_FLAGS_TEST - 560])) & 2 for c in range(channels))
        for c in range(channels):
            for a in accs[c]:
                a.set_tentative(not flags & ABOVE)
            v, a = tr["ch"][c], accs[c]
            if flags & MOD_OPEN:
                a[AVGMOD1].add(float(v[0]), float(v[2]))
                a[AVGMOD2].add(float(v[1]), float(v[2]))
                a[WINMOD].add(float(v[0]), 1.)
            if flags & LOUD_OPEN:
                a[NOISELOUD].add(float(v[3]), 1.)
            a[NMR].add(float(v[4]), 1.)
            a[RELDIST].add(1. if v[5] > 1.41253754462275 else 0., 1.)
            if c == 0:
                if tr["p_detect"] > 0.5:
                    a[ADB].add(float(tr["steps"]), 1.)
                a[MFPD].add(float(tr["p_detect"]), 1.)
            if sc[c][S_BW_REF - 560] > 346.:
                a[BW_REF].add(float(sc[c][S_BW_REF - 560]), 1.)
                a[BW_TEST].add(float(sc[c][S_BW_TEST - 560]), 1.)
            if energy:
                a[EHS].add(1000. * float(sc[c][S_EHS - 560]), 1.)
        sig += float(sum(sc[c][S_SIG_E - 560] for c in range(channels)))
        noise += float(sum(sc[c][S_NOISE_E - 560] for c in range(channels)))
    movs = []
    for i in range(11):
        nch = 1 if i in (ADB, MFPD) else channels
        movs.append(sum(accs[c][i].value() for c in range(nch)) / nch)
    di, odg = network(movs)
    with np.errstate(divide="ignore", invalid="ignore"):
        snr = float(10 * np.log10(np.float64(sig) / np.float64(noise)))
    return dict(movs=np.array(movs), di=di, odg=odg, totalsnr=snr, frames=count)


def assert_reading(got, exp, where):
    print(where, "movs", got["movs"], exp["movs"], "di", got["di"], exp["di"], "odg", got["odg"], exp["odg"],
          "snr", got["totalsnr"], exp["totalsnr"])
    assert got["frames"] == exp["frames"] and got["fb_blocks"] == 0, (where, got["frames"], exp["frames"])
    assert np.array_equal(np.isnan(got["movs"]), np.isnan(exp["movs"])), (where, got["movs"], exp["movs"])
    ok = ~np.isnan(exp["movs"])
    np.testing.assert_allclose(got["movs"][ok], exp["movs"][ok], rtol=MOV_RTOL, atol=0, err_msg=str(where))
    for k in ("di", "odg"):
        assert math.isnan(got[k]) == math.isnan(exp[k]), (where, k, got[k], exp[k])
        assert math.isnan(exp[k]) or abs(got[k] - exp[k]) <= DI_ATOL, (where, k, got[k], exp[k])
    g, e = got["totalsnr"], exp["totalsnr"]
    assert (math.isnan(g) and math.isnan(e)) or g == e or abs(g - e) <= MOV_RTOL * abs(e), (where, g, e)


def raw(result_rows):
    return np.ascontiguousarray(result_rows.cpu().numpy())


# ---- 1, 2: identity with the trajectory and with the end result ------------------------------------------------------
@pytest.mark.parametrize("interval", (1000, 3072, 48000))
def test_windows_from_zero_are_the_trajectory_points(gpu, interval):
    import gstpeaq_amd
    import torch
    seen = 0
    for case in cases():
        d = pair_data(gpu, case)
        m = max(len(d["r"]), len(d["t"]))
        n_points = -(-m // interval)
        lengths = [(k + 1) * interval for k in range(n_points)]
        windows = [(0, L) for L in lengths]
        pts, _ = gstpeaq_amd.batch_trajectory(gpu.ctx(), 0, d["ref"], d["test"], interval, n_points, d["n_ref"], d["n_test"],
                                              sync=False)
        win, res = gstpeaq_amd.batch_windows(gpu.ctx(), d["ref"], d["test"], windows, d["n_ref"], d["n_test"], sync=False)
        torch.cuda.synchronize()
        pts, win = raw(pts)[0], raw(win)[0]
        assert raw(res).tobytes() == d["plain_bytes"], case["name"]
        for k, L in enumerate(lengths):
            if L < m:
                assert win[k].tobytes() == pts[k].tobytes(), (case["name"], interval, k, win[k], pts[k])
                assert win[k][14] == F(min(L, len(d["r"]), len(d["t"])))
                seen += 1
            else:                                      # reaches the end of the longer signal: the flushed end result
                assert win[k].tobytes() == d["plain_bytes"], (case["name"], interval, k)
    assert seen > 6


def test_a_window_over_the_whole_pair_is_the_end_result_and_that_is_batch_runs(gpu):
    import gstpeaq_amd
    import torch
    for case in cases():
        d = pair_data(gpu, case)
        m = max(len(d["r"]), len(d["t"]))
        windows = [(0, m), (0, m + 1), (0, 0xFFFFFFFF)]
        win, res = gstpeaq_amd.batch_windows(gpu.ctx(), d["ref"], d["test"], windows, d["n_ref"], d["n_test"], sync=False)
        torch.cuda.synchronize()
        assert raw(res).tobytes() == d["plain_bytes"], case["name"]
        for k in range(len(windows)):
            assert raw(win)[0][k].tobytes() == d["plain_bytes"], (case["name"], k)
        assert raw(win)[0][0][14] == d["total"]


# ---- 3: windows in mid-stream against the model -------------------------------------------------------------------
def test_the_model_reproduces_the_shipped_path_on_whole_pairs(gpu):
    for case in cases():
        d = pair_data(gpu, case)
        exp = model(d["frames"], d["scalars"], d["r"].shape[1], 0, d["total"])
        assert_reading(d["plain"], exp, (case["name"], "whole pair"))


def test_mid_stream_windows_match_the_model(gpu):
    import gstpeaq_amd
    empty_or_nan = begins_in_gap = ends_in_gap = compared = 0
    for case in cases():
        d = pair_data(gpu, case)
        n_ref, n_test, channels = len(d["r"]), len(d["t"]), d["r"].shape[1]
        m = max(n_ref, n_test)
        windows = np.concatenate([gstpeaq_amd.sliding_windows(m, L, hop)
                                  for L, hop in ((24000, 12000), (48000, 4096), (3000, 1000))])
        win, res = gstpeaq_amd.batch_windows(gpu.ctx(), d["ref"], d["test"], windows, d["n_ref"], d["n_test"])
        assert len(win[0]) == len(windows)
        above = d["frames"]["flags"] & ABOVE
        for k, (start, length) in enumerate(windows.tolist()):
            first, count = window_frames(n_ref, n_test, start, length)
            assert (first, count) == gstpeaq_amd.window_frames(n_ref, n_test, start, length)
            assert count < 120
            exp = model(d["frames"], d["scalars"], channels, first, count)
            got = win[0][k]
            assert_reading(got, exp, (case["name"], k, start, length, first, count))
            compared += 1
            empty_or_nan += bool(count == 0 or np.isnan(got["movs"]).any())
            # a gap: frames below the data boundary after the pair's first frame above it
            if count and above[:first].any():
                begins_in_gap += not above[first]
                ends_in_gap += not above[first + count - 1]
    print("compared", compared, "empty or NaN", empty_or_nan, "begin in a gap", begins_in_gap, "end in a gap", ends_in_gap)
    assert empty_or_nan >= 1 and begins_in_gap >= 1 and ends_in_gap >= 1


# ---- 4: launch seams -------------------------------------------------------------------------------------------------
def test_windows_across_launch_boundaries(gpu):
    """128 stereo pairs of 10 s: the batch path cuts them into 8 launches of 64 frames, a one-pair batch is one launch"""
    import gstpeaq_amd
    import torch
    ctx = gpu.ctx()
    n, pairs = 480000, 128
    ref, test = gstpeaq_amd.synth_fill(ctx, 700, pairs, 2, n)
    windows = np.concatenate([gstpeaq_amd.sliding_windows(n, 96000, 48000),
                              np.array([[65000, 1500], [0, n]], dtype=np.uint32)])
    d_win, d_res = gstpeaq_amd.batch_windows(ctx, ref, test, windows, sync=False)
    tm = ctx.last_timing()
    assert tm["frontend_launches"] > 1, tm
    torch.cuda.synchronize()
    whole = gstpeaq_amd.batch_run(ctx, 0, ref, test, sync=False)
    torch.cuda.synchronize()
    win, res, whole = raw(d_win), raw(d_res), raw(whole)
    assert res.tobytes() == whole.tobytes()
    assert win[:, -1].tobytes() == whole.tobytes()
    for p in (0, 37, 64, 127):
        one, one_res = gstpeaq_amd.batch_windows(ctx, ref[p:p + 1], test[p:p + 1], windows, sync=False)
        assert ctx.last_timing()["frontend_launches"] == 1
        torch.cuda.synchronize()
        assert raw(one)[0].tobytes() == win[p].tobytes(), (p, raw(one)[0], win[p])
        assert raw(one_res)[0].tobytes() == res[p].tobytes()
    for k, (start, length) in enumerate(windows.tolist()):
        assert (win[:, k, 14] == gstpeaq_amd.window_frames(n, n, start, length)[1]).all()


# ---- 5: the one-pair entry; nothing of a windows run is left in the context -------------------------------------
def test_host_memory_entry_equals_the_batch_entry(gpu):
    import gstpeaq_amd
    case = dict(kind="synth", seed=21, channels=2, n=100000, test_trim=1500)
    r, t = case_defs.make_inputs(case)
    windows = gstpeaq_amd.sliding_windows(100000, 24000, 12000)
    got = gstpeaq_amd.run_pair_windows(gpu.ctx(), r, t, windows)
    ref, test, n_ref, n_test = to_device([(r, t)])
    win, res = gstpeaq_amd.batch_windows(gpu.ctx(), ref, test, windows, n_ref, n_test)
    assert len(got["windows"]) == len(windows)
    for k in range(len(windows)):
        for key in ("movs", "di", "odg", "totalsnr", "frames", "fb_blocks"):
            np.testing.assert_array_equal(got["windows"][k][key], win[0][k][key], err_msg=f"{k} {key}")
    for key in ("movs", "di", "odg", "totalsnr", "frames", "fb_blocks"):
        np.testing.assert_array_equal(got["result"][key], res[0][key])


def test_no_leakage_into_a_later_batch(gpu):
    """a batch_run after a windows run on the same context returns the bytes it returns on a fresh context"""
    import gstpeaq_amd
    import torch
    inputs = [case_defs.make_inputs(c) for c in cases() if c["channels"] == 2]
    ref, test, n_ref, n_test = to_device(inputs)
    ctx = gpu.ctx()
    gstpeaq_amd.batch_windows(ctx, ref, test, gstpeaq_amd.sliding_windows(120000, 24000, 12000), n_ref, n_test)
    after = gstpeaq_amd.batch_run(ctx, 0, ref, test, n_ref, n_test, sync=False)
    fresh_ctx = gstpeaq_amd.Context(0)
    fresh = gstpeaq_amd.batch_run(fresh_ctx, 0, ref, test, n_ref, n_test, sync=False)
    torch.cuda.synchronize()
    assert after.cpu().numpy().tobytes() == fresh.cpu().numpy().tobytes()
    fresh_ctx.close()


# ---- 6: the CLI --------------------------------------------------------------------------------------------------------
def test_cli_windows(gpu, tmp_path):
    import gstpeaq_amd
    r, t = case_defs.make_inputs(dict(kind="synth", seed=22, channels=1, n=100000, ref_trim=700))
    write_wav(tmp_path / "ref.wav", r, bits=32, fmt_float=True)
    write_wav(tmp_path / "test.wav", t, bits=32, fmt_float=True)
    plain = subprocess.run([str(gst_env.CLI), tmp_path / "ref.wav", tmp_path / "test.wav"],
                           capture_output=True, text=True, timeout=300)
    out = subprocess.run([str(gst_env.CLI), "--windows=1:0.5", tmp_path / "ref.wav", tmp_path / "test.wav"],
                         capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and out.returncode == 0, (plain.stderr, out.stderr, out.stdout)
    lines = out.stdout.strip().splitlines()
    windows = gstpeaq_amd.sliding_windows(max(len(r), len(t)), 48000, 24000)
    exp = gstpeaq_amd.run_pair_windows(gpu.ctx(), r, t, windows)["windows"]
    assert len(lines) == len(windows) + 2, out.stdout
    assert lines[-2:] == plain.stdout.strip().splitlines()[-2:]
    for k, line in enumerate(lines[:-2]):
        word = line.split()
        assert word[0] == "window" and len(word) == 6, line
        start, length = windows[k].tolist()
        want = "%.3f %.3f %.0f %.3f %.3f" % (start / 48000., (start + length) / 48000., exp[k]["frames"], exp[k]["odg"],
                                             exp[k]["di"])
        got, want = [float(x) for x in word[1:]], [float(x) for x in want.split()]
        assert all(g == w or (math.isnan(g) and math.isnan(w)) for g, w in zip(got, want)), (k, line, want)
    assert any("nan" not in line for line in lines[:-2])

"""Scores of time spans inside each pair in the advanced version (peaq_batch_run_adv_spans, include/peaq_amd.h; DESIGN.md
28): a span's reading is the read-out of the five accumulators that start fresh before the span's first FFT frame /
filter-bank block and are given what the pair's own accumulators are given in the span's frames and blocks -- a view into
the running stream.  Pinned here, on the default (FP64) engine,
  * bit for bit against the advanced trajectory's points (spans {0, L < m}) and the end result (spans {0, L >= m}),
  * for spans in mid-stream against a NumPy restatement of the accumulator rules (movaccum.c: add, tentative / saved,
    read-out; tests/test_gpu_windows.py's Acc with RMS_ASYM added) fed the run's own per-frame and per-block values --
    batch_trace's records and debug_frontend's scalars --, a model that is first held against the shipped path on the
    whole pair,
  * across the launch boundaries of both paths, for the one-pair entry, for leakage into a later batch, and for the CLI.
Needs an MI355X (`-m gpu`).

Tolerance of the model comparison: model and device do the same FP64 operations in the same order and differ by at most
one rounding per accumulated term (the device fuses multiply-adds) plus a few at the read-out.  A span has at most 250
blocks and 47 frames: 250 * 2^-52 < 6e-14.  The MOVs whose terms are all non-negative are held to rtol = 1e-13.
SegmentalNMR sums signed dB values: it is held to 1e-13 * (sum |v| / den), which the model computes alongside.  DI and
ODG are held to 1e-10, and every compared reading asserts that this covers the network's sensitivity to MOV errors of
that size: sum_j |wy_j| / 4 * sum_i |wx_ij| * err_i / (amax_i - amin_i) (a sigmoid's slope is at most 1 / 4), times
(0.22 + 3.98) / 4 for the ODG."""
import math
import subprocess

import numpy as np
import pytest

import cases as case_defs
import gst_env
from test_conformance_runner import write_wav
from test_gpu_windows import AVG, RMS, Acc, F, raw, sigmoid, to_device, window_frames

pytestmark = pytest.mark.gpu

CASE_NAMES = ("gap1_mono", "gap3_stereo", "synth_quiet_60dB", "synth_quiet_36dB", "synth_s0_stereo",
              "synth_ragged_test_short")
MOV_RTOL, DI_ATOL = 1e-13, 1e-10
ABOVE, MOD_OPEN, LOUD_OPEN = 1, 2, 4
# the front end's scalars in debug_frontend's record (PEAQ_DEBUG_RECORD_DOUBLES = 576: five band vectors of 112, then)
S_EHS, S_FLAGS_REF, S_FLAGS_TEST, S_SIG_E, S_NOISE_E = 562, 563, 564, 565, 566
RMSMOD, NLASYM, SEGNMR, EHS, LINDIST = range(5)            # the order of the advanced version's MOVs
RMS_ASYM = 1000                                            # (a mode tests/test_gpu_windows.py's Acc does not have)
MODE = {RMSMOD: RMS, NLASYM: RMS_ASYM, SEGNMR: AVG, EHS: AVG, LINDIST: AVG}
KEYS = ("movs", "di", "odg", "totalsnr", "frames", "fb_blocks")


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback in the product)")
    import gpu_common
    return gpu_common


def cases():
    by_name = {c["name"]: c for c in case_defs.e2e_cases() if c["advanced"] == 1}
    return [by_name[n] for n in CASE_NAMES]


def B(a):
    return a // 192


def span_blocks(n_ref, n_test, start, length):
    """the block rule of include/peaq_amd.h, restated"""
    import gstpeaq_amd
    n, m, total = min(n_ref, n_test), max(n_ref, n_test), gstpeaq_amd.frame_count(n_ref, n_test, True)
    e = start + length
    first = total if start >= m else B(min(start, n))
    end = total if e >= m else B(min(e, n))
    return first, end - first


_PAIR = {}


def pair_data(gpu, case):
    """one pair's inputs on the device, its plain result, its two traces and its front-end scalars: made once per case"""
    import gstpeaq_amd
    import torch
    name = case["name"]
    if name not in _PAIR:
        r, t = case_defs.make_inputs(case)
        ref, test, n_ref, n_test = to_device([(r, t)])
        ctx = gpu.ctx("default")
        plain = gstpeaq_amd.batch_run(ctx, 1, ref, test, n_ref, n_test, sync=False)
        torch.cuda.synchronize()
        trace = gstpeaq_amd.batch_trace(ctx, 1, ref, test, n_ref, n_test)
        total, total_b = int(trace["n_frames"][0]), int(trace["n_blocks"][0])
        assert total == gstpeaq_amd.frame_count(len(r), len(t))
        assert total_b == gstpeaq_amd.frame_count(len(r), len(t), True)
        fe = gstpeaq_amd.debug_frontend(ctx, 55, torch.from_numpy(r).cuda(), torch.from_numpy(t).cuda(), total)
        _PAIR[name] = dict(r=r, t=t, ref=ref, test=test, n_ref=n_ref, n_test=n_test, plain_bytes=plain.cpu().numpy().tobytes(),
                           plain=gstpeaq_amd.capi._result_dict(plain.cpu().numpy()[0], True),
                           frames=trace["frames"][0][:total], blocks=trace["blocks"][0][:total_b], scalars=fe,
                           total=total, total_b=total_b)
    return _PAIR[name]


# ---- the model: movaccum.c's rules on Python floats, with the mode the advanced version adds ----------------------
class AdvAcc(Acc):
    def add(self, v, w):                           # movaccum.c:368-425
        if self.mode != RMS_ASYM:
            return Acc.add(self, v, w)
        if self.status != "init":
            self.num += v * v
            self.num2 += w * w
            self.den += 1.

    def value(self):                               # movaccum.c:448-477, one channel's term
        if self.mode != RMS_ASYM:
            return Acc.value(self)
        num, den, num2, _ = self.saved if self.status == "tentative" else (self.num, self.den, self.num2, self.mx)
        if den == 0:
            return math.nan if num == 0 and num2 == 0 else math.inf
        return math.sqrt(num / den) + 0.5 * math.sqrt(num2 / den)


# the advanced version's network as this project's read-out has it (finalize_state and the na_* tables of
# gstpeaq_amd/csrc/peaq_backend.hip)
AMIN = [13.298751, 0.041073, -25.018791, 0.061560, 0.02452]
AMAX = [2166.5, 13.24326, 13.46708, 10.226771, 14.224874]
WX = [[21.211773, -39.013052, -1.382553, -14.545348, -0.320899], [-8.981803, 19.956049, 0.935389, -1.686586, -3.238586],
      [1.633830, -2.877505, -7.442935, 5.606502, -1.783120], [6.103821, 19.587435, -0.240284, 1.088213, -0.511314],
      [11.556344, 3.892028, 9.720441, -3.287205, -11.031250]]
WXB = [1.330890, 2.686103, 2.096598, -1.327851, 3.087055]
WY = [-4.696996, -3.289959, 7.004782, 6.651897, 4.009144]


def network(movs):
    x = list(WXB)
    for i in range(5):
        m = (movs[i] - AMIN[i]) / (AMAX[i] - AMIN[i])
        for j in range(5):
            x[j] += WX[i][j] * m
    di = -1.360308
    for j in range(5):
        di += WY[j] * sigmoid(x[j])
    return di, -3.98 + (0.22 - -3.98) * sigmoid(di)


def di_sensitivity(err):
    """the largest change of DI that MOV errors of err[i] can make: a sigmoid's slope is at most 1 / 4"""
    return sum(abs(WY[j]) / 4. * sum(abs(WX[i][j]) * err[i] / (AMAX[i] - AMIN[i]) for i in range(5)) for j in range(5))


def model(d, channels, first, count, first_b, count_b):
    """the reading of frames [first, first + count) and blocks [first_b, first_b + count_b): the routing of
    peaq_backend_fft.inc:502-534 and peaq_backend_fb.inc:116-263 into fresh accumulators"""
    accs = [[AdvAcc(MODE[i]) for i in range(5)] for _ in range(channels)]
    seg_abs = [AdvAcc(AVG) for _ in range(channels)]      # SegmentalNMR's sum |v| / den, for its tolerance
    sig = noise = 0.
    for f in range(first, first + count):
        tr, sc = d["frames"][f], d["scalars"][f]
        flags = int(tr["flags"])
        energy = any((int(sc[c][S_FLAGS_REF]) | int(sc[c][S_FLAGS_TEST])) & 2 for c in range(channels))
        for c in range(channels):
            for a in (accs[c][SEGNMR], accs[c][EHS], seg_abs[c]):
                a.set_tentative(not flags & ABOVE)
            accs[c][SEGNMR].add(float(tr["ch"][c][0]), 1.)
            seg_abs[c].add(abs(float(tr["ch"][c][0])), 1.)
            if energy:
                accs[c][EHS].add(1000. * float(sc[c][S_EHS]), 1.)
        sig += float(sum(sc[c][S_SIG_E] for c in range(channels)))
        noise += float(sum(sc[c][S_NOISE_E] for c in range(channels)))
    for b in range(first_b, first_b + count_b):
        tr = d["blocks"][b]
        flags = int(tr["flags"])
        for c in range(channels):
            v, a = tr["ch"][c], accs[c]
            for i in (RMSMOD, NLASYM, LINDIST):
                a[i].set_tentative(not flags & ABOVE)
            if flags & MOD_OPEN:
                a[RMSMOD].add(float(v[0]), float(v[1]))
            if flags & LOUD_OPEN:
                a[NLASYM].add(float(v[2]), float(v[3]))
                a[LINDIST].add(float(v[4]), 1.)
    movs = [sum(accs[c][i].value() for c in range(channels)) / channels for i in range(5)]
    di, odg = network(movs)
    with np.errstate(divide="ignore", invalid="ignore"):
        snr = float(10 * np.log10(np.float64(sig) / np.float64(noise)))
    return dict(movs=np.array(movs), di=di, odg=odg, totalsnr=snr, frames=count, fb_blocks=count_b,
                seg_abs=sum(a.value() for a in seg_abs) / channels)


def assert_reading(got, exp, where):
    print(where, "movs", got["movs"], exp["movs"], "di", got["di"], exp["di"], "odg", got["odg"], exp["odg"],
          "snr", got["totalsnr"], exp["totalsnr"], "seg_abs", exp["seg_abs"])
    assert got["frames"] == exp["frames"] and got["fb_blocks"] == exp["fb_blocks"], (where, got["frames"], got["fb_blocks"])
    assert np.array_equal(np.isnan(got["movs"]), np.isnan(exp["movs"])), (where, got["movs"], exp["movs"])
    err = [0.] * 5
    for i in range(5):
        g, e = float(got["movs"][i]), float(exp["movs"][i])
        if math.isnan(e):
            continue
        err[i] = MOV_RTOL * (exp["seg_abs"] if i == SEGNMR else abs(e))
        assert g == e or abs(g - e) <= err[i], (where, i, g, e, err[i])
    for k in ("di", "odg"):
        assert math.isnan(got[k]) == math.isnan(exp[k]), (where, k, got[k], exp[k])
        assert math.isnan(exp[k]) or abs(got[k] - exp[k]) <= DI_ATOL, (where, k, got[k], exp[k])
    if not math.isnan(exp["di"]) and all(math.isfinite(x) for x in err):
        assert di_sensitivity(err) * max(1., (0.22 + 3.98) / 4.) <= DI_ATOL, (where, err, di_sensitivity(err))
    g, e = got["totalsnr"], exp["totalsnr"]
    assert (math.isnan(g) and math.isnan(e)) or g == e or abs(g - e) <= MOV_RTOL * abs(e), (where, g, e)


# ---- 1, 2: identity with the trajectory and with the end result ------------------------------------------------------
@pytest.mark.parametrize("interval", (1000, 3072, 48000))
def test_spans_from_zero_are_the_trajectory_points(gpu, interval):
    import gstpeaq_amd
    import torch
    seen = 0
    ctx = gpu.ctx("default")
    for case in cases():
        d = pair_data(gpu, case)
        n = min(len(d["r"]), len(d["t"]))
        m = max(len(d["r"]), len(d["t"]))
        n_points = -(-m // interval)
        lengths = [(k + 1) * interval for k in range(n_points)]
        spans = [(0, L) for L in lengths]
        pts, _ = gstpeaq_amd.batch_trajectory(ctx, 1, d["ref"], d["test"], interval, n_points, d["n_ref"], d["n_test"],
                                              sync=False)
        spn, res = gstpeaq_amd.batch_adv_spans(ctx, d["ref"], d["test"], spans, d["n_ref"], d["n_test"], sync=False)
        torch.cuda.synchronize()
        pts, spn = raw(pts)[0], raw(spn)[0]
        assert raw(res).tobytes() == d["plain_bytes"], case["name"]
        for k, L in enumerate(lengths):
            if L < m:
                assert spn[k].tobytes() == pts[k].tobytes(), (case["name"], interval, k, spn[k], pts[k])
                assert spn[k][14] == F(min(L, n)) and spn[k][15] == B(min(L, n)), (case["name"], k, spn[k][14:])
                seen += 1
            else:                                      # reaches the end of the longer signal: the flushed end result
                assert spn[k].tobytes() == d["plain_bytes"], (case["name"], interval, k, spn[k])
    assert seen > 6


def test_a_span_over_the_whole_pair_is_the_end_result_and_that_is_batch_runs(gpu):
    import gstpeaq_amd
    import torch
    for case in cases():
        d = pair_data(gpu, case)
        m = max(len(d["r"]), len(d["t"]))
        spans = [(0, m), (0, m + 1), (0, 0xFFFFFFFF)]
        spn, res = gstpeaq_amd.batch_adv_spans(gpu.ctx("default"), d["ref"], d["test"], spans, d["n_ref"], d["n_test"],
                                               sync=False)
        torch.cuda.synchronize()
        assert raw(res).tobytes() == d["plain_bytes"], case["name"]
        for k in range(len(spans)):
            assert raw(spn)[0][k].tobytes() == d["plain_bytes"], (case["name"], k, raw(spn)[0][k])
        assert raw(spn)[0][0][14] == d["total"] and raw(spn)[0][0][15] == d["total_b"]


# ---- 3: spans in mid-stream against the model ---------------------------------------------------------------------
def test_the_model_reproduces_the_shipped_path_on_whole_pairs(gpu):
    for case in cases():
        d = pair_data(gpu, case)
        exp = model(d, d["r"].shape[1], 0, d["total"], 0, d["total_b"])
        assert_reading(d["plain"], exp, (case["name"], "whole pair"))


def test_mid_stream_spans_match_the_model(gpu):
    import gstpeaq_amd
    empty_or_nan = begins_in_gap = ends_in_gap = loud_turns = compared = 0
    for case in cases():
        d = pair_data(gpu, case)
        n_ref, n_test, channels = len(d["r"]), len(d["t"]), d["r"].shape[1]
        m = max(n_ref, n_test)
        spans = np.concatenate([gstpeaq_amd.sliding_windows(m, L, hop)
                                for L, hop in ((24000, 12000), (48000, 4096), (3000, 1000))])
        spn, res = gstpeaq_amd.batch_adv_spans(gpu.ctx("default"), d["ref"], d["test"], spans, d["n_ref"], d["n_test"])
        assert len(spn[0]) == len(spans)
        above, above_b = d["frames"]["flags"] & ABOVE, d["blocks"]["flags"] & ABOVE
        loud = d["blocks"]["flags"] & LOUD_OPEN
        for k, (start, length) in enumerate(spans.tolist()):
            first, count = window_frames(n_ref, n_test, start, length)
            first_b, count_b = span_blocks(n_ref, n_test, start, length)
            assert (first, count) == gstpeaq_amd.window_frames(n_ref, n_test, start, length)
            assert (first_b, count_b) == gstpeaq_amd.span_blocks(n_ref, n_test, start, length)
            assert count <= 47 and count_b <= 250
            exp = model(d, channels, first, count, first_b, count_b)
            got = spn[0][k]
            assert_reading(got, exp, (case["name"], k, start, length, first, count, first_b, count_b))
            compared += 1
            empty_or_nan += bool(count == 0 or count_b == 0 or np.isnan(got["movs"]).any())
            # a gap: units below the data boundary after the pair's first unit above it
            in_f = bool(count and above[:first].any())
            in_b = bool(count_b and above_b[:first_b].any())
            begins_in_gap += (in_f and not above[first]) or (in_b and not above_b[first_b])
            ends_in_gap += (in_f and not above[first + count - 1]) or (in_b and not above_b[first_b + count_b - 1])
            loud_turns += bool(count_b and loud[first_b] != loud[first_b + count_b - 1])
    print("compared", compared, "empty or NaN", empty_or_nan, "begin in a gap", begins_in_gap, "end in a gap", ends_in_gap,
          "LOUD_OPEN turns", loud_turns)
    assert empty_or_nan >= 1 and begins_in_gap >= 1 and ends_in_gap >= 1 and loud_turns >= 1


# ---- 4: launch seams -------------------------------------------------------------------------------------------------
def test_spans_across_launch_boundaries(gpu):
    """128 stereo pairs of 10 s: the batch path cuts them into 8 FFT launches of 64 frames and filter-bank launches of
    840, 840 and 820 blocks; a one-pair batch is one launch per path"""
    import gstpeaq_amd
    import torch
    ctx = gpu.ctx("default")
    n, pairs = 480000, 128
    ref, test = gstpeaq_amd.synth_fill(ctx, 700, pairs, 2, n)
    spans = np.concatenate([gstpeaq_amd.sliding_windows(n, 96000, 48000),
                            np.array([[65000, 1500], [161000, 600], [322000, 1200], [0, n]], dtype=np.uint32)])
    d_spn, d_res = gstpeaq_amd.batch_adv_spans(ctx, ref, test, spans, sync=False)
    tm = ctx.last_timing()
    assert tm["frontend_launches"] > 1 and tm["fb_launches"] > 1, tm
    torch.cuda.synchronize()
    whole = gstpeaq_amd.batch_run(ctx, 1, ref, test, sync=False)
    torch.cuda.synchronize()
    spn, res, whole = raw(d_spn), raw(d_res), raw(whole)
    assert res.tobytes() == whole.tobytes()
    assert spn[:, -1].tobytes() == whole.tobytes()
    for p in (0, 37, 64, 127):
        one, one_res = gstpeaq_amd.batch_adv_spans(ctx, ref[p:p + 1], test[p:p + 1], spans, sync=False)
        assert ctx.last_timing()["frontend_launches"] == 1
        torch.cuda.synchronize()
        assert raw(one)[0].tobytes() == spn[p].tobytes(), (p, raw(one)[0], spn[p])
        assert raw(one_res)[0].tobytes() == res[p].tobytes()
    seam_f = seam_b = 0
    for k, (start, length) in enumerate(spans.tolist()):
        first, count = gstpeaq_amd.window_frames(n, n, start, length)
        first_b, count_b = gstpeaq_amd.span_blocks(n, n, start, length)
        assert (first, count) == window_frames(n, n, start, length)
        assert (first_b, count_b) == span_blocks(n, n, start, length)
        assert (spn[:, k, 14] == count).all() and (spn[:, k, 15] == count_b).all(), (k, spn[0, k, 14:], count, count_b)
        seam_f += first < 64 < first + count
        seam_b += (first_b < 840 < first_b + count_b) + (first_b < 1680 < first_b + count_b)
    assert seam_f >= 2 and seam_b >= 4                  # (the short spans across a seam, and the long ones)


# ---- 5: the one-pair entry; nothing of a spans run is left in the context ---------------------------------------
def test_host_memory_entry_equals_the_batch_entry(gpu):
    import gstpeaq_amd
    case = dict(kind="synth", seed=21, channels=2, n=100000, test_trim=1500)
    r, t = case_defs.make_inputs(case)
    spans = gstpeaq_amd.sliding_windows(100000, 24000, 12000)
    got = gstpeaq_amd.run_pair_adv_spans(gpu.ctx("default"), r, t, spans)
    ref, test, n_ref, n_test = to_device([(r, t)])
    spn, res = gstpeaq_amd.batch_adv_spans(gpu.ctx("default"), ref, test, spans, n_ref, n_test)
    assert len(got["spans"]) == len(spans)
    for k in range(len(spans)):
        for key in KEYS:
            np.testing.assert_array_equal(got["spans"][k][key], spn[0][k][key], err_msg=f"{k} {key}")
    for key in KEYS:
        np.testing.assert_array_equal(got["result"][key], res[0][key])
    assert any(not np.isnan(s["movs"]).any() for s in got["spans"])


@pytest.mark.parametrize("advanced", (0, 1))
def test_no_leakage_into_a_later_batch(gpu, advanced):
    """a batch_run after a spans run on the same context returns the bytes it returns on a fresh context"""
    import gstpeaq_amd
    import torch
    inputs = [case_defs.make_inputs(c) for c in cases() if c["channels"] == 2]
    ref, test, n_ref, n_test = to_device(inputs)
    ctx = gpu.ctx("default")
    gstpeaq_amd.batch_adv_spans(ctx, ref, test, gstpeaq_amd.sliding_windows(120000, 24000, 12000), n_ref, n_test)
    after = gstpeaq_amd.batch_run(ctx, advanced, ref, test, n_ref, n_test, sync=False)
    fresh_ctx = gstpeaq_amd.Context(0)
    fresh = gstpeaq_amd.batch_run(fresh_ctx, advanced, ref, test, n_ref, n_test, sync=False)
    torch.cuda.synchronize()
    assert after.cpu().numpy().tobytes() == fresh.cpu().numpy().tobytes()
    fresh_ctx.close()


# ---- 6: the CLI --------------------------------------------------------------------------------------------------------
def test_cli_spans(gpu, tmp_path):
    import gstpeaq_amd
    r, t = case_defs.make_inputs(dict(kind="synth", seed=22, channels=1, n=100000, ref_trim=700))
    write_wav(tmp_path / "ref.wav", r, bits=32, fmt_float=True)
    write_wav(tmp_path / "test.wav", t, bits=32, fmt_float=True)
    plain = subprocess.run([str(gst_env.CLI), "--advanced", tmp_path / "ref.wav", tmp_path / "test.wav"],
                           capture_output=True, text=True, timeout=300)
    out = subprocess.run([str(gst_env.CLI), "--advanced", "--spans=1:0.5", tmp_path / "ref.wav", tmp_path / "test.wav"],
                         capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and out.returncode == 0, (plain.stderr, out.stderr, out.stdout)
    lines = out.stdout.strip().splitlines()
    spans = gstpeaq_amd.sliding_windows(max(len(r), len(t)), 48000, 24000)
    exp = gstpeaq_amd.run_pair_adv_spans(gpu.ctx("default"), r, t, spans)["spans"]
    assert len(lines) == len(spans) + 2, out.stdout
    assert lines[-2:] == plain.stdout.strip().splitlines()[-2:]
    for k, line in enumerate(lines[:-2]):
        word = line.split()
        assert word[0] == "span" and len(word) == 7, line
        start, length = spans[k].tolist()
        want = "%.3f %.3f %.0f %.0f %.3f %.3f" % (start / 48000., (start + length) / 48000., exp[k]["frames"],
                                                  exp[k]["fb_blocks"], exp[k]["odg"], exp[k]["di"])
        got, want = [float(x) for x in word[1:]], [float(x) for x in want.split()]
        assert all(g == w or (math.isnan(g) and math.isnan(w)) for g, w in zip(got, want)), (k, line, want)
    assert any("nan" not in line for line in lines[:-2])

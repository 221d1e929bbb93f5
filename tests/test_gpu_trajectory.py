"""Trajectories (peaq_batch_run_trajectory, include/peaq_amd.h): readings at fixed intervals through every pair of a
batch.  Point k of a pair is what a session that has been pushed the first min((k + 1) interval, n) samples of each
signal, and has not been flushed, reads (gstpeaq.c:484-497) -- pinned here against the CPU oracle fed the same way
(orc_session_results mid-stream), against the HIP session, across the batch path's launch boundaries, and for the
end result against peaq_batch_run.  Needs an MI355X (`-m gpu`)."""
import subprocess

import numpy as np
import pytest

import cases as case_defs
import gst_env
import oracle_lib as orc
from test_conformance_runner import write_wav

pytestmark = pytest.mark.gpu

# from tests/cases.py: mono and stereo, a ragged pair, a mid-stream gap (NORMAL -> TENTATIVE -> NORMAL), and the quiet
# pairs whose loudness gate opens late (NaN readings until it does)
CASE_NAMES = ("synth_s10_mono", "gap1_mono", "synth_quiet_60dB",
              "synth_s0_stereo", "synth_ragged_test_short", "synth_quiet_36dB", "synth_quiet_84dB")
# 100: points that have no frame yet and several points per frame; 1000: several per frame; 3072 = 3 hops; 1 s
INTERVALS = (100, 1000, 3072, 48000)


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback in the product)")
    import gpu_common
    return gpu_common


def cases_of(channels):
    by_name = {c["name"]: c for c in case_defs.e2e_cases() if c["advanced"] == 0}
    return [by_name[n] for n in CASE_NAMES if by_name[n]["channels"] == channels]


def F(a):
    a = np.asarray(a, dtype=np.int64)
    return np.where(a >= 2048, (a - 2048) // 1024 + 1, 0)


def B(a):
    return np.asarray(a, dtype=np.int64) // 192


def n_points_for(inputs, interval):
    """readings up to the end of the longest signal, and two more past it (the final unflushed state again)"""
    return -(-max(max(len(r), len(t)) for r, t in inputs) // interval) + 2


def point_ends(n_ref, n_test, interval, n_points):
    k = np.arange(n_points, dtype=np.int64)
    return np.minimum((k + 1) * interval, n_ref), np.minimum((k + 1) * interval, n_test)


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


def incremental(session, ref, test, interval, n_points):
    """read `session` after each point's samples: the first min((k + 1) interval, n) of either signal, unflushed"""
    er, et = point_ends(len(ref), len(test), interval, n_points)
    out, pr, pt = [], 0, 0
    for k in range(n_points):
        if er[k] > pr:
            session.push_ref(ref[pr:er[k]])
            pr = int(er[k])
        if et[k] > pt:
            session.push_test(test[pt:et[k]])
            pt = int(et[k])
        out.append(session.results())
    return out


_ORACLE = {}


def oracle_points(case, advanced, interval, n_points):
    key = (case["name"], advanced, interval, n_points)
    if key not in _ORACLE:                           # (the same for both FIR modes)
        ref, test = case_defs.make_inputs(case)
        s = orc.Session(advanced, ref.shape[1])
        _ORACLE[key] = incremental(s, ref, test, interval, n_points)
        s.close()
    return _ORACLE[key]


def hip_session_points(gpu, advanced, ref, test, interval, n_points):
    import gstpeaq_amd
    s = gstpeaq_amd.Session(gpu.ctx(), advanced, ref.shape[1])
    out = incremental(s, ref, test, interval, n_points)
    s.close()
    return out


def assert_same_reading(got, exp, rtol, odg_tol, where):
    assert np.array_equal(np.isnan(got["movs"]), np.isnan(exp["movs"])), (where, got["movs"], exp["movs"])
    ok = ~np.isnan(exp["movs"])
    np.testing.assert_allclose(got["movs"][ok], exp["movs"][ok], rtol=rtol, atol=0, err_msg=str(where))
    for k in ("di", "odg", "totalsnr"):
        g, e = got[k], exp[k]
        if np.isnan(e) or np.isinf(e):
            assert g == e or (np.isnan(g) and np.isnan(e)), (where, k, g, e)
        else:
            assert abs(g - e) <= (odg_tol if k != "totalsnr" else 0) + rtol * abs(e), (where, k, g, e)


@pytest.mark.parametrize("interval", INTERVALS)
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("advanced", [0, 1])
def test_points_match_the_oracle_read_mid_stream(gpu, advanced, channels, interval, fir_mode):
    """Every point at the tolerances of tests/gpu_common.py.  The opt-in split-FP16 engine's "movs" / "odg" bounds are
    those of whole items, whose accumulators average thousands of blocks; a reading a few blocks after an accumulator
    opened (gstpeaq.c:988, block 125) is close to ONE block's value and is held to that engine's per-block bound
    ("blocks"), its last reading -- all the blocks of the item -- to "movs" / "odg" again."""
    import gstpeaq_amd
    cases = cases_of(channels)
    inputs = [case_defs.make_inputs(c) for c in cases]
    n_points = n_points_for(inputs, interval)
    ref, test, n_ref, n_test = to_device(inputs)
    points, results = gstpeaq_amd.batch_trajectory(gpu.ctx(), advanced, ref, test, interval, n_points, n_ref, n_test)
    seen_nan = False
    for p, (case, (r, t)) in enumerate(zip(cases, inputs)):
        exp = oracle_points(case, advanced, interval, n_points)
        er, et = point_ends(len(r), len(t), interval, n_points)
        a = np.minimum(er, et)
        for k in range(n_points):
            g, e = points[p][k], exp[k]
            where = (case["name"], k)
            assert g["frames"] == e["frames"] == F(a[k]), (where, g["frames"], e["frames"])
            assert g["fb_blocks"] == (B(a[k]) if advanced else 0), where
            per_block = advanced and gpu.mode() == "f16x3" and k < n_points - 1
            rtol = gpu.tol("blocks") if per_block else gpu.tol("movs", advanced)
            odg_atol = gpu.tol("blocks") if per_block else gpu.tol("odg", advanced) if advanced else 1e-6
            gpu.compare_result(g, e, rtol=rtol, atol=1e-9, odg_atol=odg_atol)
            seen_nan |= bool(np.isnan(g["movs"]).any())
        # points past the end of both signals: the final unflushed reading, again
        last = F(min(len(r), len(t)))
        assert points[p][-1]["frames"] == points[p][-2]["frames"] == last
        assert points[p][-1]["odg"] == points[p][-2]["odg"] or np.isnan(points[p][-1]["odg"])
    if interval < 2048:
        assert seen_nan                              # the first points have no frame yet: empty accumulators


@pytest.mark.parametrize("interval", INTERVALS)
@pytest.mark.parametrize("advanced", [0, 1])
def test_points_equal_the_hip_session_read_mid_stream(gpu, advanced, interval, fir_mode):
    """same kernels, same per-frame arithmetic as the session: the basic version bit for bit; the filter bank walks the
    stream in other tile alignments (tests/test_gpu_parity.py, test_session_streaming_equals_batch)"""
    import gstpeaq_amd
    rtol = gpu.tol("chunks") if advanced else 0.
    for channels in (1, 2):
        cases = cases_of(channels)
        inputs = [case_defs.make_inputs(c) for c in cases]
        n_points = n_points_for(inputs, interval)
        ref, test, n_ref, n_test = to_device(inputs)
        points, _ = gstpeaq_amd.batch_trajectory(gpu.ctx(), advanced, ref, test, interval, n_points, n_ref, n_test)
        for p, (case, (r, t)) in enumerate(zip(cases, inputs)):
            exp = hip_session_points(gpu, advanced, r, t, interval, n_points)
            a = np.minimum(*point_ends(len(r), len(t), interval, n_points))
            for k in range(n_points):
                g, e = points[p][k], exp[k]
                assert g["frames"] == e["frames"] == F(a[k]), (case["name"], k)
                assert g["fb_blocks"] == e["fb_blocks"] == (B(a[k]) if advanced else 0), (case["name"], k)
                assert_same_reading(g, e, rtol, rtol, (case["name"], k))


@pytest.mark.parametrize("advanced", [0, 1])
def test_points_across_launch_boundaries(gpu, advanced):
    """128 stereo pairs of 10 s, a point per frame: the batch path cuts them into 8 launches of 64 frames and, in the
    advanced version, 3 filter-bank launches of 840 blocks -- points on both sides of every seam"""
    import gstpeaq_amd
    ctx = gpu.ctx()
    n, pairs, seed0, interval = 480000, 128, 500, 1024
    ref, test = gstpeaq_amd.synth_fill(ctx, seed0, pairs, 2, n)
    n_points = -(-n // interval)
    d_points, d_results = gstpeaq_amd.batch_trajectory(ctx, advanced, ref, test, interval, n_points, sync=False)
    tm = ctx.last_timing()
    assert tm["frontend_launches"] > 1, tm
    if advanced:
        assert tm["fb_launches"] > 1, tm
    import torch
    torch.cuda.synchronize()
    pts = d_points.cpu().numpy()
    a = np.minimum((np.arange(n_points) + 1) * interval, n)
    assert (pts[:, :, 14] == F(a)[None, :]).all()
    assert (pts[:, :, 15] == (B(a) if advanced else 0 * a)[None, :]).all()
    # the flushed end result: byte for byte that of peaq_batch_run
    whole = gstpeaq_amd.batch_run(ctx, advanced, ref, test, sync=False)
    torch.cuda.synchronize()
    assert whole.cpu().numpy().tobytes() == d_results.cpu().numpy().tobytes()
    # four pairs at every point against HIP sessions
    rtol = gpu.tol("chunks") if advanced else 0.
    for p in (0, 37, 64, 127):
        r, t = ref[p].cpu().numpy(), test[p].cpu().numpy()
        exp = hip_session_points(gpu, advanced, r, t, interval, n_points)
        for k in range(n_points):
            g = gstpeaq_amd.capi._result_dict(pts[p, k], advanced)
            assert g["frames"] == exp[k]["frames"] and g["fb_blocks"] == exp[k]["fb_blocks"], (p, k)
            assert_same_reading(g, exp[k], rtol, rtol, (p, k))


@pytest.mark.parametrize("advanced", [0, 1])
def test_no_leakage_into_a_later_batch(gpu, advanced):
    """a batch_run after a trajectory on the same context returns the bytes it returns on a fresh context"""
    import gstpeaq_amd
    import torch
    inputs = [case_defs.make_inputs(c) for c in cases_of(2)]
    ref, test, n_ref, n_test = to_device(inputs)
    ctx = gpu.ctx()
    gstpeaq_amd.batch_trajectory(ctx, advanced, ref, test, 1000, 123, n_ref, n_test)
    after = gstpeaq_amd.batch_run(ctx, advanced, ref, test, n_ref, n_test, sync=False)
    fresh_ctx = gstpeaq_amd.Context(0)
    fresh = gstpeaq_amd.batch_run(fresh_ctx, advanced, ref, test, n_ref, n_test, sync=False)
    torch.cuda.synchronize()
    assert after.cpu().numpy().tobytes() == fresh.cpu().numpy().tobytes()
    fresh_ctx.close()


@pytest.mark.parametrize("advanced", [0, 1])
def test_host_memory_entry_equals_the_batch_entry(gpu, advanced):
    import gstpeaq_amd
    case = dict(kind="synth", seed=21, channels=2, n=100000, test_trim=1500)
    r, t = case_defs.make_inputs(case)
    pts, res = gstpeaq_amd.run_pair_trajectory(gpu.ctx(), advanced, r, t, 5000, 22)
    ref, test, n_ref, n_test = to_device([(r, t)])
    bp, br = gstpeaq_amd.batch_trajectory(gpu.ctx(), advanced, ref, test, 5000, 22, n_ref, n_test)
    for k in range(22):
        for key in ("movs", "di", "odg", "totalsnr", "frames", "fb_blocks"):
            np.testing.assert_array_equal(pts[k][key], bp[0][k][key], err_msg=f"{k} {key}")
    for key in ("movs", "di", "odg", "totalsnr", "frames", "fb_blocks"):
        np.testing.assert_array_equal(res[key], br[0][key])
    whole = gstpeaq_amd.run_pair(gpu.ctx(), advanced, r, t)
    np.testing.assert_array_equal(res["movs"], whole["movs"])
    assert res["odg"] == whole["odg"]


@pytest.mark.parametrize("advanced", [0, 1])
def test_cli_interval(gpu, advanced, tmp_path):
    import gstpeaq_amd
    r, t = case_defs.make_inputs(dict(kind="synth", seed=22, channels=1, n=100000, ref_trim=700))
    write_wav(tmp_path / "ref.wav", r, bits=32, fmt_float=True)
    write_wav(tmp_path / "test.wav", t, bits=32, fmt_float=True)
    flags = ["--advanced"] if advanced else []
    plain = subprocess.run([str(gst_env.CLI), *flags, tmp_path / "ref.wav", tmp_path / "test.wav"],
                           capture_output=True, text=True, timeout=300)
    out = subprocess.run([str(gst_env.CLI), *flags, "--interval=0.5", tmp_path / "ref.wav", tmp_path / "test.wav"],
                         capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and out.returncode == 0, (plain.stderr, out.stderr)
    lines = out.stdout.strip().splitlines()
    n_max = max(len(r), len(t))
    n_points = -(-n_max // 24000)
    assert len(lines) == n_points + 2, out.stdout
    assert lines[-2:] == plain.stdout.strip().splitlines()[-2:]
    pts, _ = gstpeaq_amd.run_pair_trajectory(gpu.ctx(), advanced, r, t, 24000, n_points)
    for k, line in enumerate(lines[:-2]):
        end = min((k + 1) * 24000, n_max) / 48000.
        # (the C library prints a NaN with its sign, "-nan")
        assert line.replace("-nan", "nan") == "Time %.3f s: ODG %.3f, DI %.3f" % (end, pts[k]["odg"], pts[k]["di"]), \
            (k, line)
    assert any("nan" not in line for line in lines[:-2])

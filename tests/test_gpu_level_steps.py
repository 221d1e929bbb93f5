"""peaq_session_set_level in mid-stream (include/peaq_amd.h), through the C ABI only: sessions that follow the schedules
of tests/cases.py:level_step_cases() against the REAL reference driven along the same schedules on one thread
(tests/golden/ref_e2e_level_steps.json), read after every push against the CPU oracle's session, and the identities,
refusals and the reset that the header states.  The level reaches the kernels as per-launch arguments; what crosses a
launch is state computed at the OLD level -- the FFT model's smeared excitation, the pattern layer's adapters, the filter
bank's high-pass state and the tail of filtered samples the next launch's FIR windows reach back into, from whose peak
the split-FP16 engine picks its scale.  Needs an MI355X (`-m gpu`)."""
import ctypes as C
import json

import numpy as np
import pytest

import cases as case_defs
import oracle_lib as orc

pytestmark = pytest.mark.gpu

PEAQ_ERR_ARG = -1
NAMES = sorted({c["name"] for c in case_defs.level_step_cases()})
MID_STREAM = ("step_up_mono", "step_up_stereo", "step_down_mono", "step_down_stereo", "step_extremes_stereo")


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback in the product)")
    import gpu_common
    return gpu_common


_RECS, _INPUTS, _ORACLE = {}, {}, {}


def record(name, advanced):
    if not _RECS:
        import gpu_common
        for r in json.loads((gpu_common.GOLD / "ref_e2e_level_steps.json").read_text()):
            _RECS[r["case"]["name"], r["case"]["advanced"]] = r
    return _RECS[name, advanced]


def inputs(case):
    if case["name"] not in _INPUTS:
        _INPUTS[case["name"]] = case_defs.make_inputs(case)
    return _INPUTS[case["name"]]


def pushes_of(schedule):
    return [e for e in schedule if e[0] != "l"]


def hip_run(gpu, case, schedule=None, level=None, readings=None, meter=None, before_flush=None):
    """a HIP session along the case's schedule (or another one), flushed -> its results; readings: a list that receives
    the results read behind every push"""
    import gstpeaq_amd
    ref, test = inputs(case)
    s = gstpeaq_amd.Session(gpu.ctx(), case["advanced"], case["channels"],
                            playback_level=case["level"] if level is None else level)
    if meter:
        s.set_meter(meter)
    case_defs.run_schedule(s, ref, test, case["schedule"] if schedule is None else schedule,
                           after_push=None if readings is None else lambda: readings.append(s.results()))
    if before_flush:
        before_flush(s)
    s.flush()
    got = s.results()
    s.close()
    return got


def oracle_readings(case):
    """the oracle's session along the case's schedule, read behind every push, and flushed (the same for both engines)"""
    key = case["name"], case["advanced"]
    if key not in _ORACLE:
        ref, test = inputs(case)
        s = orc.Session(case["advanced"], case["channels"], case["level"])
        out = []
        case_defs.run_schedule(s, ref, test, case["schedule"], after_push=lambda: out.append(s.results()))
        s.flush()
        _ORACLE[key] = out, s.results()
        s.close()
    return _ORACLE[key]


def assert_same(gpu, a, b, advanced, what):
    """two runs of the same stream: bit for bit in the basic version and on the default engine, the other engine at its
    `chunks` bound; NaN places and counts exact everywhere"""
    assert a["frames"] == b["frames"] and a["fb_blocks"] == b["fb_blocks"], what
    if not advanced or gpu.mode() == "default":
        for k in ("movs", "di", "odg", "totalsnr"):
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k, a[k], b[k])
        return
    rtol = gpu.tol("chunks")
    assert np.array_equal(np.isnan(a["movs"]), np.isnan(b["movs"])), what
    ok = ~np.isnan(b["movs"])
    np.testing.assert_allclose(a["movs"][ok], b["movs"][ok], rtol=rtol, atol=0, err_msg=str(what))
    for k in ("di", "odg", "totalsnr"):
        assert (np.isnan(a[k]) and np.isnan(b[k])) or abs(a[k] - b[k]) <= rtol * (1 + abs(b[k])), (what, k, a[k], b[k])


def differs(a, b):
    return not np.allclose(a["movs"], b["movs"], rtol=1e-6, atol=0, equal_nan=True)


def worst(got, exp_movs, exp_odg):
    exp = np.array([float(v) for v in exp_movs])
    ok = ~np.isnan(exp) & (exp != 0)
    rel = float(np.max(np.abs(got["movs"][ok] - exp[ok]) / np.abs(exp[ok]))) if ok.any() else 0.
    return rel, abs(got["odg"] - float(exp_odg))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("advanced", [0, 1])
def test_sessions_follow_the_reference_across_level_changes(gpu, advanced, name, fir_mode):
    """every record of ref_e2e_level_steps.json at the bounds of tests/gpu_common.py: MOVs, DI / ODG, NaN places MOV by
    MOV, frame and block counts exact, totalsnr as compare_result holds it"""
    rec = record(name, advanced)
    got = hip_run(gpu, rec["case"])
    rel, dodg = worst(got, rec["movs"], rec["odg"])
    print(f"LEVELSTEP {name} advanced={advanced} engine={gpu.mode()}: worst MOV {rel:.3e} relative, |dODG| {dodg:.3e}")
    assert got["fb_blocks"] == rec["fb_frames"]
    gpu.compare_result(got, rec, rtol=gpu.tol("movs", advanced), atol=1e-9, odg_atol=gpu.tol("odg", advanced))


@pytest.mark.parametrize("name", MID_STREAM)
@pytest.mark.parametrize("advanced", [0, 1])
def test_readings_behind_every_push_match_the_oracle(gpu, advanced, name, fir_mode):
    """peaq_session_results behind every push against the oracle's session read at the same points, in the way and at
    the bounds of tests/test_gpu_trajectory.py (a reading of the split-FP16 engine that is not the stream's last is
    held to that engine's per-block bound): the first reading that goes wrong names the push, and with it the frame"""
    case = record(name, advanced)["case"]
    exp, exp_end = oracle_readings(case)
    got = []
    got_end = hip_run(gpu, case, readings=got)
    assert len(got) == len(exp) == len(pushes_of(case["schedule"]))
    pos, k, seen_nan = {"r": 0, "t": 0}, 0, False
    for op, v in case["schedule"]:
        if op == "l":
            continue
        pos[op] += v
        a = min(pos.values())
        where = (name, "push", k, dict(pos))
        frames = (a - 2048) // 1024 + 1 if a >= 2048 else 0
        assert got[k]["frames"] == exp[k]["frames"] == frames, (where, got[k]["frames"], exp[k]["frames"])
        assert got[k]["fb_blocks"] == (a // 192 if advanced else 0), where
        per_block = advanced and gpu.mode() == "f16x3"
        rtol = gpu.tol("blocks") if per_block else gpu.tol("movs", advanced)
        odg_atol = gpu.tol("blocks") if per_block else gpu.tol("odg", advanced) if advanced else 1e-6
        try:
            gpu.compare_result(got[k], exp[k], rtol=rtol, atol=1e-9, odg_atol=odg_atol)
        except AssertionError as e:
            raise AssertionError(f"{where}: {e}") from e
        seen_nan |= bool(np.isnan(got[k]["movs"]).any())
        k += 1
    assert seen_nan                                  # the first readings have no frame yet
    assert got_end["frames"] == exp_end["frames"] == 93
    gpu.compare_result(got_end, exp_end, rtol=gpu.tol("movs", advanced), atol=1e-9,
                       odg_atol=gpu.tol("odg", advanced) if advanced else 1e-6)


@pytest.mark.parametrize("advanced", [0, 1])
def test_identities(gpu, advanced, fir_mode):
    case = record("step_up_stereo", advanced)["case"]
    pushes = pushes_of(case["schedule"])
    plain = hip_run(gpu, case, schedule=pushes)
    stepped = hip_run(gpu, case)
    assert differs(plain, stepped)
    # a set to the level the session has, before every push, equals no set
    again = hip_run(gpu, case, schedule=[e for p in pushes for e in (["l", case["level"]], p)])
    assert_same(gpu, again, plain, advanced, "set to the current level")
    # a set before the first push equals creation at that level
    created = hip_run(gpu, case, schedule=pushes, level=112.0)
    set_first = hip_run(gpu, case, schedule=[["l", 112.0]] + pushes, level=60.0)
    assert differs(created, plain)
    assert_same(gpu, set_first, created, advanced, "set before the first push")
    # a set after the flush leaves the result unchanged
    import gstpeaq_amd
    ref, test = inputs(case)
    s = gstpeaq_amd.Session(gpu.ctx(), advanced, case["channels"], playback_level=case["level"])
    case_defs.run_schedule(s, ref, test, case["schedule"])
    s.flush()
    before = s.results()
    s.set_level(130.0)
    after = s.results()
    s.close()
    assert_same(gpu, after, before, advanced, "set after the flush")
    assert_same(gpu, before, stepped, advanced, "the same schedule on a second run")
    # the meter on (windows of 8 frames) changes no end result
    metered = hip_run(gpu, case, meter=8)
    assert_same(gpu, metered, stepped, advanced, "with the meter on")


@pytest.mark.parametrize("advanced", [0, 1])
def test_one_stream_cut_into_other_buffers(gpu, advanced, fir_mode):
    """the up case in buffers of 192, 1000 and 4096 samples, each cut at the step: the level changes with both pads at
    sample 48128 every time, so frames 0 .. 45 and blocks 0 .. 249 run at 92 dB and the rest at 112 dB however the
    launches fall -- blocks 250 .. 257 with FIR windows that reach across the step.  Bit-equal in the basic version,
    the filter bank at the `chunks` bound (it walks the stream in other tile alignments)."""
    rec = record("step_up_stereo", advanced)
    case = rec["case"]
    got = {}
    for chunk in (192, 1000, 4096):
        sched = case_defs.level_schedule(case["n"], chunk, [(case_defs.LEVEL_STEP_AT, 112.0)])
        assert (chunk == 4096) == (sched == case["schedule"])
        got[chunk] = hip_run(gpu, case, schedule=sched)
        gpu.compare_result(got[chunk], rec, rtol=gpu.tol("movs", advanced), atol=1e-9, odg_atol=gpu.tol("odg", advanced))
    rtol = gpu.tol("chunks") if advanced else 0.
    for chunk in (192, 1000):
        a, b = got[chunk], got[4096]
        assert a["frames"] == b["frames"] == 93 and a["fb_blocks"] == b["fb_blocks"]
        np.testing.assert_allclose(a["movs"], b["movs"], rtol=rtol, atol=0, err_msg=str(chunk))
        for k in ("di", "odg", "totalsnr"):
            assert abs(a[k] - b[k]) <= rtol * (1 + abs(b[k])), (chunk, k, a[k], b[k])


@pytest.mark.parametrize("advanced", [0, 1])
def test_refused_levels_change_nothing(gpu, advanced, fir_mode):
    """-1, 130.0001, NaN and a NULL session: PEAQ_ERR_ARG, the level and the stream as before"""
    import gstpeaq_amd
    L = gstpeaq_amd.load_library()
    case = record("step_up_stereo", advanced)["case"]
    stepped = hip_run(gpu, case)
    assert L.peaq_session_set_level(None, C.c_double(92.0)) == PEAQ_ERR_ARG

    def refused(s):
        for bad in (-1.0, 130.0001, float("nan")):
            assert L.peaq_session_set_level(s.h, C.c_double(bad)) == PEAQ_ERR_ARG, bad
        assert L.peaq_session_set_level(None, C.c_double(60.0)) == PEAQ_ERR_ARG

    class Refusing:
        """the session, with the refused calls in front of every accepted set and every eighth push"""
        def __init__(self, s):
            self.s, self.n = s, 0

        def set_level(self, v):
            refused(self.s)
            self.s.set_level(v)
            refused(self.s)

        def push_ref(self, x):
            self.n += 1
            if self.n % 8 == 0:
                refused(self.s)
            self.s.push_ref(x)

        def push_test(self, x):
            self.s.push_test(x)

    ref, test = inputs(case)
    s = gstpeaq_amd.Session(gpu.ctx(), advanced, case["channels"], playback_level=case["level"])
    refused(s)
    case_defs.run_schedule(Refusing(s), ref, test, case["schedule"])
    refused(s)
    s.flush()
    got = s.results()
    s.close()
    assert_same(gpu, got, stepped, advanced, "with refused calls")
    # the bounds themselves are accepted (gstpeaq.c:275-281: 0 .. 130)
    s = gstpeaq_amd.Session(gpu.ctx(), advanced, 1)
    assert L.peaq_session_set_level(s.h, C.c_double(0.0)) == 0 and L.peaq_session_set_level(s.h, C.c_double(130.0)) == 0
    s.close()


@pytest.mark.parametrize("advanced", [0, 1])
def test_reset_keeps_the_level_last_set(gpu, advanced, fir_mode):
    """peaq_session_reset starts the stream over and keeps the level (include/peaq_amd.h): a session that ran the up
    case (created at 92 dB, left at 112 dB), reset and fed the pair again, equals a session created at 112 dB"""
    import gstpeaq_amd
    case = record("step_up_stereo", advanced)["case"]
    pushes = pushes_of(case["schedule"])
    ref, test = inputs(case)
    created = hip_run(gpu, case, schedule=pushes, level=112.0)
    at_92 = hip_run(gpu, case, schedule=pushes)
    assert differs(created, at_92)
    s = gstpeaq_amd.Session(gpu.ctx(), advanced, case["channels"], playback_level=case["level"])
    case_defs.run_schedule(s, ref, test, case["schedule"])
    s.flush()
    s.reset()
    case_defs.run_schedule(s, ref, test, pushes)
    s.flush()
    got = s.results()
    # ... and a level set right after the reset holds for the new stream
    s.reset()
    s.set_level(case["level"])
    case_defs.run_schedule(s, ref, test, pushes)
    s.flush()
    back = s.results()
    s.close()
    assert_same(gpu, got, created, advanced, "reset keeps the level")
    assert_same(gpu, back, at_92, advanced, "a set after the reset")

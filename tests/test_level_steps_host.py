"""The playback level changed in mid-stream (the element's playback_level property, gstpeaq.c:508-515 ->
fftearmodel.c:305-314, fbearmodel.c:249-254): the oracle's orc_session_set_level / orc_fftmodel_set_level /
orc_fbmodel_set_level against the REAL reference driven on one thread along the schedules of
tests/cases.py:level_step_cases() (oracle/ref_harness.c `sched`; fixtures by tools/make_golden.py level_steps ->
tests/golden/ref_e2e_level_steps.json, ref_stages_level_step.npz), the condition the cases' inputs keep, and the
identities a level set must obey.  CPU only; tests/test_gpu_level_steps.py holds the HIP sessions to the same records."""
import json
from pathlib import Path

import numpy as np
import pytest

import cases as case_defs
import oracle_lib as orc
from test_oracle_golden import check_against_reference

GOLD = Path(__file__).parent / "golden"


def _records():
    return json.loads((GOLD / "ref_e2e_level_steps.json").read_text())


def _id(rec):
    return f"{rec['case']['name']}-{'adv' if rec['case']['advanced'] else 'basic'}"


def oracle_along(case, schedule=None, level=None, trace_frames=0):
    """the oracle's session along the case's schedule (or another one), flushed -> (results, trace or None)"""
    ref, test = case_defs.make_inputs(case)
    s = orc.Session(case["advanced"], case["channels"], case["level"] if level is None else level)
    trace = s.trace_basic(trace_frames) if trace_frames else None
    case_defs.run_schedule(s, ref, test, case["schedule"] if schedule is None else schedule)
    s.flush()
    got = s.results()
    s.close()
    return got, trace


def test_the_fixture_holds_every_case_as_it_is_defined_today():
    recs = _records()
    assert [r["case"] for r in recs] == case_defs.level_step_cases()
    names = {r["case"]["name"] for r in recs}
    assert len(recs) == 2 * len(names) == 20
    for r in recs:
        assert r["frames"] == 93 and r["fb_frames"] == (500 if r["case"]["advanced"] else 0), _id(r)


def test_schedules_are_what_the_cases_say():
    """every sample of both pads is pushed exactly once; the level is set where the case says, with both pads at the
    stated samples; no buffer spans a level change"""
    by = {c["name"]: c for c in case_defs.level_step_cases() if not c["advanced"]}

    def sets(case):
        pos, out = {"r": 0, "t": 0}, []
        for op, v in case["schedule"]:
            if op == "l":
                out.append((pos["r"], pos["t"], v))
            else:
                pos[op] += v
        assert pos == {"r": case["n"], "t": case["n"]}
        return out

    at = case_defs.LEVEL_STEP_AT
    assert at == 47 * 1024 and at // 192 == 250
    assert sets(by["step_up_mono"]) == sets(by["step_up_stereo"]) == [(at, at, 112.0)]
    assert sets(by["step_down_mono"]) == sets(by["step_down_stereo"]) == [(at, at, 60.0)]
    assert sets(by["step_waiting_stereo"]) == [(at + 5000, at, 112.0)]
    assert sets(by["step_low_mono"]) == [(at, at, 0.0), (at + 10000, at + 10000, 92.0)]
    assert sets(by["step_flush_only_stereo"]) == [(96000, 96000, 112.0)]
    assert sets(by["step_headroom_up_mono"]) == [(at, at, 130.0)] and by["step_headroom_up_mono"]["level"] == 60.0
    assert sets(by["step_headroom_down_mono"]) == [(at, at, 60.0)] and by["step_headroom_down_mono"]["level"] == 130.0
    ext = sets(by["step_extremes_stereo"])
    assert ext == [(1000 * k, 1000 * k, 130.0 if k % 2 else 60.0) for k in range(1, 96)]
    assert max(v for op, v in by["step_extremes_stereo"]["schedule"] if op != "l") == 1000
    for name in ("step_headroom_up_mono", "step_headroom_down_mono"):
        r, t = case_defs.make_inputs(by[name])
        assert 1 - 2 ** -23 <= max(np.abs(r).max(), np.abs(t).max()) <= 1.0


@pytest.mark.parametrize("idx", range(len(_records())), ids=[_id(r) for r in _records()])
def test_oracle_follows_the_reference_across_level_changes(idx):
    """at the bound tests/test_oracle_golden.py holds the end-to-end and the constant-level records to"""
    rec = _records()[idx]
    got, _ = oracle_along(rec["case"])
    check_against_reference(got, rec, rtol=1e-9, atol=1e-9)
    # the record pins the schedule, not just the levels: at either constant level the result is another one
    exp = np.array([float(v) for v in rec["movs"]])
    for level in {rec["case"]["level"]} | {v for op, v in rec["case"]["schedule"] if op == "l"}:
        other, _ = oracle_along(rec["case"], schedule=[e for e in rec["case"]["schedule"] if e[0] != "l"], level=level)
        assert not np.allclose(other["movs"], exp, rtol=1e-6, atol=0, equal_nan=True), level


@pytest.mark.parametrize("case", [c for c in case_defs.level_step_cases() if not c["advanced"]],
                         ids=lambda c: c["name"])
def test_reldistframes_is_off_its_threshold(case):
    """As for the severe cases (tests/test_severe_cases_host.py): a condition on the INPUTS.  RelDistFrames counts the
    frames whose largest band noise-to-mask ratio exceeds 1.5 dB (movs.c:1021-1023); no frame of any case, run along
    its schedule in the oracle, comes nearer to that threshold than 0.1 dB.  Two cases took other seeds for it
    (tests/cases.py:level_step_cases)."""
    _, trace = oracle_along(case, trace_frames=93)
    with np.errstate(divide="ignore"):
        db = 10 * np.log10(trace["nmr_max"])
    fin = np.isfinite(db)
    assert fin.sum() >= 80 * case["channels"]
    margin = np.abs(db[fin] - 1.5).min()
    print(f"{case['name']}: nearest frame {margin:.3f} dB from the 1.5 dB threshold")
    assert margin >= 0.1, margin


# ---- the ear models alone across one step ------------------------------------------------------------------

@pytest.mark.parametrize("bands", [109, 55])
@pytest.mark.parametrize("sig", ["synth5_ref", "synth5_test"])
def test_fft_ear_stages_across_a_level_step(bands, sig):
    """bounds: those of test_fft_ear_stages_match_reference (tests/test_oracle_golden.py)"""
    g = np.load(GOLD / "ref_stages_level_step.npz")
    st = case_defs.LEVEL_STEP_STAGE
    x = case_defs.level_step_stage_inputs()[sig]
    out = orc.fftear(bands, x, st["frames"], 1024, level=st["level"], steps=[(st["frame"], st["to"])])
    for k in ("unsmeared", "excitation", "loudness"):
        np.testing.assert_allclose(out[k], g[f"fft{bands}_{sig}_{k}"], rtol=1e-10, err_msg=k)
    assert np.array_equal(out["energy"], g[f"fft{bands}_{sig}_energy"])
    if bands == 109 and sig == "synth5_ref":
        near = slice(st["frame"] - 3, st["frame"] + 4)
        for k in ("power", "weighted"):
            a, b = g[f"fft_{sig}_{k}_near"], g[f"fft_{sig}_{k}_far"]
            assert a.shape == (7, 1025) and b.shape == (st["frames"], 257)
            # (atol relative to the largest bin of the FRAME: the spectra on the two sides of the step are 20 dB apart)
            for f in range(7):
                np.testing.assert_allclose(out[k][near][f], a[f], rtol=1e-9, atol=1e-13 * a[f].max(), err_msg=f"{k} {f}")
            for f in range(st["frames"]):
                np.testing.assert_allclose(out[k][f, ::4], b[f], rtol=1e-9, atol=1e-13 * out[k][f].max(), err_msg=f"{k} {f}")
    # the fixture crosses the step: in front of it the run at the old level, bit for bit; behind it the spectra and the
    # unsmeared patterns (no memory) of a run at the new level, the excitation still carrying the quieter frames' smearing
    old = orc.fftear(bands, x, st["frames"], 1024, level=st["level"])
    new = orc.fftear(bands, x, st["frames"], 1024, level=st["to"])
    f = st["frame"]
    for k in ("power", "unsmeared", "excitation"):
        assert np.array_equal(out[k][:f], old[k][:f]), k
    assert np.array_equal(out["power"][f:], new["power"][f:]) and np.array_equal(out["unsmeared"][f:], new["unsmeared"][f:])
    assert (out["excitation"][f] <= new["excitation"][f]).all()
    assert (out["excitation"][f] < new["excitation"][f] * (1 - 1e-3)).any()


@pytest.mark.parametrize("sig", ["synth5_ref", "synth5_test"])
def test_filterbank_stages_across_a_level_step(sig):
    """bound: that of test_filterbank_stages_match_reference"""
    g = np.load(GOLD / "ref_stages_level_step.npz")
    st = case_defs.LEVEL_STEP_STAGE
    x = case_defs.level_step_stage_inputs()[sig]
    out = orc.fbear(x, st["blocks"], level=st["level"], steps=[(st["block"], st["to"])])
    for k in ("unsmeared", "excitation", "loudness"):
        assert g[f"fb_{sig}_{k}"].shape[0] == st["blocks"]
        np.testing.assert_allclose(out[k], g[f"fb_{sig}_{k}"], rtol=1e-11, err_msg=k)
    old = orc.fbear(x, st["blocks"], level=st["level"])
    new = orc.fbear(x, st["blocks"], level=st["to"])
    b = st["block"]
    assert np.array_equal(out["excitation"][:b], old["excitation"][:b])
    # the FIR windows of the first blocks behind the step reach back into samples scaled at the old level (the longest
    # filter spans 1456 samples, 7.6 blocks), and the smearing's memory is longer still
    assert not np.allclose(out["unsmeared"][b], new["unsmeared"][b], rtol=1e-3)
    assert not np.allclose(out["excitation"][b + 8], new["excitation"][b + 8], rtol=1e-3)


# ---- identities of the oracle ------------------------------------------------------------------------------

def _same(a, b):
    return (a["movs"].tobytes() == b["movs"].tobytes() and a["frames"] == b["frames"]
            and np.array([a["di"], a["odg"], a["totalsnr"]]).tobytes() == np.array([b["di"], b["odg"], b["totalsnr"]]).tobytes())


@pytest.mark.parametrize("advanced", [0, 1])
def test_oracle_identities(advanced):
    case = [c for c in case_defs.level_step_cases() if c["name"] == "step_up_stereo" and c["advanced"] == advanced][0]
    pushes = [e for e in case["schedule"] if e[0] != "l"]
    plain, _ = oracle_along(case, schedule=pushes)
    # a set to the level the session already has, before every push: nothing changes, bit for bit
    again, _ = oracle_along(case, schedule=[e for p in pushes for e in (["l", case["level"]], p)])
    assert _same(plain, again)
    # a set before the first push equals creation at that level
    created, _ = oracle_along(case, schedule=pushes, level=112.0)
    set_first, _ = oracle_along(case, schedule=[["l", 112.0]] + pushes, level=60.0)
    assert _same(created, set_first) and not _same(created, plain)
    # a set after the flush changes no result
    ref, test = case_defs.make_inputs(case)
    s = orc.Session(advanced, case["channels"], case["level"])
    case_defs.run_schedule(s, ref, test, case["schedule"])
    s.flush()
    before = s.results()
    s.set_level(130.0)
    after = s.results()
    s.flush()                                          # (nothing is left to flush)
    assert _same(before, after) and _same(before, s.results())
    s.close()
    stepped, _ = oracle_along(case)
    assert _same(before, stepped) and not _same(stepped, plain)

"""The oracle's back ends on records (tests/oracle_lib.py backend_records*), pinned to its sample path: the records of
a pair carry exactly the doubles the sample path computes between its two steps, so the result and the per-frame
trace must be the sample path's bit for bit -- any difference is a bug in the split.  Then every scenario of
tests/backend_scenarios.py is held to the conditions its name states, in the oracle, so that none of them can stop
exercising its gate unnoticed.  No GPU."""
import numpy as np
import pytest

import backend_scenarios as scn
import cases as case_defs
import oracle_lib as orc

PIN_CASES = [
    dict(kind="synth", seed=5, channels=1, n=72000),
    dict(kind="synth", seed=6, channels=2, n=60000, test_trim=900),
    dict(kind="synth", seed=1, channels=2, n=60000),             # leading digital silence
    dict(kind="synth", seed=9, channels=2, n=40000, atten_shift=9),   # around the detector thresholds
    dict(kind="synth", seed=26, channels=2, n=40000, identical=1),
    dict(kind="synth", seed=41, channels=2, n=60000, gaps=[(20000, 9000), (40000, 3000)]),   # silence in mid-stream
    *case_defs.severe_stage_cases(),
]
PIN_IDS = ["mono", "stereo-ragged", "lead-silence", "quiet", "identical", "mid-gaps", *case_defs.SEVERE_STAGE_NAMES]


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same_result(got, exp):
    assert got["frames"] == exp["frames"]
    assert np.array_equal(np.isnan(got["movs"][:len(exp["movs"])]), np.isnan(exp["movs"]))
    for k in ("movs", "di", "odg", "totalsnr"):
        g = got[k][:len(exp[k])] if k == "movs" else got[k]
        assert same_bits(g, exp[k]), (k, g, exp[k])


@pytest.mark.parametrize("case", PIN_CASES, ids=PIN_IDS)
def test_basic_records_path_is_the_sample_path(case):
    ref, test = case_defs.make_inputs(case)
    n_frames = orc.count_frames(len(ref), len(test))
    exp = orc.run_pair(0, ref, test)
    assert exp["frames"] == n_frames
    got = orc.backend_records(orc.frontend_records(109, ref, test, n_frames))
    assert_same_result(got, exp)
    trace = orc.mov_trace(ref, test, n_frames)
    for name in orc.MOV_TRACE:
        assert same_bits(got["trace"][name], trace[name]), name


@pytest.mark.parametrize("case", PIN_CASES, ids=PIN_IDS)
def test_advanced_records_path_is_the_sample_path(case):
    ref, test = case_defs.make_inputs(case)
    n_frames, n_blocks = orc.count_frames(len(ref), len(test)), orc.count_blocks(len(ref), len(test))
    exp = orc.run_pair(1, ref, test)
    assert exp["frames"] == n_frames
    got = orc.backend_records_advanced(orc.fb_records(ref, test, n_blocks), orc.frontend_records(55, ref, test, n_frames))
    assert_same_result(got, exp)
    eblk, efrm = orc.mov_trace_advanced(ref, test, n_blocks, n_frames)
    for name in orc.MOV_TRACE_ADV_BLOCK:
        assert same_bits(got["trace_blocks"][name], eblk[name]), name
    for name in orc.MOV_TRACE_ADV_FRAME:
        assert same_bits(got["trace_frames"][name], efrm[name]), name


@pytest.mark.parametrize("advanced", [0, 1], ids=["basic", "advanced"])
@pytest.mark.parametrize("field", orc.SETTINGS_FIELDS)
def test_settings_act_on_the_records_path_as_on_the_sample_path(field, advanced):
    """each settings.h switch flipped: the records path is still the sample path, bit for bit (the switches of the ear
    models and of EHS act where the records are made, the others in the second step)"""
    ref, test = case_defs.make_inputs(PIN_CASES[0])
    n_frames, n_blocks = orc.count_frames(len(ref), len(test)), orc.count_blocks(len(ref), len(test))
    orc.set_settings(**{field: 1 - orc.SETTINGS_DEFAULT[field]})
    try:
        exp = orc.run_pair(advanced, ref, test)
        if advanced:
            got = orc.backend_records_advanced(orc.fb_records(ref, test, n_blocks),
                                               orc.frontend_records(55, ref, test, n_frames))
        else:
            got = orc.backend_records(orc.frontend_records(109, ref, test, n_frames))
    finally:
        orc.set_settings()
    assert_same_result(got, exp)


def test_floor_setting_doubles_the_steps_of_the_minus_1_5_dB_scenario():
    """-1.5 dB: trunc() gives one step per band, floor() two (movs.c:1256-1260), so ADB moves by log10(2)"""
    by = {s[0]: s for s in scn.basic_scenarios()}
    plain = orc.backend_records(by["E-minus-1.5dB"][1])
    orc.set_settings(**by["E-minus-1.5dB-floor"][2]["settings"])
    try:
        floored = orc.backend_records(by["E-minus-1.5dB-floor"][1])
    finally:
        orc.set_settings()
    assert abs(floored["movs"][scn.ADB] - plain["movs"][scn.ADB] - np.log10(2.)) < 1e-12


# ---------------------------------------------------------------------------
# the scenarios of tests/backend_scenarios.py: conditions on the inputs, asserted from the oracle's own trace
# ---------------------------------------------------------------------------


def gate_conditions(loud_ref, loud_test, evaluated, want, n):
    """loud_* [frames, channels]: the gate's two loudness values; evaluated [frames]: the frames that began with the
    gate closed.  The gate opens on frame `want` (None: never), and while it is closed -- the opening frame
    included -- every value is at least 1 % away from 0.1 sone."""
    frames = np.flatnonzero(evaluated)
    last = n - 1 if want is None else want
    assert np.array_equal(frames, np.arange(last + 1)), (frames, want)
    both = np.stack([loud_ref[frames], loud_test[frames]])
    assert np.all(np.abs(both - 0.1) >= 0.001), both
    opened = ((loud_ref[frames] > 0.1) & (loud_test[frames] > 0.1)).any(1)
    assert np.array_equal(np.flatnonzero(opened), [] if want is None else [want]), (np.flatnonzero(opened), want)


def nan_places(movs, notes):
    assert sorted(np.flatnonzero(np.isnan(movs)).tolist()) == sorted(notes["nan"]), (movs, notes["nan"])


@pytest.fixture
def settings_of():
    def apply(notes):
        orc.set_settings(**notes.get("settings", {}))
    yield apply
    orc.set_settings()


@pytest.mark.parametrize("idx", range(len(scn.basic_scenarios())), ids=[s[0] for s in scn.basic_scenarios()])
def test_basic_scenario_sits_where_it_says(idx, settings_of):
    name, rec, notes = scn.basic_scenarios()[idx]
    assert rec.shape[1] == notes["channels"] and rec.shape[0] <= 140
    settings_of(notes)
    o = orc.backend_records(rec)
    n = rec.shape[0]
    gate = o["gate"]
    gate_conditions(gate[:, :, 0], gate[:, :, 1], ~np.isnan(gate[:, 0, 0]), notes.get("gate", 0), n)
    nan_places(o["movs"], notes)
    notes["check"](o)


@pytest.mark.parametrize("idx", range(len(scn.advanced_scenarios())), ids=[s[0] for s in scn.advanced_scenarios()])
def test_advanced_scenario_sits_where_it_says(idx, settings_of):
    name, fb, ff, notes = scn.advanced_scenarios()[idx]
    assert fb.shape[1] == ff.shape[1] == notes["channels"] and fb.shape[0] <= 160 and ff.shape[0] <= 30
    settings_of(notes)
    o = orc.backend_records_advanced(fb, ff)
    gate = o["gate"]
    gate_conditions(gate[:, :, 0], gate[:, :, 1], ~np.isnan(gate[:, 0, 0]), notes.get("gate", 0), fb.shape[0])
    nan_places(o["movs"], notes)
    notes["check"](o)

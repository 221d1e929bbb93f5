"""Severe degradation (tests/cases.py:severe_cases): the generator, the population the real reference's goldens
must keep, the distance of the one discrete MOV decision that can be checked here (RelDistFrames) from its threshold.
CPU only.  The oracle against the 40 new records: tests/test_oracle_golden.py picks them up by itself."""
import json
import math

import numpy as np
import pytest

import cases as case_defs
import oracle_lib as orc

ROWS = ("sev_quant2", "sev_quant3", "sev_box8x3", "sev_hold4", "sev_box8x3_quant3", "sev_hold4_quant3", "sev_dropouts",
        "sev_foreign", "sev_silent_test", "sev_overdriven")
NAMES = [f"{r}_{c}" for r in ROWS for c in ("stereo", "mono")]
RESEEDED = {"sev_quant2_stereo": 64, "sev_quant2_mono": 65, "sev_quant3_stereo": 68}   # see test_reldistframes_...
CASES = case_defs.severe_cases()


@pytest.fixture(scope="module")
def records(golden_dir):
    recs = json.loads((golden_dir / "ref_e2e.json").read_text())
    return [r for r in recs if r["case"]["name"] in NAMES]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def test_case_list():
    assert [c["name"] for c in CASES] == NAMES and len(set(NAMES)) == 20
    for c in CASES:
        stereo = c["name"].endswith("_stereo")
        assert c["kind"] == "synth" and c["n"] == 48000 and c["from_ref"] == 1
        assert c["channels"] == (2 if stereo else 1)
        assert c["seed"] == RESEEDED.get(c["name"], 60 if stereo else 61)
    for adv in (0, 1):
        assert [c["name"] for c in case_defs.e2e_cases() if c["advanced"] == adv][-20:] == NAMES


@pytest.mark.parametrize("case", CASES, ids=NAMES)
def test_inputs_are_float32_and_reproducible(case):
    ref, test = case_defs.make_inputs(case)
    ref2, test2 = case_defs.make_inputs(dict(case))
    for a, b in ((ref, ref2), (test, test2)):
        assert a.dtype == np.float32 and a.shape == (48000, case["channels"]) and a.flags["C_CONTIGUOUS"]
        assert np.array_equal(_bits(a), _bits(b))
    # the pair's reference is that of the seeded pair, untouched by the degradations
    assert np.array_equal(_bits(ref), _bits(case_defs.synth_np.pair(case["seed"], case["channels"], 48000)[0]))
    assert np.isfinite(test).all() and np.abs(test).max() <= 1.0


def test_box8_against_a_scalar_loop():
    f = np.float32
    x = case_defs.synth_np.pair(60, 2, 64)[0]
    want = np.zeros_like(x)
    for c in range(2):
        for n in range(64):
            s = [x[n - j, c] if n - j >= 0 else f(0) for j in range(8)]
            want[n, c] = f(f(f(f(s[0] + s[1]) + f(s[2] + s[3])) + f(f(s[4] + s[5]) + f(s[6] + s[7]))) * f(0.125))
    got = case_defs.box8(x)
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want))
    assert x.any() and not np.array_equal(got, x)


def test_the_other_degradations_do_what_they_say():
    by = {c["name"]: c for c in CASES}
    ref, t = case_defs.make_inputs(by["sev_hold4_stereo"])
    assert np.array_equal(t, ref[4 * (np.arange(48000) // 4)])
    ref, t = case_defs.make_inputs(by["sev_quant2_mono"])
    assert np.array_equal(t * 4, np.round(t * 4)) and np.abs(t - ref).max() <= 0.125
    ref, t = case_defs.make_inputs(by["sev_overdriven_stereo"])
    assert np.array_equal(t, np.clip(ref * np.float32(10), -1, 1)) and (np.abs(t) == 1).mean() > 0.1
    ref, t = case_defs.make_inputs(by["sev_foreign_mono"])
    assert np.array_equal(_bits(t), _bits(case_defs.synth_np.pair(161, 1, 48000)[0])) and not np.array_equal(t, ref)
    ref, t = case_defs.make_inputs(by["sev_silent_test_stereo"])
    assert not t.any() and ref.any()
    ref, t = case_defs.make_inputs(by["sev_dropouts_mono"])
    gone = np.zeros(48000, bool)
    for s in range(2400, 48000, 4800):
        gone[s:s + 960] = True
    assert not t[gone].any() and np.array_equal(t[~gone], ref[~gone]) and gone.sum() == 9600


def test_goldens_hold_the_population(records):
    assert len(records) == 40
    basic = [r for r in records if not r["case"]["advanced"]]
    adv = [r for r in records if r["case"]["advanced"]]
    assert [r["case"]["name"] for r in basic] == NAMES and [r["case"]["name"] for r in adv] == NAMES
    assert all(r["frames"] == 46 for r in records) and all(r["fb_frames"] == 250 for r in adv)
    odg = np.array([float(r["odg"]) for r in basic])
    assert (odg < -2.2).sum() >= 9 and np.nanmin(odg) <= -3.8, odg
    di = np.array([float(r["di"]) for r in adv])
    assert (di == case_defs.DI_SATURATED).sum() >= 6, di
    assert ((np.abs(di - case_defs.DI_SATURATED) < 1e-4) & (di != case_defs.DI_SATURATED)).sum() >= 2, di
    # NaN results of pairs that are neither empty nor silent on both pads, where the table of the case set has them
    nan = {adv_: {r["case"]["name"] for r in recs if math.isnan(float(r["odg"]))} for adv_, recs in ((0, basic), (1, adv))}
    rows = lambda *names: {f"{n}_{c}" for n in names for c in ("stereo", "mono")}
    assert nan[0] == rows("sev_quant2", "sev_silent_test", "sev_overdriven")
    assert nan[1] == rows("sev_silent_test")
    for r in records:
        if math.isnan(float(r["odg"])):
            assert math.isnan(float(r["di"])) and any(math.isnan(float(v)) for v in r["movs"])
            assert case_defs.make_inputs(r["case"])[0].any()
    # basic NaN beside a finite advanced result
    assert not (rows("sev_quant2", "sev_overdriven") & nan[1])


@pytest.mark.parametrize("case", CASES, ids=NAMES)
def test_reldistframes_is_off_its_threshold(case):
    """RelDistFrames counts the frames whose largest band noise-to-mask ratio exceeds 1.5 dB (movs.c:1021-1023).  A
    condition on the INPUTS, not a tolerance: no frame of any case comes nearer to the threshold than 0.1 dB, many
    orders more than any rounding moves the ratio.  A case that misses it gets another seed (RESEEDED: at seeds 60 / 61
    the nearest frames of sev_quant2 stereo / mono and sev_quant3 stereo were 0.006 / 0.082 / 0.0996 dB away)."""
    ref, test = case_defs.make_inputs(case)
    nmr = orc.mov_trace(ref, test, 46)["nmr_max"]
    with np.errstate(divide="ignore"):
        db = 10 * np.log10(nmr)
    fin = np.isfinite(db)
    assert fin.sum() >= 40 * case["channels"]
    margin = np.abs(db[fin] - 1.5).min()
    print(f"{case['name']}: nearest frame {margin:.3f} dB from the 1.5 dB threshold")
    assert margin >= 0.1, margin


@pytest.mark.parametrize("bands", [109, 55])
def test_dropouts_frame_22_noise_is_ill_conditioned(bands):
    """The one per-frame quantity of the severe set that gets a bound of its own in the GPU stage tests (tests/cases.py,
    SEV_DROPOUTS_MONO_FRAME22_NOISE_MOVES): the figure recorded there is the oracle's own largest movement among the
    frame's bands, measured here; the GPU test takes each band's own."""
    case = next(c for c in CASES if c["name"] == "sev_dropouts_mono")
    ref, test = case_defs.make_inputs(case)
    assert not test[22528:22560].any() and np.array_equal(test[22560:24576], ref[22560:24576])
    a = orc.frontend_records(bands, ref, test, 46)[:, 0, 448:448 + bands]
    b = orc.frontend_records(bands, ref, case_defs.ulp_perturbed(test), 46)[:, 0, 448:448 + bands]
    move = np.abs(b - a) / a
    recorded = case_defs.SEV_DROPOUTS_MONO_FRAME22_NOISE_MOVES[bands]
    print(f"{bands} bands: noise of frame 22 moves by up to {move[22].max():.3e}")
    assert 0.98 * recorded <= move[22].max() <= 1.02 * recorded
    assert 2e-5 < np.median(move[22]) < 6e-5 and move[22].min() > 1e-7     # every band of the frame is affected
    # and no other frame whose noise is not the floor of identical signals moves as much
    others = np.where(a != orc.BAND_POWER_FLOOR, move, 0)
    others[22] = 0
    assert others.max() < 0.25 * move[22].max()

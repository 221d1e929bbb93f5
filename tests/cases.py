"""Parity case definitions shared by tools/make_golden.py (which runs the REAL
reference on them in the build container) and by the tests (which run the
oracle / the HIP path on the same inputs).  A case is a small dict; inputs are
rebuilt from it deterministically."""
import numpy as np

import synth_np


def make_inputs(case):
    """-> (ref, test): float32 [n, channels] arrays (lengths may differ)."""
    kind = case["kind"]
    ch = case.get("channels", 1)
    if kind == "raw":                                  # the caller's own samples on both pads
        return case["_x"], case["_x"].copy()
    if kind == "synth":
        ref, test = synth_np.pair(case["seed"], ch, case["n"])
        if case.get("identical") or case.get("from_ref"):   # from_ref: the degradations below make the test signal
            test = ref.copy()
        if case.get("swap"):
            ref, test = test, ref
        sh = case.get("atten_shift", 0)
        if sh:
            ref = ref * np.float32(2.0 ** -sh)
            test = test * np.float32(2.0 ** -sh)
        ref = ref[: case["n"] - case.get("ref_trim", 0)]
        test = test[: case["n"] - case.get("test_trim", 0)]
        ref, test = np.ascontiguousarray(ref), np.ascontiguousarray(test)
        # input classes beyond "a clean pair" (all float32 arithmetic, in this order)
        if case.get("chan_gain"):                      # channels at different levels (binaural maxima, movs.c:1224-1276)
            g = np.asarray(case["chan_gain"], dtype=np.float32)[None, :]
            ref, test = ref * g, test * g
        if case.get("gain"):                           # drive into full scale ...
            ref, test = ref * np.float32(case["gain"]), test * np.float32(case["gain"])
        # severe degradations of the test signal alone: element-wise float32 operations in a fixed association, so
        # that the bits are the same on every machine (no convolve / dot, whose summation order the library chooses)
        for _ in range(case.get("box8_test", 0)):
            test = box8(test)
        if case.get("hold_test"):                      # sample-and-hold
            h = case["hold_test"]
            test = test[h * (np.arange(len(test)) // h)]
        if case.get("quant_test"):                     # requantise to steps of 2^-k
            q = np.float32(2 ** case["quant_test"])
            test = np.round(test * q) / q
        if case.get("test_gain"):                      # overdrive the test signal only ...
            test = test * np.float32(case["test_gain"])
        if case.get("clip"):                           # ... and clip hard: "both" or "test"
            if case["clip"] == "both":
                ref = np.clip(ref, np.float32(-1), np.float32(1))
            test = np.clip(test, np.float32(-1), np.float32(1))
        if case.get("foreign_test"):                   # an unrelated programme on the test pad
            test = synth_np.pair(case["seed"] + 100, ch, case["n"])[0]
        if case.get("silent_test"):
            test = np.zeros_like(test)
        if case.get("dc_ref"):
            ref = ref + np.float32(case["dc_ref"])
        if case.get("dc_test"):
            test = test + np.float32(case["dc_test"])
        if case.get("invert_test"):
            test = -test
        for start, length in case.get("gaps", ()):     # digital silence in mid-stream (NORMAL -> TENTATIVE -> NORMAL in the
            who = case.get("gap_who", "both")          # accumulators, movaccum.c:317-352; the detector looks at ref only)
            if who in ("both", "ref"):
                ref[start:start + length] = 0
            if who in ("both", "test"):
                test[start:start + length] = 0
        return np.ascontiguousarray(ref, dtype=np.float32), np.ascontiguousarray(test, dtype=np.float32)
    if kind == "ats":
        ref = synth_np.audiotestsrc(case["wave_ref"], case["n"])
        test = synth_np.audiotestsrc(case["wave_test"], case["n"])
        if ch == 2:
            ref = np.repeat(ref, 2, axis=1)
            test = np.repeat(test, 2, axis=1)
        return ref, test
    if kind == "silence":
        z = np.zeros((case["n"], ch), dtype=np.float32)
        return z, z.copy()
    raise ValueError(kind)


def box8(x):
    """One pass of the 8-tap mean over [n, channels] float32, zero history: every sum in float32, in this association."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = len(x)
    p = np.concatenate([np.zeros((7,) + x.shape[1:], np.float32), x])
    s = [p[7 - j:7 - j + n] for j in range(8)]       # s[j][n] = x[n - j]
    return (((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]))) * np.float32(0.125)


def e2e_cases():
    """End-to-end cases run through the reference element."""
    cases = []
    for adv in (0, 1):
        # the reference's own regression pipelines (runtest-1.0.sh); basic ODGs 0.171 / -2.007
        cases.append(dict(name="ats_sine_identical", kind="ats", wave_ref="sine", wave_test="sine", n=131072, channels=1))
        cases.append(dict(name="ats_saw_triangle", kind="ats", wave_ref="saw", wave_test="triangle", n=131072, channels=1))
        cases.append(dict(name="ats_saw_triangle_stereo", kind="ats", wave_ref="saw", wave_test="triangle", n=65536, channels=2))
        for seed in range(8):
            cases.append(dict(name=f"synth_s{seed}_stereo", kind="synth", seed=seed, channels=2, n=120000))
        for seed in (10, 11, 12, 13):
            cases.append(dict(name=f"synth_s{seed}_mono", kind="synth", seed=seed, channels=1, n=72000))
        cases.append(dict(name="synth_10s_stereo", kind="synth", seed=42, channels=2, n=480000))
        cases.append(dict(name="synth_ragged_test_short", kind="synth", seed=21, channels=2, n=100000, test_trim=1500))
        cases.append(dict(name="synth_ragged_ref_short", kind="synth", seed=22, channels=1, n=100000, ref_trim=700))
        cases.append(dict(name="synth_sub_frame", kind="synth", seed=23, channels=2, n=1500))
        cases.append(dict(name="synth_exact_frame", kind="synth", seed=24, channels=1, n=2048))
        cases.append(dict(name="synth_frame_and_hop", kind="synth", seed=25, channels=2, n=3072))
        cases.append(dict(name="synth_identical", kind="synth", seed=26, channels=2, n=96000, identical=1))
        cases.append(dict(name="synth_swapped", kind="synth", seed=27, channels=2, n=96000, swap=1))
        cases.append(dict(name="synth_quiet_36dB", kind="synth", seed=28, channels=2, n=96000, atten_shift=6))
        cases.append(dict(name="synth_quiet_60dB", kind="synth", seed=29, channels=1, n=96000, atten_shift=10))
        cases.append(dict(name="synth_quiet_84dB", kind="synth", seed=30, channels=2, n=96000, atten_shift=14))
        cases.append(dict(name="silence", kind="silence", channels=2, n=48000))
        cases += input_class_cases()
        cases += severe_cases()
        for c in cases:
            c.setdefault("advanced", adv)
    return cases


def input_class_cases():
    """Input classes a clean seeded pair does not reach (round 6): digital silence in MID-stream -- one gap, three
    gaps, whole frames and parts of frames, in both signals / the reference only / the test only --, hard clipping at
    full scale, DC offsets, a polarity-inverted test signal, channels 40 dB apart."""
    one, three = [(40000, 20000)], [(20000, 6000), (50000, 12000), (90000, 3000)]
    return [
        dict(name="gap1_stereo", kind="synth", seed=40, channels=2, n=120000, gaps=one),
        dict(name="gap3_stereo", kind="synth", seed=41, channels=2, n=120000, gaps=three),
        dict(name="gap1_mono", kind="synth", seed=42, channels=1, n=120000, gaps=one),
        dict(name="gap3_mono", kind="synth", seed=43, channels=1, n=120000, gaps=three),
        dict(name="gap3_ref_only_stereo", kind="synth", seed=44, channels=2, n=120000, gaps=three, gap_who="ref"),
        dict(name="gap1_test_only_mono", kind="synth", seed=45, channels=1, n=120000, gaps=one, gap_who="test"),
        dict(name="clip_both_stereo", kind="synth", seed=46, channels=2, n=96000, gain=6.0, clip="both"),
        dict(name="clip_test_mono", kind="synth", seed=47, channels=1, n=96000, gain=3.0, clip="test"),
        dict(name="dc_offsets_stereo", kind="synth", seed=48, channels=2, n=96000, dc_ref=0.05, dc_test=-0.125),
        dict(name="inverted_test_stereo", kind="synth", seed=49, channels=2, n=96000, invert_test=1),
        dict(name="channels_40dB_apart", kind="synth", seed=50, channels=2, n=96000, chan_gain=[1.0, 0.01]),
    ]


DI_SATURATED = -2.3424810000000003      # advanced DI: the output bias + the weights of the hidden units that sit at exactly 1


def severe_cases():
    """Severe degradation, below the ODG -2.2 at which the seeded pairs' own degradation saturates: down to the ODG
    formula's floor, the advanced DI at its saturated value (every hidden sigmoid exactly 0 or 1), and MOV accumulators
    that never receive a frame (NaN MOV, DI and ODG in pairs that are neither empty nor silent).  1 s each (46 frames,
    250 filter-bank blocks); the test signal is made from the pair's reference."""
    drop = [(s, 960) for s in range(2400, 48000, 4800)]
    # (name, degradation, seeds stereo / mono).  Seeds 60 / 61, except where a frame of that pair has its largest
    # noise-to-mask ratio within 0.1 dB of RelDistFrames' 1.5 dB threshold (tests/test_severe_cases_host.py: 0.006,
    # 0.082 and 0.0996 dB for the first three below at 60 / 61 / 60); those take the first seed from 62 upwards that
    # keeps the margin and the row's pattern of NaN results, one seed per case.
    rows = [
        ("sev_quant2", dict(quant_test=2), (64, 65)),
        ("sev_quant3", dict(quant_test=3), (68, 61)),
        ("sev_box8x3", dict(box8_test=3), (60, 61)),
        ("sev_hold4", dict(hold_test=4), (60, 61)),
        ("sev_box8x3_quant3", dict(box8_test=3, quant_test=3), (60, 61)),
        ("sev_hold4_quant3", dict(hold_test=4, quant_test=3), (60, 61)),
        ("sev_dropouts", dict(gaps=drop, gap_who="test"), (60, 61)),
        ("sev_foreign", dict(foreign_test=1), (60, 61)),
        ("sev_silent_test", dict(silent_test=1), (60, 61)),
        ("sev_overdriven", dict(test_gain=10, clip="test"), (60, 61)),
    ]
    cases = []
    for name, keys, (stereo, mono) in rows:
        cases.append(dict(name=f"{name}_stereo", kind="synth", seed=stereo, channels=2, n=48000, from_ref=1, **keys))
        cases.append(dict(name=f"{name}_mono", kind="synth", seed=mono, channels=1, n=48000, from_ref=1, **keys))
    return cases


SEVERE_STAGE_NAMES = ("sev_hold4_stereo", "sev_box8x3_mono", "sev_quant2_stereo", "sev_foreign_stereo", "sev_dropouts_mono",
                      "sev_overdriven_stereo", "sev_silent_test_mono")


# sev_dropouts_mono, FFT frame 22 (samples 22528 .. 24575): the dropout 21600 .. 22559 covers only the frame's first 32
# samples, where the Hann window is below 2.5e-3, so every band's noise Pr - 2 sqrt(Pr Pt) + Pt is what is left of two
# nearly equal spectra.  Moving 1 % of the test signal's samples by one float32 ulp (ulp_perturbed below) moves the
# ORACLE's own noise in the bands of that frame by up to this much, relative, per band count -- measured on the CPU,
# tests/test_severe_cases_host.py.  The stage test holds each band of that frame to 4 x the band's own movement, and
# every other frame to its usual 1e-6.
SEV_DROPOUTS_MONO_FRAME22_NOISE_MOVES = {109: 2.32e-3, 55: 4.97e-4}


def ulp_perturbed(x, seed=0, share=0.01):
    """x [n, channels] float32 with `share` of its rows moved one ulp upwards: the probe of a quantity's conditioning"""
    idx = np.random.default_rng(seed).choice(len(x), int(len(x) * share), replace=False)
    y = x.copy()
    y[idx] = np.nextafter(x[idx], np.float32(np.inf))
    return y


def severe_stage_cases():
    """the severe cases the stage-level tests walk through (a failure end to end must say where it comes from)"""
    by = {c["name"]: c for c in severe_cases()}
    return [by[n] for n in SEVERE_STAGE_NAMES]


def level_cases():
    """playback_level other than the default (the level enters both ear models' input scaling)"""
    cases = []
    for adv in (0, 1):
        for level, seed in ((60.0, 3), (75.5, 4), (105.0, 5), (130.0, 6)):
            cases.append(dict(name=f"synth_s{seed}_L{level:g}", kind="synth", seed=seed, channels=2, n=96000,
                              level=level, advanced=adv))
    return cases


def resampled_cases():
    """pairs at other sampling rates than 48 kHz, which the reference's CLI takes through audioresample
    (peaq.c:154-209): the samples of a seeded pair, declared to run at `rate`"""
    cases = []
    for adv in (0, 1):
        for rate, channels, seed, seconds in ((44100, 2, 31, 4), (44100, 1, 32, 4), (32000, 2, 33, 4), (96000, 1, 34, 3)):
            cases.append(dict(name=f"synth_s{seed}_{rate}Hz", kind="synth", seed=seed, channels=channels,
                              n=rate * seconds, rate=rate, advanced=adv))
    return cases


def settings_cases():
    """cases for the settings.h variants of the reference (tests/golden/ref_e2e_settings.json)"""
    cases = []
    for adv in (0, 1):
        cases.append(dict(name="ats_saw_triangle", kind="ats", wave_ref="saw", wave_test="triangle", n=131072,
                          channels=1, advanced=adv))
        cases.append(dict(name="synth_s1_stereo", kind="synth", seed=1, channels=2, n=120000, advanced=adv))
        cases.append(dict(name="synth_s12_mono", kind="synth", seed=12, channels=1, n=72000, advanced=adv))
        cases.append(dict(name="synth_quiet_36dB", kind="synth", seed=28, channels=2, n=96000, atten_shift=6,
                          advanced=adv))
    return cases


def stage_inputs():
    """Mono signals for the stage-level dumps (ear models)."""
    ref, test = synth_np.pair(5, 1, 8192)
    return {"synth5_ref": ref[:, 0].copy(), "synth5_test": test[:, 0].copy()}

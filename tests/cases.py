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
        if case.get("peak_to"):                        # ... or exactly to it: the pair's largest |sample| becomes peak_to
            g = np.float32(case["peak_to"]) / max(np.abs(ref).max(), np.abs(test).max())
            ref, test = ref * g, test * g
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
    """playback_level other than the default (the level enters both ear models' input scaling): the eight stereo cases
    at 60 .. 130 dB first, then the lower end of the property's range 0 .. 130 (gstpeaq.c:275-281) and the two ends of
    the first eight in mono.  At 0 dB a loudness gate may never open: NaN results are recorded as the reference gives
    them."""
    cases = []
    for adv in (0, 1):
        for level, seed in ((60.0, 3), (75.5, 4), (105.0, 5), (130.0, 6)):
            cases.append(dict(name=f"synth_s{seed}_L{level:g}", kind="synth", seed=seed, channels=2, n=96000,
                              level=level, advanced=adv))
    for adv in (0, 1):
        for level, seed in ((0.0, 7), (30.0, 8), (45.0, 9)):
            cases.append(dict(name=f"synth_s{seed}_L{level:g}", kind="synth", seed=seed, channels=2, n=96000,
                              level=level, advanced=adv))
        for level, seed in ((60.0, 14), (130.0, 15)):
            cases.append(dict(name=f"synth_s{seed}_L{level:g}_mono", kind="synth", seed=seed, channels=1, n=96000,
                              level=level, advanced=adv))
    return cases


LEVEL_STEP_N = 96000        # 93 frames, 500 blocks: frame 24, block 125 and the loudness gates are behind the steps
LEVEL_STEP_AT = 48128       # = 47 * 1024: frames 0 .. 45 and blocks 0 .. 249 lie wholly in front of it


def level_schedule(n, chunk, sets, lead=0):
    """A schedule for tests/cases.py:level_step_cases(): a list of ["r", count], ["t", count] (push that many samples per
    channel on the ref / test pad) and ["l", level] (set the playback level).  Both pads are pushed alternately, ref
    first, in buffers of `chunk` samples that are cut at each position of `sets` = [(sample, level), ...]; the level is
    set once the test pad stands at `sample` and the ref pad `lead` samples further (or at its end)."""
    out, pos = [], [0, 0]
    for at, level in list(sets) + [(n, None)]:
        goal = [min(n, at + lead), at]
        while pos[0] < goal[0] or pos[1] < goal[1]:
            for p in (0, 1):
                step = min(chunk, goal[p] - pos[p])
                if step > 0:
                    out.append(["rt"[p], step])
                    pos[p] += step
        if level is not None:
            out.append(["l", float(level)])
    return out


def schedule_string(schedule):
    """the form oracle/ref_harness.c's `sched` mode reads: r:4096,t:4096,l:112,..."""
    return ",".join(f"{op}:{v if op != 'l' else repr(float(v))}" for op, v in schedule)


def run_schedule(session, ref, test, schedule, after_push=None):
    """drive a session (the oracle's or the HIP one: push_ref / push_test / set_level) along a schedule; after_push is
    called behind every push"""
    pos = {"r": 0, "t": 0}
    for op, v in schedule:
        if op == "l":
            session.set_level(v)
            continue
        x = ref if op == "r" else test
        (session.push_ref if op == "r" else session.push_test)(x[pos[op]:pos[op] + v])
        pos[op] += v
        if after_push:
            after_push()
    assert pos["r"] == len(ref) and pos["t"] == len(test), pos


def level_step_cases():
    """The playback level changed in mid-stream (gstpeaq.c:508-515): `level` is the level the element starts at,
    `schedule` what follows (level_schedule).  Recorded by tools/make_golden.py level_steps from the reference element
    driven on one thread, so that the schedule alone decides which frame and block sees which level.

      up / down       92 -> 112 / 60 dB after sample 48128 of both pads, buffers of 4096: a step of +20 / -32 dB into
                      running state (smeared excitation, adapters, high-pass state, the filter bank's FIR tail)
      waiting         the ref pad stands 5000 samples further than the test pad at the change: the four frames and 26
                      blocks that wait for the test pad take the new level
      extremes        buffers of 1000 samples on each pad, the level alternating 60 / 130 dB from one round (ref, then
                      test) to the next: every launch of a session has another level than the one before
      low             92 -> 0 dB at 48128 and back to 92 dB 10000 samples later
      flush_only      the level changes behind the last push: the flush frame alone takes it (500 whole blocks: the
                      filter bank has no flush block)
      headroom_up / headroom_down
                      a pair whose largest sample is at full scale (1 to a float32 rounding), 60 -> 130 / 130 -> 60 dB at 48128: the FIR
                      window behind the step holds a tail filtered at a level 70 dB away

    Seeds: 70 .. 79 in the table's order, except where a frame of the basic version, run along the schedule in the
    oracle, has its largest noise-to-mask ratio within 0.1 dB of RelDistFrames' 1.5 dB threshold
    (tests/test_level_steps_host.py).  Those take the first seed from 80 upwards that keeps the margin, one seed per
    case: step_down_stereo 81 (73 came to 0.048 dB, 80 to 0.010 dB), step_waiting_stereo 83 (74: 0.005 dB,
    82: 0.029 dB)."""
    n, at = LEVEL_STEP_N, LEVEL_STEP_AT
    rounds = -(-n // 1000)
    rows = [
        ("up_mono", 70, 1, {}, 92.0, level_schedule(n, 4096, [(at, 112.0)])),
        ("up_stereo", 71, 2, {}, 92.0, level_schedule(n, 4096, [(at, 112.0)])),
        ("down_mono", 72, 1, {}, 92.0, level_schedule(n, 4096, [(at, 60.0)])),
        ("down_stereo", 81, 2, {}, 92.0, level_schedule(n, 4096, [(at, 60.0)])),
        ("waiting_stereo", 83, 2, {}, 92.0, level_schedule(n, 4096, [(at, 112.0)], lead=5000)),
        ("extremes_stereo", 75, 2, {}, 60.0,
         level_schedule(n, 1000, [(1000 * k, 130.0 if k % 2 else 60.0) for k in range(1, rounds)])),
        ("low_mono", 76, 1, {}, 92.0, level_schedule(n, 4096, [(at, 0.0), (at + 10000, 92.0)])),
        ("flush_only_stereo", 77, 2, {}, 92.0, level_schedule(n, 4096, [(n, 112.0)])),
        ("headroom_up_mono", 78, 1, dict(peak_to=1.0), 60.0, level_schedule(n, 4096, [(at, 130.0)])),
        ("headroom_down_mono", 79, 1, dict(peak_to=1.0), 130.0, level_schedule(n, 4096, [(at, 60.0)])),
    ]
    cases = []
    for adv in (0, 1):
        for name, seed, channels, keys, level, schedule in rows:
            cases.append(dict(name=f"step_{name}", kind="synth", seed=seed, channels=channels, n=n, level=level,
                              schedule=schedule, advanced=adv, **keys))
    return cases


# stage dumps across one step (tests/golden/ref_stages_level_step.npz): the ear models alone, mono, 92 -> 112 dB set
# before FFT frame 20 / filter-bank block 100, 40 frames / 200 blocks of the signals of stage_inputs()' pair run longer
LEVEL_STEP_STAGE = dict(level=92.0, to=112.0, frame=20, frames=40, block=100, blocks=200)


def level_step_stage_inputs():
    n = max((LEVEL_STEP_STAGE["frames"] - 1) * 1024 + 2048, LEVEL_STEP_STAGE["blocks"] * 192)
    ref, test = synth_np.pair(5, 1, n)
    return {"synth5_ref": ref[:, 0].copy(), "synth5_test": test[:, 0].copy()}


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

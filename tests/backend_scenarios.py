"""Hand-built records that put every discrete decision of the back ends on a chosen side of its gate.

A waveform cannot be steered onto a gate with a provable margin; a record can.  The back ends take records as they
stand (noise in bands, bandwidths, EHS, flags and energies untouched, excitations within 1e-13:
tests/test_gpu_backend_stage.py), so each scenario below is ONE neutral frame repeated, varied only in what the
scenario is about, and says in its notes which outcome that must have.  tests/test_backend_records_host.py holds
every scenario to its notes in the oracle (no GPU); tests/test_gpu_backend_gates.py runs the HIP back ends on them.

The neutral frame: a smooth excitation pattern, the test's 0.8 of the reference's times a slow spectral tilt (a plain
fraction leaves both noise loudness MOVs at zero on every frame, and their gate undecidable); both alternate
between two levels from frame to frame (the test less deeply, so that the modulation patterns differ and do not
cancel) unless the scenario needs the excitation exactly -- then both rise by 1 % per frame: with the smearing filter
starting from zero a rising input passes max(filtered, input) unchanged, and unlike a constant one it keeps the
modulation away from zero (there |L - L_prev| is what rounding leaves, and the modulation differences with it); noise at a tenth of the mask; bw_ref 500,
bw_test 400; EHS 0.01; flags 3 / 2 (above the boundary detector's threshold, energy bit of both signals).

A scenario is (name, records, notes) -- advanced: (name, fb_records, fft_records, notes) -- with notes:
  channels    1 or 2
  settings    settings.h switches that differ from the shipped values (oracle_lib.SETTINGS_FIELDS), or absent
  positions   the frames (blocks: block_positions) at which something is decided: where the launches are cut
  nan         the MOV indices that are NaN in the result, all others are not
  gate        the frame / block on which the loudness gate opens (None: never); absent: opens on frame 0
  steady      the smeared excitations are the records' own (see above)
  check       function(result of oracle_lib.backend_records*) asserting the scenario's named outcome
The sizes are the smallest at which each decision exists: at most 140 frames, or 160 blocks and 30 frames."""
import functools

import numpy as np

import oracle_lib as orc

NB, NB_ADV, NB_FB = 109, 55, 40
# front-end record (gstpeaq_amd/csrc/peaq_device.h kPub*)
R_UNSM_REF, R_UNSM_TEST, R_LOUD_REF, R_LOUD_TEST, R_NOISE = 0, 112, 224, 336, 448
R_BW_REF, R_BW_TEST, R_EHS, R_FL_REF, R_FL_TEST, R_SIG_E, R_NOISE_E = 560, 561, 562, 563, 564, 565, 566
# filter-bank record (kFbRec*)
B_UNSM_REF, B_UNSM_TEST, B_EXC_REF, B_EXC_TEST, B_FLAG = 0, 40, 80, 120, 160
# MOV indices (gstpeaq.c:86-108)
BW_REF, BW_TEST, NMR, WINMOD, ADB, EHS, AVGMOD1, AVGMOD2, NOISELOUD, MFPD, RELDIST = range(11)
A_RMSMOD, A_NLASYM, A_SEGNMR, A_EHS, A_LINDIST = range(5)

RATIO = 0.8                       # test / reference
LEVELS = ((1., 1.), (1.21, 1.1))   # (reference, test) level of even / odd frames
RISE = 1.01                       # steady scenarios: level of frame f + 1 over that of frame f
QUIET = 1e-5                      # quiet excitations: this times the neutral pattern (gate loudness well below 0.1 sone)
VOTE_M = 1e-9                     # scenario C's margin: 1e4 times the 1e-13 hand-built excitations are held to
VOTE = 10 ** 0.15                 # 1.5 dB as a power ratio (movs.c:1016: 1.41253754462275)


def pattern(bands):
    b = np.arange(bands)
    return 1e4 * (1. + 0.5 * np.cos(2. * np.pi * (b + 0.5) / bands))


def tilt(bands):
    """the test's spectral shape against the reference's: three slow waves over the bands between 0.4 and 1.6, so that
    the test exceeds the reference in some bands after level adaptation (the noise loudness MOVs are not all zero)"""
    return 1. + 0.6 * np.sin(6. * np.pi * (np.arange(bands) + 0.5) / bands)


def set_unsm(rec, ref, test):
    """rec [..., 576]: both unsmeared excitations [..., bands] and their 0.3rd powers (modpatt.c:235)"""
    nb = ref.shape[-1]
    rec[..., R_UNSM_REF:R_UNSM_REF + nb] = ref
    rec[..., R_UNSM_TEST:R_UNSM_TEST + nb] = test
    rec[..., R_LOUD_REF:R_LOUD_REF + nb] = ref ** 0.3
    rec[..., R_LOUD_TEST:R_LOUD_TEST + nb] = test ** 0.3


def levels(n, steady):
    """[frames, 2]: the level of reference and test in every frame"""
    if steady:
        return np.tile(RISE ** np.arange(n)[:, None], (1, 2))
    lv = np.ones((n, 2))
    lv[1::2] = LEVELS[1]
    return lv


def neutral(n, channels=1, bands=NB, steady=False):
    """n neutral frames; channel 1's pattern is 0.9 of channel 0's"""
    rec = np.zeros((n, channels, 576))
    e = pattern(bands)
    lv = levels(n, steady)
    mask_diff = orc.tables(bands)["mask_diff"]
    for c in range(channels):
        ec = e * (0.9 if c else 1.)
        set_unsm(rec[:, c], lv[:, :1] * ec, lv[:, 1:] * ec * RATIO * tilt(bands))
        rec[:, c, R_NOISE:R_NOISE + bands] = 0.1 * ec / mask_diff
    rec[:, :, R_BW_REF], rec[:, :, R_BW_TEST] = 500., 400.
    rec[:, :, R_EHS] = 0.01
    rec[:, :, R_FL_REF], rec[:, :, R_FL_TEST] = 3., 2.
    rec[:, :, R_SIG_E], rec[:, :, R_NOISE_E] = 1., 0.01
    return rec


def neutral_blocks(n, channels=1):
    """n neutral filter-bank blocks: the forward-masked excitation is the unsmeared one.  The test's tilt changes
    sign every four blocks: the pattern adaptation cannot settle on it, and the noise loudness of RmsNoiseLoudAsymA
    stays several times above the 0.1 below which movs.c:565 sets it to zero."""
    rec = np.zeros((n, channels, 168))
    e = pattern(NB_FB)
    lv = levels(n, False)
    sign = np.where((np.arange(n) // 4) % 2 == 0, 1., -1.)[:, None]
    tl = 1. + sign * (tilt(NB_FB) - 1.)
    for c in range(channels):
        ec = e * (0.9 if c else 1.)
        rec[:, c, B_UNSM_REF:B_UNSM_REF + NB_FB] = rec[:, c, B_EXC_REF:B_EXC_REF + NB_FB] = lv[:, :1] * ec
        rec[:, c, B_UNSM_TEST:B_UNSM_TEST + NB_FB] = rec[:, c, B_EXC_TEST:B_EXC_TEST + NB_FB] = lv[:, 1:] * ec * RATIO * tl
    rec[:, :, B_FLAG] = 1.
    return rec


def smeared(unsm, bands=NB):
    """fftearmodel.c:496-504 on unsm [frames, bands] from a zero state"""
    a = orc.tables(bands)["ear_tc"]
    f, out = np.zeros(unsm.shape[1]), np.empty_like(unsm)
    for k, u in enumerate(unsm):
        f = a * f + (1. - a) * u
        out[k] = np.maximum(f, u)
    return out


def set_above(rec, above, channel=0):
    """bit 0 of the reference's flag word (block records: the flag) per frame, in one channel; the other channels' is cleared"""
    above = np.asarray(above, dtype=bool)
    if rec.shape[2] == 168:
        rec[:, :, B_FLAG] = 0.
        rec[:, channel, B_FLAG] = above
    else:
        rec[:, :, R_FL_REF] -= rec[:, :, R_FL_REF] % 2
        rec[:, channel, R_FL_REF] += above


def above_mask(n, first=0, gaps=()):
    m = np.arange(n) >= first
    for a, b in gaps:
        m[a:b] = False
    return m


def counted(above, last=None):
    """the frames whose values the read-out of an accumulator sees (movaccum.c:317-362, 438-481): none before the first
    frame above the threshold; then every frame, above or not -- unless the pair ends below the threshold, when the
    read-out is the snapshot taken as the last gap opened"""
    above = np.asarray(above, dtype=bool)
    n = len(above)
    if not above.any():
        return np.zeros(n, dtype=bool)
    first = int(np.flatnonzero(above)[0])
    end = n
    if not above[-1]:
        end = int(np.flatnonzero(above)[-1]) + 1
    m = np.zeros(n, dtype=bool)
    m[first:end] = True
    return m


def close(a, b, rtol):
    return abs(a - b) <= rtol * abs(b)


# ---------------------------------------------------------------------------
# basic version
# ---------------------------------------------------------------------------
def status_scenario(name, n, above, channels=1, flag_channel=0):
    """A: bw_ref = 500 + frame and EHS = 0.01 (1 + frame) name the frames an accumulator counted; MFPD (a maximum of a
    filter that runs on behind the snapshot) and WinModDiff (a window over four frames) follow from the trace"""
    rec = neutral(n, channels)
    f = np.arange(n, dtype=np.float64)
    rec[:, :, R_BW_REF] = 500. + f[:, None]
    rec[:, :, R_EHS] = 0.01 * (1. + f[:, None])
    set_above(rec, above, flag_channel)
    cnt = counted(above)
    pos = sorted({int(k) for k in np.flatnonzero(np.diff(np.concatenate([[False], above])) != 0)})
    n24 = int((cnt & (np.arange(n) >= 24)).sum())      # counted frames that pass gstpeaq.c:871
    nan = ([WINMOD] if n24 < 4 else []) + ([AVGMOD1, AVGMOD2, NOISELOUD] if n24 == 0 else [])

    def check(o):
        mv, tr = o["movs"], o["trace"]
        if not cnt.any():
            assert np.array_equal(np.isnan(mv), [i not in (ADB, MFPD) for i in range(11)]) and mv[ADB] == 0. and mv[MFPD] == 0.
            return
        assert close(mv[BW_REF], (500. + f[cnt]).mean(), 1e-14), (mv[BW_REF], np.flatnonzero(cnt)[[0, -1]])
        assert close(mv[EHS], (10. * (1. + f[cnt])).mean(), 1e-13)
        # MFPD: the filter sees every frame from the first above on, the maximum is read where the count ends
        filt, mx, run = 0., 0., np.arange(n) >= np.flatnonzero(cnt)[0]
        for k in np.flatnonzero(run):
            filt = 0.9 * filt + 0.1 * tr["p_detect"][k, 0]
            if cnt[k]:
                mx = max(mx, filt)
        assert close(mv[MFPD], mx, 1e-14), (mv[MFPD], mx)
        if not above[-1]:
            assert filt > mx * (1. + 1e-6)           # the filter has run on behind the snapshot
        # AvgModDiff1: frames >= 24 among the counted
        m24 = cnt & (np.arange(n) >= 24)
        if m24.any():
            w = tr["tempwt"][m24].sum(0)
            assert np.allclose(mv[AVGMOD1], ((tr["moddiff1"][m24] * tr["tempwt"][m24]).sum(0) / w).mean(), rtol=1e-12)
        else:
            assert np.isnan(mv[AVGMOD1])
        assert np.isnan(mv[WINMOD]) == (m24.sum() < 4)

    return name, rec, dict(channels=channels, positions=pos, check=check,
                           nan=nan if cnt.any() else [i for i in range(11) if i not in (ADB, MFPD)])


def gate_scenario(name, n, g, channels=1, mode="both"):
    """B: quiet excitations switch to the neutral ones so that the loudness gate opens on frame g (None: never)"""
    rec = neutral(n, channels)
    q = np.arange(n) < (n if g is None else g)
    if mode == "both":                                 # both signals of every channel quiet
        sel = [(c, s) for c in range(channels) for s in (0, 1)]
    elif mode == "ch1":                                # stereo: channel 0 stays quiet throughout, channel 1 opens the gate
        rec[:, 0, R_UNSM_REF:R_LOUD_REF] *= QUIET
        sel = [(1, 0), (1, 1)]
    else:                                              # "crossed": ref loud in channel 0 only, test loud in channel 1 only
        sel = [(0, 1), (1, 0)]
    for c, s in sel:
        lo = R_UNSM_TEST if s else R_UNSM_REF
        rec[q, c, lo:lo + 112] *= QUIET
    rec[:, :, R_LOUD_REF:R_NOISE] = rec[:, :, :R_LOUD_REF] ** 0.3
    first = None if g is None else max(24, g + 3)      # gstpeaq.c:880-881

    def check(o):
        mv, tr = o["movs"], o["trace"]
        if first is None or first >= n:
            assert np.isnan(mv[NOISELOUD]) and np.isnan(o["di"]) and np.isnan(o["odg"])
        else:
            exp = np.sqrt((tr["noiseloud"][first:] ** 2).mean(0)).mean()
            assert close(mv[NOISELOUD], exp, 1e-12), (mv[NOISELOUD], exp)
            if first + 1 < n:                          # one frame earlier or later is another value
                for other in (first - 1, first + 1):
                    assert not close(np.sqrt((tr["noiseloud"][other:] ** 2).mean(0)).mean(), exp, 1e-9)

    return name, rec, dict(channels=channels, gate=g, positions=[] if g is None else [g, g + 3], check=check,
                           nan=[NOISELOUD] if first is None else [])


def vote_scenario(name, mirrored):
    """C: RelDistFrames asks whether ANY band's noise-to-mask ratio is above 1.5 dB.  Frame k < 109: only band k is
    just above it by the margin and every other band just below (mirrored: band k just below, all others well
    below); frame 109: no band above.  Catches a vote that loses a lane, a slot or band 108."""
    n = NB + 1
    rec = neutral(n, steady=True)
    # smeared = unsmeared: the excitation rises
    mask = levels(n, True)[:, :1] * pattern(NB) / orc.tables(NB)["mask_diff"]
    ratio = np.full((n, NB), 0.5 * VOTE if mirrored else VOTE * (1. - VOTE_M))
    k = np.arange(NB)
    ratio[k, k] = VOTE * (1. - VOTE_M) if mirrored else VOTE * (1. + VOTE_M)
    rec[:, 0, R_NOISE:R_NOISE + NB] = ratio * mask
    hits = 0 if mirrored else NB

    def check(o):
        assert close(o["movs"][RELDIST], hits / n, 1e-14), o["movs"][RELDIST]
        mx = o["trace"]["nmr_max"][:, 0]
        assert np.all(np.abs(mx / 1.41253754462275 - 1.) > 0.5 * VOTE_M)      # no frame sits inside the margin

    return name, rec, dict(channels=1, steady=True, positions=[], check=check, nan=[])


def bandwidth_scenario(name, kind):
    """D: bw_ref > 346 admits a frame to both bandwidth MOVs (movs.c:797-807)"""
    n = 30
    rec = neutral(n)
    f = np.arange(n)
    if kind == "mixed":
        rec[:, 0, R_BW_REF] = np.array([346., 347., 0.])[f % 3]
        rec[:, 0, R_BW_TEST] = 300. + f
    elif kind == "none":
        rec[:, 0, R_BW_REF] = np.array([346., 0., 1.])[f % 3]
    else:                                              # "test0": counted frames whose test bandwidth is 0
        rec[:, 0, R_BW_TEST] = 0.
    ok = rec[:, 0, R_BW_REF] > 346.

    def check(o):
        mv = o["movs"]
        if not ok.any():
            assert np.isnan(mv[BW_REF]) and np.isnan(mv[BW_TEST])
        else:
            assert close(mv[BW_REF], rec[ok, 0, R_BW_REF].mean(), 1e-14)
            assert mv[BW_TEST] == 0. if kind == "test0" else close(mv[BW_TEST], rec[ok, 0, R_BW_TEST].mean(), 1e-14)

    return name, rec, dict(channels=1, positions=[], check=check, nan=[] if ok.any() else [BW_REF, BW_TEST])


def detect_scenario(name, db, adb=None, low_bands=0, settings=None):
    """E: uniform level differences ref - test of db[frame] dB (held for the frames it names), rising excitations.
    adb: the value ADB must have exactly (-0.5: frames counted, no steps; 0: no frame counted), or None"""
    db = np.asarray(db, dtype=np.float64)
    n = len(db)
    rec = neutral(n, steady=True)
    e = levels(n, True)[:, :1] * pattern(NB)
    t = e * 10. ** (-db[:, None] / 10.)
    if low_bands:                                      # both excitations below 1: l <= 0, the 1e30 branch
        e[:, :low_bands], t[:, :low_bands] = 0.5, 0.4
    set_unsm(rec[:, 0], e, t)
    steady = bool(np.all(db == db[0]))

    def check(o):
        p = o["trace"]["p_detect"][:, 0]
        assert np.all(np.abs(p - 0.5) >= 1e-3)
        d = 10. * np.log10(smeared(e) / smeared(t))
        assert np.all(np.abs(d - np.round(d)) >= 1e-6)
        if adb is not None:
            assert o["movs"][ADB] == adb, o["movs"][ADB]
        elif (p > 0.5).any():
            exp = np.log10(o["trace"]["steps"][p > 0.5, 0].mean())
            assert close(o["movs"][ADB], exp, 1e-12), (o["movs"][ADB], exp)

    notes = dict(channels=1, steady=steady, positions=[], check=check, nan=[])
    if settings:
        notes["settings"] = settings
    return name, rec, notes


def ehs_scenario(name, kind, bands=NB):
    """F: a frame's EHS is admitted if any channel's reference or test has the energy bit (movs.c:1374-1381);
    EHS = 0.01 (1 + frame) names the admitted frames"""
    n = 30
    rec = neutral(n, bands=bands)
    f = np.arange(n, dtype=np.float64)
    rec[:, 0, R_EHS] = 0.01 * (1. + f)
    fl = dict(ref=(3., 0.), test=(1., 2.), neither=(1., 0.))
    rows = [fl["ref" if k % 2 else "neither"] for k in range(n)] if kind == "alternating" else [fl[kind]] * n
    rec[:, 0, R_FL_REF], rec[:, 0, R_FL_TEST] = np.array(rows).T
    ok = (np.array(rows) >= 2.).any(1)
    idx = A_EHS if bands == NB_ADV else EHS

    def check(o):
        v = o["movs"][idx]
        assert np.isnan(v) if not ok.any() else close(v, (10. * (1. + f[ok])).mean(), 1e-13), v

    return name, rec, dict(channels=1, positions=[], check=check, nan=[] if ok.any() else [idx])


def window_scenario(name, n, first=0):
    """G: WinModDiff averages over windows of four consecutive values (movaccum.c:399-414) of the frames >= 24 that
    are not dropped in INIT"""
    rec = neutral(n)
    above = above_mask(n, first)
    set_above(rec, above)
    start = max(24, first)
    windows = n - start - 3

    def check(o):
        v, d1 = o["movs"][WINMOD], o["trace"]["moddiff1"][:, 0]
        if windows < 1:
            assert np.isnan(v)
            return
        sq = np.sqrt(d1[start:])
        w = [((sq[k:k + 4].sum()) / 4.) ** 4 for k in range(windows)]
        assert close(v, np.sqrt(np.mean(w)), 1e-12), (v, np.sqrt(np.mean(w)))

    return name, rec, dict(channels=1, positions=[first] if first else [], check=check,
                           nan=[WINMOD] if windows < 1 else [])


def totalsnr_scenario():
    """H: the energies differ per frame and channel; the sums go over both channels"""
    n = 30
    rec = neutral(n, 2)
    f = np.arange(n, dtype=np.float64)[:, None]
    c = np.arange(2, dtype=np.float64)[None, :]
    rec[:, :, R_SIG_E] = 1. + 0.1 * f + 0.01 * c
    rec[:, :, R_NOISE_E] = 0.01 * (1. + f) * (1. + c)

    def check(o):
        exp = 10. * np.log10(rec[:, :, R_SIG_E].sum() / rec[:, :, R_NOISE_E].sum())
        assert close(o["totalsnr"], exp, 1e-13), (o["totalsnr"], exp)

    return "H-totalsnr-stereo", rec, dict(channels=2, positions=[], check=check, nan=[])


def energy_bit_channel1_test():
    """A (last): stereo with the energy bit only in channel 1's TEST word: every frame's EHS is admitted, both channels'"""
    n = 30
    rec = neutral(n, 2)
    f = np.arange(n, dtype=np.float64)
    rec[:, 0, R_EHS], rec[:, 1, R_EHS] = 0.01 * (1. + f), 0.02 * (1. + f)
    rec[:, :, R_FL_REF], rec[:, :, R_FL_TEST] = 1., 0.
    rec[:, 1, R_FL_TEST] = 2.

    def check(o):
        assert close(o["movs"][EHS], 0.5 * (10. + 20.) * (1. + f).mean(), 1e-13), o["movs"][EHS]

    return "A-stereo-energy-bit-in-channel-1-test", rec, dict(channels=2, positions=[], check=check, nan=[])


@functools.lru_cache(maxsize=None)
def basic_scenarios():
    s = [status_scenario("A-never-above", 40, above_mask(40, 40))]
    s += [status_scenario(f"A-first-above-{k}", 40, above_mask(40, k)) for k in (0, 10, 23, 24, 30)]
    s += [
        status_scenario("A-gap-30-40", 50, above_mask(50, 0, [(30, 40)])),
        status_scenario("A-ends-in-gap", 40, above_mask(40, 0, [(30, 40)])),
        status_scenario("A-gap-20-28-across-24", 40, above_mask(40, 0, [(20, 28)])),
        status_scenario("A-gap-after-first-above", 40, above_mask(40, 5, [(6, 12)])),
        status_scenario("A-two-gaps", 60, above_mask(60, 2, [(26, 31), (40, 47)])),
        status_scenario("A-two-gaps-ends-in-second", 50, above_mask(50, 2, [(26, 31), (44, 50)])),
        status_scenario("A-stereo-above-in-channel-1", 40, above_mask(40, 10, [(28, 33)]), channels=2, flag_channel=1),
        energy_bit_channel1_test(),
    ]
    s += [gate_scenario(f"B-gate-opens-{g}", 40, g) for g in (0, 20, 21, 22, 30)]
    s += [
        gate_scenario("B-gate-never", 40, None),
        gate_scenario("B-stereo-channel-1-opens-22", 40, 22, channels=2, mode="ch1"),
        gate_scenario("B-stereo-crossed-until-30", 40, 30, channels=2, mode="crossed"),
        vote_scenario("C-vote-one-band-above", False),
        vote_scenario("C-vote-one-band-just-below", True),
        bandwidth_scenario("D-bw-346-347-0", "mixed"),
        bandwidth_scenario("D-bw-none-above-346", "none"),
        bandwidth_scenario("D-bw-test-0", "test0"),
        detect_scenario("E-plus-0.9dB", [0.9] * 30, adb=-0.5),
        detect_scenario("E-plus-1.5dB", [1.5] * 30),
        detect_scenario("E-minus-1.5dB", [-1.5] * 30),
        detect_scenario("E-minus-1.5dB-floor", [-1.5] * 30, settings=dict(use_floor_for_steps_above_threshold=1)),
        detect_scenario("E-0.05dB-none-detected", [0.05] * 30, adb=0.),
        detect_scenario("E-mix", [0.9] * 8 + [1.5] * 8 + [0.05] * 8 + [-1.5] * 8 + [0.9] * 8),
        detect_scenario("E-low-bands", [1.5] * 30, low_bands=10),
        ehs_scenario("F-energy-ref-only", "ref"),
        ehs_scenario("F-energy-test-only", "test"),
        ehs_scenario("F-energy-neither", "neither"),
        ehs_scenario("F-energy-alternating", "alternating"),
        window_scenario("G-27-frames-no-window", 27),
        window_scenario("G-28-frames-one-window", 28),
        window_scenario("G-first-above-26-of-31", 31, 26),
        totalsnr_scenario(),
    ]
    assert all(r.shape[0] <= 140 for _, r, _ in s)
    return s


# ---------------------------------------------------------------------------
# advanced version
# ---------------------------------------------------------------------------
def rms_modulation(tr, m):
    """RmsModDiffA over the blocks m (MODE_RMS, movaccum.c:377-381,455-457), channel mean"""
    w2 = tr["tempwt"][m] ** 2
    return np.sqrt((w2 * tr["rmsmoddiff"][m] ** 2).sum(0) / w2.sum(0)).mean()


def adv_status_scenario(name, n, above, channels=1, flag_channel=0):
    fb, ff = neutral_blocks(n, channels), neutral(30, channels, NB_ADV)
    set_above(fb, above, flag_channel)
    cnt = counted(above) & (np.arange(n) >= 125)       # gstpeaq.c:988: blocks from 125 on
    pos = sorted({int(k) for k in np.flatnonzero(np.diff(np.concatenate([[False], above])) != 0)})

    def check(o):
        mv, tr = o["movs"], o["trace_blocks"]
        if not cnt.any():
            assert np.isnan(mv[A_RMSMOD]) and np.isnan(mv[A_LINDIST])
            return
        assert close(mv[A_RMSMOD], rms_modulation(tr, cnt), 1e-12)
        assert close(mv[A_LINDIST], tr["lindist"][cnt].mean(0).mean(), 1e-12)    # the gate opened on block 0
        assert not close(tr["lindist"][cnt][1:].mean(0).mean(), mv[A_LINDIST], 1e-9)

    return name, fb, ff, dict(channels=channels, block_positions=pos, positions=[], check=check,
                              nan=[] if cnt.any() else [A_RMSMOD, A_NLASYM, A_LINDIST])


def adv_gate_scenario(name, n, g):
    fb, ff = neutral_blocks(n), neutral(30, 1, NB_ADV)
    q = np.arange(n) < (n if g is None else g)
    fb[q, :, :B_FLAG] *= QUIET
    first = None if g is None else max(125, g + 13)    # gstpeaq.c:996-997

    def check(o):
        mv, tr = o["movs"], o["trace_blocks"]
        if first is None or first >= n:
            assert np.isnan(mv[A_LINDIST]) and np.isnan(mv[A_NLASYM]) and np.isnan(o["odg"])
            return
        exp = tr["lindist"][first:].mean(0).mean()
        assert close(mv[A_LINDIST], exp, 1e-12), (mv[A_LINDIST], exp)
        for other in (first - 1, first + 1):
            assert not close(tr["lindist"][other:].mean(0).mean(), exp, 1e-9)

    return name, fb, ff, dict(channels=1, gate=g, block_positions=[] if g is None else [g, g + 13], positions=[],
                              check=check, nan=[A_NLASYM, A_LINDIST] if first is None or first >= n else [])


def adv_frames_scenario(name, above, kind, fb_above):
    """55-band frames: gaps and EHS admission for SegmentalNMRB and EHSB, the block path's gaps placed on their own"""
    _, ff, notes = ehs_scenario(name, kind, NB_ADV)
    n = len(ff)
    set_above(ff, above)
    fb = neutral_blocks(140)
    set_above(fb, fb_above)
    cnt = counted(above)
    admitted = (ff[:, 0, R_FL_REF] >= 2.) | (ff[:, 0, R_FL_TEST] >= 2.)
    f = np.arange(n, dtype=np.float64)
    bcnt = counted(fb_above) & (np.arange(140) >= 125)

    def check(o):
        mv = o["movs"]
        assert close(mv[A_SEGNMR], o["trace_frames"]["segnmr_db"][cnt].mean(0).mean(), 1e-12)
        m = cnt & admitted
        assert np.isnan(mv[A_EHS]) if not m.any() else close(mv[A_EHS], (10. * (1. + f[m])).mean(), 1e-13)
        assert close(mv[A_RMSMOD], rms_modulation(o["trace_blocks"], bcnt), 1e-12)

    pos = sorted({int(k) for k in np.flatnonzero(np.diff(np.concatenate([[False], above])) != 0)})
    bpos = sorted({int(k) for k in np.flatnonzero(np.diff(np.concatenate([[False], fb_above])) != 0)})
    return name, fb, ff, dict(channels=1, positions=pos, block_positions=bpos, check=check,
                              nan=[] if (cnt & admitted).any() else [A_EHS])


@functools.lru_cache(maxsize=None)
def advanced_scenarios():
    s = [adv_status_scenario(f"adv-A-first-above-{k}", 140, above_mask(140, k)) for k in (0, 124, 125, 130)]
    s += [
        adv_status_scenario("adv-A-gap-120-130-across-125", 140, above_mask(140, 0, [(120, 130)])),
        adv_status_scenario("adv-A-ends-in-gap", 140, above_mask(140, 0, [(135, 140)])),
        adv_status_scenario("adv-A-stereo-flag-in-channel-1", 140, above_mask(140, 3, [(128, 133)]), channels=2,
                            flag_channel=1),
    ]
    s += [adv_gate_scenario(f"adv-B-gate-opens-{g}", 160 if g == 140 else 140, g) for g in (0, 111, 112, 113, 140)]
    s += [
        adv_gate_scenario("adv-B-gate-never", 140, None),
        adv_frames_scenario("adv-F-frames-gap-ref-energy", above_mask(30, 2, [(10, 15)]), "ref",
                            above_mask(140, 0, [(126, 131)])),
        adv_frames_scenario("adv-F-frames-end-in-gap-alternating", above_mask(30, 0, [(24, 30)]), "alternating",
                            above_mask(140, 0, [(100, 127)])),
        adv_frames_scenario("adv-F-frames-no-energy", above_mask(30, 4), "neither", above_mask(140, 130)),
    ]
    assert all(fb.shape[0] <= 160 and ff.shape[0] <= 30 for _, fb, ff, _ in s)
    return s

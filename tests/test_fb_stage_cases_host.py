"""The populations of tests/fb_stage_cases.py held to what they are meant to be, with the CPU oracle alone (no GPU):
their block counts, where P2's signals fall in fb_hp_kernel's waves and workgroups, that P1 and P2 carry every band
above the internal noise ("teeth": a relative bound on a value that is all noise floor pins nothing), and that the
hand-built signals of P4 are what their names say in the oracle's own records.  The figures in the docstrings are the
oracle's, measured when the populations were written; where they speak of a signal-to-noise ratio it is
(value - internal_noise) / internal_noise of the reference's UNSMEARED plane (record columns 0 .. 39) -- the
forward-masked excitation carries the loud past for many blocks more."""
import numpy as np
import pytest

import fb_stage_cases as fsc
import oracle_lib as orc

NB = 40
HP_LANES, HP_WAVES = 64, 4       # gstpeaq_amd/csrc/peaq_fb.hip: fb_hp_kernel's wave size and kHpWaves (PEAQ_HP_WAVES)

_REC = {}


def noise():
    return orc.tables(NB)["internal_noise"]


def records(key, ref, test, **kw):
    if key not in _REC:
        _REC[key] = orc.fb_records(ref, test, orc.count_blocks(len(ref), len(test)), **kw)
    return _REC[key]


def counts(pairs):
    return [orc.count_blocks(len(r), len(t)) for r, t in pairs]


@pytest.mark.parametrize("ch", [1, 2])
def test_p1_counts_follow_count_blocks_and_cover_every_tile_tail(ch):
    """p + 1 blocks for even p; where the test signal is short the full blocks of both and one flush block.  A tile of
    fb_bank_kernel is 10 blocks: every tail 1 .. 10 occurs, and so does every signal end on, one sample before and one
    after a chunk of 16 samples and a block"""
    pairs = fsc.p1_pairs(ch)
    cnt = counts(pairs)
    assert len(pairs) == 40 and [cnt[p] for p in range(0, 40, 2)] == list(range(1, 41, 2))
    for p, (r, t) in enumerate(pairs):
        assert len(r) == 192 * p + fsc.TAILS[p % 6] and len(t) == len(r) - ((37 * p) % 400 if p & 1 else 0)
        full = min(len(r), len(t)) // 192
        assert cnt[p] == full + (max(len(r), len(t)) > 192 * full)
    assert {(c - 1) % 10 + 1 for c in cnt} == set(range(1, 11))
    assert {len(r) % 192 for r, _ in pairs} == {0, 1, 15, 16, 17, 191}
    ragged = [p for p, (r, t) in enumerate(pairs) if len(t) < len(r)]
    assert len(ragged) == 20 and any(cnt[p] < p + 1 for p in ragged)      # (some references end behind the flush block)


def test_p3_counts_straddle_the_launch_seam():
    cnt = counts(fsc.p3_pairs())
    assert cnt == [845, 841, 840, 839]
    assert [max(0, c - 840) for c in cnt] == [5, 1, 0, 0]           # the second launch's blocks at 840 blocks per launch


@pytest.mark.parametrize("ch", [1, 2])
def test_p2_layout_in_waves_and_workgroups(ch):
    """the grouping of fb_hp_kernel recomputed: signals in the order pair, channel, ref/test, 64 per wave, 4 waves per
    workgroup"""
    pairs = fsc.p2_pairs(ch)
    n_pairs, deviants, copies = fsc.p2_layout(ch)
    assert len(pairs) == n_pairs == (65 if ch == 2 else 129) and 2 * ch * n_pairs in (258, 260)
    wave, wg = fsc.wave_map(n_pairs, ch)
    assert wave.shape == (n_pairs, ch, 2) and wave.max() == 4 and wg.max() == 1
    assert (np.bincount(wave.ravel()) == [64, 64, 64, 64, 2 * ch]).all() and (wg[wave == 4] == 1).all()
    length = np.array([[[len(r), len(t)]] * ch for r, t in pairs])   # [pair, channel, ref/test]
    full = [w for w in range(5) if (length[wave == w] == fsc.P2_FULL).all()]
    with_empty = [w for w in range(5) if (length[wave == w] == 0).any()]
    mixed = [w for w in range(5) if len(set(length[wave == w].tolist())) > 1]
    assert 3 in full and 4 in full, full                # a whole wave of 64 full-length signals, and the spare-lane wave
    assert with_empty == [0, 1] and mixed == [0, 1, 2], (with_empty, mixed)
    # the deviants: at both edges of waves 0 and 1 and inside wave 2
    assert sorted(deviants.values()) == ["blocks11_100", "blocks3", "empty", "one_sample", "ref_only"]
    lanes = {kind: (int(wave[p, 0, 0]), int((2 * ch * p) % HP_LANES)) for p, kind in deviants.items()}
    # (first lane of the pair's signals; stereo: the wave's last pair, mono: its last but one)
    assert lanes == dict(empty=(0, 0), one_sample=(0, 60), ref_only=(1, 0), blocks3=(1, 60), blocks11_100=(2, 32)), lanes
    got = {kind: (len(pairs[p][0]), len(pairs[p][1])) for p, kind in deviants.items()}
    assert got == dict(empty=(0, 0), one_sample=(1, 1), ref_only=(2304, 0), blocks3=(576, 576), blocks11_100=(2212, 2212))
    assert [counts(pairs)[p] for p in sorted(deviants)] == [0, 1, 1, 3, 12]
    # the last pair is full: the packed tensors end with its last sample
    ref, test, n_ref, n_test = fsc.packed(pairs, fsc.P2_FULL)
    assert ref.shape == test.shape == (n_pairs, 2304, ch) and n_ref[-1] == n_test[-1] == 2304
    # the copies of pair 1: the same bytes, in other waves, one of them in the second workgroup
    for p in copies:
        assert ref[p].tobytes() == ref[1].tobytes() and test[p].tobytes() == test[1].tobytes()
    assert all(ref[p].tobytes() != ref[1].tobytes() for p in range(n_pairs) if p != 1 and p not in copies)
    assert [int(wave[p, 0, 0]) for p in copies] == [2, 3, 4] and int(wave[1, 0, 0]) == 0
    assert [int(wg[p, 0, 0]) for p in copies] == [0, 0, 1] and HP_LANES * HP_WAVES == 256


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("pop", ["p1", "p2"])
def test_every_band_is_above_the_internal_noise_from_block_5_on(pop, ch):
    """Teeth: over all values of the four planes in blocks >= 5, the share whose signal part (value - internal_noise)
    is below the internal noise is at most 1e-3 -- a condition on the seeds, not a tolerance (measured: P1 2.3e-4 mono,
    3.7e-4 stereo; P2 6.9e-4 and 7.4e-4, nearly all of it the forward-masked excitation of blocks 5 and 6).  Blocks
    0 .. 4 are mostly noise floor by construction: all filters are centred on a delay of 729 samples."""
    pairs = fsc.p1_pairs(ch) if pop == "p1" else fsc.p2_pairs(ch)
    n4 = np.tile(noise(), 4)
    low = total = 0
    for p, (r, t) in enumerate(pairs):
        if orc.count_blocks(len(r), len(t)) > 5:
            v = records((pop, ch, p), r, t)[5:, :, :160]
            low += int(((v - n4) < n4).sum())
            total += v.size
    print(f"{pop} channels={ch}: {low} of {total} values below twice the internal noise ({low / total:.2e})")
    assert total > 90000 and low <= 1e-3 * total, (low, total)


def p4_unsmeared_snr(name):
    c = fsc.p4_cases(orc.tables(NB)["fc"])[name]
    rec = records(("p4", name), c["ref"], c["test"], level=c["level"])
    assert rec.shape == (40, 2, 168)
    return (rec[:, 0, :NB] - noise()) / noise(), rec


def test_p4_step_down_leaves_the_quiet_half_at_the_noise_floor():
    """q = 1e-3: block 35's signal-to-noise ratio has a median within [0.1, 10] (0.97) -- an absolute error left by the
    loud half (maximum 2.8e7 times the noise) shows there at full weight; q = 0: every value of block 39 is within 5 %
    of the internal noise (3.3e-3).  The boundary flag follows the input: set in blocks 0 .. 19, clear from 20 on"""
    snr, rec = p4_unsmeared_snr("step_1e-3")
    assert 0.1 <= np.median(snr[35]) <= 10., np.median(snr[35])
    assert snr[:20].max() > 1e7
    snr0, rec0 = p4_unsmeared_snr("step_0")
    assert np.abs(snr0[39]).max() <= 0.05, np.abs(snr0[39]).max()
    for r in (rec, rec0):
        assert r[:, 0, 160].tolist() == [1.] * 20 + [0.] * 20 and r[:, 1, 160].all()


def test_p4_impulse_is_seen_in_blocks_6_to_12_and_every_tap_counts():
    """the impulse of 0.5 at sample 1000 is above the noise in blocks 6 .. 12 only (peak 2.1e5 times the noise, block 9);
    moved by one sample it changes the oracle's own records of blocks 6 .. 12 by more than 1e-3 relative in at least
    half of the bands (39 of 40 unsmeared, 39 of 40 in the excitation; 51 % and 76 % of the values) -- a window that is
    off by one tap does not pass a bound of 1e-4"""
    snr, rec = p4_unsmeared_snr("impulse")
    assert np.flatnonzero((snr > 1.).any(axis=1)).tolist() == list(range(6, 13)) and 1e5 < snr.max() < 4e5
    c = fsc.p4_cases(orc.tables(NB)["fc"])["impulse"]
    moved_ref = c["ref"].copy()
    moved_ref[:, 0] = fsc.impulse(fsc.P4_IMPULSE_AT + 1)
    moved = orc.fb_records(moved_ref, c["test"], 40)
    for lo in (0, 80):
        rel = np.abs(moved[6:13, 0, lo:lo + NB] / rec[6:13, 0, lo:lo + NB] - 1.)
        assert (rel.max(axis=0) > 1e-3).sum() >= NB // 2, (lo, (rel.max(axis=0) > 1e-3).sum())
    assert rec[:, 0, 160].tolist() == [0.] * 5 + [1.] + [0.] * 34    # five samples of |x| sum 0.5: the impulse's block only


def test_p4_dc_decays_through_the_high_pass_and_the_sines_sit_on_their_bands():
    """the constant 0.25: 5.9e4 times the noise in block 3, 0.15 times in block 29 (the two DC-rejection biquads), while
    the boundary flag -- which looks at the input, 5 x 0.25 -- stays set in every block; a sine at a band's centre
    frequency has its largest unsmeared value in that band"""
    snr, rec = p4_unsmeared_snr("dc")
    assert 3e4 < snr[3].max() < 1e5 and 0.05 < snr[29].max() < 0.5 and rec[:, 0, 160].all()
    for k, name in ((0, "sine_fc0"), (20, "sine_fc20"), (39, "sine_fc39")):
        snr, _ = p4_unsmeared_snr(name)
        assert int(np.argmax(snr[30])) == k and snr[30, k] > 1e4, (name, int(np.argmax(snr[30])))


def test_p4_levels_and_the_slope_switch_change_the_records():
    """40 dB of playback level are a factor of 1e4 in a band's signal part -- and more in the upper bands, where the
    level-dependent spreading adds to it (6.5e3 .. 1.6e5 measured); the slope switch moves the records by far more
    than any tolerance of the device tests"""
    cases = fsc.p4_cases(orc.tables(NB)["fc"])
    lo, _ = p4_unsmeared_snr("level_72")
    hi, _ = p4_unsmeared_snr("level_112")
    ratio = hi[10:] / lo[10:]
    assert ratio.min() > 5e3 and 5e3 < np.median(ratio[:, :20]) < 2e4 and ratio.max() > 5e4, (ratio.min(), ratio.max())
    c = cases["swap_slope"]
    plain = orc.fb_records(c["ref"], c["test"], 40)
    try:
        orc.set_settings(**c["settings"])
        swapped = orc.fb_records(c["ref"], c["test"], 40)
    finally:
        orc.set_settings()
    assert np.array_equal(orc.fb_records(c["ref"], c["test"], 40), plain)        # restored
    assert np.abs(swapped[10:, :, :160] / plain[10:, :, :160] - 1.).max() > 1e-2

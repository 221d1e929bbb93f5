"""The one-wave front end (frontend_pair_kernel<109>: reference and test of a frame in one wave) against the two-wave
kernel (frontend_kernel<109>) it replaces in the basic version, on the same inputs, through the stage entry
peaq_debug_frontend_pairs (launched as the batch path launches it) and the in-process switch peaq_debug_select_frontend.  Every
field of every (pair, frame, channel) record is compared.  The inputs are the smallest at which the fused wave can go
wrong where the two-wave one cannot: both buffer resources on one lane offset (mono, stereo, n_ref != n_test, a flush
frame zero-padded by the range check), the item decoding at grids that are no multiple of 8 and below / above the
prefetch distance of 64 items, a frame count that is no multiple of the frames per launch, identical signals (exact zeros
in the noise spectrum and the log ratios), digital silence on one side (+-inf ratios), the boundary detector's exact
path and the energy flag one ulp on either side of its threshold.

Tolerances: those tests/test_gpu_parity.py holds the front end to against the oracle -- flags, bandwidths and padding
exactly, roots rtol 2e-10, noise in bands 1e-6, EHS 1e-7 (NaN = NaN); the hop energies exactly (both kernels add the
same float products in the same tree).  Each comparison prints its largest relative difference per field.  Needs an MI355X."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import synth_np

pytestmark = pytest.mark.gpu

NB = 109
ROOT_REF, ROOT_TEST, NOISE, SCAL = 0, 112, 224, 336
BW_REF, BW_TEST, EHS, FLAGS_REF, FLAGS_TEST, SIG_E, NOISE_E = (SCAL + i for i in range(7))
GROUP_FLOOR = 1e-12                                  # the band sums' floor (fftearmodel.c:617): a band of an all-zero spectrum


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback in the product)")
    import gpu_common
    return gpu_common


def count_frames(n_ref, n_test):
    n = min(n_ref, n_test)
    full = (n - 2048) // 1024 + 1 if n >= 2048 else 0
    return full + (1 if max(n_ref, n_test) > full * 1024 else 0)


def both_kernels(gpu, pairs, frames_per_launch):
    """pairs: [(ref, test)] float32 [n, channels] -> the records [pair, frame, channel, 352] of the one-wave and of the
    two-wave kernel"""
    import torch
    import gstpeaq_amd
    from gstpeaq_amd import capi
    channels = pairs[0][0].shape[1]
    n_ref, n_test = [len(r) for r, _ in pairs], [len(t) for _, t in pairs]
    stride = max(n_ref + n_test)
    ref = np.zeros((len(pairs), stride, channels), dtype=np.float32)
    test = np.zeros_like(ref)
    for i, (r, t) in enumerate(pairs):
        ref[i, :len(r)], test[i, :len(t)] = r, t
    n_frames = max(count_frames(a, b) for a, b in zip(n_ref, n_test))
    d_ref, d_test = torch.from_numpy(ref).cuda(), torch.from_numpy(test).cuda()
    ctx = gpu.ctx()
    out = []
    before = capi.debug_select_frontend(ctx, 0)
    try:
        for two_waves in (0, 1):
            capi.debug_select_frontend(ctx, two_waves)
            out.append(capi.debug_frontend_pairs(ctx, d_ref, d_test, n_ref, n_test, frames_per_launch, n_frames))
    finally:
        capi.debug_select_frontend(ctx, before)
    counts = [count_frames(a, b) for a, b in zip(n_ref, n_test)]
    for rec in out:                                  # every frame a pair has was written, none beyond
        for p, c in enumerate(counts):
            assert (rec[p, :c, :, FLAGS_REF] >= 0).all() and rec[p, :c, :, ROOT_REF:ROOT_REF + NB].all()
            assert not rec[p, c:].any()
    return out[0], out[1]


def rel_diff(a, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(a - b) / np.maximum(np.abs(a), np.abs(b))
    d = np.where((a == b) | (np.isnan(a) & np.isnan(b)), 0., d)
    return float(np.max(d)) if d.size else 0.


def compare(one, two, label):
    fields = dict(root_ref=slice(ROOT_REF, ROOT_REF + NB), root_test=slice(ROOT_TEST, ROOT_TEST + NB),
                  noise=slice(NOISE, NOISE + NB), ehs=slice(EHS, EHS + 1), energies=slice(SIG_E, NOISE_E + 1))
    print(f"\n{label}: largest relative difference per field: " +
          ", ".join(f"{k} {rel_diff(one[..., s], two[..., s]):.3g}" for k, s in fields.items()))
    for name, idx in (("flags", slice(FLAGS_REF, FLAGS_TEST + 1)), ("bandwidths", slice(BW_REF, BW_TEST + 1)),
                      ("padding of root_ref", slice(ROOT_REF + NB, ROOT_TEST)), ("padding of root_test", slice(ROOT_TEST + NB, NOISE)),
                      ("padding of noise", slice(NOISE + NB, SCAL)), ("unused scalars", slice(NOISE_E + 1, 352)),
                      ("hop energies", slice(SIG_E, NOISE_E + 1))):
        assert np.array_equal(one[..., idx], two[..., idx]), (name, one[..., idx], two[..., idx])
    assert not one[..., ROOT_REF + NB:ROOT_TEST].any() and not one[..., NOISE + NB:SCAL].any() and not one[..., NOISE_E + 1:].any()
    np.testing.assert_allclose(one[..., fields["root_ref"]], two[..., fields["root_ref"]], rtol=2e-10, atol=0, err_msg="root_ref")
    np.testing.assert_allclose(one[..., fields["root_test"]], two[..., fields["root_test"]], rtol=2e-10, atol=0, err_msg="root_test")
    np.testing.assert_allclose(one[..., fields["noise"]], two[..., fields["noise"]], rtol=1e-6, atol=0, err_msg="noise in bands")
    assert np.array_equal(np.isnan(one[..., EHS]), np.isnan(two[..., EHS])), "EHS: NaN positions"
    np.testing.assert_allclose(one[..., EHS], two[..., EHS], rtol=1e-7, atol=1e-13, err_msg="ehs")


@functools.lru_cache(maxsize=None)
def synth(seed, channels, n):
    return synth_np.pair(seed, channels, n)


def cut(seed, channels, n_ref, n_test):
    r, t = synth(seed, channels, max(n_ref, n_test))
    return r[:n_ref].copy(), t[:n_test].copy()


# (samples of the reference, of the test signal) per pair: one frame; a flush frame zero-padded by the range check;
# n_ref != n_test, so that the two buffer resources differ
LENGTHS = [(2048, 2048), (2500, 2500), (4000, 5120)]


@pytest.mark.parametrize("channels", [1, 2], ids=["mono", "stereo"])
@pytest.mark.parametrize("n_pairs", [1, 3])
def test_records_equal_the_two_wave_kernels(gpu, channels, n_pairs):
    """1 or 3 pairs x 2 frames per launch x 1 or 2 channels = 2, 4, 6 or 12 items per grid: no multiple of 8 but 8 itself is
    never reached either, all below the prefetch distance; 3 frames at 2 per launch leave a launch of one."""
    lengths = LENGTHS if n_pairs == 3 else [LENGTHS[2]]
    pairs = [cut(11 + i, channels, a, b) for i, (a, b) in enumerate(lengths)]
    assert max(count_frames(a, b) for a, b in lengths) == 3
    one, two = both_kernels(gpu, pairs, frames_per_launch=2)
    compare(one, two, f"{n_pairs} pair(s), {channels} channel(s)")
    if n_pairs == 1:                                 # the other two lengths as pairs of their own
        for k in (0, 1):
            o, t = both_kernels(gpu, [cut(11 + k, channels, *LENGTHS[k])], frames_per_launch=2)
            compare(o, t, f"{LENGTHS[k][0]} samples, {channels} channel(s)")


def test_grid_above_the_prefetch_distance(gpu):
    """3 stereo pairs x 11 frames per launch = 66 items: above the prefetch distance of 64 (items 0 and 1 look ahead), no
    multiple of 8 (the XCD remap's remainder), and 12 frames leave a second launch of one frame = 6 items; the shorter
    pairs end inside the first launch (workgroups that leave at once)."""
    lengths = [(12288, 12288), (12000, 11500), (11000, 12288)]
    assert [count_frames(a, b) for a, b in lengths] == [12, 11, 10]
    one, two = both_kernels(gpu, [cut(21 + i, 2, a, b) for i, (a, b) in enumerate(lengths)], frames_per_launch=11)
    compare(one, two, "66 + 6 items")


def test_identical_signals_stay_exact(gpu):
    """test == ref: the noise spectrum is zero in every bin (noise in bands at the floor, exactly) and every log ratio is
    ln 1 = 0 -- d0 = 0, the correlation 0 / 0 in every lag, no NaN power exceeds its neighbour: EHS as the two-wave
    kernel gives it."""
    r, _ = cut(31, 2, 5120, 5120)
    one, two = both_kernels(gpu, [(r, r.copy())], frames_per_launch=3)
    compare(one, two, "identical")
    assert (one[..., NOISE:NOISE + NB] == GROUP_FLOOR).all()
    assert np.array_equal(one[..., ROOT_REF:ROOT_REF + NB], one[..., ROOT_TEST:ROOT_TEST + NB])
    assert np.array_equal(one[..., EHS], two[..., EHS], equal_nan=True) and not one[..., NOISE_E].any()


@pytest.mark.parametrize("silent", ["ref", "test"])
def test_digital_silence_on_one_side(gpu, silent):
    r, t = cut(41, 2, 4096, 4096)
    if silent == "ref":
        r = np.zeros_like(r)
    else:
        t = np.zeros_like(t)
    one, two = both_kernels(gpu, [(r, t)], frames_per_launch=3)
    compare(one, two, f"silent {silent}")
    assert np.array_equal(one[..., EHS], two[..., EHS], equal_nan=True)


THR5 = np.float32(200. / 32768 / 5)


@pytest.mark.parametrize("level", [-1, 0, 1], ids=["below", "at", "above"])
def test_boundary_detector_exact_path(gpu, level):
    """Every |sample| of the reference is 200/32768/5 or a float next to it: all five-sample window sums lie within 1e-6
    of the threshold, no single sample settles it, one lane replays the reference's float recurrence."""
    v = THR5
    for _ in range(abs(level)):
        v = np.nextafter(v, np.float32(1 if level > 0 else 0), dtype=np.float32)
    assert abs(5 * float(v) - 200. / 32768) < 1e-6 and float(v) < 200. / 32768 - 1e-6
    sign = np.where(np.arange(3072) % 3 == 0, -1, 1).astype(np.float32)
    r = (sign * v)[:, None]
    t = cut(51, 1, 3072, 3072)[1]
    one, two = both_kernels(gpu, [(r, t)], frames_per_launch=2)
    compare(one, two, f"boundary {level:+d}")


def energy_frame(case):
    """-> 2048 mono samples whose second half has the energy 8000 / 32768^2 ("at") or a double next to it: float products
    that are exact, with a double sum that is exact in any order (every term a multiple of 2^-70 below 2^-17)"""
    T = Fraction(8000, 32768 ** 2)
    ulp = Fraction(1, 2 ** 70)                       # of a double in [2^-18, 2^-17)
    assert Fraction(2) ** -18 <= T < Fraction(2) ** -17
    if case == "below":
        # 124 = 10^2 + 4^2 + 2^2 + 2^2; (2^-12 (1 - 2^-23))^2 rounds to the float 2^-24 - 2^-46; 2^24 - 1 = 4095^2 + 90^2 + 9^2 + 3^2
        x = [10 / 4096, 4 / 4096, 2 / 4096, 2 / 4096, 2. ** -12 * (1 - 2. ** -23)] + [m * 2. ** -35 for m in (4095, 90, 9, 3)]
        want = T - ulp
    else:
        x = [10 / 4096, 5 / 4096] + ([2. ** -35] if case == "above" else [])
        want = T + (ulp if case == "above" else 0)
    x = np.array(x, dtype=np.float32)
    squares = x * x                                  # float products, as the kernel forms them
    assert sum(Fraction(float(s)) for s in squares) == want
    frame = np.zeros(2048, dtype=np.float32)
    frame[1024 + 7 * np.arange(len(x))] = x          # different lanes and rows
    return frame


@pytest.mark.parametrize("ref_case,test_case", [("below", "above"), ("at", "below"), ("above", "at")])
def test_energy_flag_one_ulp_around_its_threshold(gpu, ref_case, test_case):
    r, t = energy_frame(ref_case)[:, None], energy_frame(test_case)[:, None]
    one, two = both_kernels(gpu, [(r, t)], frames_per_launch=1)
    compare(one, two, f"energy {ref_case}/{test_case}")
    want = {"below": 0, "at": 1, "above": 1}
    assert (int(one[0, 0, 0, FLAGS_REF]) >> 1) == want[ref_case] and (int(one[0, 0, 0, FLAGS_TEST]) >> 1) == want[test_case]
    assert (int(two[0, 0, 0, FLAGS_REF]) >> 1) == want[ref_case] and (int(two[0, 0, 0, FLAGS_TEST]) >> 1) == want[test_case]


GATED_MOVS = ("BandwidthRefB", "BandwidthTestB", "RelDistFramesB", "ADBB", "MFPDB")


def test_batch_run_end_to_end(gpu):
    """8 ragged stereo pairs of 2-3 s through peaq_batch_run, once per kernel."""
    import gstpeaq_amd
    from gstpeaq_amd import capi
    lengths = [96000 + 6007 * i for i in range(8)]
    assert lengths[-1] <= 144000
    inputs = [synth_np.pair(61 + i, 2, n) for i, n in enumerate(lengths)]
    ctx = gpu.ctx()
    res = []
    before = capi.debug_select_frontend(ctx, 0)
    try:
        for two_waves in (0, 1):
            capi.debug_select_frontend(ctx, two_waves)
            res.append(gpu.run_batch(inputs, 0, 2))
    finally:
        capi.debug_select_frontend(ctx, before)
    one, two = res
    assert [r["frames"] for r in one] == [r["frames"] for r in two] == [count_frames(n, n) for n in lengths]
    a, b = np.array([r["movs"] for r in one]), np.array([r["movs"] for r in two])
    odg_a, odg_b = np.array([r["odg"] for r in one]), np.array([r["odg"] for r in two])
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isnan(odg_a), np.isnan(odg_b))
    for name in GATED_MOVS:
        i = capi.MOV_NAMES_BASIC.index(name)
        rel = np.abs(a[:, i] - b[:, i]) / np.maximum(np.maximum(np.abs(a[:, i]), np.abs(b[:, i])), 1e-12)
        print(f"{name}: largest relative difference {np.nanmax(rel):.3g}")
        assert int((rel > 1e-9).sum()) == 0, (name, a[:, i], b[:, i])
    ok = ~np.isnan(odg_a)
    print(f"largest |delta ODG| {np.max(np.abs(odg_a[ok] - odg_b[ok])):.3g}")
    assert np.all(np.abs(odg_a[ok] - odg_b[ok]) <= 1e-9)

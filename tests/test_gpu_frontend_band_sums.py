"""The front end's band sums by read slots (group_bands in peaq_frontend.hip, peaq_group_sched.h) against the CPU oracle on
inputs chosen for them: four frames (5120 samples), 109 and 55 bands, of
  - seeded white noise at 0.25, so that EVERY bin carries power, with the test signal = the reference x 0.5 (the
    reference's, the test's and the noise spectrum's band sums then all see the same shares) and, separately, with an
    independent seed as the test signal;
  - a sine at the frequency where the two top bands meet (107 | 108 of 109, 53 | 54 of 55) and one where band 0 meets
    band 1: the power sits on the shared edge bin, the edge weights decide who gets how much;
  - a 17.7 kHz sine: the top band, the widest -- every pair slot in use and the odd bin that is read last;
  - an 85 Hz sine: the lowest band, whose lower edge is the first bin any band reads;
  - digital silence: the floor of 1e-12;
  - a stereo pair of the white noise and the 17.7 kHz sine,
the test signal being the reference x 0.5 where nothing else is said.  The tolerances are those of
tests/test_gpu_parity.py::test_frontend_records_match_oracle: the four band fields to rtol 2e-10, noise 1e-6, EHS 1e-7,
energies 1e-12, bandwidths and flags exact.

That the white-noise case can SEE a lost bin is asserted on the CPU alone first, from a numpy spectrum of the same
frames (Hann window, outer and middle ear weighting): in every frame the smallest interior bin of every band carries
at least 1e-4 of its band's sum (taken with both edge bins at full weight, i.e. from above) -- six orders above the
band fields' tolerance and two above the noise field's.  A band of n bins of noise has a bin below that share with
probability ~ 1e-4 n per bin, so most seeds have a few such bins somewhere in four frames; the seeds are ones that
have none (109 bands: smallest share 2.9e-4; 55 bands, with bands of up to 51 bins: 1.08e-4)."""
import functools

import numpy as np
import pytest

import oracle_lib as orc

pytestmark = pytest.mark.gpu

N = 5120
N_FRAMES = 4
FS = 48000.
FRAME = 2048
SEED = {109: 393, 55: 2427}
CASES = ["white_half", "white_independent", "edge_top", "edge_bottom", "wide_17k7", "low_85", "silence", "stereo_white_17k7"]


def band_edges(bands):
    """lower and upper edge frequencies and edge bins of the FFT ear model's bands (fftearmodel.c:701-760)"""
    dz = 27. / (bands - 1)
    z_lo, z_hi = 7. * np.arcsinh(80. / 650.), 7. * np.arcsinh(18000. / 650.)
    i = np.arange(bands)
    fl = 650. * np.sinh((z_lo + i * dz) / 7.)
    fu = 650. * np.sinh(np.minimum(z_hi, z_lo + (i + 1) * dz) / 7.)
    return fl, fu, np.floor(fl / FS * FRAME + 0.5).astype(int), np.floor(fu / FS * FRAME + 0.5).astype(int)


def _sine(freq, amp):
    return (amp * np.sin(2 * np.pi * freq * np.arange(N) / FS)).astype(np.float32)[:, None]


def _white(seed):
    return (0.25 * np.random.default_rng(seed).standard_normal(N)).astype(np.float32)[:, None]


@functools.lru_cache(maxsize=None)
def _signals(bands, name):
    fu = band_edges(bands)[1]
    half = lambda r: (r, (r * np.float32(0.5)).astype(np.float32))
    if name == "white_half":
        return half(_white(SEED[bands]))
    if name == "white_independent":
        return _white(SEED[bands]), _white(SEED[bands] + 100000)
    if name == "edge_top":
        return half(_sine(fu[bands - 2], 0.5))
    if name == "edge_bottom":
        return half(_sine(fu[0], 0.5))
    if name == "wide_17k7":
        return half(_sine(17700., 0.5))
    if name == "low_85":
        return half(_sine(85., 0.5))
    if name == "silence":
        return half(np.zeros((N, 1), np.float32))
    assert name == "stereo_white_17k7"
    return half(np.concatenate([_white(SEED[bands]), _sine(17700., 0.5)], axis=1))


@functools.lru_cache(maxsize=None)
def _oracle(bands, name):
    ref, test = _signals(bands, name)
    out = orc.frontend_records(bands, ref, test, N_FRAMES)
    out.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback in the product)")
    import gpu_common
    return gpu_common


@pytest.mark.parametrize("bands", [109, 55])
def test_white_noise_shows_every_interior_bin(bands):
    _, _, lo, hi = band_edges(bands)
    x = _signals(bands, "white_half")[0][:, 0].astype(np.float64)
    window = np.sqrt(8. / 3.) * 0.5 * (1. - np.cos(2 * np.pi * np.arange(FRAME) / (FRAME - 1)))
    f_khz = np.maximum(np.arange(FRAME // 2 + 1), 1e-9) * FS / FRAME / 1000.
    weight2 = 10. ** ((-0.6 * 3.64 * f_khz ** -0.8 + 6.5 * np.exp(-0.6 * (f_khz - 3.3) ** 2) - 1e-3 * f_khz ** 3.6) / 10.)
    smallest, interior = 1., 0
    for frame in range(N_FRAMES):
        p = np.abs(np.fft.rfft(window * x[1024 * frame:1024 * frame + FRAME])) ** 2 * weight2
        for b in range(bands):
            if hi[b] - lo[b] > 1:
                share = p[lo[b] + 1:hi[b]].min() / p[lo[b]:hi[b] + 1].sum()
                smallest = min(smallest, share)
                interior += hi[b] - lo[b] - 1
    print(f"{bands} bands: {interior // N_FRAMES} interior bins, the smallest carries {smallest:.3e} of its band's sum")
    assert interior // N_FRAMES > 600          # (656 by the tables)
    assert smallest >= 1e-4, smallest


@pytest.mark.parametrize("bands", [109, 55])
@pytest.mark.parametrize("name", CASES)
def test_band_sum_inputs_match_oracle(gpu, bands, name):
    import torch
    import gstpeaq_amd
    ref, test = _signals(bands, name)
    got = gstpeaq_amd.debug_frontend(gpu.ctx(), bands, torch.from_numpy(ref).cuda(), torch.from_numpy(test).cuda(), N_FRAMES)
    exp = _oracle(bands, name)
    for field, lo in (("unsm_ref", 0), ("unsm_test", 112), ("loud_ref", 224), ("loud_test", 336)):
        if bands == 55 and field.endswith("_test"):   # the advanced version's FFT path does not compute them
            assert not got[:, :, lo:lo + bands].any(), field
            continue
        err = np.abs(got[:, :, lo:lo + bands] / exp[:, :, lo:lo + bands] - 1.)
        print(f"{bands} bands, {name}, {field}: largest relative error {np.nanmax(err):.3e}")
        np.testing.assert_allclose(got[:, :, lo:lo + bands], exp[:, :, lo:lo + bands], rtol=2e-10, atol=0, err_msg=field)
    err = np.abs(got[:, :, 448:448 + bands] / exp[:, :, 448:448 + bands] - 1.)
    print(f"{bands} bands, {name}, noise: largest relative error {np.nanmax(err):.3e}")
    np.testing.assert_allclose(got[:, :, 448:448 + bands], exp[:, :, 448:448 + bands], rtol=1e-6, atol=0, err_msg="noise")
    if bands == 109:
        assert np.array_equal(got[:, :, 560:562], exp[:, :, 560:562]), "bandwidths"
    else:
        assert not got[:, :, 560:562].any(), "bandwidths (not computed by the advanced version)"
    assert np.array_equal(got[:, :, 563:565], exp[:, :, 563:565]), "flags"
    assert np.array_equal(np.isnan(got[:, :, 562]), np.isnan(exp[:, :, 562]))
    np.testing.assert_allclose(got[:, :, 562], exp[:, :, 562], rtol=1e-7, atol=1e-13, err_msg="ehs")
    np.testing.assert_allclose(got[:, :, 565:567], exp[:, :, 565:567], rtol=1e-12, atol=0, err_msg="energies")

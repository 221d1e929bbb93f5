"""The front end's two-stream upward spreading (peaq_frontend.hip, peaq_spread_sched.h) against the CPU oracle on inputs
chosen for it: four frames (5120 samples) of
  - a 250 Hz sine at 0.9: all energy in the lowest lanes, whose FAR terms (the helper stream's) are what the top bands get;
  - 250 Hz + 1 kHz + 6 kHz at 0.3 each;
  - a 15 kHz sine at 0.9: sources only in the top lanes, nothing may leak into the helper's lanes;
  - 100 Hz at 1e-4 and digital silence: the steepest slopes, the a^-0.8 underflow guard;
  - a stereo pair of the first and the third,
the test signal being the reference x 0.5 throughout.  The tolerances are those of
tests/test_gpu_parity.py::test_frontend_records_match_oracle: the four band fields to rtol 2e-10, noise 1e-6, EHS 1e-7,
energies 1e-12, bandwidths and flags exact.

That the far terms are VISIBLE in the 250 Hz case is asserted on the oracle alone first: its unsmeared excitation in the
top nine bands of 109 (100 .. 108) and the top five of 55 (50 .. 54) exceeds the digital-silence record's by at least
1e-6 relative -- four orders above the tolerance, so a lost or misplaced far term fails the comparison."""
import functools

import numpy as np
import pytest

import oracle_lib as orc

pytestmark = pytest.mark.gpu

N = 5120
N_FRAMES = 4
FS = 48000.


def _sine(freq, amp):
    return (amp * np.sin(2 * np.pi * freq * np.arange(N) / FS)).astype(np.float32)[:, None]


@functools.lru_cache(maxsize=None)
def _ref(name):
    if name == "low_250":
        return _sine(250., 0.9)
    if name == "three_tones":
        return (_sine(250., 0.3) + _sine(1000., 0.3) + _sine(6000., 0.3)).astype(np.float32)
    if name == "high_15k":
        return _sine(15000., 0.9)
    if name == "faint_100":
        return _sine(100., 1e-4)
    if name == "silence":
        return np.zeros((N, 1), np.float32)
    assert name == "stereo_low_high"
    return np.concatenate([_ref("low_250"), _ref("high_15k")], axis=1)


@functools.lru_cache(maxsize=None)
def _oracle(bands, name):
    ref = _ref(name)
    out = orc.frontend_records(bands, ref, (ref * np.float32(0.5)).astype(np.float32), N_FRAMES)
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
def test_far_terms_are_visible_to_the_oracle(bands):
    top = range(100, 109) if bands == 109 else range(50, 55)
    tone, silent = _oracle(bands, "low_250"), _oracle(bands, "silence")
    for b in top:
        excess = tone[:, 0, b] / silent[:, 0, b] - 1.
        print(f"{bands} bands, band {b}: unsmeared excitation of the 250 Hz tone over silence's by {excess.min():.3e} relative")
        assert (excess >= 1e-6).all(), (b, excess)


@pytest.mark.parametrize("bands", [109, 55])
@pytest.mark.parametrize("name", ["low_250", "three_tones", "high_15k", "faint_100", "silence", "stereo_low_high"])
def test_spreading_inputs_match_oracle(gpu, bands, name):
    import torch
    import gstpeaq_amd
    ref = _ref(name)
    test = (ref * np.float32(0.5)).astype(np.float32)
    got = gstpeaq_amd.debug_frontend(gpu.ctx(), bands, torch.from_numpy(ref).cuda(), torch.from_numpy(test).cuda(), N_FRAMES)
    exp = _oracle(bands, name)
    for field, lo in (("unsm_ref", 0), ("unsm_test", 112), ("loud_ref", 224), ("loud_test", 336)):
        if bands == 55 and field.endswith("_test"):   # the advanced version's FFT path does not compute them
            assert not got[:, :, lo:lo + bands].any(), field
            continue
        err = np.abs(got[:, :, lo:lo + bands] / exp[:, :, lo:lo + bands] - 1.)
        print(f"{bands} bands, {name}, {field}: largest relative error {np.nanmax(err):.3e}")
        np.testing.assert_allclose(got[:, :, lo:lo + bands], exp[:, :, lo:lo + bands], rtol=2e-10, atol=0, err_msg=field)
    np.testing.assert_allclose(got[:, :, 448:448 + bands], exp[:, :, 448:448 + bands], rtol=1e-6, atol=0, err_msg="noise")
    if bands == 109:
        assert np.array_equal(got[:, :, 560:562], exp[:, :, 560:562]), "bandwidths"
    else:
        assert not got[:, :, 560:562].any(), "bandwidths (not computed by the advanced version)"
    assert np.array_equal(got[:, :, 563:565], exp[:, :, 563:565]), "flags"
    assert np.array_equal(np.isnan(got[:, :, 562]), np.isnan(exp[:, :, 562]))
    np.testing.assert_allclose(got[:, :, 562], exp[:, :, 562], rtol=1e-7, atol=1e-13, err_msg="ehs")
    np.testing.assert_allclose(got[:, :, 565:567], exp[:, :, 565:567], rtol=1e-12, atol=0, err_msg="energies")

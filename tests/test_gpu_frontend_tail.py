"""The front end's bandwidth search and error-harmonic-structure tail against the CPU oracle, stage level
(gstpeaq_amd.debug_frontend on tiny inputs, fields and tolerances of test_gpu_parity.test_frontend_records_match_oracle).

Bandwidth search (movs.c:776-809).  The kernel holds the power spectrum in 16 register slots of 64 bins -- direct slots
q = 0..7 with bin 64 q + lane, mirror slots with bin 1024 - 64 q - lane, bin 512 in lane 0 of mirror slot 0 -- and walks
them from the top of the spectrum down, leaving at the first slot with a hit.  The cases put the top significant bin on
both sides of every slot boundary the search can meet, of the bw_ref > 346 gate and of the 921 limit: a sine centred on
bin B - 1 reaches bin B through the Hann window's main lobe (a quarter of the peak's power) and bin B + 1 only through
the leakage of the window's N - 1 denominator (-72 dB); white noise of sigma 0.01 on the test signal alone puts the zero
threshold (the test spectrum's maximum over bins 921..1023), times 10 and times 3.16, some 40 dB below the peak --
between the two.  Every case first checks on the oracle's own records that the bandwidth of the full frames IS B + 1.

Error harmonic structure (movs.c:1279-1441): both settings of EHS_SUBTRACT_DC_BEFORE_WINDOW and
CENTER_EHS_CORRELATION_WINDOW (two window tables, one set of twiddles for both transforms), on a stereo pair, on
identical signals (d0 = 0: NaN in every lag) and through the 55-band kernel, whose EHS runs on the test wave.  Needs an MI355X."""
import functools

import numpy as np
import pytest

import cases as case_defs
import oracle_lib as orc

pytestmark = pytest.mark.gpu

N = 12288                                           # ten full frames + the flush frames
N_FRAMES = (N - 2048) // 1024 + 2
FULL = 10                                           # frames 0..9 lie wholly inside the signal
BW_BINS = (345, 346, 347, 383, 384, 385, 447, 448, 511, 512, 513, 575, 576, 639, 640, 703, 704, 767, 768, 831, 832, 895,
           896, 919, 920)


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback in the product)")
    import gpu_common
    return gpu_common


def _sine(top_bin, amp=0.5):
    """mono, centred on bin top_bin - 1 of the 2048-point transform: top_bin is the highest bin of its main lobe"""
    n = np.arange(N, dtype=np.float64)
    return (amp * np.sin(2 * np.pi * (top_bin - 1) * n / 2048.)).astype(np.float32)[:, None]


def _noise(sigma=0.01, seed=1234):
    return (sigma * np.random.RandomState(seed).standard_normal(N)).astype(np.float32)[:, None]


@functools.lru_cache(maxsize=None)
def _bw_case(name):
    """-> (ref, test, the (bw_ref, bw_test) the full frames are built to have)"""
    if isinstance(name, int):                        # reference and test reach up to the same bin
        return _sine(name), _sine(name) + _noise(), (name + 1, name + 1 if name + 1 > 346 else 0)
    if name == "nothing":                            # no reference bin above ten times a loud test floor
        return _sine(600, 1e-4), _noise(0.1), (0, 0)
    if name == "test-noise-only":                    # reference passes the gate, no test bin reaches the threshold
        return _sine(600), _noise(), (601, 0)
    if name == "test-below-ref":                     # the test search starts at bw_ref and finds its own top further down
        return _sine(703), _sine(450) + _noise(), (704, 451)
    if name == "test-above-ref":                     # test content beyond bw_ref is masked by the limit: slot 640..703
        return _sine(650), _sine(650) + _sine(800, 0.25) + _noise(), (651, 651)
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def _bw_oracle(name):
    ref, test, _ = _bw_case(name)
    return orc.frontend_records(109, ref, test, N_FRAMES)


def _compare(got, exp, bands):
    """the checks of test_frontend_records_match_oracle"""
    for name, lo in (("unsm_ref", 0), ("unsm_test", 112), ("loud_ref", 224), ("loud_test", 336)):
        if bands == 55 and name.endswith("_test"):
            assert not got[:, :, lo:lo + bands].any(), name
            continue
        np.testing.assert_allclose(got[:, :, lo:lo + bands], exp[:, :, lo:lo + bands], rtol=2e-10, atol=0, err_msg=name)
    np.testing.assert_allclose(got[:, :, 448:448 + bands], exp[:, :, 448:448 + bands], rtol=1e-6, atol=0, err_msg="noise")
    if bands == 109:
        assert np.array_equal(got[:, :, 560:562], exp[:, :, 560:562]), ("bandwidths", got[:, :, 560:562], exp[:, :, 560:562])
    else:
        assert not got[:, :, 560:562].any(), "bandwidths (not computed by the advanced version)"
    assert np.array_equal(got[:, :, 563:565], exp[:, :, 563:565]), "flags"
    assert np.array_equal(np.isnan(got[:, :, 562]), np.isnan(exp[:, :, 562]))
    np.testing.assert_allclose(got[:, :, 562], exp[:, :, 562], rtol=1e-7, atol=1e-13, err_msg="ehs")
    np.testing.assert_allclose(got[:, :, 565:567], exp[:, :, 565:567], rtol=1e-12, atol=0, err_msg="energies")


@pytest.mark.parametrize("name", [*BW_BINS, "nothing", "test-noise-only", "test-below-ref", "test-above-ref"],
                         ids=lambda v: f"top{v}" if isinstance(v, int) else v)
def test_bandwidth_search_at_every_slot_boundary(gpu, name):
    import torch
    import gstpeaq_amd
    ref, test, want = _bw_case(name)
    exp = _bw_oracle(name)
    # the input is what it claims to be: by the oracle alone
    assert (exp[:FULL, 0, 560] == want[0]).all() and (exp[:FULL, 0, 561] == want[1]).all(), (want, exp[:, 0, 560:562])
    got = gstpeaq_amd.debug_frontend(gpu.ctx(), 109, torch.from_numpy(ref).cuda(), torch.from_numpy(test).cuda(), N_FRAMES)
    assert np.array_equal(got[:, :, 560:562], exp[:, :, 560:562]), (got[:, 0, 560:562], exp[:, 0, 560:562])
    _compare(got, exp, 109)


EHS_CASES = {"stereo": dict(kind="synth", seed=6, channels=2, n=N),
             "identical": dict(kind="synth", seed=6, channels=2, n=N, identical=1)}


@functools.lru_cache(maxsize=None)
def _ehs_inputs(case):
    return case_defs.make_inputs(EHS_CASES[case])


@functools.lru_cache(maxsize=None)
def _ehs_oracle(case, bands, dc_before, centred):
    ref, test = _ehs_inputs(case)
    try:
        orc.set_settings(ehs_subtract_dc_before_window=dc_before, center_ehs_correlation_window=centred)
        return orc.frontend_records(bands, ref, test, N_FRAMES)
    finally:
        orc.set_settings()


@pytest.mark.parametrize("centred", [0, 1])
@pytest.mark.parametrize("dc_before", [0, 1])
@pytest.mark.parametrize("case,bands", [("stereo", 109), ("identical", 109), ("stereo", 55)])
def test_ehs_on_both_settings_of_its_switches(gpu, case, bands, dc_before, centred):
    import torch
    import gstpeaq_amd
    ref, test = _ehs_inputs(case)
    exp = _ehs_oracle(case, bands, dc_before, centred)
    if case == "identical":
        # d0 = 0: the correlation is the reference's 0 / 0 in every lag, no NaN power exceeds its neighbour, the peak is 0
        assert (exp[:FULL, :, 562] == 0).all() and (exp[:FULL, :, 563].astype(int) & 2).all()   # (frames with energy)
    else:
        assert np.isfinite(exp[:FULL, :, 562]).all() and (exp[:FULL, :, 562] > 0).all()
        # the switches reach the result: each setting's EHS is another number
        other = _ehs_oracle(case, bands, 1 - dc_before, centred), _ehs_oracle(case, bands, dc_before, 1 - centred)
        assert all(not np.allclose(o[:FULL, :, 562], exp[:FULL, :, 562], rtol=1e-6, atol=0) for o in other)
    ctx = gpu.ctx()
    try:
        ctx.set_settings(ehs_subtract_dc_before_window=dc_before, center_ehs_correlation_window=centred)
        got = gstpeaq_amd.debug_frontend(ctx, bands, torch.from_numpy(ref).cuda(), torch.from_numpy(test).cuda(), N_FRAMES)
    finally:
        ctx.set_settings()
    _compare(got, exp, bands)

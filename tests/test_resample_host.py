"""Host side of the device rate converter (include/peaq_amd.h: peaq_resample_supported, peaq_resampled_length,
peaq_batch_resample, peaq_run_pair_rate), without a GPU: the length rule against the real chain's recorded lengths,
against the rule itself and against the CLI's converter; the supported rates; argument checks that need no device;
header and exports."""
import ctypes as C
import json
import math
import re
from pathlib import Path

import numpy as np
import pytest

import test_cli_resampler as cli

ROOT = Path(__file__).resolve().parent.parent
GOLD = json.loads((ROOT / "tests" / "golden" / "ref_e2e_resampled.json").read_text())
RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 88200, 96000, 176400, 192000)
NEW = ("peaq_resample_supported", "peaq_resampled_length", "peaq_batch_resample", "peaq_run_pair_rate",
       "peaq_resample_plan_info")


@pytest.fixture(scope="module")
def lib():
    import gstpeaq_amd
    if not gstpeaq_amd.library_path().exists():
        gstpeaq_amd.build_library()
    L = gstpeaq_amd.load_library()
    L.peaq_resampled_length.restype = C.c_uint32
    L.peaq_resampled_length.argtypes = [C.c_uint64, C.c_uint32]
    L.peaq_resample_supported.argtypes = [C.c_uint32]
    return L


def rule(n, rate):
    return (n - 1) * 48000 // rate + 1 if n else 0


def test_length_of_the_real_chain(lib):
    """audioresample's output lengths, recorded from the reference chain"""
    assert len(GOLD["records"]) == 8
    for rec in GOLD["records"]:
        case = rec["case"]
        ref, _ = __import__("cases").make_inputs(case)
        assert lib.peaq_resampled_length(len(ref), case["rate"]) == rec["samples_48k"], case["name"]


def test_length_rule_and_overflow(lib):
    for rate in RATES:
        for n in (0, 1, 2, 147, 148, 44100, 441000, 2 ** 31):
            exp = rule(n, rate)
            got = lib.peaq_resampled_length(n, rate)
            if exp > 0xFFFFFFFF:
                assert got == 0 and b"2^32" in lib.peaq_last_error(), (rate, n)
            else:
                assert got == exp, (rate, n, got, exp)
                assert lib.peaq_last_error() == b"", (rate, n)
                # the CLI evaluates the rule in double: the two never disagree by a sample
                assert exp == (math.floor(float(n - 1) * (48000. / rate)) + 1 if n else 0)
    assert rule(2 ** 31, 96000) == lib.peaq_resampled_length(2 ** 31, 96000) == 2 ** 30
    assert rule(2 ** 31, 8000) > 0xFFFFFFFF and lib.peaq_resampled_length(2 ** 31, 8000) == 0
    assert lib.peaq_last_error() != b""
    assert lib.peaq_resampled_length(100, 0) == 0 and b"rate" in lib.peaq_last_error()
    import gstpeaq_amd
    assert gstpeaq_amd.resampled_length(148, 44100) == 161
    with pytest.raises(gstpeaq_amd.PeaqError):
        gstpeaq_amd.resampled_length(2 ** 31, 8000)


@pytest.mark.skipif(not cli.CLI.exists(), reason="gstpeaq_amd/cli/peaq not built")
@pytest.mark.parametrize("rate,n", [(44100, 44100 + 148), (96000, 96001)])
def test_length_equals_the_cli_converters(lib, tmp_path, rate, n):
    x = (0.1 * np.sin(np.arange(n) * 0.05))[:, None].astype(np.float32)
    r48, t48 = cli.cli_dump(tmp_path, dict(kind="raw", rate=rate, channels=1, _x=x))
    assert len(r48) == len(t48) == lib.peaq_resampled_length(n, rate)


def test_supported_rates(lib):
    import gstpeaq_amd
    for rate in RATES + (384000, 44112):
        assert lib.peaq_resample_supported(rate) == 1, rate
        assert gstpeaq_amd.resample_supported(rate) is True
    for rate in (48000, 44101, 7999, 0, 384001, 48001):
        assert lib.peaq_resample_supported(rate) == 0, rate
        assert gstpeaq_amd.resample_supported(rate) is False


def test_argument_checks_that_need_no_device(lib):
    """rate, channels and n_pairs are looked at before the context: PEAQ_ERR_ARG with a message that names the rate"""
    vp, u32p = C.c_void_p, C.POINTER(C.c_uint32)
    lib.peaq_batch_resample.argtypes = [vp, C.c_int, C.c_uint32, C.c_int, vp, C.c_size_t, u32p, C.c_uint32, vp,
                                        C.c_size_t, u32p, vp]
    for rate in (48000, 44101, 7999):
        assert lib.peaq_batch_resample(None, 2, rate, 1, None, 0, None, 0, None, 0, None, None) == -1
        assert str(rate).encode() in lib.peaq_last_error()
    assert lib.peaq_batch_resample(None, 3, 44100, 1, None, 0, None, 0, None, 0, None, None) == -1
    assert b"channels" in lib.peaq_last_error()
    assert lib.peaq_batch_resample(None, 2, 44100, -1, None, 0, None, 0, None, 0, None, None) == -1
    assert b"n_pairs" in lib.peaq_last_error()
    assert lib.peaq_batch_resample(None, 2, 44100, 1, None, 0, None, 0, None, 0, None, None) == -1
    assert b"NULL" in lib.peaq_last_error()
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    lib.peaq_run_pair_rate.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_uint32, fp, C.c_size_t, fp, C.c_size_t, dp]
    assert lib.peaq_run_pair_rate(None, 0, 2, 92., 44101, None, 0, None, 0, None) == -1
    assert b"44101" in lib.peaq_last_error()
    assert lib.peaq_run_pair_rate(None, 0, 2, 92., 44100, None, 0, None, 0, None) == -1
    assert b"NULL" in lib.peaq_last_error()
    assert lib.peaq_run_pair_rate(None, 0, 2, 92., 48000, None, 0, None, 0, None) == -1     # peaq_run_pair's own check
    assert lib.peaq_batch_resample(None, 2, 44100, 65536, None, 0, None, 0, None, 0, None, None) == -1
    assert b"65535" in lib.peaq_last_error()
    import gstpeaq_amd
    assert lib.peaq_resample_plan_info(44100, None) == -1 and b"NULL" in lib.peaq_last_error()
    for rate in (48000, 44101):
        with pytest.raises(gstpeaq_amd.PeaqError, match=str(rate)):
            gstpeaq_amd.resample_plan(rate)


def test_header_declares_and_library_exports_the_converter(lib):
    hdr = (ROOT / "include" / "peaq_amd.h").read_text()
    assert "peaq.c:154-209" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(peaq_[a-z_0-9]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), f"{name} is declared in include/peaq_amd.h but not exported"
    import gstpeaq_amd
    for name in ("resample", "resampled_length", "resample_supported"):
        assert callable(getattr(gstpeaq_amd, name))

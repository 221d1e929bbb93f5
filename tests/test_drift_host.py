"""The host side of the drift stage without a GPU (include/peaq_amd.h, "constant drift on the device"): the Theil-Sen
fit against ten lines of numpy, peaq_drift_index against exact integer arithmetic, peaq_drift_lengths against brute
force, the record's size and constants, the workspace figure, and the argument checks of peaq_batch_estimate_drift,
peaq_batch_cut_drift and peaq_run_pair_drift, which return PEAQ_ERR_ARG with the offending value in the message before
any device is touched (a NULL context is the last thing they look at)."""
import ctypes as C
import math
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import gstpeaq_amd

PEAQ_ERR_ARG = -1
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib():
    if not gstpeaq_amd.library_path().exists():
        gstpeaq_amd.build_library()
    return gstpeaq_amd.load_library()


def err(lib):
    return lib.peaq_last_error().decode()


def u32(*v):
    return (C.c_uint32 * len(v))(*v)


def i32(*v):
    return (C.c_int32 * len(v))(*v)


def f64(*v):
    return (C.c_double * len(v))(*v)


def header_text():
    return (ROOT / "include" / "peaq_amd.h").read_text()


def header_define(name):
    return re.search(r"^#define\s+%s\s+(\S+)" % name, header_text(), flags=re.M).group(1)


# ---- the fit -------------------------------------------------------------------------------------------------------
def theil_sen(d, x, valid=None):
    """the header's fit in numpy: every operation an IEEE double operation, medians after a sort"""
    d, x = np.asarray(d, np.float64), np.asarray(x, np.float64)
    keep = np.ones(len(d), bool) if valid is None else np.asarray(valid, bool)
    d, x = d[keep], x[keep]
    if len(d) < 3:
        return 0.0, 0.0, len(d)
    i, j = np.triu_indices(len(d), 1)
    e = np.median(np.sort((d[j] - d[i]) / (x[j] - x[i])))
    a = np.median(np.sort(d - e * x))
    return float(a), float(e), len(d)


def centres(n, window=4096):
    return np.arange(n) * float(window) + window // 2


@pytest.mark.parametrize("n", [3, 4, 5, 8, 29, 30, 117, 400])
def test_fit_is_the_numpy_theil_sen_on_random_sets(lib, n):
    rng = np.random.default_rng(n)
    for trial in range(6):
        x = centres(n, (4096, 16384, 32768)[trial % 3])
        d = (rng.integers(-40, 40, n) + rng.integers(-128, 128, n) / 256.0) if trial % 2 else rng.normal(0, 5, n)
        assert gstpeaq_amd.drift_fit(d, x) == theil_sen(d, x), (n, trial)


@pytest.mark.parametrize("n", [10, 41, 200])
def test_fit_with_gross_outliers_is_the_numpy_one_and_stays_on_the_line(lib, n):
    rng = np.random.default_rng(100 + n)
    x = centres(n, 16384)
    e_true, a_true = 1.5e-4, -7.25
    d = np.round((a_true + e_true * x + rng.normal(0, 0.004, n)) * 256) / 256
    bad = rng.choice(n, (3 * n) // 10, replace=False)
    d[bad] = rng.integers(-1000, 1000, len(bad))
    a, e, nv = gstpeaq_amd.drift_fit(d, x)
    assert (a, e, nv) == theil_sen(d, x)
    assert abs(e - e_true) < 2e-6 and abs(a - a_true) < 0.05, (a, e)


def test_fit_honours_valid_and_needs_three_points(lib):
    rng = np.random.default_rng(7)
    x = centres(12)
    d = rng.normal(0, 3, 12)
    for mask in ([1] * 12, [1, 0] * 6, [0, 0, 1, 1, 1] + [0] * 7, [1, 1] + [0] * 10, [0] * 12, [0, 1, 0, 0, 0, 2, 0, 0, 0, 0, 0, 255]):
        assert gstpeaq_amd.drift_fit(d, x, mask) == theil_sen(d, x, mask), mask
    assert gstpeaq_amd.drift_fit(d[:2], x[:2]) == (0.0, 0.0, 2)
    assert gstpeaq_amd.drift_fit([], []) == (0.0, 0.0, 0)
    # three points: the middle one of three slopes, of three offsets
    assert gstpeaq_amd.drift_fit([0.0, 1.0, 4.0], [0.0, 1.0, 2.0]) == theil_sen([0.0, 1.0, 4.0], [0.0, 1.0, 2.0]) == (0.0, 2.0, 3)
    # an even count takes the mean of the two middle values
    a, e, _ = gstpeaq_amd.drift_fit([0.0, 1.0, 3.0, 6.0], [0.0, 1.0, 2.0, 3.0])
    assert e == 2.0 and (a, e, 4) == theil_sen([0.0, 1.0, 3.0, 6.0], [0.0, 1.0, 2.0, 3.0])


def test_fit_refuses(lib):
    d = f64(0, 1, 2)
    a, e = C.c_double(5), C.c_double(5)
    assert lib.peaq_drift_fit(d, d, None, 3, None, C.byref(e)) == PEAQ_ERR_ARG and "NULL" in err(lib)
    assert lib.peaq_drift_fit(None, d, None, 3, C.byref(a), C.byref(e)) == PEAQ_ERR_ARG and "NULL" in err(lib)
    assert (a.value, e.value) == (0.0, 0.0)
    big = (C.c_double * 4097)()
    assert lib.peaq_drift_fit(big, big, None, 4097, C.byref(a), C.byref(e)) == PEAQ_ERR_ARG and "4097 points" in err(lib) \
        and "4096" in err(lib), err(lib)


# ---- the index -----------------------------------------------------------------------------------------------------
def index_exact(a, e, i):
    """peaq_drift_index in exact arithmetic: the fused multiply-add is the double nearest to the exact e i + a
    (math.fma where Python has it), the product with 256 is exact, rint rounds to nearest even"""
    if hasattr(math, "fma"):
        t = math.fma(e, float(i), a)
    else:
        exact = Fraction(e) * i + Fraction(a)
        t = exact.numerator / exact.denominator          # (int / int is correctly rounded)
    g = int(np.rint(256.0 * t))
    m = (g + 128) // 256
    return m, g - 256 * m


def test_index_is_the_exact_arithmetic(lib):
    rng = np.random.default_rng(3)
    cases = [(0.0, 0.0, 0)]
    for q in (-128, -1, 0, 1, 127, 128, -129, 383):
        for i in (0, 1, 999999, 2 ** 32 - 1):
            cases.append((q / 256, 0.0, i))
    for _ in range(4000):
        a = float(rng.uniform(-70000, 70000)) if rng.integers(2) else float(rng.uniform(-2, 2))
        e = float(rng.uniform(-1e-3, 1e-3))
        i = int(rng.integers(0, 2 ** 32)) if rng.integers(2) else int(rng.integers(-5000, 5000))
        cases.append((a, e, i))
    for i in (2 ** 32 - 1, 2 ** 32 - 2, 2 ** 32, 2 ** 32 + 5, -2 ** 31):
        for e in (1e-3, -1e-3, 3.73e-5, -3.73e-5):
            cases.append((-0.37, e, i))
    for a, e, i in cases:
        m, phi = gstpeaq_amd.drift_index(a, e, i)
        assert (m, phi) == index_exact(a, e, i), (a, e, i)
        assert -128 <= phi <= 127
    # with e = 0 and a = q / 256 the index is (0, q) for every i: the shifted cut's grid point
    for q in range(-128, 128):
        assert gstpeaq_amd.drift_index(q / 256, 0.0, 2 ** 31 + q) == (0, q)


def test_index_rounds_exact_halves_to_even(lib):
    # 256 (a + e i) = k + 1/2 exactly: a = (2 k + 1) / 512 with e = 0, and e = 2^-12, i = 8 mod 16
    for k in (-130, -129, -128, -3, -2, -1, 0, 1, 2, 126, 127, 128, 255, 256):
        a = (2 * k + 1) / 512
        g = k if k % 2 == 0 else k + 1
        m = (g + 128) // 256
        assert gstpeaq_amd.drift_index(a, 0.0, 17) == (m, g - 256 * m), k
    e = 2.0 ** -12
    for i in (8, 24, 40, 16 * 12345 + 8, -8, -24):
        assert (256 * e * i) % 1 == 0.5
        assert gstpeaq_amd.drift_index(0.0, e, i) == index_exact(0.0, e, i) == ((round(256 * e * i) + 128) // 256, (round(256 * e * i) + 128) % 256 - 128)


def test_index_at_negative_positions(lib):
    for i in (-1, -255, -256, -257, -100000):
        for a, e in ((0.0, 1e-3), (17.5, -1e-3), (-0.37, 3.73e-5)):
            assert gstpeaq_amd.drift_index(a, e, i) == index_exact(a, e, i)
    assert gstpeaq_amd.drift_index(-0.5, 0.0, 0) == (0, -128)
    assert gstpeaq_amd.drift_index(-0.50390625, 0.0, 0) == (-1, 127)       # g = -129
    assert gstpeaq_amd.drift_index(0.49609375, 0.0, 0) == (0, 127) and gstpeaq_amd.drift_index(0.5, 0.0, 0) == (1, -128)


# ---- the lengths ---------------------------------------------------------------------------------------------------
def lengths_brute(lag0, a, e, n_ref, n_test):
    sr, st, common = gstpeaq_amd.aligned_lengths(lag0, n_ref, n_test)
    keep = 0
    for i in range(common):
        m, _ = index_exact(a, e, i)
        if not st + i + m < n_test:
            break
        keep += 1
    return sr, st, keep


def test_lengths_against_brute_force(lib):
    rng = np.random.default_rng(11)
    cases = [(0, 0.0, 0.0, 100, 100), (0, 0.5, 0.0, 100, 100), (0, 0.49, 0.0, 100, 100), (3, 2.0, 0.0, 50, 60),
             (-3, 2.0, 0.0, 50, 40), (0, -5.0, 1e-3, 300, 300), (0, 5.0, -1e-3, 300, 300), (10, 0.0, 1e-3, 0, 5),
             (0, 400.0, 0.0, 300, 300), (500, 0.0, 0.0, 300, 300), (-500, 1.0, 0.0, 300, 300)]
    for _ in range(300):
        cases.append((int(rng.integers(-30, 30)), float(rng.uniform(-6, 6)), float(rng.uniform(-1e-3, 1e-3)),
                      int(rng.integers(0, 900)), int(rng.integers(0, 900))))
    for lag0, a, e, n_ref, n_test in cases:
        got = gstpeaq_amd.drift_lengths(lag0, a, e, n_ref, n_test)
        assert got == lengths_brute(lag0, a, e, n_ref, n_test), (lag0, a, e, n_ref, n_test)
        assert got[:2] == gstpeaq_amd.aligned_lengths(lag0, n_ref, n_test)[:2]
        assert got[1] + got[2] <= n_test and got[0] + got[2] <= n_ref


def test_lengths_of_a_long_pair(lib):
    n = 2 ** 32 - 1
    sr, st, keep = gstpeaq_amd.drift_lengths(7, -2.25, 1e-3, n, n)
    assert (sr, st) == (0, 7)
    last = index_exact(-2.25, 1e-3, keep - 1)[0]
    assert st + keep - 1 + last < n <= st + keep + index_exact(-2.25, 1e-3, keep)[0]
    assert gstpeaq_amd.drift_lengths(7, -2.25, -1e-3, n, n) == (0, 7, n - 7)
    assert gstpeaq_amd.drift_windows(7, n, n, 4096) == (n - 7) // 4096 and gstpeaq_amd.drift_windows(0, 10 ** 6, 10 ** 6, 4095) == 0


# ---- record, constants, workspace, surface -----------------------------------------------------------------------------
def test_record_size_and_constants(lib):
    assert lib.peaq_drift_size() == 48 == C.sizeof(gstpeaq_amd.Drift) == gstpeaq_amd.DRIFT_DTYPE.itemsize
    assert [n for n, _ in gstpeaq_amd.Drift._fields_] == list(gstpeaq_amd.DRIFT_DTYPE.names)
    assert int(header_define("PEAQ_DRIFT_F_NONE")) == gstpeaq_amd.DRIFT_F_NONE == 1
    assert int(header_define("PEAQ_DRIFT_F_RANGE")) == gstpeaq_amd.DRIFT_F_RANGE == 2
    assert float(header_define("PEAQ_DRIFT_MAX_E")) == gstpeaq_amd.DRIFT_MAX_E == 1e-3
    assert header_define("PEAQ_DRIFT_MIN_WINDOW") == "4096u" and header_define("PEAQ_DRIFT_MAX_WINDOWS") == "4096u"
    assert gstpeaq_amd.DRIFT_MAX_WINDOWS == 4096 and gstpeaq_amd.DRIFT_WINDOW == 32768 and gstpeaq_amd.DRIFT_MIN_CORR == 0.5


def test_header_and_exports_stay_in_step(lib):
    hdr = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(peaq_[a-z_0-9]*drift[a-z_0-9]*)\s*\(", hdr)))
    assert declared == ["peaq_batch_cut_drift", "peaq_batch_estimate_drift", "peaq_drift_fit", "peaq_drift_index",
                        "peaq_drift_lengths", "peaq_drift_size", "peaq_drift_windows", "peaq_drift_workspace_bytes",
                        "peaq_run_pair_drift"]
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in include/peaq_amd.h but not exported"
    for name in ("estimate_drift", "cut_drift", "drift_lengths"):
        assert callable(getattr(gstpeaq_amd, name))


def test_workspace_figure():
    ws = gstpeaq_amd.drift_workspace_bytes
    assert ws(3, 1, 4096, 1) == 0 and ws(2, 0, 4096, 1) == 0 and ws(2, 65536, 4096, 1) == 0
    assert ws(2, 1, 4095, 1) == 0 and ws(2, 1, (1 << 20) + 1, 1) == 0 and ws(2, 1, 4096, 0) == 0 and ws(2, 1, 4096, 4097) == 0
    slot = 2 * 4096 * 4
    assert ws(1, 1, 4096, 1) == slot and ws(2, 1, 4096, 5) == 2 * 5 * slot and ws(2, 3, 4096, 5) == 3 * 2 * 5 * slot
    assert ws(1, 65535, 4096, 1) == (1 << 30) // slot * slot           # the staging budget
    assert ws(1, 65535, 4096, 4096) == 1 << 30                          # (8 pairs: below the 65535 slots of a grid's y extent)
    assert ws(2, 9, 1 << 20, 4096) == 4096 * 2 * (1 << 20) * 8         # one pair's slots are more than the budget


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_estimate_drift_checks_its_arguments_before_any_device(lib):
    a, b, o1, o2 = (C.c_float * 8)(), (C.c_float * 8)(), (C.c_char * 8)(), (C.c_char * 8)()
    p, q, r1, r2 = (C.cast(x, C.c_void_p) for x in (a, b, o1, o2))
    rec = (gstpeaq_amd.Drift * 3)()

    def call(channels=2, n_pairs=3, d_ref=p, d_test=q, stride=20000, n_ref=u32(20000, 9000, 13), n_test=u32(20000, 20000, 1),
             n_uniform=0, lag0=i32(0, -3, 100), window=4096, R=1024, min_corr=0.5, max_e=1e-3, w_max=4, dl=r1, sb=r2, out=rec):
        return lib.peaq_batch_estimate_drift(None, channels, n_pairs, d_ref, d_test, stride, n_ref, n_test, n_uniform, lag0,
                                             window, R, min_corr, max_e, w_max, dl, sb, out, None)

    for bad in (0, 4095, (1 << 20) + 1):
        assert call(window=bad, R=1) == PEAQ_ERR_ARG and "window %d" % bad in err(lib) and "4096" in err(lib), err(lib)
    for bad in (0, 1025, 16385):
        assert call(R=bad) == PEAQ_ERR_ARG and "R %d" % bad in err(lib) and "1024" in err(lib), err(lib)
    assert call(window=1 << 20, R=16385) == PEAQ_ERR_ARG and "R 16385" in err(lib) and "16384" in err(lib), err(lib)
    for bad in (-0.1, 1.5, float("nan")):
        assert call(min_corr=bad) == PEAQ_ERR_ARG and "min_corr" in err(lib), err(lib)
    for bad in (0.0, -1e-4, 1.1e-3, float("nan")):
        assert call(max_e=bad) == PEAQ_ERR_ARG and "max_e" in err(lib), err(lib)
    assert call(max_e=1.1e-3) == PEAQ_ERR_ARG and "0.0011" in err(lib), err(lib)
    for bad in (0, 3):
        assert call(channels=bad) == PEAQ_ERR_ARG and "channels" in err(lib) and str(bad) in err(lib), err(lib)
    assert call(n_pairs=65536) == PEAQ_ERR_ARG and "65536 pairs" in err(lib), err(lib)
    assert call(n_pairs=-1) == PEAQ_ERR_ARG and "-1" in err(lib), err(lib)
    for bad in (0, 4097):
        assert call(w_max=bad) == PEAQ_ERR_ARG and "w_max %d" % bad in err(lib), err(lib)
    assert call(w_max=3) == PEAQ_ERR_ARG and "pair 0" in err(lib) and "4 windows" in err(lib) and "w_max 3" in err(lib), err(lib)
    for name in ("d_ref", "d_test", "dl", "sb"):
        assert call(**{name: None}) == PEAQ_ERR_ARG and "NULL buffer" in err(lib), err(lib)
    for name in ("lag0", "out"):
        assert call(**{name: None}) == PEAQ_ERR_ARG and "NULL lag0 or out" in err(lib), err(lib)
    assert call(n_test=None) == PEAQ_ERR_ARG and "both" in err(lib), err(lib)
    assert call(n_ref=u32(20000, 20001, 13)) == PEAQ_ERR_ARG and "pair 1" in err(lib) and "n_ref 20001" in err(lib) \
        and "pair_stride 20000" in err(lib), err(lib)
    assert call(n_ref=None, n_test=None, n_uniform=20001) == PEAQ_ERR_ARG and "n_uniform 20001" in err(lib), err(lib)
    # everything in order: the context is looked at last
    assert call() == PEAQ_ERR_ARG and "ctx is NULL" in err(lib), err(lib)
    assert call(n_ref=None, n_test=None, n_uniform=16384) == PEAQ_ERR_ARG and "ctx is NULL" in err(lib), err(lib)
    assert call(lag0=i32(0x7FFFFFFF, -0x80000000, 0)) == PEAQ_ERR_ARG and "ctx is NULL" in err(lib), err(lib)


def test_cut_drift_checks_its_arguments_before_any_device(lib):
    buf, out = (C.c_float * 256)(), (C.c_float * 256)()
    p, q = (C.cast(x, C.c_void_p) for x in (buf, out))

    def call(channels=2, n_pairs=3, d_in=p, in_stride=16, n_in=u32(16, 16, 8), skip=u32(0, 2, 3), n_keep=u32(16, 14, 5),
             a=f64(-0.5, 0.0, 1048576.0), e=f64(1e-3, 0.0, -1e-3), d_out=q, out_stride=16):
        return lib.peaq_batch_cut_drift(None, channels, n_pairs, d_in, in_stride, n_in, skip, n_keep, a, e, d_out, out_stride, None)

    # what peaq_batch_cut_shifted refuses
    assert call(skip=u32(0, 3, 3)) == PEAQ_ERR_ARG and "pair 1" in err(lib) and "skip 3" in err(lib) and "n_keep 14" in err(lib) \
        and "in_stride 16" in err(lib), err(lib)
    assert call(out_stride=15) == PEAQ_ERR_ARG and "out_stride 15" in err(lib) and "16" in err(lib), err(lib)
    for name in ("d_in", "d_out"):
        assert call(**{name: None}) == PEAQ_ERR_ARG and "NULL buffer" in err(lib), err(lib)
    for name in ("n_in", "skip", "n_keep", "a", "e"):
        assert call(**{name: None}) == PEAQ_ERR_ARG and "NULL n_in, skip, n_keep, a or e" in err(lib), err(lib)
    for bad in (0, 3):
        assert call(channels=bad) == PEAQ_ERR_ARG and "channels" in err(lib) and str(bad) in err(lib), err(lib)
    assert call(n_pairs=65536) == PEAQ_ERR_ARG and "65536 pairs" in err(lib) and "65535" in err(lib), err(lib)
    assert call(n_pairs=-1) == PEAQ_ERR_ARG and "-1" in err(lib), err(lib)
    assert call(d_out=p) == PEAQ_ERR_ARG and "overlaps" in err(lib), err(lib)
    assert call(n_in=u32(16, 16, 17)) == PEAQ_ERR_ARG and "pair 2" in err(lib) and "n_in 17" in err(lib) \
        and "in_stride 16" in err(lib), err(lib)
    # its own
    for bad in (1048577.0, -2e6, float("nan"), float("inf")):
        assert call(a=f64(0, bad, 0)) == PEAQ_ERR_ARG and "pair 1" in err(lib) and ": a " in err(lib) and "1048576" in err(lib), err(lib)
    for bad in (1.001e-3, -0.5, float("nan"), float("-inf")):
        assert call(e=f64(0, 0, bad)) == PEAQ_ERR_ARG and "pair 2" in err(lib) and ": e " in err(lib) and "0.001" in err(lib), err(lib)
    # everything in order, the ranges' ends included: the context is looked at last
    assert call() == PEAQ_ERR_ARG and "ctx is NULL" in err(lib), err(lib)


def test_run_pair_drift_checks_its_arguments_before_any_device(lib):
    x = np.zeros((64, 2), np.float32)
    fp = x.ctypes.data_as(C.POINTER(C.c_float))
    out = np.zeros(16)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))

    def call(channels=2, level=92.0, rate=48000, max_lag=64, window=32768, mode=1, max_gain_db=40.0, ref=fp, test=fp, o=dp):
        return lib.peaq_run_pair_drift(None, 0, channels, level, rate, max_lag, window, mode, max_gain_db, ref, 64, test, 64,
                                       None, None, None, o)

    assert call(window=4095) == PEAQ_ERR_ARG and "window 4095" in err(lib), err(lib)
    assert call(window=(1 << 20) + 1) == PEAQ_ERR_ARG and "window 1048577" in err(lib), err(lib)
    assert call(mode=7) == PEAQ_ERR_ARG and "mode 7" in err(lib), err(lib)
    assert call(max_gain_db=121.0) == PEAQ_ERR_ARG and "max_gain_db 121" in err(lib), err(lib)
    assert call(max_lag=16385) == PEAQ_ERR_ARG and "16385" in err(lib), err(lib)
    assert call(max_lag=0) == PEAQ_ERR_ARG and "max_lag 0" in err(lib), err(lib)       # (the estimate is required)
    assert call(channels=3) == PEAQ_ERR_ARG and "channels" in err(lib), err(lib)
    assert call(level=131.0) == PEAQ_ERR_ARG and "playback level" in err(lib), err(lib)
    assert call(rate=500000) == PEAQ_ERR_ARG and "500000" in err(lib), err(lib)
    assert call(ref=None) == PEAQ_ERR_ARG and "NULL" in err(lib), err(lib)
    for mode in (0, 1, 0x13):
        assert call(mode=mode) == PEAQ_ERR_ARG and "NULL argument" in err(lib), (mode, err(lib))


def test_python_keywords():
    z = np.zeros((8, 1), np.float32)
    with pytest.raises(gstpeaq_amd.PeaqError, match="requires align="):
        gstpeaq_amd.run_pair(None, 0, z, z, drift=True)
    with pytest.raises(gstpeaq_amd.PeaqError, match="requires align="):
        gstpeaq_amd.capi._aligned(None, None, None, None, None, None, None, drift=16384)
    with pytest.raises(gstpeaq_amd.PeaqError, match="exclude each other"):
        gstpeaq_amd.run_pair(None, 0, z, z, align=64, drift=True, subsample=True)
    with pytest.raises(gstpeaq_amd.PeaqError, match="exclude each other"):
        gstpeaq_amd.capi._aligned(None, None, None, None, None, 64, None, drift=True, subsample=True)
    with pytest.raises(gstpeaq_amd.PeaqError, match="exclude each other"):
        gstpeaq_amd.align(None, None, None, None, drift=True, subsample=True)
    assert gstpeaq_amd.capi._drift_window(True) == 32768 and gstpeaq_amd.capi._drift_window(16384) == 16384

"""The host side of the track stage without a GPU (include/peaq_amd.h, "delay track on the device"): peaq_track_fit
against a restatement of the header's six steps in numpy doubles, bit for bit; peaq_track_segment and peaq_track_index
against exact Fraction arithmetic; peaq_track_lengths against brute force (which is also the check of the header's
argument that i + m_i does not decrease); the record's size and constants; and the argument checks of
peaq_batch_estimate_track, peaq_batch_cut_track and peaq_run_pair_track, which return PEAQ_ERR_ARG with the offending
value in the message before any device is touched (a NULL context is the last thing they look at)."""
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
NONE, RANGE = 1, 2
MAX_E = 1 / 64


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
def line(u1, u2, x1, x2, x0):
    return u1 + (u1 - u2) / (x1 - x2) * (x0 - x1)


def med3(a, b, c):
    return sorted((a, b, c))[1]


def fit_model(d, valid, window, max_e=MAX_E):
    """the header's steps 1 to 5, every operation one operation on numpy doubles"""
    f = np.float64
    d = [f(v) for v in d]
    W = len(d)
    S = max(W - 1, 1)
    x = [f(w) * f(window) + f(window // 2) for w in range(W)]
    V = [w for w in range(W) if valid is None or valid[w]]
    nv = len(V)
    res = dict(flags=0, n_windows=W, n_valid=nv, n_filled=W - nv, n_segments=S, d_min=0.0, d_max=0.0, max_abs_e=0.0,
               knots=[f(0)] * W, a=[f(0)] * S, e=[f(0)] * S)
    if nv == 0:
        res["flags"] = NONE
        return res
    u = [d[w] for w in V]
    xv = [x[w] for w in V]
    t = list(u)
    if nv >= 3:
        for j in range(1, nv - 1):
            t[j] = med3(u[j - 1], u[j], u[j + 1])
        t[0] = med3(u[0], u[1], line(u[1], u[2], xv[1], xv[2], xv[0]))
        t[-1] = med3(u[-1], u[-2], line(u[-2], u[-3], xv[-2], xv[-3], xv[-1]))
    s = [f(0)] * W
    for w in range(W):
        if w <= V[0]:
            s[w] = t[0]
        elif w >= V[-1]:
            s[w] = t[-1]
        else:
            j = max(k for k in range(nv) if V[k] <= w)
            s[w] = t[j] if V[j] == w else line(t[j], t[j + 1], xv[j], xv[j + 1], x[w])
    res["knots"] = s
    res["d_min"], res["d_max"] = min(s), max(s)
    if W == 1:
        res["a"] = [s[0]]
    else:
        e = [(s[k + 1] - s[k]) / f(window) for k in range(S)]
        res["a"] = [s[k] - e[k] * x[k] for k in range(S)]
        res["e"] = e
        res["max_abs_e"] = max(abs(v) for v in e)
    if res["max_abs_e"] > max_e:
        res["flags"] = RANGE
        res["a"], res["e"] = [f(0)] * S, [f(0)] * S
    return res


def same_fit(got, want):
    for k in ("flags", "n_windows", "n_valid", "n_filled", "n_segments"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("d_min", "d_max", "max_abs_e"):
        assert np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes(), (k, got[k], want[k])
    for k in ("knots", "a", "e"):
        assert np.asarray(got[k], np.float64).tobytes() == np.asarray(want[k], np.float64).tobytes(), (k, got[k], want[k])


def grid(values):
    """delays as the stage measures them: lag + q / 256"""
    return np.round(np.asarray(values, np.float64) * 256) / 256


FIT_CASES = {
    "line up": (-3.25 + 0.375 * np.arange(12), None, 16384),          # on the grid of 1/256: exact
    "line down, odd window": (40.0 - 1.75 * np.arange(9), None, 5001),
    "gridded line": (grid(40.0 - 1.7 * np.arange(9)), None, 5001),
    "constant": (np.full(7, 37.5), None, 4096),
    "step": (grid([2.0] * 5 + [9.25] * 6), None, 16384),
    "spike": (grid([1.0, 1.1, 1.2, 250.0, 1.4, 1.5, 1.6, 1.7]), None, 16384),
    "spike at the start": (grid([-300.0, 1.1, 1.2, 1.3, 1.4, 1.5]), None, 16384),
    "spike at the end": (grid([1.0, 1.1, 1.2, 1.3, 1.4, 777.0]), None, 16384),
    "bend": (grid(np.concatenate([0.8 * np.arange(6), 4.0 - 0.8 * np.arange(6)])), None, 16384),
    "gap at the start": (grid(0.5 * np.arange(10)), [0, 0, 0, 1, 1, 1, 1, 1, 1, 1], 4096),
    "gap in the middle": (grid(0.5 * np.arange(10)), [1, 1, 1, 0, 0, 0, 1, 1, 1, 1], 5001),
    "gap at the end": (grid(0.5 * np.arange(10)), [1, 1, 1, 1, 1, 1, 1, 0, 0, 255], 4096),
    "gaps everywhere": (grid(3.0 - 0.25 * np.arange(11) ** 1.5), [0, 1, 0, 0, 1, 1, 0, 1, 0, 1, 0], 16384),
    "nv = 0": (grid(np.arange(5.0)), [0] * 5, 4096),
    "nv = 1": (grid(np.arange(5.0) + 0.25), [0, 0, 1, 0, 0], 4096),
    "nv = 2": (grid(np.arange(5.0) * 1.5), [0, 1, 0, 0, 1], 4096),
    "W = 1": ([-12.75], None, 4096),
    "W = 1, invalid": ([-12.75], [0], 4096),
    "W = 2": ([1.0, 2.5], None, 8192),
    "W = 0": ([], None, 4096),
}


@pytest.mark.parametrize("name", sorted(FIT_CASES))
def test_fit_is_the_numpy_restatement(lib, name):
    d, valid, window = FIT_CASES[name]
    got = gstpeaq_amd.track_fit(d, valid, window=window)
    same_fit(got, fit_model(d, valid, window))
    if name.startswith("line") or name == "constant":
        # a constant drift passes the median unchanged: the knots are the delays, every segment the same line
        assert np.array_equal(got["knots"], d)
        slope = (d[-1] - d[0]) / ((len(d) - 1) * window)
        assert np.allclose(got["e"], slope, rtol=1e-12, atol=0) and got["flags"] == 0
        assert np.allclose(got["a"], d[0] - slope * (window // 2), rtol=0, atol=1e-9)
    if name == "gridded line":
        # monotone: the interior passes unchanged; an end moves at most to the line through its two neighbours, which
        # the gridding keeps within a grid step of it
        assert np.array_equal(got["knots"][1:-1], d[1:-1]) and np.abs(got["knots"] - d).max() <= 1 / 256
    if name == "step":
        assert np.array_equal(got["knots"], d)                     # the step survives
    if name.startswith("spike"):
        assert np.abs(got["knots"]).max() < 2 and got["flags"] == 0  # the wild window does not
    if name.startswith("nv = 0") or name == "W = 1, invalid":
        assert got["flags"] == NONE and not np.any(got["knots"]) and not np.any(got["a"]) and not np.any(got["e"])
    if name == "nv = 1":
        assert np.all(got["knots"] == 2.25) and np.all(got["a"] == 2.25) and not np.any(got["e"]) and got["n_filled"] == 4
    if name == "gap in the middle":
        assert np.allclose(got["knots"], d, atol=1e-12)            # filled from the neighbours, on their line


def test_fit_on_random_sets_and_at_the_range(lib):
    rng = np.random.default_rng(5)
    for trial in range(200):
        W = int(rng.integers(0, 40))
        window = int(rng.choice([4096, 5001, 16384, 1 << 20]))
        d = grid(np.cumsum(rng.normal(0, 2, W)) + rng.integers(-40, 40))
        if trial % 3 == 0 and W:
            d[rng.integers(0, W, max(1, W // 6))] = rng.integers(-1000, 1000)
        valid = (rng.random(W) < (0.8, 0.3, 1.0)[trial % 3]).astype(np.uint8)
        max_e = float(rng.choice([MAX_E, 1e-3, 1e-4]))
        same_fit(gstpeaq_amd.track_fit(d, valid, window=window, max_e=max_e), fit_model(d, valid, window, max_e))
    # a slope just under and just over max_e
    window = 4096
    for max_e in (MAX_E, 1e-3):
        rise = max_e * window
        under, over = np.nextafter(rise, 0), np.nextafter(rise, np.inf)
        for top, flag in ((under, 0), (rise, 0), (over, RANGE)):
            d = [0.0, 0.0, top, top]
            got = gstpeaq_amd.track_fit(d, window=window, max_e=max_e)
            same_fit(got, fit_model(d, None, window, max_e))
            assert got["flags"] == flag, (max_e, top, got)
            if flag:
                assert not np.any(got["a"]) and not np.any(got["e"]) and got["max_abs_e"] > max_e
                assert np.array_equal(got["knots"], d)             # the knots stay readable


def test_fit_refuses(lib):
    d, k, a, e = f64(0, 1, 2), f64(0, 0, 0), f64(0, 0), f64(0, 0)
    rec = gstpeaq_amd.Track()

    def call(d=d, n=3, window=4096, max_e=MAX_E, out=C.byref(rec), knots=k, a=a, e=e):
        return lib.peaq_track_fit(d, None, n, window, max_e, out, knots, a, e)

    assert call() == 0
    for name in ("out", "a", "e"):
        assert call(**{name: None}) == PEAQ_ERR_ARG and "NULL" in err(lib), err(lib)
    for name in ("d", "knots"):
        assert call(**{name: None}) == PEAQ_ERR_ARG and "NULL" in err(lib), err(lib)
    for bad in (0, 4095, (1 << 20) + 1):
        assert call(window=bad) == PEAQ_ERR_ARG and "window %d" % bad in err(lib), err(lib)
    assert call(n=4097) == PEAQ_ERR_ARG and "4097 windows" in err(lib) and "4096" in err(lib), err(lib)
    for bad in (0.0, -1e-3, 0.016, float("nan")):
        assert call(max_e=bad) == PEAQ_ERR_ARG and "max_e" in err(lib) and "0.015625" in err(lib), err(lib)
    assert call(max_e=0.016) == PEAQ_ERR_ARG and "0.016" in err(lib), err(lib)


# ---- segment and index ---------------------------------------------------------------------------------------------
def segment_exact(i, window, n_seg):
    h = window // 2
    return 0 if i < h else min((i - h) // window, n_seg - 1)


def index_exact(window, a, e, i):
    """peaq_track_index in exact arithmetic: the fused multiply-add is the double nearest to the exact e i + a, the
    product with 256 is exact, rint rounds to nearest even"""
    k = segment_exact(i, window, len(a))
    exact = Fraction(float(e[k])) * i + Fraction(float(a[k]))
    t = exact.numerator / exact.denominator              # (int / int is correctly rounded)
    g = int(np.rint(256.0 * t))
    m = (g + 128) // 256
    return m, g - 256 * m


def test_segment_is_the_integer_arithmetic(lib):
    for window in (4096, 5001, 16384, 1 << 20):
        h = window // 2
        for n_seg in (1, 2, 3, 7, 4095):
            for k in range(0, min(n_seg + 2, 9)):
                for i in (k * window + h - 1, k * window + h, k * window + h + 1, k * window, (k + 1) * window - 1):
                    assert gstpeaq_amd.track_segment(i, window, n_seg) == segment_exact(i, window, n_seg), (i, window, n_seg)
            for i in (0, 1, h - 1, 2 ** 32 - 1, 2 ** 32 + 5):
                assert gstpeaq_amd.track_segment(i, window, n_seg) == segment_exact(i, window, n_seg), (i, window, n_seg)
    assert gstpeaq_amd.track_segment(2500, 5001, 3) == 0 and gstpeaq_amd.track_segment(7500, 5001, 3) == 0
    assert gstpeaq_amd.track_segment(7501, 5001, 3) == 1 and gstpeaq_amd.track_segment(10 ** 6, 5001, 3) == 2


def test_index_is_the_exact_arithmetic(lib):
    rng = np.random.default_rng(3)
    for window in (5001, 4096, 16384):
        for n_seg in (1, 2, 5):
            knots = np.cumsum(rng.uniform(-1, 1, n_seg + 1) * window / 64) + rng.uniform(-50, 50)
            e = (knots[1:] - knots[:-1]) / window
            a = knots[:-1] - e * (np.arange(n_seg) * float(window) + window // 2)
            pts = [0, 1, window // 2 - 1, window // 2, n_seg * window + 5, 2 ** 31 + 7]
            for k in range(1, n_seg):
                b = window // 2 + k * window
                pts += [b - 1, b, b + 1]
            pts += [int(v) for v in rng.integers(0, (n_seg + 1) * window, 300)]
            for i in pts:
                got = gstpeaq_amd.track_index(window, a, e, i)
                assert got == index_exact(window, a, e, i), (window, n_seg, i)
                assert -128 <= got[1] <= 127
    # one segment is the drift stage's index
    for i in (0, 17, 10 ** 6):
        assert gstpeaq_amd.track_index(4096, [-0.37], [3.73e-5], i) == gstpeaq_amd.drift_index(-0.37, 3.73e-5, i)


# ---- the lengths ---------------------------------------------------------------------------------------------------
def lengths_brute(lag0, window, a, e, n_ref, n_test):
    sr, st, common = gstpeaq_amd.aligned_lengths(lag0, n_ref, n_test)
    keep, last = 0, None
    for i in range(common):
        m, _ = index_exact(window, a, e, i)
        assert last is None or i + m >= last, (i, m, last)    # the header's argument: i + m_i does not decrease
        last = i + m
        if not st + i + m < n_test:
            break
        keep += 1
    return sr, st, keep


def test_lengths_against_brute_force(lib):
    """tracks as the fit makes them, slopes up to +-1/64 and of opposite signs at a knot, windows of 4096 and 5001: the
    binary search gives the brute-force count, and i + m_i never decreases on the way there"""
    rng = np.random.default_rng(11)
    cases = []
    for trial in range(40):
        window = (4096, 5001)[trial % 2]
        W = int(rng.integers(1, 6))
        steep = trial % 4 < 2
        rises = rng.choice([-1.0, 1.0], W) * (window / 64 if steep else rng.uniform(0, window / 200, W))
        d = grid(np.cumsum(rises) + rng.uniform(-5, 5))
        fit = gstpeaq_amd.track_fit(d, window=window)
        assert fit["flags"] == 0
        n_test = int(rng.integers(window // 2, (W + 1) * window))
        n_ref = int(n_test + rng.integers(-300, 300))
        cases.append((int(rng.integers(-30, 30)), window, fit["a"], fit["e"], n_ref, n_test))
    cases.append((0, 4096, np.zeros(1), np.zeros(1), 100, 100))
    cases.append((3, 4096, np.array([2.0]), np.zeros(1), 50, 60))
    cases.append((0, 4096, np.array([400.0]), np.zeros(1), 300, 300))
    cases.append((500, 4096, np.zeros(1), np.zeros(1), 300, 300))
    for lag0, window, a, e, n_ref, n_test in cases:
        got = gstpeaq_amd.track_lengths(lag0, window, a, e, n_ref, n_test)
        assert got == lengths_brute(lag0, window, a, e, n_ref, n_test), (lag0, window, list(a), list(e), n_ref, n_test)
        assert got[:2] == gstpeaq_amd.aligned_lengths(lag0, n_ref, n_test)[:2]
    # one segment: the drift stage's lengths
    assert gstpeaq_amd.track_lengths(7, 4096, [-2.25], [1e-3], 10 ** 6, 10 ** 6) == gstpeaq_amd.drift_lengths(7, -2.25, 1e-3, 10 ** 6, 10 ** 6)


# ---- record, constants, surface ----------------------------------------------------------------------------------------
def test_record_size_and_constants(lib):
    assert lib.peaq_track_size() == 48 == C.sizeof(gstpeaq_amd.Track) == gstpeaq_amd.TRACK_DTYPE.itemsize
    assert [n for n, _ in gstpeaq_amd.Track._fields_] == list(gstpeaq_amd.TRACK_DTYPE.names)
    assert set(gstpeaq_amd.TRACK_DTYPE.names) == {"lag0", "flags", "n_windows", "n_valid", "n_filled", "n_segments", "d_min",
                                                  "d_max", "max_abs_e"}
    assert int(header_define("PEAQ_TRACK_F_NONE")) == gstpeaq_amd.TRACK_F_NONE == 1
    assert int(header_define("PEAQ_TRACK_F_RANGE")) == gstpeaq_amd.TRACK_F_RANGE == 2
    assert float(header_define("PEAQ_TRACK_MAX_E")) == gstpeaq_amd.TRACK_MAX_E == 1 / 64
    assert float(header_define("PEAQ_TRACK_MAX_STEP")) == gstpeaq_amd.TRACK_MAX_STEP == 1 / 256
    assert "(1u << 20)" in re.search(r"^#define\s+PEAQ_TRACK_MAX_SEGMENTS_PER_CALL\s+(.*)$", header_text(), flags=re.M).group(1)
    assert gstpeaq_amd.TRACK_MAX_SEGMENTS_PER_CALL == 1 << 20 and gstpeaq_amd.TRACK_WINDOW == 16384
    assert 2 * 8 * gstpeaq_amd.TRACK_MAX_SEGMENTS_PER_CALL == 16 << 20          # a and e of a call: 16 MiB of staging


def test_header_and_exports_stay_in_step(lib):
    hdr = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(peaq_[a-z_0-9]*track[a-z_0-9]*)\s*\(", hdr)))
    assert declared == ["peaq_batch_cut_track", "peaq_batch_estimate_track", "peaq_run_pair_track", "peaq_track_fit",
                        "peaq_track_index", "peaq_track_lengths", "peaq_track_segment", "peaq_track_size"]
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in include/peaq_amd.h but not exported"
    for name in ("Track", "TRACK_DTYPE", "track_fit", "track_index", "track_lengths", "estimate_track", "cut_track"):
        assert hasattr(gstpeaq_amd, name), name


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_estimate_track_checks_its_arguments_before_any_device(lib):
    a, b, o1, o2 = (C.c_float * 8)(), (C.c_float * 8)(), (C.c_char * 8)(), (C.c_char * 8)()
    p, q, r1, r2 = (C.cast(x, C.c_void_p) for x in (a, b, o1, o2))
    rec, line = (gstpeaq_amd.Track * 3)(), (gstpeaq_amd.Drift * 3)()
    kn, sa, se = (C.c_double * 12)(), (C.c_double * 9)(), (C.c_double * 9)()

    def call(channels=2, n_pairs=3, d_ref=p, d_test=q, stride=20000, n_ref=u32(20000, 9000, 13), n_test=u32(20000, 20000, 1),
             n_uniform=0, lag0=i32(0, -3, 100), window=4096, R=1024, min_corr=0.5, max_e=MAX_E, w_max=4, dl=r1, sb=r2,
             drift=line, out=rec, knots=kn, seg_stride=3, sa=sa, se=se):
        return lib.peaq_batch_estimate_track(None, channels, n_pairs, d_ref, d_test, stride, n_ref, n_test, n_uniform, lag0,
                                             window, R, min_corr, max_e, w_max, dl, sb, drift, out, knots, seg_stride, sa, se, None)

    # its own
    for bad in (0.0, -1e-4, 0.0157, float("nan")):
        assert call(max_e=bad) == PEAQ_ERR_ARG and "max_e" in err(lib) and "0.015625" in err(lib), err(lib)
    assert call(max_e=0.0157) == PEAQ_ERR_ARG and "0.0157" in err(lib), err(lib)
    assert call(seg_stride=2) == PEAQ_ERR_ARG and "seg_stride 2" in err(lib) and "w_max 4" in err(lib), err(lib)
    assert call(seg_stride=0, w_max=1) == PEAQ_ERR_ARG and "seg_stride 0" in err(lib), err(lib)
    for name in ("out", "knots", "sa", "se"):
        assert call(**{name: None}) == PEAQ_ERR_ARG and "NULL out, knots, a or e" in err(lib), err(lib)
    # what peaq_batch_estimate_drift refuses, under this entry point's name
    for bad in (0, 4095, (1 << 20) + 1):
        assert call(window=bad, R=1) == PEAQ_ERR_ARG and "window %d" % bad in err(lib) and "peaq_batch_estimate_track" in err(lib), err(lib)
    for bad in (0, 1025, 16385):
        assert call(R=bad) == PEAQ_ERR_ARG and "R %d" % bad in err(lib) and "1024" in err(lib), err(lib)
    for bad in (-0.1, 1.5, float("nan")):
        assert call(min_corr=bad) == PEAQ_ERR_ARG and "min_corr" in err(lib), err(lib)
    for bad in (0, 3):
        assert call(channels=bad) == PEAQ_ERR_ARG and "channels" in err(lib) and str(bad) in err(lib), err(lib)
    assert call(n_pairs=65536) == PEAQ_ERR_ARG and "65536 pairs" in err(lib), err(lib)
    assert call(n_pairs=-1) == PEAQ_ERR_ARG and "-1" in err(lib), err(lib)
    assert call(w_max=0) == PEAQ_ERR_ARG and "w_max 0" in err(lib), err(lib)
    assert call(w_max=4097, seg_stride=4096) == PEAQ_ERR_ARG and "w_max 4097" in err(lib), err(lib)
    assert call(w_max=3) == PEAQ_ERR_ARG and "pair 0" in err(lib) and "4 windows" in err(lib) and "w_max 3" in err(lib), err(lib)
    for name in ("d_ref", "d_test", "dl", "sb"):
        assert call(**{name: None}) == PEAQ_ERR_ARG and "NULL buffer" in err(lib), err(lib)
    assert call(lag0=None) == PEAQ_ERR_ARG and "NULL lag0" in err(lib), err(lib)
    assert call(n_test=None) == PEAQ_ERR_ARG and "both" in err(lib), err(lib)
    assert call(n_ref=u32(20000, 20001, 13)) == PEAQ_ERR_ARG and "pair 1" in err(lib) and "n_ref 20001" in err(lib) \
        and "pair_stride 20000" in err(lib), err(lib)
    assert call(n_ref=None, n_test=None, n_uniform=20001) == PEAQ_ERR_ARG and "n_uniform 20001" in err(lib), err(lib)
    # everything in order (the line's record may be NULL; max_e beyond the drift stage's 1e-3): the context is looked at last
    assert call() == PEAQ_ERR_ARG and "ctx is NULL" in err(lib), err(lib)
    assert call(drift=None) == PEAQ_ERR_ARG and "ctx is NULL" in err(lib), err(lib)
    assert call(seg_stride=7, max_e=1e-4) == PEAQ_ERR_ARG and "ctx is NULL" in err(lib), err(lib)


def test_cut_track_checks_its_arguments_before_any_device(lib):
    buf, out = (C.c_float * 256)(), (C.c_float * 256)()
    p, q = (C.cast(x, C.c_void_p) for x in (buf, out))
    # pair 0: two segments that meet at x_1 = 6144 (a_1 = a_0 + (e_0 - e_1) x_1); pair 2: the ranges' ends
    good_a = f64(-0.5, -0.5 + (MAX_E + MAX_E) * 6144, 0.0, 9.0, 1048576.0, 9.0)
    good_e = f64(MAX_E, -MAX_E, 0.0, 9.0, -MAX_E, 9.0)

    def with_(arr, k, v):
        vals = list(arr)
        vals[k] = v
        return f64(*vals)

    def call(channels=2, n_pairs=3, d_in=p, in_stride=16, n_in=u32(16, 16, 8), skip=u32(0, 2, 3), n_keep=u32(16, 14, 5),
             window=4096, n_seg=u32(2, 1, 1), seg_stride=2, a=good_a, e=good_e, d_out=q, out_stride=16):
        return lib.peaq_batch_cut_track(None, channels, n_pairs, d_in, in_stride, n_in, skip, n_keep, window, n_seg, seg_stride,
                                        a, e, d_out, out_stride, None)

    # what peaq_batch_cut_drift refuses
    assert call(skip=u32(0, 3, 3)) == PEAQ_ERR_ARG and "pair 1" in err(lib) and "skip 3" in err(lib) and "n_keep 14" in err(lib) \
        and "in_stride 16" in err(lib), err(lib)
    assert call(out_stride=15) == PEAQ_ERR_ARG and "out_stride 15" in err(lib) and "16" in err(lib), err(lib)
    for name in ("d_in", "d_out"):
        assert call(**{name: None}) == PEAQ_ERR_ARG and "NULL buffer" in err(lib), err(lib)
    for name in ("n_in", "skip", "n_keep", "n_seg", "a", "e"):
        assert call(**{name: None}) == PEAQ_ERR_ARG and "NULL n_in, skip, n_keep, n_seg, a or e" in err(lib), err(lib)
    for bad in (0, 3):
        assert call(channels=bad) == PEAQ_ERR_ARG and "channels" in err(lib) and str(bad) in err(lib), err(lib)
    assert call(n_pairs=65536) == PEAQ_ERR_ARG and "65536 pairs" in err(lib) and "65535" in err(lib), err(lib)
    assert call(n_pairs=-1) == PEAQ_ERR_ARG and "-1" in err(lib), err(lib)
    assert call(d_out=p) == PEAQ_ERR_ARG and "overlaps" in err(lib), err(lib)
    assert call(n_in=u32(16, 16, 17)) == PEAQ_ERR_ARG and "pair 2" in err(lib) and "n_in 17" in err(lib) \
        and "in_stride 16" in err(lib), err(lib)
    # its own
    for bad in (0, 4095, (1 << 20) + 1):
        assert call(window=bad) == PEAQ_ERR_ARG and "window %d" % bad in err(lib) and "4096" in err(lib), err(lib)
    assert call(n_seg=u32(2, 0, 1)) == PEAQ_ERR_ARG and "pair 1" in err(lib) and "n_seg 0" in err(lib), err(lib)
    assert call(n_seg=u32(2, 1, 3)) == PEAQ_ERR_ARG and "pair 2" in err(lib) and "n_seg 3" in err(lib) and "seg_stride 2" in err(lib), err(lib)
    for bad in (1048577.0, -2e6, float("nan"), float("inf")):
        assert call(a=with_(good_a, 2, bad)) == PEAQ_ERR_ARG and "pair 1, segment 0" in err(lib) and ": a " in err(lib) \
            and "1048576" in err(lib), err(lib)
    for bad in (0.0157, -0.5, float("nan"), float("-inf")):
        assert call(e=with_(good_e, 4, bad)) == PEAQ_ERR_ARG and "pair 2, segment 0" in err(lib) and ": e " in err(lib) \
            and "0.015625" in err(lib), err(lib)
    # segments that do not meet at their knot: 1/128 sample apart
    assert call(a=with_(good_a, 1, -0.5 + 2 * MAX_E * 6144 + 1 / 128)) == PEAQ_ERR_ARG and "pair 0, segment 1" in err(lib) \
        and "step of 0.0078" in err(lib) and "0.00390625" in err(lib), err(lib)
    # more segments than a call takes: 257 pairs of 4095 (the arrays are looked at only up to the first refusal)
    n = 257
    many = (C.c_uint32 * n)(*([4095] * n))
    zeros = (C.c_uint32 * n)()
    big = (C.c_float * 8)()
    assert 4095 * n > 1 << 20
    assert lib.peaq_batch_cut_track(None, 1, n, C.cast(buf, C.c_void_p), 0, zeros, zeros, zeros, 4096, many, 4095, good_a, good_e,
                                    C.cast(big, C.c_void_p), 0, None) == PEAQ_ERR_ARG and "%d segments" % (4095 * n) in err(lib) \
        and "1048576" in err(lib), err(lib)
    # everything in order, the ranges' ends included: the context is looked at last
    assert call() == PEAQ_ERR_ARG and "ctx is NULL" in err(lib), err(lib)


def test_run_pair_track_checks_its_arguments_before_any_device(lib):
    x = np.zeros((64, 2), np.float32)
    fp = x.ctypes.data_as(C.POINTER(C.c_float))
    out = np.zeros(16)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))

    def call(channels=2, level=92.0, rate=48000, max_lag=64, window=16384, mode=1, max_gain_db=40.0, ref=fp, test=fp, o=dp):
        return lib.peaq_run_pair_track(None, 0, channels, level, rate, max_lag, window, mode, max_gain_db, ref, 64, test, 64,
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
    with pytest.raises(gstpeaq_amd.PeaqError, match="track= requires align="):
        gstpeaq_amd.run_pair(None, 0, z, z, track=True)
    with pytest.raises(gstpeaq_amd.PeaqError, match="track= requires align="):
        gstpeaq_amd.capi._aligned(None, None, None, None, None, None, None, track=16384)
    with pytest.raises(gstpeaq_amd.PeaqError, match="track= and drift= exclude each other"):
        gstpeaq_amd.run_pair(None, 0, z, z, align=64, track=True, drift=True)
    with pytest.raises(gstpeaq_amd.PeaqError, match="track= and subsample=True exclude each other"):
        gstpeaq_amd.run_pair(None, 0, z, z, align=64, track=True, subsample=True)
    with pytest.raises(gstpeaq_amd.PeaqError, match="exclude each other"):
        gstpeaq_amd.capi._aligned(None, None, None, None, None, 64, None, track=True, drift=True)
    with pytest.raises(gstpeaq_amd.PeaqError, match="exclude each other"):
        gstpeaq_amd.align(None, None, None, None, track=True, subsample=True)
    with pytest.raises(gstpeaq_amd.PeaqError, match="exclude each other"):
        gstpeaq_amd.align(None, None, None, None, track=True, drift=8192)
    assert gstpeaq_amd.capi._track_window(True) == 16384 and gstpeaq_amd.capi._track_window(5001) == 5001

"""CPU-side tests of live alignment (peaq_session_set_align, include/peaq_amd.h "live alignment"): rule
A's arithmetic (peaq_live_align_plan) and rule B's read-out (peaq_delay_watch_pick) against restatements in Python, the
sizes of the public structs, and the refusals that need no session.  No GPU.  (What a session refuses once it has been
pushed to, or reads with a half switched off, is in tests/test_gpu_live_align.py.)"""
import ctypes as C
import math

import numpy as np
import pytest

U32P = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def lib():
    import gstpeaq_amd
    if not gstpeaq_amd.library_path().exists():
        gstpeaq_amd.build_library()
    L = gstpeaq_amd.load_library()
    L.peaq_last_error.restype = C.c_char_p
    return L


def plan_rule(max_lag, probe, have_ref, have_test, lag):
    """rule A in Python"""
    probe = probe or 48000 + 2 * max_lag
    skip_ref = min(-lag, have_ref) if lag < 0 else 0
    skip_test = min(lag, have_test) if lag >= 0 else 0
    return min(have_ref, probe), min(have_test, probe), skip_ref, skip_test


def test_the_plan_against_rule_a_on_a_grid():
    import gstpeaq_amd
    below_probe = below_skip = default_probe = 0
    for max_lag, probe in ((256, 4096), (256, None), (1, 2049), (16384, None), (16384, 1 << 20), (113, 8192)):
        p = probe or 48000 + 2 * max_lag
        haves = (0, 1, 36, 37, 112, 113, 114, 255, 256, 257, 5000, p - 1, p, p + 1, 3 * p, 1 << 33)
        for lag in sorted({-max_lag, -113 if max_lag >= 113 else -1, -1, 0, 1, 37 if max_lag >= 37 else 1, max_lag}):
            for have_ref in haves:
                for have_test in haves:
                    got = gstpeaq_amd.live_align_plan(max_lag, have_ref, have_test, lag, probe=probe)
                    assert got == plan_rule(max_lag, probe, have_ref, have_test, lag), (max_lag, probe, have_ref, have_test, lag)
                    below_probe += have_ref < p or have_test < p
                    below_skip += (lag > 0 and have_test < lag) or (lag < 0 and have_ref < -lag)
                    default_probe += probe is None
    assert below_probe and below_skip and default_probe
    # the corners by hand: the late pad drops the lag, the skip stops at what the pad holds, nothing is cut at the tail
    assert gstpeaq_amd.live_align_plan(256, 31700, 31700, 37, probe=4096) == (4096, 4096, 0, 37)
    assert gstpeaq_amd.live_align_plan(256, 31700, 31700, -113, probe=4096) == (4096, 4096, 113, 0)
    assert gstpeaq_amd.live_align_plan(256, 5000, 5000, 256, probe=8192) == (5000, 5000, 0, 256)
    assert gstpeaq_amd.live_align_plan(256, 5000, 100, 256, probe=8192) == (5000, 100, 0, 100)
    assert gstpeaq_amd.live_align_plan(256, 50, 5000, -256, probe=8192) == (50, 5000, 50, 0)
    assert gstpeaq_amd.live_align_plan(256, 10 ** 6, 10 ** 6, 0)[:2] == (48512, 48512)


def test_the_plan_leaves_out_what_is_not_asked_for_and_refuses_what_rule_a_does_not_cover(lib):
    import gstpeaq_amd
    cfg = gstpeaq_amd.LiveAlignConfig(256, 4096, 0, 0)
    only = C.c_uint32(0xdead)
    assert lib.peaq_live_align_plan(C.byref(cfg), 9000, 9000, 37, None, None, None, C.byref(only)) == 0
    assert only.value == 37
    assert lib.peaq_live_align_plan(None, 9000, 9000, 37, None, None, None, None) == -1
    assert lib.peaq_last_error().decode() == "peaq_live_align_plan: cfg is NULL"
    for lag in (257, -257, 2 ** 31 - 1, -2 ** 31):
        assert lib.peaq_live_align_plan(C.byref(cfg), 9000, 9000, lag, None, None, None, None) == -1
        assert f"lag {lag} is outside" in lib.peaq_last_error().decode()
    off = gstpeaq_amd.LiveAlignConfig(0, 0, 4, 0)
    assert lib.peaq_live_align_plan(C.byref(off), 9000, 9000, 0, None, None, None, None) == -1
    assert lib.peaq_last_error().decode() == "peaq_live_align_plan: max_lag 0 sets no acquisition"


def pick_rule(c, e_ref, e_test):
    """rule B's read-out in Python"""
    e2 = e_ref * e_test
    if not (math.isfinite(e2) and all(math.isfinite(x) for x in c)):
        return dict(offset=0, peak=0.0, runner_up=0.0, norm=math.nan)
    if not e2 > 0:
        return dict(offset=0, peak=0.0, runner_up=0.0, norm=0.0)
    norm = math.sqrt(e2)
    best = max(abs(x) for x in c)
    tied = [d for d in range(-31, 32) if abs(c[d + 31]) >= best - 1e-12 * norm]
    offset = min(tied, key=lambda d: (abs(d), d < 0))
    return dict(offset=offset, peak=c[offset + 31], runner_up=max(abs(c[d + 31]) for d in range(-31, 32) if d != offset),
                norm=norm)


def same(a, b):
    return a.keys() == b.keys() and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)


def test_the_pick_against_rule_b():
    import gstpeaq_amd
    rng = np.random.default_rng(5)

    def lags(**at):
        c = np.zeros(63)
        for d, v in at.items():
            c[int(d.replace("m", "-").replace("p", "")) + 31] = v
        return c

    norm = 4.0                                              # e_ref e_test = 16
    cases = [
        ("an exact tie at +-d: the positive d", lags(p5=3.0, m5=3.0), 5),
        ("an exact tie at +-d, opposite signs", lags(p5=-3.0, m5=3.0), 5),
        ("a tie between 2 and -1: the smaller |d|", lags(p2=3.0, m1=-3.0), -1),
        ("0.5e-12 norm apart counts as tied", lags(p7=3.0, p1=3.0 - 0.5e-12 * norm), 1),
        ("2e-12 norm apart does not", lags(p7=3.0, p1=3.0 - 2e-12 * norm), 7),
        ("the edge lags", lags(m31=2.0, p31=-2.0, p30=1.0), 31),
        ("a negative peak", lags(m31=-2.5, p30=1.0), -31),
    ]
    for what, c, want in cases:
        got = gstpeaq_amd.delay_watch_pick(c, 8.0, 2.0)
        assert got["offset"] == want and got["norm"] == norm and got["peak"] == c[want + 31], (what, got)
        assert same(got, pick_rule(c, 8.0, 2.0)), (what, got)
    assert gstpeaq_amd.delay_watch_pick(lags(p7=3.0, p1=3.0 - 2e-12 * norm), 8.0, 2.0)["runner_up"] == 3.0 - 2e-12 * norm
    # all zeros, silence on one side, and what is not a number
    assert gstpeaq_amd.delay_watch_pick(np.zeros(63), 0.0, 0.0) == dict(offset=0, peak=0.0, runner_up=0.0, norm=0.0)
    assert gstpeaq_amd.delay_watch_pick(np.zeros(63), 5.0, 0.0) == dict(offset=0, peak=0.0, runner_up=0.0, norm=0.0)
    for c, e_ref, e_test in ((lags(p3=math.nan, p1=1.0), 1.0, 1.0), (lags(p3=1.0), math.nan, 1.0),
                             (lags(p3=1.0), 1.0, math.inf), (lags(m9=math.inf), 1.0, 1.0)):
        got = gstpeaq_amd.delay_watch_pick(c, e_ref, e_test)
        assert (got["offset"], got["peak"], got["runner_up"]) == (0, 0.0, 0.0) and math.isnan(got["norm"]), got
        assert same(got, pick_rule(c, e_ref, e_test))
    for _ in range(300):
        c = rng.standard_normal(63) * rng.choice([1.0, 1e-6, 1e6])
        if rng.random() < 0.5:                              # some exact and some near ties
            i, j = rng.integers(0, 63, 2)
            c[j] = c[i] * rng.choice([1.0, -1.0]) * (1.0 - rng.choice([0.0, 1e-13, 1e-11]))
        e_ref, e_test = float(np.abs(c).max()) * 2, float(np.abs(c).max()) * 3
        assert same(gstpeaq_amd.delay_watch_pick(c, e_ref, e_test), pick_rule(list(c), e_ref, e_test))


def test_the_pick_leaves_out_what_is_not_asked_for(lib):
    c = (C.c_double * 63)()
    c[31 + 4] = -2.0
    off = C.c_int32(99)
    lib.peaq_delay_watch_pick.argtypes = [C.POINTER(C.c_double), C.c_double, C.c_double, C.POINTER(C.c_int32),
                                          C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    assert lib.peaq_delay_watch_pick(c, 1.0, 4.0, C.byref(off), None, None, None) == 0 and off.value == 4
    assert lib.peaq_delay_watch_pick(None, 1.0, 4.0, C.byref(off), None, None, None) == -1
    assert lib.peaq_last_error().decode() == "peaq_delay_watch_pick: c is NULL"


def test_the_structs_have_the_sizes_the_library_says(lib):
    import gstpeaq_amd
    lib.peaq_live_delay_size.restype = C.c_size_t
    lib.peaq_delay_watch_size.restype = C.c_size_t
    assert lib.peaq_live_delay_size() == C.sizeof(gstpeaq_amd.LiveDelay) == 6 * 4 + 32
    assert lib.peaq_delay_watch_size() == C.sizeof(gstpeaq_amd.DelayWatch) == 8 + 4 * 4 + 5 * 8 + 63 * 8
    assert C.sizeof(gstpeaq_amd.LiveAlignConfig) == 16


def test_the_entries_refuse_what_needs_no_device(lib):
    import gstpeaq_amd
    cfg = gstpeaq_amd.LiveAlignConfig(256, 4096, 4, 0)
    assert lib.peaq_session_set_align(None, C.byref(cfg)) == -1
    assert lib.peaq_last_error().decode() == "peaq_session_set_align: session is NULL"
    d, w = gstpeaq_amd.LiveDelay(), gstpeaq_amd.DelayWatch()
    s = C.c_void_p(0x5000)                                  # never dereferenced: the checks below come first
    for entry, out in ((lib.peaq_session_align_read, d), (lib.peaq_session_watch_read, w)):
        assert entry(None, C.byref(out)) == -1
        assert entry(s, None) == -1
        assert lib.peaq_last_error().decode().endswith(": NULL argument")
    assert lib.peaq_broker_set_align(None, C.byref(cfg)) == -1
    assert lib.peaq_last_error().decode() == "peaq_broker_set_align: broker is NULL"
    for entry, out in ((lib.peaq_broker_align_read, d), (lib.peaq_broker_watch_read, w)):
        assert entry(None, 0, C.byref(out)) == -1
        assert lib.peaq_last_error().decode().endswith(": NULL argument")
    for fields, words in (((16385, 0, 0, 0), "max_lag 16385 is outside 0 .. 16384"),
                          ((256, 2303, 0, 0), "probe 2303 is outside max_lag + 2048 = 2304 .. 1048576"),
                          ((256, (1 << 20) + 1, 0, 0), "probe 1048577 is outside max_lag + 2048 = 2304 .. 1048576"),
                          ((0, 100, 4, 0), "probe 100 is outside max_lag + 2048 = 2048 .. 1048576"),
                          ((0, 0, 65537, 0), "watch_frames 65537 is outside 0 .. 65536"),
                          ((256, 0, 4, 7), "reserved 7 must be 0"),
                          ((0, 0, 0, 1), "reserved 1 must be 0")):
        bad = gstpeaq_amd.LiveAlignConfig(*fields)
        assert lib.peaq_session_set_align(s, C.byref(bad)) == -1, fields
        msg = lib.peaq_last_error().decode()
        assert msg == "peaq_session_set_align: " + words, msg
        assert lib.peaq_live_align_plan(C.byref(bad), 1, 1, 0, None, None, None, None) == -1, fields
        assert lib.peaq_last_error().decode().startswith("peaq_live_align_plan: "), fields
    # the limits themselves are inside
    for fields in ((16384, 0, 0, 0), (256, 2304, 0, 0), (256, 1 << 20, 65536, 0)):
        ok = gstpeaq_amd.LiveAlignConfig(*fields)
        assert lib.peaq_live_align_plan(C.byref(ok), 1, 1, 0, None, None, None, None) == 0, fields


def test_python_binding_exports_live_alignment():
    import gstpeaq_amd
    for name in ("live_align_plan", "delay_watch_pick", "LiveAlignConfig", "LiveDelay", "DelayWatch", "WATCH_LAGS"):
        assert hasattr(gstpeaq_amd, name) and name in gstpeaq_amd.__all__, name
    for name in ("set_align", "align_read", "watch_read"):
        assert hasattr(gstpeaq_amd.Session, name) and hasattr(gstpeaq_amd.Broker, name), name

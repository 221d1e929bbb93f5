"""The wide delay search's host side without a GPU (include/peaq_amd.h, "wide delay search on the device"):
peaq_wide_factor against its restatement, peaq_wide_taps against the formula evaluated with mpmath, the argument checks
of every new entry point, which return PEAQ_ERR_ARG with the entry's name and the value in the message before any device
is touched (a valid call ends at "ctx is NULL"), peaq_wide_workspace_bytes, the names in the header, the library and the
Python binding, the record's size, and the CLI's usage errors."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import gst_env
import gstpeaq_amd

ROOT = Path(__file__).resolve().parent.parent
PEAQ_ERR_ARG = -1
FACTORS = (2, 4, 8, 16, 32, 64)


@pytest.fixture(scope="module")
def lib():
    if not gstpeaq_amd.library_path().exists():
        gstpeaq_amd.build_library()
    return gstpeaq_amd.load_library()


def err(lib):
    return lib.peaq_last_error().decode()


# ---- definitions ------------------------------------------------------------------------------------------------------
def restated_factor(max_offset):
    if not 1 <= max_offset <= 1 << 20:
        return 0
    return next(M for M in FACTORS if -(-max_offset // M) <= 16384)


def test_wide_factor_over_a_grid(lib):
    grid = {0, 1, 2, 16384, 32768, 32769, 1 << 20, (1 << 20) + 1, 0xFFFFFFFF}
    for M in FACTORS:
        grid |= {16384 * M - 1, 16384 * M, 16384 * M + 1}
    for v in sorted(grid):
        assert gstpeaq_amd.wide_factor(v) == restated_factor(v), v
    assert gstpeaq_amd.wide_factor(1) == 2 and gstpeaq_amd.wide_factor(32768) == 2 and gstpeaq_amd.wide_factor(32769) == 4
    for M in FACTORS:
        assert gstpeaq_amd.wide_factor(16384 * M) == M
        assert gstpeaq_amd.wide_factor(16384 * M + 1) == (2 * M if M < 64 else 0)
    assert gstpeaq_amd.wide_factor(1 << 20) == 64 and gstpeaq_amd.wide_factor((1 << 20) + 1) == 0


@pytest.mark.parametrize("M", FACTORS)
def test_wide_taps_against_the_formula(lib, M):
    import mpmath as mp
    mp.mp.dps = 40
    h = gstpeaq_amd.wide_taps(M)
    assert h.dtype == np.float64 and h.shape == (16 * M + 1,)
    assert np.array_equal(h, h[::-1])                   # symmetric bit for bit
    assert abs(h.sum() - 1.) < 1e-3
    centre = h[8 * M]
    assert centre == 0.75 / M
    i0b = mp.besseli(0, mp.mpf("5.65"))
    for j in range(0, 8 * M + 1):
        x = mp.mpf(3 * j) / (4 * M)
        sinc = mp.mpf(1) if j == 0 else mp.sin(mp.pi * x) / (mp.pi * x)
        want = mp.mpf(3) / (4 * M) * sinc * mp.besseli(0, mp.mpf("5.65") * mp.sqrt(1 - (mp.mpf(j) / (8 * M)) ** 2)) / i0b
        # a few FP64 roundings of a convergent series
        assert abs(mp.mpf(float(h[8 * M + j])) - want) <= mp.mpf("1e-15") * centre, (M, j, h[8 * M + j], want)


def test_wide_taps_refusals(lib):
    h = (C.c_double * 2048)()
    for bad in (0, 1, 3, 6, 48, 128, 0xFFFFFFFF):
        assert lib.peaq_wide_taps(bad, h) == PEAQ_ERR_ARG and "peaq_wide_taps" in err(lib) and "M %d" % bad in err(lib), err(lib)
    assert lib.peaq_wide_taps(16, None) == PEAQ_ERR_ARG and "h is NULL" in err(lib)
    assert lib.peaq_wide_taps(64, h) == 1025
    with pytest.raises(gstpeaq_amd.PeaqError):
        gstpeaq_amd.wide_taps(3)


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_decimate_checks_its_arguments_before_any_device(lib):
    buf = (C.c_float * 64)()
    buf2 = (C.c_float * 64)()
    p, q = C.cast(buf, C.c_void_p), C.cast(buf2, C.c_void_p)
    who = "peaq_batch_decimate"

    def call(channels=2, n_pairs=1, d_in=p, in_stride=16, n_in=None, n_uniform=16, M=2, mode=0, d_out=q, out_stride=8, ctx=None):
        return lib.peaq_batch_decimate(ctx, channels, n_pairs, d_in, in_stride, n_in, n_uniform, M, mode, d_out, out_stride, None)

    for bad in (0, 1, 3, 128):
        assert call(M=bad) == PEAQ_ERR_ARG and who in err(lib) and "M %d" % bad in err(lib), err(lib)
    for bad in (-1, 2):
        assert call(mode=bad) == PEAQ_ERR_ARG and who in err(lib) and "mode %d" % bad in err(lib), err(lib)
    assert call(out_stride=7) == PEAQ_ERR_ARG and who in err(lib) and "out_stride 7" in err(lib) and "(8 samples)" in err(lib)
    assert call(n_uniform=17) == PEAQ_ERR_ARG and who in err(lib) and "n_uniform 17 passes in_stride 16" in err(lib), err(lib)
    lens = (C.c_uint32 * 1)(17)
    assert call(n_in=lens) == PEAQ_ERR_ARG and who in err(lib) and "n_in 17 passes in_stride 16" in err(lib), err(lib)
    assert call(d_in=None) == PEAQ_ERR_ARG and who in err(lib) and "NULL buffer" in err(lib)
    assert call(d_out=None) == PEAQ_ERR_ARG and who in err(lib) and "NULL buffer" in err(lib)
    for bad in (0, 3):
        assert call(channels=bad) == PEAQ_ERR_ARG and who in err(lib) and "not %d" % bad in err(lib), err(lib)
    assert call(n_pairs=65536) == PEAQ_ERR_ARG and who in err(lib) and "65536 pairs" in err(lib)
    assert call(n_pairs=-1) == PEAQ_ERR_ARG and who in err(lib)
    assert call(d_out=p) == PEAQ_ERR_ARG and who in err(lib) and "overlaps" in err(lib)
    assert call() == PEAQ_ERR_ARG and who in err(lib) and "ctx is NULL" in err(lib)
    assert call(channels=1, M=64, mode=1, out_stride=1) == PEAQ_ERR_ARG and "ctx is NULL" in err(lib)


def test_estimate_delay_wide_checks_its_arguments_before_any_device(lib):
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    rec = (gstpeaq_amd.WideDelay * 2)()
    who = "peaq_batch_estimate_delay_wide"

    def call(channels=2, n_pairs=1, ref=p, test=p, stride=16, n_ref=None, n_test=None, n_uniform=16, max_offset=400000, mode=1,
             max_lag=4096, out=rec, ctx=None):
        return lib.peaq_batch_estimate_delay_wide(ctx, channels, n_pairs, ref, test, stride, n_ref, n_test, n_uniform,
                                                  max_offset, mode, max_lag, out, None)

    for bad in (0, (1 << 20) + 1, 0xFFFFFFFF):
        assert call(max_offset=bad) == PEAQ_ERR_ARG and who in err(lib) and "max_offset %d" % bad in err(lib), err(lib)
    for bad in (-1, 2):
        assert call(mode=bad) == PEAQ_ERR_ARG and who in err(lib) and "mode %d" % bad in err(lib), err(lib)
    for bad in (0, 16385, 0xFFFFFFFF):
        assert call(max_lag=bad) == PEAQ_ERR_ARG and who in err(lib) and "max_lag %d" % bad in err(lib), err(lib)
    assert call(channels=3) == PEAQ_ERR_ARG and who in err(lib) and "channels" in err(lib)
    assert call(n_pairs=65536) == PEAQ_ERR_ARG and who in err(lib) and "65535" in err(lib)
    assert call(n_pairs=-1) == PEAQ_ERR_ARG and who in err(lib)
    assert call(ref=None) == PEAQ_ERR_ARG and who in err(lib) and "NULL buffer" in err(lib)
    assert call(test=None) == PEAQ_ERR_ARG and who in err(lib) and "NULL buffer" in err(lib)
    assert call(out=None) == PEAQ_ERR_ARG and who in err(lib) and "NULL out" in err(lib)
    lens = (C.c_uint32 * 1)(17)
    ok = (C.c_uint32 * 1)(16)
    assert call(n_ref=ok) == PEAQ_ERR_ARG and who in err(lib) and "both" in err(lib)
    assert call(n_ref=lens, n_test=ok) == PEAQ_ERR_ARG and who in err(lib) and "n_ref 17 passes pair_stride 16" in err(lib)
    assert call(n_ref=ok, n_test=lens) == PEAQ_ERR_ARG and who in err(lib) and "n_test 17 passes pair_stride 16" in err(lib)
    assert call(n_uniform=17) == PEAQ_ERR_ARG and who in err(lib) and "n_uniform 17" in err(lib)
    assert call() == PEAQ_ERR_ARG and who in err(lib) and "ctx is NULL" in err(lib)
    assert call(max_offset=1, mode=0, max_lag=1, n_ref=ok, n_test=ok) == PEAQ_ERR_ARG and "ctx is NULL" in err(lib)


def test_run_pair_wide_checks_its_arguments_before_any_device(lib):
    x = (C.c_float * 64)()
    out = (C.c_double * 16)()
    who = "peaq_run_pair_wide"

    def call(channels=2, rate=48000, max_offset=400000, mode=1, max_lag=4096, level=92., ref=x, res=out, ctx=None):
        return lib.peaq_run_pair_wide(ctx, 0, channels, level, rate, max_offset, mode, max_lag, ref, 32, x, 32, None, res)

    for bad in (0, (1 << 20) + 1):
        assert call(max_offset=bad) == PEAQ_ERR_ARG and who in err(lib) and "max_offset %d" % bad in err(lib), err(lib)
    assert call(mode=2) == PEAQ_ERR_ARG and who in err(lib) and "mode 2" in err(lib)
    for bad in (0, 16385):
        assert call(max_lag=bad) == PEAQ_ERR_ARG and who in err(lib) and "max_lag %d" % bad in err(lib), err(lib)
    assert call(channels=3) == PEAQ_ERR_ARG and who in err(lib) and "channels" in err(lib)
    assert call(level=131.) == PEAQ_ERR_ARG and who in err(lib)
    assert call(rate=7999) == PEAQ_ERR_ARG and who in err(lib) and "7999" in err(lib)
    assert call() == PEAQ_ERR_ARG and who in err(lib) and "ctx is NULL" in err(lib)


def test_python_refuses_wide_without_align_and_with_the_window_stages():
    with pytest.raises(ValueError, match="wide= requires align="):
        gstpeaq_amd.batch_run(None, 0, None, None, wide=400000)
    with pytest.raises(ValueError, match="wide= requires align="):
        gstpeaq_amd.run_pair(None, 0, np.zeros((8, 1), np.float32), np.zeros((8, 1), np.float32), wide=400000)
    for other in ("drift", "track", "steps"):
        with pytest.raises(ValueError, match="wide= and %s= exclude each other" % other):
            gstpeaq_amd.batch_run(None, 0, None, None, align=4096, wide=400000, **{other: True})
        with pytest.raises(ValueError, match="wide= and %s= exclude each other" % other):
            gstpeaq_amd.run_pair(None, 0, np.zeros((8, 1), np.float32), np.zeros((8, 1), np.float32), align=4096, wide=400000,
                                 **{other: True})


# ---- workspace --------------------------------------------------------------------------------------------------------
def test_workspace_is_monotone_in_n_max_and_stops_growing_with_n_pairs(lib):
    ws = gstpeaq_amd.wide_workspace_bytes
    assert ws(2, 0, 480000, 400000) == 0 and ws(3, 1, 480000, 400000) == 0 and ws(2, 1, 480000, 0) == 0
    assert ws(2, 1, 480000, (1 << 20) + 1) == 0 and ws(2, 65536, 480000, 400000) == 0
    # one pair: two cut buffers, two decimated ones (M = 32), two records
    assert ws(2, 1, 480000, 400000) == 2 * 480000 * 2 * 4 + 2 * 15000 * 4 + 2 * 32
    for channels in (1, 2):
        for max_offset in (1, 32768, 400000, 1 << 20):
            last = 0
            for n_max in (0, 1, 2, 3, 63, 64, 65, 48000, 480000, 4800000, 48000000, 0xFFFFFFFF):
                v = ws(channels, 50, n_max, max_offset)
                assert v >= last and v > 0, (n_max, v, last)
                last = v
            last = 0
            for n_pairs in (1, 2, 3, 64, 65, 1000, 4096, 65535):
                v = ws(channels, n_pairs, 480000, max_offset)
                assert v >= last, (n_pairs, v, last)
                last = v
            assert ws(channels, 65535, 480000, max_offset) == ws(channels, 30000, 480000, max_offset) <= (1 << 30)
    assert ws(2, 65535, 0xFFFFFFFF, 1 << 20) == ws(2, 1, 0xFFFFFFFF, 1 << 20)


# ---- names ------------------------------------------------------------------------------------------------------------
ENTRIES = {"peaq_wide_factor", "peaq_wide_taps", "peaq_wide_delay_size", "peaq_wide_workspace_bytes", "peaq_batch_decimate",
           "peaq_batch_estimate_delay_wide", "peaq_run_pair_wide"}
NAME = r"peaq_[a-z_0-9]*(?:wide|decimate)[a-z_0-9]*"


def test_the_header_declares_what_the_library_exports(lib):
    header = (ROOT / "include" / "peaq_amd.h").read_text()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)       # (comments speak of the entries as `name (...)` too)
    declared = set(re.findall(r"\b(" + NAME + r")\s*\(", code))
    exported = {m.decode() for m in re.findall(rb"\x00(" + NAME.encode() + rb")(?=\x00)",
                                               gstpeaq_amd.library_path().read_bytes())}
    exported = {n for n in exported if hasattr(lib, n)}
    assert declared == ENTRIES, declared
    assert exported == ENTRIES, exported
    for name in ENTRIES:
        assert not re.search("window|drift|track", name), name
    for define in ("PEAQ_WIDE_WAVEFORM   0", "PEAQ_WIDE_ENVELOPE   1", "PEAQ_WIDE_CHUNK      248", "PEAQ_WIDE_F_NONE  1",
                   "PEAQ_WIDE_F_RANGE 2", "PEAQ_WIDE_F_EDGE  4"):
        assert "#define " + define in header, define
    assert "wide delay search on the device" in header
    assert header.index("sub-sample delay on the device ---") < header.index("wide delay search on the device ---") < \
        header.index("constant drift on the device ---")


def test_python_binding_exports_the_wide_search():
    names = ("WIDE_WAVEFORM", "WIDE_ENVELOPE", "WIDE_CHUNK", "wide_factor", "wide_taps", "decimate", "estimate_delay_wide",
             "wide_workspace_bytes", "WideDelay", "WIDE_F_NONE", "WIDE_F_RANGE", "WIDE_F_EDGE")
    for name in names:
        assert hasattr(gstpeaq_amd, name) and name in gstpeaq_amd.__all__, name
    assert (gstpeaq_amd.WIDE_WAVEFORM, gstpeaq_amd.WIDE_ENVELOPE, gstpeaq_amd.WIDE_CHUNK) == (0, 1, 248)
    assert (gstpeaq_amd.WIDE_F_NONE, gstpeaq_amd.WIDE_F_RANGE, gstpeaq_amd.WIDE_F_EDGE) == (1, 2, 4)


def test_the_record_is_80_bytes(lib):
    assert C.sizeof(gstpeaq_amd.WideDelay) == 80 == lib.peaq_wide_delay_size() == gstpeaq_amd.WIDE_DELAY_DTYPE.itemsize
    assert gstpeaq_amd.WideDelay.fine.offset == 16 and gstpeaq_amd.WideDelay.coarse.offset == 48
    assert "typedef struct {            /* 80 bytes */" in (ROOT / "include" / "peaq_amd.h").read_text()


# ---- the CLI ----------------------------------------------------------------------------------------------------------
def cli(*args):
    if not gst_env.CLI.exists():
        subprocess.run(["make", "-C", str(gst_env.CLI.parent)], check=True, capture_output=True)
    return subprocess.run([str(gst_env.CLI), *args], capture_output=True, text=True, timeout=60)


def test_cli_wide_usage_errors_and_help():
    for bad in ("--align-wide=", "--align-wide=x", "--align-wide=0", "--align-wide=-1", "--align-wide=21.9", "--align-wide=5:",
                "--align-wide=5:both", "--align-wide=:envelope", "--align-wide=nan"):
        out = cli(bad, "ref.wav", "test.wav")
        assert out.returncode == 1 and "invalid wide offset" in out.stderr, (bad, out.stderr)
    for other, message in (("--list=pairs.txt", "--align-wide is not taken with --list"),
                           ("--interval=1", "--align-wide belongs to the plain one-call mode"),
                           ("--trace=y.csv", "--align-wide belongs to the plain one-call mode"),
                           ("--match-gain", "--align-wide is not taken with --match-gain"),
                           ("--align-subsample", "--align-wide is not taken with another --align-... option"),
                           ("--align-drift", "--align-wide is not taken with another --align-... option"),
                           ("--align-track", "--align-wide is not taken with another --align-... option"),
                           ("--align-steps", "--align-wide is not taken with another --align-... option")):
        args = ("--align-wide=8", other) if other.startswith("--list") else ("--align-wide=8", other, "ref.wav", "test.wav")
        out = cli(*args)
        assert out.returncode == 1 and message in out.stderr, (other, out.stderr)
    # the outputs that are runs of their own refuse it through the condition they have, their messages unchanged
    for own in ("--bands=y.csv", "--pattern-bands=y.csv", "--band-summary=y.csv", "--windows=1"):
        out = cli("--align-wide", own, "ref.wav", "test.wav")
        assert out.returncode == 1 and own.split("=")[0] + " is a run of its own" in out.stderr and \
            "an --align-... beyond --align" in out.stderr, (own, out.stderr)
    out = cli("--help")
    assert out.returncode == 0 and "--align-wide[=SECONDS[:waveform|envelope]]" in out.stdout

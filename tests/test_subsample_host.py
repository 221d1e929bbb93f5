"""The host side of the sub-sample stage without a GPU (include/peaq_amd.h, "sub-sample delay on the device"): the two
tables of peaq_subsample_tables against numpy and the header's formulas, the record's size, and the argument checks of
peaq_batch_refine_delay, peaq_batch_cut_shifted and peaq_run_pair_subsample, which return PEAQ_ERR_ARG with the
offending value in the message before any device is touched (a NULL context is the last thing they look at)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import gstpeaq_amd

PEAQ_ERR_ARG = -1
ROOT = Path(__file__).resolve().parent.parent
BETA = 8.49


@pytest.fixture(scope="module")
def lib():
    if not gstpeaq_amd.library_path().exists():
        gstpeaq_amd.build_library()
    return gstpeaq_amd.load_library()


@pytest.fixture(scope="module")
def tables(lib):
    return gstpeaq_amd.subsample_tables()


def err(lib):
    return lib.peaq_last_error().decode()


def u32(*v):
    return (C.c_uint32 * len(v))(*v)


def i32(*v):
    return (C.c_int32 * len(v))(*v)


def header_define(name):
    text = (ROOT / "include" / "peaq_amd.h").read_text()
    return int(re.search(r"^#define\s+%s\s+(\w+)" % name, text, flags=re.M).group(1), 0)


def window(x, half):
    u = np.clip(np.abs(x) / half, 0.0, 1.0)
    return np.where(np.abs(x) < half, np.i0(BETA * np.sqrt(1.0 - u * u)) / np.i0(BETA), 0.0)


def test_tables_are_the_header_formulas(tables):
    corr, shift = tables
    assert corr.shape == (256, 33) and shift.shape == (256, 65)
    tau = np.arange(-128, 128)[:, None] / 256.0
    x = tau - np.arange(-16, 17)[None, :]
    assert np.max(np.abs(corr - np.sinc(x) * window(x, 17.0))) <= 1e-15
    y = np.arange(-32, 33)[None, :] - tau
    want = np.sinc(y) * window(y, 33.0)
    rows = np.arange(256) != 128                        # (row q = 0 is set, not evaluated: next test)
    assert np.max(np.abs(shift[rows] - want[rows])) <= 1e-15
    assert np.max(np.abs(shift[128] - want[128])) <= 1e-15


def test_shift_row_zero_is_exactly_the_impulse(tables):
    impulse = np.zeros(65)
    impulse[32] = 1.0
    assert np.array_equal(tables[1][128], impulse)
    assert not np.signbit(tables[1][128]).any()


def test_every_shift_row_sums_to_one(tables):
    assert np.max(np.abs(tables[1].sum(axis=1) - 1.0)) < 1e-3


def test_shift_table_is_symmetric_in_q_and_o(tables):
    shift = tables[1]
    for q in range(1, 128):
        assert np.max(np.abs(shift[128 + q] - shift[128 - q][::-1])) <= 1e-15, q


def test_record_size_and_constants(lib):
    assert lib.peaq_subdelay_size() == 40 == C.sizeof(gstpeaq_amd.SubDelay) == gstpeaq_amd.SUBDELAY_DTYPE.itemsize
    for name, value in (("PEAQ_SUB_STEPS", gstpeaq_amd.SUB_STEPS), ("PEAQ_SUB_LAGS", gstpeaq_amd.SUB_LAGS),
                        ("PEAQ_SUB_HALF", gstpeaq_amd.SUB_HALF), ("PEAQ_SUB_F_NONE", gstpeaq_amd.SUB_F_NONE),
                        ("PEAQ_SUB_F_EDGE", gstpeaq_amd.SUB_F_EDGE)):
        assert header_define(name) == value, name
    assert (gstpeaq_amd.SUB_STEPS, gstpeaq_amd.SUB_LAGS, gstpeaq_amd.SUB_HALF) == (256, 16, 32)
    assert lib.peaq_subsample_tables(None, None) == PEAQ_ERR_ARG and "NULL" in err(lib)


def test_refine_delay_checks_its_arguments_before_any_device(lib):
    a, b, o = (C.c_float * 256)(), (C.c_float * 256)(), (C.c_char * 160)()
    p, q, r = (C.cast(x, C.c_void_p) for x in (a, b, o))

    def call(channels=2, n_pairs=3, d_ref=p, d_test=q, stride=16, n_ref=u32(16, 14, 13), n_test=u32(16, 16, 1), n_uniform=0,
             lag=i32(0, -3, 100), d_out=r):
        return lib.peaq_batch_refine_delay(None, channels, n_pairs, d_ref, d_test, stride, n_ref, n_test, n_uniform, lag, d_out, None)

    for bad in (0, 3):
        assert call(channels=bad) == PEAQ_ERR_ARG and "channels" in err(lib) and str(bad) in err(lib), err(lib)
    assert call(n_pairs=65536) == PEAQ_ERR_ARG and "65536 pairs" in err(lib) and "65535" in err(lib), err(lib)
    assert call(n_pairs=-1) == PEAQ_ERR_ARG and "-1" in err(lib), err(lib)
    for name in ("d_ref", "d_test", "d_out"):
        assert call(**{name: None}) == PEAQ_ERR_ARG and "NULL buffer" in err(lib), err(lib)
    assert call(lag=None) == PEAQ_ERR_ARG and "NULL lag" in err(lib), err(lib)
    assert call(n_test=None) == PEAQ_ERR_ARG and "both" in err(lib), err(lib)
    assert call(n_ref=u32(16, 17, 13)) == PEAQ_ERR_ARG and "pair 1" in err(lib) and "n_ref 17" in err(lib) \
        and "pair_stride 16" in err(lib), err(lib)
    assert call(n_test=u32(16, 16, 0xFFFFFFFF)) == PEAQ_ERR_ARG and "pair 2" in err(lib) and "n_test 4294967295" in err(lib), err(lib)
    assert call(n_ref=None, n_test=None, n_uniform=17) == PEAQ_ERR_ARG and "n_uniform 17" in err(lib), err(lib)
    # a lag beyond a signal's length is no error (the pair gets PEAQ_SUB_F_NONE): the context is looked at last
    assert call(lag=i32(0x7FFFFFFF, -0x80000000, 16)) == PEAQ_ERR_ARG and "ctx is NULL" in err(lib), err(lib)
    assert call(n_ref=None, n_test=None, n_uniform=16) == PEAQ_ERR_ARG and "ctx is NULL" in err(lib), err(lib)
    assert call(n_pairs=0, d_ref=None, d_test=None, d_out=None, lag=None) == PEAQ_ERR_ARG and "ctx is NULL" in err(lib)


def test_cut_shifted_checks_its_arguments_before_any_device(lib):
    buf, out = (C.c_float * 256)(), (C.c_float * 256)()
    p, q = (C.cast(x, C.c_void_p) for x in (buf, out))

    def call(channels=2, n_pairs=3, d_in=p, in_stride=16, n_in=u32(16, 16, 8), skip=u32(0, 2, 3), n_keep=u32(16, 14, 5),
             qq=i32(-128, 0, 127), d_out=q, out_stride=16):
        return lib.peaq_batch_cut_shifted(None, channels, n_pairs, d_in, in_stride, n_in, skip, n_keep, qq, d_out, out_stride, None)

    # what peaq_batch_cut refuses
    assert call(skip=u32(0, 3, 3)) == PEAQ_ERR_ARG and "pair 1" in err(lib) and "skip 3" in err(lib) and "n_keep 14" in err(lib) \
        and "in_stride 16" in err(lib), err(lib)
    assert call(skip=u32(0, 2, 0xFFFFFFFF)) == PEAQ_ERR_ARG and "4294967295" in err(lib), err(lib)
    assert call(out_stride=15) == PEAQ_ERR_ARG and "out_stride 15" in err(lib) and "16" in err(lib), err(lib)
    for name in ("d_in", "d_out"):
        assert call(**{name: None}) == PEAQ_ERR_ARG and "NULL buffer" in err(lib), err(lib)
    for name in ("n_in", "skip", "n_keep", "qq"):
        assert call(**{name: None}) == PEAQ_ERR_ARG and "NULL n_in, skip, n_keep or q" in err(lib), err(lib)
    for bad in (0, 3):
        assert call(channels=bad) == PEAQ_ERR_ARG and "channels" in err(lib) and str(bad) in err(lib), err(lib)
    assert call(n_pairs=65536) == PEAQ_ERR_ARG and "65536 pairs" in err(lib) and "65535" in err(lib), err(lib)
    assert call(n_pairs=-1) == PEAQ_ERR_ARG and "-1" in err(lib), err(lib)
    assert call(d_out=C.c_void_p(p.value + 95 * 4)) == PEAQ_ERR_ARG and "overlaps" in err(lib), err(lib)
    assert call(d_out=p) == PEAQ_ERR_ARG and "overlaps" in err(lib), err(lib)
    # its own
    for bad in (-129, 128, 256, -0x80000000):
        assert call(qq=i32(0, bad, 0)) == PEAQ_ERR_ARG and "pair 1" in err(lib) and "q %d" % bad in err(lib), err(lib)
    assert call(n_in=u32(16, 16, 17)) == PEAQ_ERR_ARG and "pair 2" in err(lib) and "n_in 17" in err(lib) \
        and "in_stride 16" in err(lib), err(lib)
    # everything in order, the grid's two ends included: the context is looked at last
    assert call(d_out=C.c_void_p(p.value + 96 * 4)) == PEAQ_ERR_ARG and "ctx is NULL" in err(lib), err(lib)
    assert call() == PEAQ_ERR_ARG and "ctx is NULL" in err(lib)


def test_run_pair_subsample_checks_its_arguments_before_any_device(lib):
    x = np.zeros((64, 2), np.float32)
    fp = x.ctypes.data_as(C.POINTER(C.c_float))
    out = np.zeros(16)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))

    def call(channels=2, level=92.0, rate=48000, max_lag=64, mode=1, max_gain_db=40.0, ref=fp, test=fp, o=dp):
        return lib.peaq_run_pair_subsample(None, 0, channels, level, rate, max_lag, mode, max_gain_db, ref, 64, test, 64, None,
                                           None, None, o)

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


def test_python_keyword_needs_align():
    with pytest.raises(gstpeaq_amd.PeaqError, match="requires align="):
        gstpeaq_amd.run_pair(None, 0, np.zeros((8, 1), np.float32), np.zeros((8, 1), np.float32), subsample=True)
    with pytest.raises(gstpeaq_amd.PeaqError, match="requires align="):
        gstpeaq_amd.capi._aligned(None, None, None, None, None, None, None, subsample=True)


def test_workspace_figure():
    ws = gstpeaq_amd.subdelay_workspace_bytes
    row = 33 * 8
    assert ws(2, 0, 480000) == 0 and ws(3, 4, 480000) == 0
    assert ws(2, 1, 1) == 2 * row and ws(2, 1, 4096) == 2 * row and ws(2, 1, 4097) == 3 * row and ws(1, 1, 0) == 2 * row
    assert ws(1, 7, 3 * 4096 + 7) == 7 * 5 * row
    one = ws(2, 1, 0xFFFFFFFF)
    assert one == (-(-0xFFFFFFFF // 4096) + 1) * row
    assert ws(2, 65535, 0xFFFFFFFF) == one                # (one pair's row is more than the 256 MiB the groups stop at)
    assert ws(2, 65535, 48000 * 600) == 256 << 20


def test_launches_pass_no_dynamic_lds():
    text = (ROOT / "gstpeaq_amd" / "csrc" / "peaq_frac.hip").read_text()
    launches = re.findall(r"hipLaunchKernelGGL\((\w+), dim3\([^;]*?\), dim3\((\d+)\), (\w+), stream", text)
    assert sorted(k for k, _, _ in launches) == ["frac_corr_kernel", "frac_cut_kernel", "frac_pick_kernel", "frac_sum_kernel"], launches
    assert all(block == "256" and lds == "0" for _, block, lds in launches), launches

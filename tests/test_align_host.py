"""The aligner's host side without a GPU (include/peaq_amd.h, "time alignment on the device"): peaq_aligned_lengths
against its restatement, peaq_align_workspace_bytes, and the argument checks of every new entry point, which return
PEAQ_ERR_ARG with a message before any device is touched (a NULL context where the order of the checks allows it)."""
import ctypes as C

import pytest

import gstpeaq_amd

PEAQ_ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    if not gstpeaq_amd.library_path().exists():
        gstpeaq_amd.build_library()
    return gstpeaq_amd.load_library()


def restated(lag, n_ref, n_test):
    skip_ref, skip_test = min(max(-lag, 0), n_ref), min(max(lag, 0), n_test)
    return skip_ref, skip_test, min(n_ref - skip_ref, n_test - skip_test)


def test_aligned_lengths_over_a_grid(lib):
    lengths = (0, 1, 2047, 2048, 96000)
    for lag in range(-5000, 5001, 137):
        for n_ref in lengths:
            for n_test in lengths:
                got = gstpeaq_amd.aligned_lengths(lag, n_ref, n_test)
                assert got == restated(lag, n_ref, n_test), (lag, n_ref, n_test, got)
                assert got[0] + got[2] <= n_ref and got[1] + got[2] <= n_test
    # a lag beyond a signal leaves nothing in common
    assert gstpeaq_amd.aligned_lengths(3000, 96000, 2048)[2] == 0
    assert gstpeaq_amd.aligned_lengths(-3000, 2047, 96000)[2] == 0
    assert gstpeaq_amd.aligned_lengths(4096, 96000, 96000 + 4096) == (0, 4096, 96000)
    assert gstpeaq_amd.aligned_lengths(-4096, 96000, 96000 - 4096) == (4096, 0, 96000 - 4096)
    # NULL outputs are skipped
    n = C.c_uint32(7)
    lib.peaq_aligned_lengths(5, 100, 50, None, None, C.byref(n))
    assert n.value == 45


def err(lib):
    return lib.peaq_last_error().decode()


def test_estimate_delay_checks_its_arguments_before_any_device(lib):
    buf = (C.c_float * 64)()
    rec = (gstpeaq_amd.Delay * 2)()
    p = C.cast(buf, C.c_void_p)
    out = C.cast(rec, C.c_void_p)

    def call(channels=2, n_pairs=1, ref=p, test=p, stride=16, max_lag=4096, d_out=out, ctx=None):
        return lib.peaq_batch_estimate_delay(ctx, channels, n_pairs, ref, test, stride, None, None, 16, max_lag, d_out, None)

    for bad in (0, 16385, 0xFFFFFFFF):
        assert call(max_lag=bad) == PEAQ_ERR_ARG and "max_lag %d" % bad in err(lib), err(lib)
    assert call(channels=3) == PEAQ_ERR_ARG and "channels" in err(lib)
    assert call(n_pairs=65536) == PEAQ_ERR_ARG and "65535" in err(lib)
    assert call(n_pairs=-1) == PEAQ_ERR_ARG
    assert call(ref=None) == PEAQ_ERR_ARG and "NULL buffer" in err(lib)
    assert call(test=None) == PEAQ_ERR_ARG and "NULL buffer" in err(lib)
    assert call(d_out=None) == PEAQ_ERR_ARG and "NULL buffer" in err(lib)
    assert call() == PEAQ_ERR_ARG and "ctx is NULL" in err(lib)


def test_cut_checks_its_arguments_before_any_device(lib):
    buf = (C.c_float * 64)()
    buf2 = (C.c_float * 64)()
    p, q = C.cast(buf, C.c_void_p), C.cast(buf2, C.c_void_p)
    one = (C.c_uint32 * 1)(0)

    def call(channels=2, n_pairs=1, d_in=p, d_out=q, skip=one, keep=one, ctx=None):
        return lib.peaq_batch_cut(ctx, channels, n_pairs, d_in, 16, skip, keep, d_out, 16, None)

    assert call(channels=3) == PEAQ_ERR_ARG and "channels" in err(lib)
    assert call(channels=0) == PEAQ_ERR_ARG
    assert call(n_pairs=65536) == PEAQ_ERR_ARG and "65535" in err(lib)
    assert call(d_in=None) == PEAQ_ERR_ARG and "NULL buffer" in err(lib)
    assert call(d_out=None) == PEAQ_ERR_ARG and "NULL buffer" in err(lib)
    assert call(skip=None) == PEAQ_ERR_ARG and "NULL" in err(lib)
    assert call() == PEAQ_ERR_ARG and "ctx is NULL" in err(lib)


def test_run_pair_aligned_checks_its_arguments_before_any_device(lib):
    x = (C.c_float * 64)()
    out = (C.c_double * 16)()

    def call(channels=2, rate=48000, max_lag=4096, level=92., ref=x, res=out, ctx=None):
        return lib.peaq_run_pair_aligned(ctx, 0, channels, level, rate, max_lag, ref, 32, x, 32, None, res)

    for bad in (0, 16385):
        assert call(max_lag=bad) == PEAQ_ERR_ARG and "max_lag %d" % bad in err(lib), err(lib)
    assert call(channels=3) == PEAQ_ERR_ARG and "channels" in err(lib)
    assert call(level=131.) == PEAQ_ERR_ARG
    assert call(rate=7999) == PEAQ_ERR_ARG and "7999" in err(lib)
    assert call() == PEAQ_ERR_ARG and "NULL" in err(lib)


def test_workspace_is_monotone_and_zero_for_no_pairs(lib):
    ws = gstpeaq_amd.align_workspace_bytes
    assert ws(2, 0, 480000, 4096) == 0 and ws(1, 0, 0, 1) == 0
    assert ws(2, 1, 480000, 4096) > 0
    for channels in (1, 2):
        assert ws(1, 8, 96000, 4096) <= ws(channels, 8, 96000, 4096) <= ws(2, 8, 96000, 4096)
        last = 0
        for n_pairs in (1, 2, 3, 64, 65, 1000, 4096, 65535):
            v = ws(channels, n_pairs, 480000, 4096)
            assert v >= last, (n_pairs, v, last)
            last = v
        last = 0
        for n_max in (0, 1, 511, 512, 513, 48000, 480000, 4800000, 48000000, 0xFFFFFFFF):
            v = ws(channels, 50, n_max, 4096)
            assert v >= last, (n_max, v, last)
            last = v
        last = 0
        for max_lag in (1, 511, 512, 513, 1024, 4095, 4096, 4097, 8192, 16384):
            v = ws(channels, 50, 480000, max_lag)
            assert v >= last, (max_lag, v, last)
            last = v
    # pairs are taken in groups: the scratch stops growing at about 1 GiB (or one pair's, if that is more)
    assert ws(2, 65535, 480000, 4096) <= (1 << 30)
    assert ws(2, 65535, 0xFFFFFFFF, 16384) == ws(2, 1, 0xFFFFFFFF, 16384)

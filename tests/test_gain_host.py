"""The host side of the gain stage without a GPU (include/peaq_amd.h, "level and polarity matching on the device"): the
record's size, the argument checks of peaq_batch_measure_gain, peaq_batch_cut_scaled, peaq_run_pair_matched and
peaq_batch_run_host_matched, which return PEAQ_ERR_ARG with the offending value in the message before any device is
touched (a NULL context is the last thing they look at), and peaq_gain_workspace_bytes."""
import ctypes as C
import re
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


def header_define(name):
    text = (ROOT / "include" / "peaq_amd.h").read_text()
    return int(re.search(r"^#define\s+%s\s+(\w+)" % name, text, flags=re.M).group(1), 0)


def test_record_is_80_bytes_and_the_feed_keeps_its_24(lib):
    assert lib.peaq_gain_size() == 80 == C.sizeof(gstpeaq_amd.Gain) == gstpeaq_amd.GAIN_DTYPE.itemsize
    assert lib.peaq_feed_size() == 24 == C.sizeof(gstpeaq_amd.Feed)


def test_binding_and_header_agree_on_the_constants():
    for name, value in (("PEAQ_GAIN_OFF", 0), ("PEAQ_GAIN_LSQ", gstpeaq_amd.GAIN_MODES["lsq"]),
                        ("PEAQ_GAIN_RMS", gstpeaq_amd.GAIN_MODES["rms"]), ("PEAQ_GAIN_POLARITY", gstpeaq_amd.GAIN_MODES["polarity"]),
                        ("PEAQ_GAIN_PER_CHANNEL", gstpeaq_amd.GAIN_PER_CHANNEL), ("PEAQ_GAIN_F_SILENT", gstpeaq_amd.GAIN_F_SILENT),
                        ("PEAQ_GAIN_F_NONFINITE", gstpeaq_amd.GAIN_F_NONFINITE), ("PEAQ_GAIN_F_ZERO", gstpeaq_amd.GAIN_F_ZERO),
                        ("PEAQ_GAIN_F_RANGE", gstpeaq_amd.GAIN_F_RANGE)):
        assert header_define(name) == value, name
    assert (gstpeaq_amd.gain_mode("lsq"), gstpeaq_amd.gain_mode("rms", True), gstpeaq_amd.gain_mode(None)) == (1, 0x12, 0)
    with pytest.raises(gstpeaq_amd.PeaqError, match="loud"):
        gstpeaq_amd.gain_mode("loud")


def test_measure_gain_checks_its_arguments_before_any_device(lib):
    a, b, o = (C.c_float * 256)(), (C.c_float * 256)(), (C.c_char * 320)()
    p, q, r = (C.cast(x, C.c_void_p) for x in (a, b, o))

    def call(channels=2, n_pairs=3, d_ref=p, ref_stride=16, skip_ref=u32(0, 2, 3), d_test=q, test_stride=20,
             skip_test=u32(4, 0, 7), n=u32(16, 14, 13), mode=1, max_gain_db=40.0, d_out=r):
        return lib.peaq_batch_measure_gain(None, channels, n_pairs, d_ref, ref_stride, skip_ref, d_test, test_stride, skip_test,
                                           n, mode, max_gain_db, d_out, None)

    for bad in (4, 0x20 | 1, 0x14, -1, 0x100):
        assert call(mode=bad) == PEAQ_ERR_ARG and "mode %d" % bad in err(lib), err(lib)
    for bad in (0.0, -3.0, 120.5, float("inf")):
        assert call(max_gain_db=bad) == PEAQ_ERR_ARG and "max_gain_db" in err(lib) and ("%f" % bad) in err(lib), err(lib)
    assert call(max_gain_db=float("nan")) == PEAQ_ERR_ARG and "max_gain_db" in err(lib) and "nan" in err(lib).lower(), err(lib)
    for bad in (0, 3):
        assert call(channels=bad) == PEAQ_ERR_ARG and "channels" in err(lib) and str(bad) in err(lib), err(lib)
    assert call(n_pairs=65536) == PEAQ_ERR_ARG and "65536 pairs" in err(lib) and "65535" in err(lib), err(lib)
    assert call(n_pairs=-1) == PEAQ_ERR_ARG and "-1" in err(lib), err(lib)
    for name in ("d_ref", "d_test", "d_out"):
        assert call(**{name: None}) == PEAQ_ERR_ARG and "NULL buffer" in err(lib), err(lib)
    for name in ("skip_ref", "skip_test", "n"):
        assert call(**{name: None}) == PEAQ_ERR_ARG and "NULL skip_ref, skip_test or n" in err(lib), err(lib)
    assert call(skip_ref=u32(0, 3, 3)) == PEAQ_ERR_ARG and "pair 1" in err(lib) and "skip_ref 3" in err(lib) \
        and "n 14" in err(lib) and "ref_stride 16" in err(lib), err(lib)
    assert call(skip_test=u32(4, 0, 8)) == PEAQ_ERR_ARG and "pair 2" in err(lib) and "skip_test 8" in err(lib) \
        and "n 13" in err(lib) and "test_stride 20" in err(lib), err(lib)
    assert call(skip_ref=u32(0, 2, 0xFFFFFFFF)) == PEAQ_ERR_ARG and "4294967295" in err(lib), err(lib)   # (no wrap-around)
    # everything in order, every mode and the largest max_gain_db: the context is looked at last
    for mode in (0, 1, 2, 3, 0x10, 0x11, 0x12, 0x13):
        assert call(mode=mode, max_gain_db=120.0) == PEAQ_ERR_ARG and "ctx is NULL" in err(lib), (mode, err(lib))
    assert call(n_pairs=0, d_ref=None, d_test=None, d_out=None, skip_ref=None, skip_test=None, n=None) == PEAQ_ERR_ARG \
        and "ctx is NULL" in err(lib)


def test_cut_scaled_checks_its_arguments_before_any_device(lib):
    buf, out, g = (C.c_float * 256)(), (C.c_float * 256)(), (C.c_char * 320)()
    p, q, r = (C.cast(x, C.c_void_p) for x in (buf, out, g))

    def call(channels=2, n_pairs=3, d_in=p, in_stride=16, skip=u32(0, 2, 3), n_keep=u32(16, 14, 5), d_gain=r, d_out=q,
             out_stride=16):
        return lib.peaq_batch_cut_scaled(None, channels, n_pairs, d_in, in_stride, skip, n_keep, d_gain, d_out, out_stride, None)

    assert call(skip=u32(0, 3, 3)) == PEAQ_ERR_ARG and "pair 1" in err(lib) and "skip 3" in err(lib) and "n_keep 14" in err(lib) \
        and "in_stride 16" in err(lib), err(lib)
    assert call(skip=u32(0, 2, 0xFFFFFFFF)) == PEAQ_ERR_ARG and "4294967295" in err(lib), err(lib)
    assert call(out_stride=15) == PEAQ_ERR_ARG and "out_stride 15" in err(lib) and "16" in err(lib), err(lib)
    for name in ("d_in", "d_out"):
        assert call(**{name: None}) == PEAQ_ERR_ARG and "NULL buffer" in err(lib), err(lib)
    assert call(d_gain=None) == PEAQ_ERR_ARG and "NULL d_gain" in err(lib), err(lib)
    for name in ("skip", "n_keep"):
        assert call(**{name: None}) == PEAQ_ERR_ARG and "NULL skip or n_keep" in err(lib), err(lib)
    for bad in (0, 3):
        assert call(channels=bad) == PEAQ_ERR_ARG and "channels" in err(lib) and str(bad) in err(lib), err(lib)
    assert call(n_pairs=65536) == PEAQ_ERR_ARG and "65536 pairs" in err(lib) and "65535" in err(lib), err(lib)
    # 3 pairs of 16 stereo samples are 96 floats
    assert call(d_out=C.c_void_p(p.value + 95 * 4)) == PEAQ_ERR_ARG and "overlaps" in err(lib), err(lib)
    assert call(d_out=p) == PEAQ_ERR_ARG and "overlaps" in err(lib), err(lib)
    assert call(d_out=C.c_void_p(p.value + 96 * 4)) == PEAQ_ERR_ARG and "ctx is NULL" in err(lib), err(lib)
    assert call() == PEAQ_ERR_ARG and "ctx is NULL" in err(lib)


def test_run_pair_matched_checks_its_arguments_before_any_device(lib):
    x = np.zeros((64, 2), np.float32)
    fp = x.ctypes.data_as(C.POINTER(C.c_float))
    out = np.zeros(16)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))

    def call(channels=2, level=92.0, rate=48000, max_lag=64, mode=1, max_gain_db=40.0, ref=fp, test=fp, o=dp):
        return lib.peaq_run_pair_matched(None, 0, channels, level, rate, max_lag, mode, max_gain_db, ref, 64, test, 64, None, None, o)

    assert call(mode=7) == PEAQ_ERR_ARG and "mode 7" in err(lib), err(lib)
    assert call(max_gain_db=121.0) == PEAQ_ERR_ARG and "max_gain_db 121" in err(lib), err(lib)
    assert call(max_lag=16385) == PEAQ_ERR_ARG and "16385" in err(lib), err(lib)
    assert call(channels=3) == PEAQ_ERR_ARG and "channels" in err(lib), err(lib)
    assert call(level=131.0) == PEAQ_ERR_ARG and "playback level" in err(lib), err(lib)
    assert call(rate=500000) == PEAQ_ERR_ARG and "500000" in err(lib), err(lib)
    assert call(ref=None) == PEAQ_ERR_ARG and "NULL" in err(lib), err(lib)
    assert call(max_lag=0) == PEAQ_ERR_ARG and "NULL argument" in err(lib), err(lib)     # (0: no alignment; the context is NULL)


def test_run_host_matched_refuses_what_the_shared_feed_refuses_and_the_gain_arguments(lib, monkeypatch):
    monkeypatch.delenv("PEAQ_AMD_FEED_THREADS", raising=False)
    x = np.zeros(64, np.int16)
    refs = (gstpeaq_amd.HostSignal * 2)()
    tests = (gstpeaq_amd.HostTest * 2)()
    for r in refs:
        r.data, r.n = x.ctypes.data, 32
    for t in tests:
        t.data, t.n, t.ref = x.ctypes.data, 32, 1
    out = np.zeros((2, 16))
    dp = out.ctypes.data_as(C.POINTER(C.c_double))

    def call(feed=None, level=92.0, mode=2, max_gain_db=40.0, n_refs=2):
        feed = feed or gstpeaq_amd.make_feed("s16", 1, align=64)
        return lib.peaq_batch_run_host_matched(None, 0, level, C.byref(feed), mode, max_gain_db, n_refs, refs, 2, tests, dp, None, None)

    assert call(mode=5) == PEAQ_ERR_ARG and "mode 5" in err(lib) and "peaq_batch_run_host_matched" in err(lib), err(lib)
    assert call(mode=0x23) == PEAQ_ERR_ARG and "mode 35" in err(lib), err(lib)
    assert call(max_gain_db=0.0) == PEAQ_ERR_ARG and "max_gain_db 0" in err(lib), err(lib)
    assert call(max_gain_db=float("nan")) == PEAQ_ERR_ARG and "max_gain_db" in err(lib), err(lib)
    bad = gstpeaq_amd.make_feed("s16", 1)
    bad.struct_size = 28
    assert call(feed=bad) == PEAQ_ERR_ARG and "28" in err(lib), err(lib)
    assert call(feed=gstpeaq_amd.make_feed("s16", 3)) == PEAQ_ERR_ARG and "channels" in err(lib), err(lib)
    assert call(feed=gstpeaq_amd.make_feed("s16", 1, align=16385)) == PEAQ_ERR_ARG and "16385" in err(lib), err(lib)
    assert call(level=-1.0) == PEAQ_ERR_ARG and "playback level" in err(lib), err(lib)
    assert call(n_refs=1) == PEAQ_ERR_ARG and "test 0" in err(lib) and "reference 1 of 1" in err(lib), err(lib)
    for mode in (0, 1, 0x13):
        assert call(mode=mode) == PEAQ_ERR_ARG and "ctx is NULL" in err(lib), (mode, err(lib))


def test_workspace_figure(lib):
    chunk = header_define("PEAQ_GAIN_CHUNK")
    ws = gstpeaq_amd.gain_workspace_bytes
    assert ws(2, 0, 480000) == 0 and ws(1, 0, 0) == 0
    assert ws(3, 4, 480000) == 0                        # (channels)
    per_chunk = 6 * 8                                   # three sums, two channels, FP64
    assert ws(2, 1, 1) == per_chunk and ws(2, 1, chunk) == per_chunk and ws(2, 1, chunk + 1) == 2 * per_chunk
    assert ws(2, 1, 0) == per_chunk                     # (a row is never empty)
    assert ws(1, 7, 3 * chunk + 7) == 7 * 4 * per_chunk
    assert ws(2, 4096, 480000) == 4096 * -(-480000 // chunk) * per_chunk
    # grows with n_max ...
    sizes = [ws(2, 16, n) for n in (1000, 48000, 480000, 4800000)]
    assert sizes == sorted(sizes) and len(set(sizes)) == 4, sizes
    # ... and stops growing with n_pairs: pairs are taken in groups of at most 256 MiB of partials
    n_max = 0xFFFFFFFF
    one = ws(2, 1, n_max)
    assert one == -(-n_max // chunk) * per_chunk
    assert ws(2, 5, n_max) == 5 * one and ws(2, 6, n_max) == ws(2, 65535, n_max) == 256 << 20
    # the feed's figure: the cut buffers, the records and the partials on top of the shared feed's
    feed = gstpeaq_amd.make_feed("s16", 2, align=64, chunk_pairs=8)
    plain = gstpeaq_amd.feed_refs_workspace_bytes(feed, 0, 4, 32, 480000)
    assert lib.peaq_feed_matched_workspace_bytes(C.byref(feed), 0, 0, 4, 32, 480000) == plain
    assert lib.peaq_feed_matched_workspace_bytes(C.byref(feed), 0, 1, 4, 32, 480000) == plain + 3 * 8 * 80 + ws(2, 8, 480000)
    assert lib.peaq_feed_matched_workspace_bytes(C.byref(feed), 0, 9, 4, 32, 480000) == 0
    unaligned = gstpeaq_amd.make_feed("s16", 2, chunk_pairs=8)
    assert lib.peaq_feed_matched_workspace_bytes(C.byref(unaligned), 0, 2, 4, 32, 480000) == \
        gstpeaq_amd.feed_refs_workspace_bytes(unaligned, 0, 4, 32, 480000) + 2 * 8 * 480000 * 8 + 3 * 8 * 80 + ws(2, 8, 480000)


def test_launches_pass_no_dynamic_lds():
    text = (ROOT / "gstpeaq_amd" / "csrc" / "peaq_gain.hip").read_text()
    launches = re.findall(r"hipLaunchKernelGGL\((\w+), dim3\([^;]*?\), dim3\((\d+)\), (\w+), stream", text)
    assert sorted(k for k, _, _ in launches) == ["gain_cut_kernel", "gain_finish_kernel", "gain_measure_kernel"], launches
    assert all(block == "256" and lds == "0" for _, block, lds in launches), launches

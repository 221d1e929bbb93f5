"""CPU-side checks of the filter-bank band-trace entry points (peaq_fb_band_count, peaq_fb_band_tables,
peaq_batch_run_fb_bands, peaq_run_pair_fb_bands, `peaq --fb-bands`; include/peaq_amd.h): the tables are the oracle's,
and every argument the header says is refused is refused with PEAQ_ERR_ARG before a context or a device is touched --
the calls below pass no context at all, or one that is never dereferenced -- with a message that names the value."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import gst_env
import oracle_lib as orc

NAMES = ["moddiff", "modwt", "noiseloud", "missing", "lindist", "unsm_ref", "unsm_test", "exc_ref", "exc_test",
         "adapt_ref", "adapt_test", "mod_ref", "mod_test"]


@pytest.fixture(scope="module")
def lib():
    import gstpeaq_amd
    if not gstpeaq_amd.library_path().exists():
        gstpeaq_amd.build_library()
    L = gstpeaq_amd.load_library()
    L.peaq_last_error.restype = C.c_char_p
    return L


def batch_fb_bands(lib, channels=2, n_pairs=2, pair_stride=48000, n_ref=None, n_test=None, n_uniform=48000, planes=4,
                   bands=0x1000, block_stride=250, ctx=None, ref=0x100000, test=0x200000):
    """peaq_batch_run_fb_bands with made-up device addresses: nothing may get as far as reading them"""
    u32p = C.POINTER(C.c_uint32)
    a = None if n_ref is None else np.ascontiguousarray(n_ref, dtype=np.uint32)
    b = None if n_test is None else np.ascontiguousarray(n_test, dtype=np.uint32)
    rc = lib.peaq_batch_run_fb_bands(ctx, channels, 92.0, n_pairs, C.c_void_p(ref), C.c_void_p(test), pair_stride,
                                     None if a is None else a.ctypes.data_as(u32p),
                                     None if b is None else b.ctypes.data_as(u32p), n_uniform, planes,
                                     C.c_void_p(bands) if bands else None, block_stride, C.c_void_p(0x3000), None)
    return rc, lib.peaq_last_error().decode()


def test_count_and_tables_are_the_oracle_s(lib):
    assert lib.peaq_fb_band_count() == 40
    dp = C.POINTER(C.c_double)
    fc, noise = np.full(41, -7.), np.full(41, -7.)
    assert lib.peaq_fb_band_tables(fc.ctypes.data_as(dp), noise.ctypes.data_as(dp)) == 0
    assert fc[40] == -7. and noise[40] == -7.           # exactly 40 entries are written
    exp = orc.tables(40)
    np.testing.assert_allclose(fc[:40], exp["fc"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(noise[:40], exp["internal_noise"], rtol=1e-12, atol=0)
    only = np.zeros(40)                                  # either pointer may be NULL, not both
    assert lib.peaq_fb_band_tables(None, only.ctypes.data_as(dp)) == 0 and np.array_equal(only, noise[:40])
    only[:] = 0.
    assert lib.peaq_fb_band_tables(only.ctypes.data_as(dp), None) == 0 and np.array_equal(only, fc[:40])
    assert lib.peaq_fb_band_tables(None, None) == -1
    import gstpeaq_amd
    pfc, pn = gstpeaq_amd.fb_band_tables()
    assert np.array_equal(pfc, fc[:40]) and np.array_equal(pn, noise[:40])


def test_planes_are_checked_first_and_by_value(lib):
    rc, msg = batch_fb_bands(lib, planes=0)
    assert rc == -1 and "peaq_batch_run_fb_bands: planes is 0" in msg
    for planes in (0x2000, 0x2001, 1 << 31, 0x1FFF | 0x4000):
        rc, msg = batch_fb_bands(lib, planes=planes)
        assert rc == -1 and f"planes {planes} has a bit above 4096" in msg, msg
    for planes in (1, 4, 0x1000, 0x1FFF):               # every plane there is gets past this check
        rc, msg = batch_fb_bands(lib, planes=planes)
        assert rc == -1 and "ctx is NULL" in msg, msg


def test_the_row_array_is_checked_without_a_context(lib):
    rc, msg = batch_fb_bands(lib, bands=0)
    assert rc == -1 and "d_bands is NULL" in msg
    for addr in (0x1008, 0x1004, 0x100f):
        rc, msg = batch_fb_bands(lib, bands=addr)
        assert rc == -1 and "d_bands is not 16-byte aligned" in msg


def test_a_block_stride_below_the_longest_pair_s_count_is_refused_by_name(lib):
    assert lib.peaq_frame_count(48000, 48000, 1) == 250
    rc, msg = batch_fb_bands(lib, block_stride=249)
    assert rc == -1 and "block_stride 249 is below the longest pair's 250 blocks" in msg
    rc, msg = batch_fb_bands(lib, channels=1, block_stride=0)
    assert rc == -1 and "block_stride 0 is below the longest pair's 250 blocks" in msg
    # ragged: the longest pair counts, whichever side is the longer one (the flush block takes what is left of either)
    assert lib.peaq_frame_count(192, 1000, 1) == 2
    rc, msg = batch_fb_bands(lib, n_ref=[100, 192], n_test=[150, 1000], block_stride=1)
    assert rc == -1 and "block_stride 1 is below the longest pair's 2 blocks" in msg
    rc, msg = batch_fb_bands(lib, n_ref=[100, 192], n_test=[150, 1000], block_stride=2)
    assert rc == -1 and "ctx is NULL" in msg


def test_what_peaq_batch_run_refuses_is_refused_here_too(lib):
    """with planes, rows and stride in order the call reaches the common driver's checks, still without a device"""
    rc, msg = batch_fb_bands(lib)
    assert rc == -1 and "peaq_batch_run_fb_bands: ctx is NULL" in msg
    ctx = C.c_void_p(0x5000)                            # never dereferenced: the checks below come first
    rc, msg = batch_fb_bands(lib, ctx=ctx, channels=3)
    assert rc == -1 and "peaq_batch_run_fb_bands: channels must be 1 or 2" in msg
    rc, msg = batch_fb_bands(lib, ctx=ctx, n_pairs=-1)
    assert rc == -1 and "n_pairs < 0" in msg
    rc, msg = batch_fb_bands(lib, ctx=ctx, ref=0)
    assert rc == -1 and "NULL buffer" in msg
    rc, msg = batch_fb_bands(lib, ctx=ctx, test=0)
    assert rc == -1 and "NULL buffer" in msg
    rc, msg = batch_fb_bands(lib, ctx=ctx, n_ref=[10, 10])
    assert rc == -1 and "both n_ref and n_test or neither" in msg
    rc, _ = batch_fb_bands(lib, ctx=ctx, n_pairs=0)
    assert rc == 0                                      # no pairs: nothing to do, as peaq_batch_run


def test_host_pair_entry_checks_its_arguments(lib):
    fp = C.POINTER(C.c_float)
    x = np.zeros(4096, dtype=np.float32)
    px = x.ctypes.data_as(fp)
    buf = C.c_void_p(0x1000)

    def call(channels=1, level=92.0, rate=48000, max_lag=0, planes=4, bands=buf, ctx=None):
        rc = lib.peaq_run_pair_fb_bands(ctx, channels, level, rate, max_lag, px, 4096, px, 4096, planes, bands, 8,
                                        None, None, None)
        return rc, lib.peaq_last_error().decode()

    rc, msg = call(planes=0)
    assert rc == -1 and "peaq_run_pair_fb_bands: planes is 0" in msg
    rc, msg = call(planes=0x2000)
    assert rc == -1 and "planes 8192 has a bit above 4096" in msg
    rc, msg = call(bands=None)
    assert rc == -1 and "bands is NULL" in msg
    rc, msg = call(max_lag=20000)
    assert rc == -1 and "20000" in msg
    rc, msg = call(rate=7000)
    assert rc == -1 and "7000" in msg
    rc, msg = call(channels=5)
    assert rc == -1 and "channels must be 1 or 2" in msg
    rc, msg = call()
    assert rc == -1 and "ctx is NULL" in msg


def test_python_binding_exports_the_fb_band_trace(lib):
    import gstpeaq_amd
    assert callable(gstpeaq_amd.batch_fb_bands) and callable(gstpeaq_amd.run_pair_fb_bands)
    assert callable(gstpeaq_amd.fb_band_tables)
    assert gstpeaq_amd.FB_BAND_PLANES == {n: 1 << k for k, n in enumerate(NAMES)}
    assert list(gstpeaq_amd.FB_BAND_PLANES) == NAMES    # the order of the slots
    assert gstpeaq_amd.fb_band_planes_mask(("mod_test", "moddiff")) == 0x1001
    assert gstpeaq_amd.fb_band_planes_mask("noiseloud") == 4 and gstpeaq_amd.fb_band_planes_mask(5) == 5
    with pytest.raises(gstpeaq_amd.PeaqError, match="unknown filter-bank band plane 'nmr'"):
        gstpeaq_amd.fb_band_planes_mask(("noiseloud", "nmr"))


def cli(*args):
    if not gst_env.CLI.exists():
        subprocess.run(["make", "-C", str(gst_env.CLI.parent)], check=True, capture_output=True)
    return subprocess.run([str(gst_env.CLI), *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("flag", ["--fb-bands", "--fb-bands=", "--fb-bands=:noiseloud"])
def test_cli_fb_bands_without_a_file_name_is_a_usage_error(flag):
    out = cli("--advanced", flag, "ref.wav", "test.wav")
    assert out.returncode == 1 and "--fb-bands needs a file name" in out.stderr, (out.returncode, out.stderr)


def test_cli_fb_bands_usage_errors_and_help():
    out = cli("--fb-bands=x.csv", "ref.wav", "test.wav")
    assert out.returncode == 1 and "--fb-bands needs --advanced" in out.stderr
    out = cli("--advanced", "--fb-bands=x.csv", "--interval=1", "ref.wav", "test.wav")
    assert out.returncode == 1 and "--fb-bands belongs to the plain one-call mode" in out.stderr
    out = cli("--advanced", "--fb-bands=x.csv", "--list=pairs.txt")
    assert out.returncode == 1 and "--fb-bands belongs to the plain one-call mode" in out.stderr
    out = cli("--advanced", "--fb-bands=x.csv", "--trace=y.csv", "ref.wav", "test.wav")
    assert out.returncode == 1 and "--fb-bands is a run of its own" in out.stderr
    out = cli("--advanced", "--fb-bands=x.csv", "--bands=y.csv", "ref.wav", "test.wav")
    assert out.returncode == 1 and "--fb-bands is a run of its own" in out.stderr
    out = cli("--advanced", "--fb-bands=x.csv:", "ref.wav", "test.wav")
    assert out.returncode == 1 and "no plane after the colon" in out.stderr
    out = cli("--help")
    assert out.returncode == 0 and "--fb-bands=FILE[:PLANES]" in out.stdout

"""CPU-side checks of the band-trace entry points (peaq_band_count, peaq_band_row, peaq_band_tables,
peaq_batch_run_bands, peaq_run_pair_bands, `peaq --bands`; include/peaq_amd.h): the tables are the oracle's, and every
argument the header says is refused is refused with PEAQ_ERR_ARG before a context or a device is touched -- the calls
below pass no context at all, or one that is never dereferenced -- with a message that names the value."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import gst_env
import oracle_lib as orc


@pytest.fixture(scope="module")
def lib():
    import gstpeaq_amd
    if not gstpeaq_amd.library_path().exists():
        gstpeaq_amd.build_library()
    L = gstpeaq_amd.load_library()
    L.peaq_last_error.restype = C.c_char_p
    return L


def batch_bands(lib, advanced=0, channels=2, n_pairs=2, pair_stride=48000, n_ref=None, n_test=None, n_uniform=48000,
                planes=1, bands=0x1000, frame_stride=46, ctx=None, ref=0x100000, test=0x200000):
    """peaq_batch_run_bands with made-up device addresses: nothing may get as far as reading them"""
    u32p = C.POINTER(C.c_uint32)
    a = None if n_ref is None else np.ascontiguousarray(n_ref, dtype=np.uint32)
    b = None if n_test is None else np.ascontiguousarray(n_test, dtype=np.uint32)
    rc = lib.peaq_batch_run_bands(ctx, advanced, channels, 92.0, n_pairs, C.c_void_p(ref), C.c_void_p(test), pair_stride,
                                  None if a is None else a.ctypes.data_as(u32p),
                                  None if b is None else b.ctypes.data_as(u32p), n_uniform, planes,
                                  C.c_void_p(bands) if bands else None, frame_stride, C.c_void_p(0x3000), None)
    return rc, lib.peaq_last_error().decode()


@pytest.mark.parametrize("advanced,bands", [(0, 109), (1, 55)])
def test_counts_rows_and_tables_are_the_oracle_s(lib, advanced, bands):
    assert lib.peaq_band_count(advanced) == bands
    assert lib.peaq_band_row(advanced) == bands + 1 and lib.peaq_band_row(advanced) % 2 == 0
    dp = C.POINTER(C.c_double)
    fc, md = np.full(bands + 1, -7.), np.full(bands + 1, -7.)
    assert lib.peaq_band_tables(advanced, fc.ctypes.data_as(dp), md.ctypes.data_as(dp)) == 0
    assert fc[bands] == -7. and md[bands] == -7.        # [count] entries are written, no pad
    exp = orc.tables(bands)
    np.testing.assert_allclose(fc[:bands], exp["fc"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(md[:bands], exp["mask_diff"], rtol=1e-12, atol=0)
    only = np.zeros(bands)                               # either pointer may be NULL, not both
    assert lib.peaq_band_tables(advanced, None, only.ctypes.data_as(dp)) == 0 and np.array_equal(only, md[:bands])
    assert lib.peaq_band_tables(advanced, None, None) == -1
    import gstpeaq_amd
    pfc, pmd = gstpeaq_amd.band_tables(advanced)
    assert np.array_equal(pfc, fc[:bands]) and np.array_equal(pmd, md[:bands])


def test_planes_are_checked_first_and_by_value(lib):
    rc, msg = batch_bands(lib, planes=0)
    assert rc == -1 and "peaq_batch_run_bands: planes is 0" in msg
    for planes in (32, 33, 1 << 31, 31 | 64):
        rc, msg = batch_bands(lib, planes=planes)
        assert rc == -1 and f"planes {planes} has a bit above 16" in msg, msg
    for planes, extra in ((4, 4), (8, 8), (16, 16), (31, 28), (1 | 8, 8), (2 | 4, 4)):
        rc, msg = batch_bands(lib, advanced=1, planes=planes)
        assert rc == -1 and f"planes {planes} asks for a plane the advanced version does not have ({extra}" in msg, msg
    for planes in (1, 2, 3):                            # the planes the 55-band path has get past this check
        rc, msg = batch_bands(lib, advanced=1, planes=planes)
        assert rc == -1 and "ctx is NULL" in msg, msg


def test_the_row_array_is_checked_without_a_context(lib):
    rc, msg = batch_bands(lib, bands=0)
    assert rc == -1 and "d_bands is NULL" in msg
    for addr in (0x1008, 0x1004, 0x100f):
        rc, msg = batch_bands(lib, bands=addr)
        assert rc == -1 and "d_bands is not 16-byte aligned" in msg


def test_a_frame_stride_below_the_longest_pair_s_count_is_refused_by_name(lib):
    assert lib.peaq_frame_count(48000, 48000, 0) == 46
    rc, msg = batch_bands(lib, frame_stride=45)
    assert rc == -1 and "frame_stride 45 is below the longest pair's 46 frames" in msg
    rc, msg = batch_bands(lib, advanced=1, planes=3, frame_stride=0)
    assert rc == -1 and "frame_stride 0 is below the longest pair's 46 frames" in msg
    # ragged: the longest pair counts, whichever side is the longer one (the flush frame takes what is left of either)
    assert lib.peaq_frame_count(2048, 9000, 0) == 2
    rc, msg = batch_bands(lib, n_ref=[3000, 2048], n_test=[2048, 9000], frame_stride=1)
    assert rc == -1 and "frame_stride 1 is below the longest pair's 2 frames" in msg
    rc, msg = batch_bands(lib, n_ref=[3000, 2048], n_test=[2048, 9000], frame_stride=2)
    assert rc == -1 and "ctx is NULL" in msg


def test_what_peaq_batch_run_refuses_is_refused_here_too(lib):
    """with planes, rows and stride in order the call reaches the common driver's checks, still without a device"""
    rc, msg = batch_bands(lib)
    assert rc == -1 and "peaq_batch_run_bands: ctx is NULL" in msg
    ctx = C.c_void_p(0x5000)                            # never dereferenced: the checks below come first
    rc, msg = batch_bands(lib, ctx=ctx, channels=3)
    assert rc == -1 and "peaq_batch_run_bands: channels must be 1 or 2" in msg
    rc, msg = batch_bands(lib, ctx=ctx, n_pairs=-1)
    assert rc == -1 and "n_pairs < 0" in msg
    rc, msg = batch_bands(lib, ctx=ctx, ref=0)
    assert rc == -1 and "NULL buffer" in msg
    rc, msg = batch_bands(lib, ctx=ctx, test=0)
    assert rc == -1 and "NULL buffer" in msg
    rc, msg = batch_bands(lib, ctx=ctx, n_ref=[10, 10])
    assert rc == -1 and "both n_ref and n_test or neither" in msg
    rc, _ = batch_bands(lib, ctx=ctx, n_pairs=0)
    assert rc == 0                                      # no pairs: nothing to do, as peaq_batch_run


def test_host_pair_entry_checks_its_arguments(lib):
    fp = C.POINTER(C.c_float)
    x = np.zeros(4096, dtype=np.float32)
    px = x.ctypes.data_as(fp)
    buf = C.c_void_p(0x1000)

    def call(advanced=0, channels=1, level=92.0, rate=48000, max_lag=0, planes=1, bands=buf, ctx=None):
        rc = lib.peaq_run_pair_bands(ctx, advanced, channels, level, rate, max_lag, px, 4096, px, 4096, planes, bands, 8,
                                     None, None, None)
        return rc, lib.peaq_last_error().decode()

    rc, msg = call(planes=0)
    assert rc == -1 and "peaq_run_pair_bands: planes is 0" in msg
    rc, msg = call(planes=64)
    assert rc == -1 and "planes 64 has a bit above 16" in msg
    rc, msg = call(advanced=1, planes=16)
    assert rc == -1 and "planes 16 asks for a plane the advanced version does not have" in msg
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


def test_python_binding_exports_the_band_trace(lib):
    import gstpeaq_amd
    assert callable(gstpeaq_amd.batch_bands) and callable(gstpeaq_amd.run_pair_bands)
    assert gstpeaq_amd.BAND_PLANES == dict(nmr=1, exc_ref=2, exc_test=4, detect=8, steps=16)
    assert list(gstpeaq_amd.BAND_PLANES) == ["nmr", "exc_ref", "exc_test", "detect", "steps"]   # the order of the slots
    assert gstpeaq_amd.band_planes_mask(("steps", "nmr")) == 17 and gstpeaq_amd.band_planes_mask("detect") == 8
    assert gstpeaq_amd.band_planes_mask(5) == 5
    with pytest.raises(gstpeaq_amd.PeaqError, match="unknown band plane 'loudness'"):
        gstpeaq_amd.band_planes_mask(("nmr", "loudness"))


def cli(*args):
    if not gst_env.CLI.exists():
        subprocess.run(["make", "-C", str(gst_env.CLI.parent)], check=True, capture_output=True)
    return subprocess.run([str(gst_env.CLI), *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("flag", ["--bands", "--bands=", "--bands=:nmr"])
def test_cli_bands_without_a_file_name_is_a_usage_error(flag):
    out = cli(flag, "ref.wav", "test.wav")
    assert out.returncode == 1 and "--bands needs a file name" in out.stderr, (out.returncode, out.stderr)


def test_cli_bands_usage_errors_and_help():
    out = cli("--bands=x.csv", "--interval=1", "ref.wav", "test.wav")
    assert out.returncode == 1 and "--bands belongs to the plain one-call mode" in out.stderr
    out = cli("--bands=x.csv", "--list=pairs.txt")
    assert out.returncode == 1 and "--bands belongs to the plain one-call mode" in out.stderr
    out = cli("--bands=x.csv", "--trace=y.csv", "ref.wav", "test.wav")
    assert out.returncode == 1 and "--bands is a run of its own" in out.stderr
    out = cli("--bands=x.csv:", "ref.wav", "test.wav")
    assert out.returncode == 1 and "no plane after the colon" in out.stderr
    out = cli("--bands=x.csv:nmr,detect", "--advanced", "ref.wav", "test.wav")
    assert out.returncode == 1 and "the advanced version has the planes nmr and exc_ref only" in out.stderr
    out = cli("--help")
    assert out.returncode == 0 and "--bands=FILE[:PLANES]" in out.stdout

"""CPU-side checks of the pattern-band entry points (peaq_pattern_band_tables, peaq_batch_run_pattern_bands,
peaq_run_pair_pattern_bands, `peaq --pattern-bands`; include/peaq_amd.h): the tables are the oracle's, and every argument
the header says is refused is refused with PEAQ_ERR_ARG before a context or a device is touched -- the calls below pass
no context at all, or one that is never dereferenced -- with a message that names the value.

Also here, because it needs no GPU: recipe(), the thirteen planes in numpy from the unsmeared excitations with the
oracle's level adapter and modulation processor and the header's formulas, and its own check against the oracle's frame
values on the six pairs of tests/test_gpu_bands.py (three pairs, mono and stereo).  tests/test_gpu_pattern_bands.py
feeds the same recipe with the device's planes."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import gst_env
import oracle_lib as orc
from test_gpu_bands import pairs_of

NB = 109
NAMES = ["moddiff1", "moddiff2", "modwt", "noiseloud", "unsm_ref", "unsm_test", "exc_ref", "exc_test", "adapt_ref",
         "adapt_test", "mod_ref", "mod_test", "avgloud_ref"]   # in the order of the bits, which is the order of the slots
BITS = {n: 1 << k for k, n in enumerate(NAMES)}
ALL = 0x1FFF
TERMS = ["moddiff1", "moddiff2", "modwt", "noiseloud"]
INPUTS = ["unsm_ref", "unsm_test"]

_ORACLE = {}


def counts_of(channels):
    return [orc.count_frames(len(r), len(t)) for r, t in pairs_of(channels)]


def oracle_inputs(channels, p):
    """the unsmeared excitations of pair p from the oracle's 109-band front-end records (offsets 0 and 112): dict name ->
    [frames, channels, 109]; computed once, shared, never changed"""
    if (channels, p) not in _ORACLE:
        ref, test = pairs_of(channels)[p]
        rec = orc.frontend_records(NB, ref, test, orc.count_frames(len(ref), len(test)))
        _ORACLE[channels, p] = dict(unsm_ref=rec[:, :, 0:NB], unsm_test=rec[:, :, 112:112 + NB])
    return _ORACLE[channels, p]


def recipe(inp):
    """the eleven planes the back end makes of the two unsmeared excitations (dict name -> [frames, channels, 109]):
    time smearing as tests/test_gpu_bands.py::expected, the oracle's level adapter and modulation processor, the
    header's formulas in numpy; also `margin`, m = (A - B) / max (|A|, |B|) with A = stest at and B = sref ar, the two
    sides of NOISELOUD's hinge"""
    tab = orc.tables(NB)
    n, a = tab["internal_noise"], tab["ear_tc"]
    ur, ut = inp["unsm_ref"], inp["unsm_test"]
    nf, channels, _ = ur.shape
    sm = np.zeros((2, channels, NB))
    e = np.zeros((2, nf, channels, NB))
    for f in range(nf):                              # fftearmodel.c:496-504
        for i, u in enumerate((ur[f], ut[f])):
            sm[i] = a * sm[i] + (1 - a) * u
            e[i, f] = np.maximum(sm[i], u)
    out = dict(exc_ref=e[0], exc_test=e[1])
    for k in TERMS + ["adapt_ref", "adapt_test", "mod_ref", "mod_test", "avgloud_ref", "margin"]:
        out[k] = np.zeros_like(ur)
    for c in range(channels):
        ar, at = orc.leveladapt(NB, e[0][:, c], e[1][:, c])
        mr, lr = orc.modproc(NB, ur[:, c])
        mt, _ = orc.modproc(NB, ut[:, c])
        out["adapt_ref"][:, c], out["adapt_test"][:, c], out["mod_ref"][:, c], out["mod_test"][:, c] = ar, at, mr, mt
        out["avgloud_ref"][:, c] = lr
        diff = np.abs(mr - mt)                                                 # movs.c:224-251
        out["moddiff1"][:, c] = diff / (1. + mr)
        out["moddiff2"][:, c] = np.where(mt >= mr, 1., 0.1) * diff / (0.01 + mr)
        out["modwt"][:, c] = lr / (lr + 100. * np.power(n, 0.3))
        sref, stest = 0.15 * mr + 0.5, 0.15 * mt + 0.5                        # movs.c:709-743 as gstpeaq.c:880-886 calls it
        beta = np.exp(-1.5 * (at - ar) / ar)
        out["noiseloud"][:, c] = np.power(n / stest, 0.23) * (
            np.power(1. + np.maximum(stest * at - sref * ar, 0.) / (n + sref * ar * beta), 0.23) - 1.)
        big, small = stest * at, sref * ar
        out["margin"][:, c] = (big - small) / np.maximum(np.abs(big), np.abs(small))
    return out


def frame_values(planes):
    """the frame record's four values per channel from the four term planes -> [frames, channels, 4]"""
    return np.stack([100. / NB * planes["moddiff1"].sum(axis=-1), 100. / NB * planes["moddiff2"].sum(axis=-1),
                     planes["modwt"].sum(axis=-1), 24. / NB * planes["noiseloud"].sum(axis=-1)], axis=-1)


# ---- the recipe itself, on the CPU oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
def test_the_recipe_reproduces_the_oracle_s_frame_values_and_lies_on_both_sides_of_the_hinge(channels):
    """recipe() on the oracle's own records gives the oracle's four frame values on every frame, frames below 24 and the
    flush frame included (8e-14 relative measured; held to 1e-12).  What the GPU tests lean on: in every pair and
    channel both sides of NOISELOUD's hinge occur beyond 1e-9, 20 to 51 % of the values lie below it, and the recipe is
    exactly 0 there; hinge-adjacent values exist (the smallest |m| is about 3e-6, above 1e-9)"""
    for p, nf in enumerate(counts_of(channels)):
        ref, test = pairs_of(channels)[p]
        want = orc.mov_trace(ref, test, nf)
        out = recipe(oracle_inputs(channels, p))
        got = frame_values(out)
        assert nf in (30, 31) and got.shape == (nf, channels, 4)
        for k, name in enumerate(("moddiff1", "moddiff2", "tempwt", "noiseloud")):
            rel = float(np.max(np.abs(got[:, :, k] - want[name]) / np.abs(want[name])))
            print(f"pattern-bands-recipe channels={channels} pair={p} {name}: max rel dev {rel:.3e}")
            np.testing.assert_allclose(got[:, :, k], want[name], rtol=1e-12, atol=0, err_msg=f"pair {p} {name}")
        for c in range(channels):
            m = out["margin"][:, c]
            below, above = m < -1e-9, m > 1e-9
            share = np.count_nonzero(below) / m.size
            print(f"pattern-bands-recipe channels={channels} pair={p} channel={c}: {100 * share:.1f} % below the hinge, "
                  f"smallest |m| {float(np.min(np.abs(m))):.3e}")
            assert below.any() and above.any(), (p, c)
            assert 0.195 <= share <= 0.515, (p, c, share)
            assert (out["noiseloud"][:, c][below] == 0.).all(), (p, c)
            assert 1e-9 < np.min(np.abs(m)) < 1e-3, (p, c, float(np.min(np.abs(m))))   # (2.8e-6 .. 9.7e-5 measured)


# ---- the entry points ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import gstpeaq_amd
    if not gstpeaq_amd.library_path().exists():
        gstpeaq_amd.build_library()
    L = gstpeaq_amd.load_library()
    L.peaq_last_error.restype = C.c_char_p
    return L


def batch_pattern_bands(lib, channels=2, n_pairs=2, pair_stride=48000, n_ref=None, n_test=None, n_uniform=48000,
                        planes=8, bands=0x1000, frame_stride=46, ctx=None, ref=0x100000, test=0x200000):
    """peaq_batch_run_pattern_bands with made-up device addresses: nothing may get as far as reading them"""
    u32p = C.POINTER(C.c_uint32)
    a = None if n_ref is None else np.ascontiguousarray(n_ref, dtype=np.uint32)
    b = None if n_test is None else np.ascontiguousarray(n_test, dtype=np.uint32)
    rc = lib.peaq_batch_run_pattern_bands(ctx, channels, 92.0, n_pairs, C.c_void_p(ref), C.c_void_p(test), pair_stride,
                                          None if a is None else a.ctypes.data_as(u32p),
                                          None if b is None else b.ctypes.data_as(u32p), n_uniform, planes,
                                          C.c_void_p(bands) if bands else None, frame_stride, C.c_void_p(0x3000), None)
    return rc, lib.peaq_last_error().decode()


def test_tables_are_the_oracle_s(lib):
    dp = C.POINTER(C.c_double)
    fc, noise = np.full(NB + 1, -7.), np.full(NB + 1, -7.)
    assert lib.peaq_pattern_band_tables(fc.ctypes.data_as(dp), noise.ctypes.data_as(dp)) == 0
    assert fc[NB] == -7. and noise[NB] == -7.            # [109] entries are written, no pad
    exp = orc.tables(NB)
    np.testing.assert_allclose(fc[:NB], exp["fc"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(noise[:NB], exp["internal_noise"], rtol=1e-12, atol=0)
    only = np.zeros(NB)                                  # either pointer may be NULL, not both
    assert lib.peaq_pattern_band_tables(None, only.ctypes.data_as(dp)) == 0 and np.array_equal(only, noise[:NB])
    assert lib.peaq_pattern_band_tables(only.ctypes.data_as(dp), None) == 0 and np.array_equal(only, fc[:NB])
    assert lib.peaq_pattern_band_tables(None, None) == -1
    assert "peaq_pattern_band_tables: NULL argument" in lib.peaq_last_error().decode()
    import gstpeaq_amd
    pfc, pn = gstpeaq_amd.pattern_band_tables()
    assert np.array_equal(pfc, fc[:NB]) and np.array_equal(pn, noise[:NB])


def test_planes_are_checked_first_and_by_value(lib):
    rc, msg = batch_pattern_bands(lib, planes=0)
    assert rc == -1 and "peaq_batch_run_pattern_bands: planes is 0" in msg
    for planes in (0x2000, 0x2001, 1 << 31, ALL | 0x4000):
        rc, msg = batch_pattern_bands(lib, planes=planes)
        assert rc == -1 and f"planes {planes} has a bit above 4096" in msg, msg
    for planes in (1, 8, 0x1000, ALL):                   # every plane there is gets past this check
        rc, msg = batch_pattern_bands(lib, planes=planes)
        assert rc == -1 and "ctx is NULL" in msg, msg


def test_the_row_array_is_checked_without_a_context(lib):
    rc, msg = batch_pattern_bands(lib, bands=0)
    assert rc == -1 and "d_bands is NULL" in msg
    for addr in (0x1008, 0x1004, 0x100f):
        rc, msg = batch_pattern_bands(lib, bands=addr)
        assert rc == -1 and "d_bands is not 16-byte aligned" in msg


def test_a_frame_stride_below_the_longest_pair_s_count_is_refused_by_name(lib):
    assert lib.peaq_frame_count(48000, 48000, 0) == 46
    rc, msg = batch_pattern_bands(lib, frame_stride=45)
    assert rc == -1 and "frame_stride 45 is below the longest pair's 46 frames" in msg
    rc, msg = batch_pattern_bands(lib, planes=ALL, frame_stride=0)
    assert rc == -1 and "frame_stride 0 is below the longest pair's 46 frames" in msg
    # ragged: the longest pair counts, whichever side is the longer one (the flush frame takes what is left of either)
    assert lib.peaq_frame_count(2048, 9000, 0) == 2
    rc, msg = batch_pattern_bands(lib, n_ref=[3000, 2048], n_test=[2048, 9000], frame_stride=1)
    assert rc == -1 and "frame_stride 1 is below the longest pair's 2 frames" in msg
    rc, msg = batch_pattern_bands(lib, n_ref=[3000, 2048], n_test=[2048, 9000], frame_stride=2)
    assert rc == -1 and "ctx is NULL" in msg


def test_what_peaq_batch_run_refuses_is_refused_here_too(lib):
    """with planes, rows and stride in order the call reaches the common driver's checks, still without a device"""
    rc, msg = batch_pattern_bands(lib)
    assert rc == -1 and "peaq_batch_run_pattern_bands: ctx is NULL" in msg
    ctx = C.c_void_p(0x5000)                            # never dereferenced: the checks below come first
    rc, msg = batch_pattern_bands(lib, ctx=ctx, channels=3)
    assert rc == -1 and "peaq_batch_run_pattern_bands: channels must be 1 or 2" in msg
    rc, msg = batch_pattern_bands(lib, ctx=ctx, n_pairs=-1)
    assert rc == -1 and "n_pairs < 0" in msg
    rc, msg = batch_pattern_bands(lib, ctx=ctx, ref=0)
    assert rc == -1 and "NULL buffer" in msg
    rc, msg = batch_pattern_bands(lib, ctx=ctx, test=0)
    assert rc == -1 and "NULL buffer" in msg
    rc, msg = batch_pattern_bands(lib, ctx=ctx, n_ref=[10, 10])
    assert rc == -1 and "both n_ref and n_test or neither" in msg
    rc, _ = batch_pattern_bands(lib, ctx=ctx, n_pairs=0)
    assert rc == 0                                      # no pairs: nothing to do, as peaq_batch_run


def test_host_pair_entry_checks_its_arguments(lib):
    fp = C.POINTER(C.c_float)
    x = np.zeros(4096, dtype=np.float32)
    px = x.ctypes.data_as(fp)
    buf = C.c_void_p(0x1000)

    def call(channels=1, level=92.0, rate=48000, max_lag=0, planes=8, bands=buf, ctx=None):
        rc = lib.peaq_run_pair_pattern_bands(ctx, channels, level, rate, max_lag, px, 4096, px, 4096, planes, bands, 8,
                                             None, None, None)
        return rc, lib.peaq_last_error().decode()

    rc, msg = call(planes=0)
    assert rc == -1 and "peaq_run_pair_pattern_bands: planes is 0" in msg
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


def test_python_binding_exports_the_pattern_band_trace(lib):
    import gstpeaq_amd
    assert callable(gstpeaq_amd.batch_pattern_bands) and callable(gstpeaq_amd.run_pair_pattern_bands)
    assert gstpeaq_amd.PATTERN_BAND_PLANES == BITS
    assert list(gstpeaq_amd.PATTERN_BAND_PLANES) == NAMES   # the order of the slots
    assert gstpeaq_amd.pattern_band_planes_mask(("avgloud_ref", "moddiff1")) == 0x1001
    assert gstpeaq_amd.pattern_band_planes_mask("noiseloud") == 8 and gstpeaq_amd.pattern_band_planes_mask(5) == 5
    with pytest.raises(gstpeaq_amd.PeaqError, match="unknown pattern band plane 'nmr'"):
        gstpeaq_amd.pattern_band_planes_mask(("noiseloud", "nmr"))


def cli(*args):
    if not gst_env.CLI.exists():
        subprocess.run(["make", "-C", str(gst_env.CLI.parent)], check=True, capture_output=True)
    return subprocess.run([str(gst_env.CLI), *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("flag", ["--pattern-bands", "--pattern-bands=", "--pattern-bands=:noiseloud"])
def test_cli_pattern_bands_without_a_file_name_is_a_usage_error(flag):
    out = cli(flag, "ref.wav", "test.wav")
    assert out.returncode == 1 and "--pattern-bands needs a file name" in out.stderr, (out.returncode, out.stderr)


def test_cli_pattern_bands_usage_errors_and_help():
    out = cli("--pattern-bands=x.csv", "--advanced", "ref.wav", "test.wav")
    assert out.returncode == 1 and "--pattern-bands covers the basic version only" in out.stderr
    assert "--fb-bands" in out.stderr
    out = cli("--pattern-bands=x.csv", "--interval=1", "ref.wav", "test.wav")
    assert out.returncode == 1 and "--pattern-bands belongs to the plain one-call mode" in out.stderr
    out = cli("--pattern-bands=x.csv", "--list=pairs.txt")
    assert out.returncode == 1 and "--pattern-bands belongs to the plain one-call mode" in out.stderr
    for other in ("--trace=y.csv", "--bands=y.csv", "--match-gain"):
        out = cli("--pattern-bands=x.csv", other, "ref.wav", "test.wav")
        assert out.returncode == 1 and "--pattern-bands is a run of its own" in out.stderr, (other, out.stderr)
    out = cli("--pattern-bands=x.csv:", "ref.wav", "test.wav")
    assert out.returncode == 1 and "no plane after the colon" in out.stderr
    out = cli("--help")
    assert out.returncode == 0 and "--pattern-bands=FILE[:PLANES]" in out.stdout and "avgloud_ref" in out.stdout

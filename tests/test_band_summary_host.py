"""CPU-side checks of the band summary (peaq_band_summary_rows, peaq_batch_run_band_summary, peaq_run_pair_band_summary,
`peaq --band-summary`; include/peaq_amd.h): the names are exported, every argument the header says is refused is refused
with PEAQ_ERR_ARG before a context or a device is touched -- the calls below pass no context at all, or one that is never
dereferenced -- with a message that names the value.

Also here, because it needs no GPU: summarise(), the header's table of rows in numpy with strict left-to-right sums, and
its own check on the CPU oracle's values: fed with the oracle's per-band planes (tests/test_gpu_bands.py::expected,
tests/test_pattern_bands_host.py::recipe on the oracle's unsmeared excitations) and the flags restated in
tests/test_gpu_trace.py, its rows reproduce the oracle's TotalNMR, AvgModDiff1 and AvgModDiff2.  That holds the
definition of the COUNTED frames against the reference's accumulators before any GPU is involved.
tests/test_gpu_band_summary.py feeds the same function with the device's planes.

Inputs: the three pairs of tests/test_gpu_bands.py (31 / 31 / 30 frames), one "gapped" pair -- the same tone plus noise
under an envelope that is exactly zero at the start, over one interior stretch after frame 24 and at the end, 45 frames --
and one all-silent pair, mono and stereo.

Tolerances of the three MOVs: 1e-9 dB for TotalNMR, 1e-10 relative for the other two.  Every term is non-negative and a
sum has fewer than 1e4 additions, so reordering it changes it by less than 1e4 x 2^-53 = 1.2e-12 relative; 10 log10 turns
1.2e-12 relative into 5e-12 dB."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import gst_env
import oracle_lib as orc
from test_gpu_bands import expected, pairs_of
from test_gpu_trace import ABOVE, FLUSH, LOUD_OPEN, MOD_OPEN, expected_flags
from test_pattern_bands_host import oracle_inputs, recipe

NB = {0: 109, 1: 55}
ROWS = ["nmr_sum", "nmr_max", "nmr_disturbed", "exc_ref_sum", "exc_test_sum", "moddiff1_wsum", "moddiff2_wsum",
        "noiseloud_sum"]
DISTURBED = 1.41253754462275                         # RelDistFrames' 1.5 dB, movs.c:1019
N_GAPPED = 2048 + 43 * 1024 + 300                    # 44 full frames and a flush frame
# the envelope's zero stretches in samples: frames 0-2, 28-30 and 40-44 (the flush frame) lie wholly inside one
# (frame f is samples [1024 f, 1024 f + 2048))
GAPS = [(0, 4 * 1024), (28 * 1024, 32 * 1024), (40 * 1024, N_GAPPED)]
GAPPED, SILENT = 3, 4                                # their places behind the three pairs of tests/test_gpu_bands.py

_PAIRS, _PLANES = {}, {}


def all_pairs(channels):
    """[(ref, test)] x 5: the three pairs of tests/test_gpu_bands.py, the gapped pair, the all-silent pair"""
    if channels not in _PAIRS:
        rng = np.random.default_rng(23)
        t = np.arange(N_GAPPED)[:, None] / 48000.
        f = np.array([1000., 3150.])[:channels][None, :]
        env = np.ones((N_GAPPED, 1), dtype=bool)
        for a, b in GAPS:
            env[a:b] = False
        ref = (0.05 * np.sin(2 * np.pi * f * t) + 0.00025 * rng.standard_normal((N_GAPPED, channels))).astype(np.float32)
        test = (ref + np.float32(1e-3) * rng.standard_normal((N_GAPPED, channels)).astype(np.float32)).astype(np.float32)
        zero = np.float32(0.)
        gapped = (np.where(env, ref, zero), np.where(env, test, zero))
        silent = (np.zeros((N_GAPPED, channels), dtype=np.float32), np.zeros((N_GAPPED, channels), dtype=np.float32))
        _PAIRS[channels] = pairs_of(channels) + [gapped, silent]
    return _PAIRS[channels]


def counts_of(channels):
    return [orc.count_frames(len(r), len(t)) for r, t in all_pairs(channels)]


def flags_of(channels, p):
    """the frames' flags of pair p as tests/test_gpu_trace.py restates them on the CPU"""
    ref, test = all_pairs(channels)[p]
    fl, _ = expected_flags(ref, test, counts_of(channels)[p], False, f"channels {channels} pair {p}")
    return fl


def oracle_planes(channels, p):
    """the basic version's seven planes of pair p from the CPU oracle: dict name -> [frames, channels, 109]; computed
    once, shared, never changed.  The three pairs of tests/test_gpu_bands.py through expected() and recipe() on
    oracle_inputs(); the two pairs of this file the same way from their own front-end records"""
    if (channels, p) not in _PLANES:
        if p < 3:
            exp, pat = expected(109, channels, p), recipe(oracle_inputs(channels, p))
            nmr, er, et = exp["nmr"], exp["exc_ref"], exp["exc_test"]
        else:
            ref, test = all_pairs(channels)[p]
            rec, tab = orc.frontend_records(109, ref, test, counts_of(channels)[p]), orc.tables(109)
            pat = recipe(dict(unsm_ref=rec[:, :, 0:109], unsm_test=rec[:, :, 112:112 + 109]))
            er, et = pat["exc_ref"], pat["exc_test"]
            nmr = rec[:, :, 448:448 + 109] * tab["mask_diff"] / er              # movs.c:1002-1022
        _PLANES[channels, p] = dict(nmr=nmr, exc_ref=er, exc_test=et,
                                    **{k: pat[k] for k in ("moddiff1", "moddiff2", "modwt", "noiseloud")})
    return _PLANES[channels, p]


def seq_sum(x):
    """the sum over axis 0 as a running sum in index order (np.sum adds pairwise); zeros for no term"""
    return np.cumsum(x, axis=0)[-1] if len(x) else np.zeros(x.shape[1:])


def summarise(planes, flags, weight=None):
    """The table of include/peaq_amd.h.  planes: dict name -> [frames, channels, nb] with nmr and exc_ref (advanced
    version) and exc_test, moddiff1, moddiff2, modwt, noiseloud (basic version); flags: [frames], the frame trace's;
    weight: [frames, channels], the frames' W (default: the sum of modwt over the bands).  -> rows [channels, R, nb + 1],
    the denominators in the last entry"""
    flags = np.asarray(flags)
    nf, channels, nb = planes["nmr"].shape
    basic = "exc_test" in planes
    rows = np.zeros((channels, 8 if basic else 4, nb + 1))
    above = np.flatnonzero(flags & ABOVE)
    if not above.size:
        return rows
    counted = np.zeros(nf, dtype=bool)
    counted[above[0]:above[-1] + 1] = True
    n = int(np.count_nonzero(counted))
    r = planes["nmr"][counted]
    rows[:, 0, :nb] = seq_sum(r)
    rows[:, 1, :nb] = r.max(axis=0)
    rows[:, 2, :nb] = np.count_nonzero(r > DISTURBED, axis=0)
    rows[:, 3, :nb] = seq_sum(planes["exc_ref"][counted])
    rows[:, :4, nb] = n
    if basic:
        rows[:, 4, :nb] = seq_sum(planes["exc_test"][counted])
        rows[:, 4, nb] = n
        mod = counted & ((flags & MOD_OPEN) != 0)
        w = (planes["modwt"].sum(axis=-1) if weight is None else np.asarray(weight))[mod]
        for k, name in ((5, "moddiff1"), (6, "moddiff2")):
            rows[:, k, :nb] = seq_sum(w[:, :, None] * planes[name][mod])
            rows[:, k, nb] = seq_sum(w)
        loud = counted & ((flags & LOUD_OPEN) != 0)
        rows[:, 7, :nb] = seq_sum(planes["noiseloud"][loud])
        rows[:, 7, nb] = np.count_nonzero(loud)
    return rows


def movs_of(rows):
    """(TotalNMR, AvgModDiff1, AvgModDiff2) of the basic version from a pair's rows [channels, 8, 110], by the header's
    identities; NaN where nothing was counted, like the MOVs themselves"""
    nb = rows.shape[-1] - 1
    with np.errstate(divide="ignore", invalid="ignore"):
        nmr = np.mean(10. * np.log10(rows[:, 0, :nb].sum(axis=-1) / (nb * rows[:, 0, nb])))
        md1 = np.mean(100. / nb * rows[:, 5, :nb].sum(axis=-1) / rows[:, 5, nb])
        md2 = np.mean(100. / nb * rows[:, 6, :nb].sum(axis=-1) / rows[:, 6, nb])
    return nmr, md1, md2


# ---- the inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
def test_the_gapped_pair_has_every_kind_of_frame_and_the_silent_pair_none(channels):
    cnt = counts_of(channels)
    assert cnt == [31, 31, 30, 45, 45]
    fl = flags_of(channels, GAPPED)
    above = np.flatnonzero(fl & ABOVE)
    first, last = int(above[0]), int(above[-1])
    inside = np.arange(first, last + 1)
    assert first >= 2 and first == 3                                           # leading frames below the boundary
    interior = inside[(fl[inside] & ABOVE) == 0]
    assert interior.size >= 2 and interior.min() > 24 and list(interior) == [28, 29, 30]
    assert cnt[GAPPED] - 1 - last >= 2 and last == 39                          # trailing ones, the flush frame among them
    assert fl[-1] & FLUSH and not fl[-1] & ABOVE
    assert (fl[inside] & MOD_OPEN).any() and (fl[inside] & LOUD_OPEN).any()
    assert not (flags_of(channels, SILENT) & ABOVE).any()
    for p in range(3):                                                         # (every frame of the other three counts)
        assert (flags_of(channels, p) & ABOVE).all()


# ---- summarise() on the CPU oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
def test_summarise_reproduces_the_oracle_s_movs(channels):
    for p, (ref, test) in enumerate(all_pairs(channels)):
        rows = summarise(oracle_planes(channels, p), flags_of(channels, p))
        want = orc.run_pair(0, ref, test)["movs"]
        nmr, md1, md2 = movs_of(rows)
        if p == SILENT:
            assert not rows.any() and np.isnan([nmr, md1, md2]).all() and np.isnan([want[2], want[6], want[7]]).all()
            continue
        print(f"band-summary-host channels={channels} pair={p}: TotalNMR {nmr - want[2]:+.3e} dB, AvgModDiff1 "
              f"{md1 / want[6] - 1:+.3e}, AvgModDiff2 {md2 / want[7] - 1:+.3e}, counted {rows[0, 0, 109]:.0f}")
        assert abs(nmr - want[2]) <= 1e-9, (p, nmr, want[2])
        assert abs(md1 / want[6] - 1.) <= 1e-10, (p, md1, want[6])
        assert abs(md2 / want[7] - 1.) <= 1e-10, (p, md2, want[7])
    assert summarise(oracle_planes(channels, GAPPED), flags_of(channels, GAPPED))[0, 0, 109] == 37


def test_summarise_counts_the_frames_between_the_first_and_the_last_above_the_boundary():
    """on made-up planes: leading and trailing frames below the boundary do not count, those in between do; the gates
    pick among the counted frames; the threshold is strict"""
    nf, nb = 9, 3
    fl = np.array([0, ABOVE, 0, ABOVE | MOD_OPEN, MOD_OPEN, ABOVE | MOD_OPEN | LOUD_OPEN, MOD_OPEN | LOUD_OPEN, 0, FLUSH])
    v = (1. + np.arange(nf))[:, None, None] * np.ones((nf, 1, nb))
    planes = dict(nmr=v * np.array([1., DISTURBED / 4., 0.1]), exc_ref=v, exc_test=2 * v, moddiff1=v, moddiff2=3 * v,
                  modwt=np.ones((nf, 1, nb)), noiseloud=v)
    rows = summarise(planes, fl)
    assert (rows[0, :5, nb] == 5).all()                                        # frames 1 .. 5
    assert list(rows[0, 0, :nb] / np.array([1., DISTURBED / 4., 0.1])) == pytest.approx([20., 20., 20.])
    assert list(rows[0, 1, :nb]) == [6., 6. * DISTURBED / 4., 6. * 0.1]
    assert list(rows[0, 2, :nb]) == [5., 2., 0.]                               # 4 x DISTURBED / 4 is not above it; 5 x, 6 x are
    assert list(rows[0, 3, :nb]) == [20.] * 3 and list(rows[0, 4, :nb]) == [40.] * 3
    assert rows[0, 5, nb] == 9. and list(rows[0, 5, :nb]) == [3. * 15.] * 3    # frames 3, 4, 5; W = 3
    assert list(rows[0, 6, :nb]) == [9. * 15.] * 3
    assert rows[0, 7, nb] == 1. and list(rows[0, 7, :nb]) == [6.] * 3          # frame 5 alone: 6 lies behind the last
    assert not summarise(planes, fl & ~np.uint32(ABOVE)).any()
    assert summarise({k: planes[k] for k in ("nmr", "exc_ref")}, fl).shape == (1, 4, nb + 1)


# ---- the entry points ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import gstpeaq_amd
    if not gstpeaq_amd.library_path().exists():
        gstpeaq_amd.build_library()
    L = gstpeaq_amd.load_library()
    L.peaq_last_error.restype = C.c_char_p
    return L


def test_every_declared_name_is_exported(lib):
    for name in ("peaq_band_summary_rows", "peaq_batch_run_band_summary", "peaq_run_pair_band_summary"):
        assert hasattr(lib, name), name
    assert lib.peaq_band_summary_rows(0) == 8 and lib.peaq_band_summary_rows(1) == 4
    assert lib.peaq_band_summary_rows(7) == 4                                  # any non-zero value is the advanced version


def batch_band_summary(lib, advanced=0, channels=2, n_pairs=2, pair_stride=48000, n_ref=None, n_test=None,
                       n_uniform=48000, summary=0x1000, ctx=None, ref=0x100000, test=0x200000):
    """peaq_batch_run_band_summary with made-up device addresses: nothing may get as far as reading them"""
    u32p = C.POINTER(C.c_uint32)
    a = None if n_ref is None else np.ascontiguousarray(n_ref, dtype=np.uint32)
    b = None if n_test is None else np.ascontiguousarray(n_test, dtype=np.uint32)
    rc = lib.peaq_batch_run_band_summary(ctx, advanced, channels, 92.0, n_pairs, C.c_void_p(ref), C.c_void_p(test),
                                         pair_stride, None if a is None else a.ctypes.data_as(u32p),
                                         None if b is None else b.ctypes.data_as(u32p), n_uniform,
                                         C.c_void_p(summary) if summary else None, C.c_void_p(0x3000), None)
    return rc, lib.peaq_last_error().decode()


@pytest.mark.parametrize("advanced", [0, 1])
def test_the_summary_array_is_checked_first_and_by_value(lib, advanced):
    rc, msg = batch_band_summary(lib, advanced, summary=0)
    assert rc == -1 and "peaq_batch_run_band_summary: d_summary is NULL" in msg
    for addr in (0x1008, 0x1004, 0x100f):
        rc, msg = batch_band_summary(lib, advanced, summary=addr)
        assert rc == -1 and f"d_summary 0x{addr:x} is not 16-byte aligned" in msg, msg
    rc, msg = batch_band_summary(lib, advanced, summary=0x1010)
    assert rc == -1 and "ctx is NULL" in msg


@pytest.mark.parametrize("advanced", [0, 1])
def test_what_peaq_batch_run_refuses_is_refused_here_too(lib, advanced):
    rc, msg = batch_band_summary(lib, advanced)
    assert rc == -1 and "peaq_batch_run_band_summary: ctx is NULL" in msg
    ctx = C.c_void_p(0x5000)                            # never dereferenced: the checks below come first
    rc, msg = batch_band_summary(lib, advanced, ctx=ctx, channels=3)
    assert rc == -1 and "peaq_batch_run_band_summary: channels must be 1 or 2, not 3" in msg
    rc, msg = batch_band_summary(lib, advanced, ctx=ctx, n_pairs=-1)
    assert rc == -1 and "n_pairs < 0" in msg
    rc, msg = batch_band_summary(lib, advanced, ctx=ctx, ref=0)
    assert rc == -1 and "NULL buffer" in msg
    rc, msg = batch_band_summary(lib, advanced, ctx=ctx, test=0)
    assert rc == -1 and "NULL buffer" in msg
    rc, msg = batch_band_summary(lib, advanced, ctx=ctx, n_ref=[10, 10])
    assert rc == -1 and "both n_ref and n_test or neither" in msg
    rc, _ = batch_band_summary(lib, advanced, ctx=ctx, n_pairs=0)
    assert rc == 0                                      # no pairs: nothing to do, as peaq_batch_run


def test_host_pair_entry_checks_its_arguments(lib):
    fp = C.POINTER(C.c_float)
    x = np.zeros(4096, dtype=np.float32)
    px = x.ctypes.data_as(fp)
    buf = C.c_void_p(0x1000)

    def call(advanced=0, channels=1, level=92.0, rate=48000, max_lag=0, summary=buf, ctx=None):
        rc = lib.peaq_run_pair_band_summary(ctx, advanced, channels, level, rate, max_lag, px, 4096, px, 4096, summary,
                                            None, None)
        return rc, lib.peaq_last_error().decode()

    rc, msg = call(summary=None)
    assert rc == -1 and "peaq_run_pair_band_summary: summary is NULL" in msg
    rc, msg = call(max_lag=20000)
    assert rc == -1 and "20000" in msg
    rc, msg = call(rate=7000)
    assert rc == -1 and "7000" in msg
    rc, msg = call(channels=5)
    assert rc == -1 and "channels must be 1 or 2" in msg
    for advanced in (0, 1):
        rc, msg = call(advanced=advanced)
        assert rc == -1 and "ctx is NULL" in msg


def test_python_binding_exports_the_band_summary(lib):
    import gstpeaq_amd
    assert callable(gstpeaq_amd.batch_band_summary) and callable(gstpeaq_amd.run_pair_band_summary)
    assert list(gstpeaq_amd.BAND_SUMMARY_ROWS) == ROWS
    for name in ("batch_band_summary", "run_pair_band_summary", "BAND_SUMMARY_ROWS"):
        assert name in gstpeaq_amd.__all__


def test_named_views_divide_by_the_rows_own_denominators_and_are_nan_without_one():
    from gstpeaq_amd.capi import _band_summary_views
    planes = oracle_planes(1, GAPPED)
    rows = np.stack([summarise(planes, flags_of(1, GAPPED)), np.zeros((1, 8, 110))])     # [pairs, channels, R, row]
    v = _band_summary_views(rows, 109)
    assert list(v["counted"][:, 0]) == [37, 0]
    for name in ("nmr_mean", "nmr_max", "nmr_disturbed", "exc_ref_mean", "exc_test_mean", "moddiff1", "moddiff2",
                 "noiseloud_mean"):
        assert v[name].shape == (2, 1, 109) and np.isnan(v[name][1]).all() and np.isfinite(v[name][0]).all(), name
    assert np.array_equal(v["nmr_mean"][0, 0], rows[0, 0, 0, :109] / 37) and np.array_equal(v["nmr_max"][0], rows[0, 0, 1:2, :109])
    assert ((v["nmr_disturbed"][0] >= 0) & (v["nmr_disturbed"][0] <= 1)).all()
    _, md1, md2 = movs_of(rows[0])
    assert v["moddiff1"][0, 0].sum() == pytest.approx(md1, rel=1e-12) and v["moddiff2"][0, 0].sum() == pytest.approx(md2, rel=1e-12)
    adv = _band_summary_views(np.zeros((1, 2, 4, 56)), 55)
    assert sorted(adv) == ["counted", "exc_ref_mean", "nmr_disturbed", "nmr_max", "nmr_mean"]


def cli(*args):
    if not gst_env.CLI.exists():
        subprocess.run(["make", "-C", str(gst_env.CLI.parent)], check=True, capture_output=True)
    return subprocess.run([str(gst_env.CLI), *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("flag", ["--band-summary", "--band-summary="])
def test_cli_band_summary_without_a_file_name_is_a_usage_error(flag):
    out = cli(flag, "ref.wav", "test.wav")
    assert out.returncode == 1 and "--band-summary needs a file name" in out.stderr, (out.returncode, out.stderr)


def test_cli_band_summary_usage_errors_and_help():
    out = cli("--band-summary=x.csv", "--interval=1", "ref.wav", "test.wav")
    assert out.returncode == 1 and "--band-summary belongs to the plain one-call mode" in out.stderr
    out = cli("--band-summary=x.csv", "--list=pairs.txt")
    assert out.returncode == 1 and "--band-summary belongs to the plain one-call mode" in out.stderr
    for other in ("--trace=y.csv", "--bands=y.csv", "--pattern-bands=y.csv", "--match-gain", "--align-subsample",
                  "--align-drift", "--align-track", "--align-steps"):
        out = cli("--band-summary=x.csv", other, "ref.wav", "test.wav")
        assert out.returncode == 1 and "--band-summary is a run of its own" in out.stderr, (other, out.stderr)
    out = cli("--band-summary=x.csv", "--fb-bands=y.csv", "--advanced", "ref.wav", "test.wav")
    assert out.returncode == 1 and "--band-summary is a run of its own" in out.stderr, out.stderr
    out = cli("--help")
    assert out.returncode == 0 and "--band-summary=FILE" in out.stdout and "moddiff1_wsum" in out.stdout

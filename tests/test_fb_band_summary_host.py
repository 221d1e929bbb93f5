"""CPU-side checks of the filter-bank band summary (peaq_fb_band_summary_rows, peaq_fb_band_summary_row,
peaq_batch_run_fb_band_summary, peaq_run_pair_fb_band_summary, `peaq --advanced --fb-band-summary`; include/peaq_amd.h):
the names are exported, every argument the header says is refused is refused with PEAQ_ERR_ARG before a context or a
device is touched -- the calls below pass no context at all, or one that is never dereferenced -- with a message that
names the value: the rules and words tests/test_output_entries_host.py holds the other output entries to.

Also here, because it needs no GPU: summarise_fb(), the header's table of rows in numpy with strict in-order sums, and
its own check on the CPU oracle: fed with tests/test_gpu_fb_bands.py::recipe on the oracle's block records and the flags
restated in tests/test_gpu_trace.py, its rows reproduce the oracle's RmsModDiff, RmsNoiseLoudAsym and AvgLinDist through
the header's three identities.  That holds the definition of the COUNTED blocks, of the two gates and of the weights
against the reference's accumulators before any GPU is involved.  tests/test_gpu_fb_band_summary.py feeds the same
function with the device's planes.

Inputs, mono and stereo: tests/test_gpu_fb_bands.py's signal recipe (seed 5) at N = 192 x 200 + 100 samples -- 201
blocks, 76 of them behind block 125 -- as a plain pair (noise at 1e-2), a ragged pair (noise at 1e-3, the test signal 700
samples shorter: 197 blocks), a gapped pair (noise at 1e-2; reference and test wholly zero over blocks 0 .. 4, 150 .. 158
and from 185 on) and an all-silent pair.

Tolerance of the three identities: 1e-10 relative, the one tests/test_band_summary_host.py holds its identities to.  Every
term is non-negative and a sum has fewer than 1e4 additions, so reordering it changes it by less than 1e4 x 2^-53 =
1.2e-12 relative.  Measured on the CPU oracle over the six non-silent pairs: at most 2.2e-16
(RmsModDiff), 2.2e-16 (RmsNoiseLoudAsym) and 1.2e-14 (AvgLinDist, on the ragged pair, whose terms are the smallest)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import gst_env
import oracle_lib as orc
from test_gpu_fb_bands import block_values, recipe
from test_gpu_trace import ABOVE, FLUSH, LOUD_OPEN, MOD_OPEN, expected_flags

NB, ROW, R = 40, 42, 7
ROWS = ["exc_ref_sum", "exc_test_sum", "moddiff_wsum", "moddiff_sq", "noiseloud_sq", "missing_sq", "lindist_sum"]
VIEWS = ["exc_ref_mean", "exc_test_mean", "moddiff", "moddiff_sq_share", "noiseloud_sq_share", "missing_sq_share",
         "lindist_mean"]
N = 192 * 200 + 100                                  # 200 full blocks and the flush block
# the gapped pair's zero stretches in samples: blocks 0 .. 4, 150 .. 158 and 185 .. 200 (block b is samples
# [192 b, 192 b + 192))
GAPS = [(0, 5 * 192), (150 * 192, 159 * 192), (185 * 192, N)]
PLAIN, RAGGED, GAPPED, SILENT = 0, 1, 2, 3
PLANES = ["exc_ref", "exc_test", "moddiff", "modwt", "noiseloud", "missing", "lindist"]   # what summarise_fb() reads

_PAIRS, _INPUTS, _PLANES, _FLAGS = {}, {}, {}, {}


def all_pairs(channels):
    """[(ref, test)] x 4: plain, ragged, gapped, silent"""
    if channels not in _PAIRS:
        rng = np.random.default_rng(5)
        t = np.arange(N)[:, None] / 48000.
        f = np.array([1000., 3150.])[:channels][None, :]
        ref = (0.05 * np.sin(2 * np.pi * f * t) + 0.00025 * rng.standard_normal((N, channels))).astype(np.float32)
        tests = [(ref + np.float32(s) * rng.standard_normal((N, channels)).astype(np.float32)).astype(np.float32)
                 for s in (1e-2, 1e-3, 1e-2)]
        env = np.ones((N, 1), dtype=bool)
        for a, b in GAPS:
            env[a:b] = False
        zero = np.float32(0.)
        silent = np.zeros((N, channels), dtype=np.float32)
        _PAIRS[channels] = [(ref, tests[0]), (ref, np.ascontiguousarray(tests[1][:N - 700])),
                            (np.where(env, ref, zero), np.where(env, tests[2], zero)), (silent, silent.copy())]
    return _PAIRS[channels]


def counts_of(channels):
    return [orc.count_blocks(len(r), len(t)) for r, t in all_pairs(channels)]


def flags_of(channels, p):
    """the blocks' flags of pair p as tests/test_gpu_trace.py restates them on the CPU"""
    if (channels, p) not in _FLAGS:
        ref, test = all_pairs(channels)[p]
        _FLAGS[channels, p], _ = expected_flags(ref, test, counts_of(channels)[p], True, f"channels {channels} pair {p}")
    return _FLAGS[channels, p]


def oracle_inputs(channels, p):
    """the four input planes of pair p from the oracle's block records: dict name -> [blocks, channels, 40]; computed
    once, shared, never changed"""
    if (channels, p) not in _INPUTS:
        ref, test = all_pairs(channels)[p]
        rec = orc.fb_records(ref, test, counts_of(channels)[p])
        _INPUTS[channels, p] = {name: rec[:, :, 40 * k:40 * k + 40]
                                for k, name in enumerate(("unsm_ref", "unsm_test", "exc_ref", "exc_test"))}
    return _INPUTS[channels, p]


def oracle_planes(channels, p, swap=1):
    """the seven planes summarise_fb() reads, of pair p, from the CPU oracle's block records through
    tests/test_gpu_fb_bands.py::recipe: dict name -> [blocks, channels, 40]; computed once, shared, never changed"""
    if (channels, p, swap) not in _PLANES:
        inp = oracle_inputs(channels, p)
        with np.errstate(divide="ignore", invalid="ignore"):       # (the silent stretches: 0 / 0 in blocks that are not read)
            rec = recipe(inp, swap)
        _PLANES[channels, p, swap] = dict(exc_ref=inp["exc_ref"], exc_test=inp["exc_test"],
                                          **{k: rec[k] for k in PLANES[2:]})
    return _PLANES[channels, p, swap]


def seq_sum(x):
    """the sum over axis 0 as a running sum in index order (np.sum adds pairwise); zeros for no term"""
    return np.cumsum(x, axis=0)[-1] if len(x) else np.zeros(x.shape[1:])


def summarise_fb(planes, flags, block=None):
    """The table of include/peaq_amd.h.  planes: dict name -> [blocks, channels, 40] with PLANES; flags: [blocks], the
    block trace's; block: [blocks, channels, 5], the block trace's ch -- where given, W, D, L and M are taken from it
    (D = ch[c][0] sqrt 40 / 100), otherwise they are made of the planes as the header defines them.  -> rows
    [channels, 7, 42]: the denominator in entry 40, entry 41 zero"""
    flags = np.asarray(flags)
    nblk, channels, nb = planes["exc_ref"].shape
    rows = np.zeros((channels, R, nb + 2))
    above = np.flatnonzero(flags & ABOVE)
    if not above.size:
        return rows
    counted = np.zeros(nblk, dtype=bool)
    counted[above[0]:above[-1] + 1] = True
    if block is None:
        w, d = planes["modwt"].sum(axis=-1), planes["moddiff"].sum(axis=-1)
        raw, m = 0.6 * planes["noiseloud"].sum(axis=-1), 0.6 * planes["missing"].sum(axis=-1)
        l = np.where(raw < 0.1, 0., raw)
    else:
        block = np.asarray(block)
        w, d, l, m = block[:, :, 1], block[:, :, 0] * (np.sqrt(40.) / 100.), block[:, :, 2], block[:, :, 3]
    rows[:, 0, :nb] = seq_sum(planes["exc_ref"][counted])
    rows[:, 1, :nb] = seq_sum(planes["exc_test"][counted])
    rows[:, 0:2, nb] = np.count_nonzero(counted)
    mod = counted & ((flags & MOD_OPEN) != 0)
    rows[:, 2, :nb] = seq_sum(w[mod][:, :, None] * planes["moddiff"][mod])
    rows[:, 2, nb] = seq_sum(w[mod])
    w2 = w[mod] * w[mod]
    rows[:, 3, :nb] = seq_sum(w2[:, :, None] * (d[mod][:, :, None] * planes["moddiff"][mod]))
    rows[:, 3, nb] = seq_sum(w2)
    loud = counted & ((flags & LOUD_OPEN) != 0)
    rows[:, 4, :nb] = seq_sum(l[loud][:, :, None] * planes["noiseloud"][loud])
    rows[:, 5, :nb] = seq_sum(m[loud][:, :, None] * planes["missing"][loud])
    rows[:, 6, :nb] = seq_sum(planes["lindist"][loud])
    rows[:, 4:7, nb] = np.count_nonzero(loud)
    return rows


def movs_of(rows):
    """(RmsModDiff, RmsNoiseLoudAsym, AvgLinDist) of the advanced version from a pair's rows [channels, 7, 42], by the
    header's identities; NaN where nothing was counted, like the MOVs themselves"""
    nb = rows.shape[-1] - 2
    s = rows[:, :, :nb].sum(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        rms = np.mean(100. / np.sqrt(nb) * np.sqrt(s[:, 3] / rows[:, 3, nb]))
        asym = np.mean(np.sqrt(0.6 * s[:, 4] / rows[:, 4, nb]) + 0.5 * np.sqrt(0.6 * s[:, 5] / rows[:, 5, nb]))
        lin = np.mean(0.6 * s[:, 6] / rows[:, 6, nb])
    return rms, asym, lin


def counted_range(flags):
    above = np.flatnonzero(np.asarray(flags) & ABOVE)
    return (int(above[0]), int(above[-1])) if above.size else None


# ---- the inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
def test_the_inputs_have_the_blocks_the_summary_has_to_tell_apart(channels):
    assert counts_of(channels) == [201, 197, 201, 201]
    fl = flags_of(channels, GAPPED)
    assert counted_range(fl) == (5, 184)
    inside = np.arange(5, 185)
    interior = inside[(fl[inside] & ABOVE) == 0]
    assert list(interior) == list(range(150, 159))                             # the interior gap lies inside the range
    assert fl[-1] & FLUSH and not fl[-1] & ABOVE
    assert (fl[inside] & LOUD_OPEN).any() and (fl[inside] & MOD_OPEN).any()
    assert counted_range(flags_of(channels, SILENT)) is None
    for p in (PLAIN, RAGGED):
        assert (flags_of(channels, p) & ABOVE).all()
    for p in (PLAIN, RAGGED, GAPPED):                                          # no counted, gated block sits on the floor
        f = flags_of(channels, p)
        a, b = counted_range(f)
        open_ = np.flatnonzero((f & LOUD_OPEN) != 0)
        open_ = open_[(open_ >= a) & (open_ <= b)]
        assert open_.size
        _, raw = block_values(oracle_planes(channels, p))
        dist = float(np.min(np.abs(raw[open_] - 0.1)))
        print(f"fb-band-summary-host channels={channels} pair={p}: {open_.size} counted LOUD_OPEN blocks, "
              f"0.6 sum NOISELOUD at least {dist:.3e} from the floor")
        assert dist > 1e-9, (p, dist)


# ---- summarise_fb() on the CPU oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
def test_summarise_fb_reproduces_the_oracle_s_movs(channels):
    for p, (ref, test) in enumerate(all_pairs(channels)):
        rows = summarise_fb(oracle_planes(channels, p), flags_of(channels, p))
        want = orc.run_pair(1, ref, test)["movs"]
        got = movs_of(rows)
        if p == SILENT:
            assert not rows.any() and np.isnan(got).all() and np.isnan([want[0], want[1], want[4]]).all()
            continue
        dev = [g / w - 1. for g, w in zip(got, (want[0], want[1], want[4]))]
        print(f"fb-band-summary-host channels={channels} pair={p}: RmsModDiff {dev[0]:+.3e}, RmsNoiseLoudAsym "
              f"{dev[1]:+.3e}, AvgLinDist {dev[2]:+.3e}, counted {rows[0, 0, NB]:.0f}, loud blocks {rows[0, 4, NB]:.0f}")
        assert max(abs(x) for x in dev) <= 1e-10, (p, got, want)
        assert not rows[:, :, NB + 1].any()
    assert summarise_fb(oracle_planes(channels, GAPPED), flags_of(channels, GAPPED))[0, 0, NB] == 180


@pytest.mark.parametrize("channels", [1, 2])
def test_summarise_fb_follows_the_swap_switch_like_the_oracle(channels):
    ref, test = all_pairs(channels)[GAPPED]
    orc.set_settings(swap_mod_patts_for_noise_loudness_movs=0)
    try:
        want = orc.run_pair(1, ref, test)["movs"]
    finally:
        orc.set_settings()
    rows = summarise_fb(oracle_planes(channels, GAPPED, swap=0), flags_of(channels, GAPPED))
    for g, w in zip(movs_of(rows), (want[0], want[1], want[4])):
        assert abs(g / w - 1.) <= 1e-10, (g, w)
    dflt = summarise_fb(oracle_planes(channels, GAPPED), flags_of(channels, GAPPED))
    assert np.array_equal(rows[:, :5], dflt[:, :5]) and not np.array_equal(rows[:, 5], dflt[:, 5]) \
        and not np.array_equal(rows[:, 6], dflt[:, 6])


def test_summarise_fb_on_three_bands_and_six_blocks():
    """made-up planes with known sums: a leading and a trailing block below the boundary do not count, the one in
    between does; the gates pick among the counted blocks; W, W^2 D, L and M weight their rows; a floored L gives 0"""
    nb = 3
    fl = np.array([MOD_OPEN, ABOVE, MOD_OPEN | LOUD_OPEN, ABOVE | MOD_OPEN, ABOVE | MOD_OPEN | LOUD_OPEN,
                   MOD_OPEN | LOUD_OPEN | FLUSH])
    v = (1. + np.arange(6))[:, None, None] * np.ones((6, 1, nb))               # block i holds i + 1 in every band
    planes = dict(exc_ref=v, exc_test=2 * v, moddiff=v * np.array([1., 2., 3.]), modwt=np.ones((6, 1, nb)) / 3.,
                  noiseloud=v / 6., missing=v * np.array([1., 0., 2.]), lindist=3 * v)
    rows = summarise_fb(planes, fl)
    assert rows.shape == (1, 7, nb + 2) and not rows[:, :, nb + 1].any()
    assert (rows[0, :2, nb] == 4).all()                                        # blocks 1 .. 4
    assert list(rows[0, 0, :nb]) == [14.] * 3 and list(rows[0, 1, :nb]) == [28.] * 3
    # blocks 2, 3, 4 have MOD_OPEN; W = 1 (up to the rounding of 3 x 1/3), D = 6 (i + 1)
    assert rows[0, 2, nb] == pytest.approx(3.) and list(rows[0, 2, :nb]) == pytest.approx([12., 24., 36.])
    assert rows[0, 3, nb] == pytest.approx(3.)
    assert list(rows[0, 3, :nb]) == pytest.approx([6. * 50., 12. * 50., 18. * 50.])     # sum (i+1)^2 = 9 + 16 + 25
    # blocks 2 and 4 have LOUD_OPEN; L = 0.6 x 3 (i + 1) / 6 = 0.3 (i + 1) (0.9, 1.5), M = 0.6 x 3 (i + 1) = 1.8 (i + 1)
    assert (rows[0, 4:, nb] == 2).all()
    assert list(rows[0, 4, :nb]) == pytest.approx([0.9 * 0.5 + 1.5 * 5. / 6.] * 3)
    assert list(rows[0, 5, :nb]) == pytest.approx([1.8 * 34., 0., 3.6 * 34.])
    assert list(rows[0, 6, :nb]) == [24.] * 3
    rms, asym, lin = movs_of(rows)
    assert rms == pytest.approx(100. / np.sqrt(3.) * np.sqrt(36. * 50. / 3.))  # sqrt (sum W^2 D^2 / sum W^2)
    assert lin == pytest.approx(0.6 * 72. / 2.)
    assert asym == pytest.approx(np.sqrt((0.81 + 2.25) / 2.) + 0.5 * np.sqrt((5.4 ** 2 + 9. ** 2) / 2.))
    # a block whose 0.6 sum NOISELOUD is below 0.1 contributes 0 to row 4 and still counts in m
    quiet = dict(planes, noiseloud=planes["noiseloud"] * np.where(np.arange(6) == 2, 0.01, 1.)[:, None, None])
    q = summarise_fb(quiet, fl)
    assert q[0, 4, nb] == 2 and list(q[0, 4, :nb]) == pytest.approx([1.5 * 5. / 6.] * 3)
    assert not summarise_fb(planes, fl & ~np.uint32(ABOVE)).any()
    only_first = summarise_fb(planes, np.where(np.arange(6) == 1, fl, fl & ~np.uint32(ABOVE)))
    assert (only_first[0, :2, nb] == 1).all() and not only_first[0, 2:].any()


# ---- the entry points ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import gstpeaq_amd
    if not gstpeaq_amd.library_path().exists():
        gstpeaq_amd.build_library()
    L = gstpeaq_amd.load_library()
    L.peaq_last_error.restype = C.c_char_p
    return L


def test_every_declared_name_is_exported(lib):
    for name in ("peaq_fb_band_summary_rows", "peaq_fb_band_summary_row", "peaq_batch_run_fb_band_summary",
                 "peaq_run_pair_fb_band_summary"):
        assert hasattr(lib, name), name
    assert lib.peaq_fb_band_summary_rows() == 7 and lib.peaq_fb_band_summary_row() == 42


def batch_fb_band_summary(lib, channels=2, n_pairs=2, pair_stride=48000, n_ref=None, n_test=None, n_uniform=48000,
                          summary=0x1000, ctx=None, ref=0x100000, test=0x200000):
    """peaq_batch_run_fb_band_summary with made-up device addresses: nothing may get as far as reading them"""
    u32p = C.POINTER(C.c_uint32)
    a = None if n_ref is None else np.ascontiguousarray(n_ref, dtype=np.uint32)
    b = None if n_test is None else np.ascontiguousarray(n_test, dtype=np.uint32)
    rc = lib.peaq_batch_run_fb_band_summary(ctx, channels, 92.0, n_pairs, C.c_void_p(ref), C.c_void_p(test), pair_stride,
                                            None if a is None else a.ctypes.data_as(u32p),
                                            None if b is None else b.ctypes.data_as(u32p), n_uniform,
                                            C.c_void_p(summary) if summary else None, C.c_void_p(0x3000), None)
    return rc, lib.peaq_last_error().decode()


def test_the_summary_array_is_checked_first_and_by_value(lib):
    rc, msg = batch_fb_band_summary(lib, summary=0)
    assert rc == -1 and "peaq_batch_run_fb_band_summary: d_summary is NULL" in msg
    for addr in (0x1008, 0x1004, 0x100f):
        rc, msg = batch_fb_band_summary(lib, summary=addr)
        assert rc == -1 and f"d_summary 0x{addr:x} is not 16-byte aligned" in msg, msg
        assert msg.startswith("peaq_batch_run_fb_band_summary: "), msg
    rc, msg = batch_fb_band_summary(lib, summary=0x1010)
    assert rc == -1 and msg == "peaq_batch_run_fb_band_summary: ctx is NULL", msg


def test_what_peaq_batch_run_refuses_is_refused_here_too(lib):
    rc, msg = batch_fb_band_summary(lib)
    assert rc == -1 and "peaq_batch_run_fb_band_summary: ctx is NULL" in msg
    ctx = C.c_void_p(0x5000)                            # never dereferenced: the checks below come first
    rc, msg = batch_fb_band_summary(lib, ctx=ctx, channels=3)
    assert rc == -1 and "peaq_batch_run_fb_band_summary: channels must be 1 or 2, not 3" in msg
    rc, msg = batch_fb_band_summary(lib, ctx=ctx, n_pairs=-1)
    assert rc == -1 and "n_pairs < 0" in msg
    rc, msg = batch_fb_band_summary(lib, ctx=ctx, ref=0)
    assert rc == -1 and "NULL buffer" in msg
    rc, msg = batch_fb_band_summary(lib, ctx=ctx, test=0)
    assert rc == -1 and "NULL buffer" in msg
    rc, msg = batch_fb_band_summary(lib, ctx=ctx, n_ref=[10, 10])
    assert rc == -1 and "both n_ref and n_test or neither" in msg
    rc, _ = batch_fb_band_summary(lib, ctx=ctx, n_pairs=0)
    assert rc == 0                                      # no pairs: nothing to do, as peaq_batch_run


def test_host_pair_entry_checks_its_arguments(lib):
    fp = C.POINTER(C.c_float)
    x = np.zeros(4096, dtype=np.float32)
    px = x.ctypes.data_as(fp)
    buf = C.c_void_p(0x1000)

    def call(channels=1, level=92.0, rate=48000, max_lag=0, summary=buf, ctx=None):
        rc = lib.peaq_run_pair_fb_band_summary(ctx, channels, level, rate, max_lag, px, 4096, px, 4096, summary, None, None)
        return rc, lib.peaq_last_error().decode()

    rc, msg = call(summary=None)
    assert rc == -1 and msg == "peaq_run_pair_fb_band_summary: summary is NULL", msg
    rc, msg = call(summary=None, max_lag=20000)         # its own argument first, before max_lag
    assert rc == -1 and msg == "peaq_run_pair_fb_band_summary: summary is NULL", msg
    rc, msg = call(max_lag=20000)
    assert rc == -1 and msg.startswith("peaq_run_pair_fb_band_summary: max_lag 20000 is outside 1 .. "), msg
    rc, msg = call(rate=7000)
    assert rc == -1 and "7000" in msg
    rc, msg = call(channels=5)
    assert rc == -1 and "channels must be 1 or 2" in msg and "5" in msg
    rc, msg = call()
    assert rc == -1 and msg == "peaq_run_pair_fb_band_summary: NULL argument: ctx is NULL", msg


def test_python_binding_exports_the_fb_band_summary(lib):
    import gstpeaq_amd
    assert callable(gstpeaq_amd.batch_fb_band_summary) and callable(gstpeaq_amd.run_pair_fb_band_summary)
    assert list(gstpeaq_amd.FB_BAND_SUMMARY_ROWS) == ROWS
    for name in ("batch_fb_band_summary", "run_pair_fb_band_summary", "FB_BAND_SUMMARY_ROWS"):
        assert name in gstpeaq_amd.__all__


def test_named_views_divide_by_their_denominators_and_are_nan_without_one():
    from gstpeaq_amd.capi import _fb_band_summary_views
    one = summarise_fb(oracle_planes(1, GAPPED), flags_of(1, GAPPED))
    rows = np.stack([one, np.zeros((1, R, ROW))])                              # [pairs, channels, 7, 42]
    v = _fb_band_summary_views(rows)
    assert sorted(v) == sorted(VIEWS + ["counted"]) and list(v["counted"][:, 0]) == [180, 0]
    for name in VIEWS:
        assert v[name].shape == (2, 1, NB) and np.isnan(v[name][1]).all() and np.isfinite(v[name][0]).all(), name
    assert np.array_equal(v["exc_ref_mean"][0, 0], one[0, 0, :NB] / 180) and np.array_equal(v["exc_test_mean"][0, 0], one[0, 1, :NB] / 180)
    assert np.array_equal(v["moddiff"][0, 0], one[0, 2, :NB] / one[0, 2, NB])
    assert np.array_equal(v["lindist_mean"][0, 0], one[0, 6, :NB] / one[0, 6, NB])
    for name, k in (("moddiff_sq_share", 3), ("noiseloud_sq_share", 4), ("missing_sq_share", 5)):
        assert v[name][0, 0].sum() == pytest.approx(1., rel=1e-12), name
        assert np.array_equal(v[name][0, 0], one[0, k, :NB] / one[0, k, :NB].sum()), name
    # a row without a denominator of its own kind is NaN though the pair has counted blocks (no LOUD_OPEN block)
    early = one.copy()
    early[:, 4:] = 0.
    w = _fb_band_summary_views(early)
    assert np.isnan(w["noiseloud_sq_share"]).all() and np.isnan(w["lindist_mean"]).all() and np.isfinite(w["moddiff"]).all()


def cli(*args):
    if not gst_env.CLI.exists():
        subprocess.run(["make", "-C", str(gst_env.CLI.parent)], check=True, capture_output=True)
    return subprocess.run([str(gst_env.CLI), *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("flag", ["--fb-band-summary", "--fb-band-summary="])
def test_cli_fb_band_summary_without_a_file_name_is_a_usage_error(flag):
    out = cli("--advanced", flag, "ref.wav", "test.wav")
    assert out.returncode == 1 and "--fb-band-summary needs a file name" in out.stderr, (out.returncode, out.stderr)


def test_cli_fb_band_summary_usage_errors_and_help():
    out = cli("--fb-band-summary=x.csv", "ref.wav", "test.wav")
    assert out.returncode == 1 and "--fb-band-summary needs --advanced" in out.stderr, out.stderr
    out = cli("--advanced", "--fb-band-summary=x.csv", "--interval=1", "ref.wav", "test.wav")
    assert out.returncode == 1 and "--fb-band-summary belongs to the plain one-call mode" in out.stderr
    out = cli("--advanced", "--fb-band-summary=x.csv", "--list=pairs.txt")
    assert out.returncode == 1 and "--fb-band-summary belongs to the plain one-call mode" in out.stderr
    for other in ("--trace=y.csv", "--bands=y.csv", "--fb-bands=y.csv", "--band-summary=y.csv", "--match-gain",
                  "--align-subsample", "--align-drift", "--align-track", "--align-steps"):
        out = cli("--advanced", "--fb-band-summary=x.csv", other, "ref.wav", "test.wav")
        assert out.returncode == 1 and "--fb-band-summary is a run of its own" in out.stderr, (other, out.stderr)
    out = cli("--advanced", "--fb-band-summary=x.csv", "--pattern-bands=y.csv", "ref.wav", "test.wav")
    assert out.returncode == 1, out.stderr              # (--pattern-bands and --advanced exclude each other first)
    out = cli("--help")
    assert out.returncode == 0 and "--fb-band-summary=FILE" in out.stdout
    for name in ROWS:
        assert name in out.stdout, name

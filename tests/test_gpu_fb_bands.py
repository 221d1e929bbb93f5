"""Band traces of the filter-bank path (peaq_batch_run_fb_bands, include/peaq_amd.h): the values the filter-bank back end
has per block, channel and band of every pair of an advanced batch, before accumulation -- pinned here against the CPU
oracle's block records (the four input planes), against a numpy recipe of the oracle's level adapter and modulation
processor fed with the DEVICE's own input planes (the back end alone: the filter bank's error does not enter, so the
check is the same in both FIR modes), against the block trace of the same inputs (identities on device values only), for
their layout under plane masks, across the launch seam of the filter-bank path, for the results of the same call, and
through the host entry and the CLI.  Needs an MI355X (`-m gpu`); the recipe's own check against the oracle does not.

Inputs: tests/test_gpu_bands.py's signal recipe (seed 5) at N = 192 x 140 + 100 samples -- 141 blocks (140 full and the
flush block; blocks from 125 on have both gates of gstpeaq.c:988/996 open), 26 frames -- and three test signals: the
reference plus white noise at 1e-2, at 1.5e-4 and, 700 samples shorter (137 blocks, a ragged pair), at 1e-3.

MODDIFF, NOISELOUD, MISSING and LINDIST are differences of nearly equal quantities where the signals agree.  Their
deviation from the recipe is |got - want| / (|want| + 1e-6 max |want| of that plane and pair), and each plane's bound
TERM_BOUND is ten times the largest value measured on the first run on an MI355X over the three pairs and both channel
counts (DESIGN.md 21 has the figures), below the project's ceiling of 1e-6 for cancellation-limited values."""
import subprocess

import numpy as np
import pytest

import gst_env
import oracle_lib as orc
from test_conformance_runner import write_wav
from test_gpu_trajectory import to_device

gpu_test = pytest.mark.gpu

N = 192 * 140 + 100
NB = 40
NAMES = ["moddiff", "modwt", "noiseloud", "missing", "lindist", "unsm_ref", "unsm_test", "exc_ref", "exc_test",
         "adapt_ref", "adapt_test", "mod_ref", "mod_test"]    # in the order of the bits, which is the order of the slots
BITS = {n: 1 << k for k, n in enumerate(NAMES)}
ALL = 0x1FFF
TERMS = ["moddiff", "modwt", "noiseloud", "missing", "lindist"]
INPUTS = ["unsm_ref", "unsm_test", "exc_ref", "exc_test"]
SENTINEL = -777.25                                   # what the tests put into the row arrays before a run
# measured on the first run on an MI355X: the largest deviation (as defined above) from the recipe over all blocks and
# bands of the three pairs, both channel counts, both FIR modes and both values of the swap switch, per plane (each
# over 2 x 2 x (141 + 141 + 137) x 3 x 40 = 201 120 values):
#   MODDIFF 3.375e-9, NOISELOUD 2.224e-9, MISSING 1.301e-9, LINDIST 4.975e-10 -> ten times that, each plane its own
# (the patterns they are differences of: ADAPT 3.1e-15, MOD 5.7e-12 relative, MODWT 6.7e-16)
TERM_BOUND = dict(moddiff=3.4e-8, noiseloud=2.3e-8, missing=1.4e-8, lindist=5.0e-9)
assert max(TERM_BOUND.values()) <= 1e-6              # the ceiling: a larger measured value is a finding, not a tolerance


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback in the product)")
    import gpu_common
    return gpu_common


_PAIRS, _ORACLE, _RUNS, _RECIPES = {}, {}, {}, {}


def pairs_of(channels):
    """[(ref, test)] x 3: noise at 1e-2, at 1.5e-4, and the ragged pair at 1e-3 whose test signal is 700 samples shorter"""
    if channels not in _PAIRS:
        rng = np.random.default_rng(5)
        t = np.arange(N)[:, None] / 48000.
        f = np.array([1000., 3150.])[:channels][None, :]
        ref = (0.05 * np.sin(2 * np.pi * f * t) + 0.00025 * rng.standard_normal((N, channels))).astype(np.float32)
        tests = [(ref + np.float32(s) * rng.standard_normal((N, channels)).astype(np.float32)).astype(np.float32)
                 for s in (1e-2, 1.5e-4, 1e-3)]
        tests[2] = np.ascontiguousarray(tests[2][:N - 700])
        _PAIRS[channels] = [(ref, x) for x in tests]
    return _PAIRS[channels]


def counts_of(channels):
    return [orc.count_blocks(len(r), len(t)) for r, t in pairs_of(channels)]


def oracle_inputs(channels, p):
    """the four input planes of pair p from the oracle's block records: dict name -> [blocks, channels, 40]; computed
    once, shared, never changed"""
    if (channels, p) not in _ORACLE:
        ref, test = pairs_of(channels)[p]
        rec = orc.fb_records(ref, test, orc.count_blocks(len(ref), len(test)))
        _ORACLE[channels, p] = {name: rec[:, :, 40 * k:40 * k + 40] for k, name in enumerate(INPUTS)}
    return _ORACLE[channels, p]


def noise_term(n, alpha, f, m_ref, m_test, e_ref, e_test):
    """movs.c:709-743, the band's term before the sum"""
    sref, stest = f * m_ref + 1., f * m_test + 1.
    beta = np.exp(-alpha * (e_test - e_ref) / e_ref)
    return np.power(n / stest, 0.23) * (np.power(1. + np.maximum(stest * e_test - sref * e_ref, 0.) /
                                                 (n + sref * e_ref * beta), 0.23) - 1.)


def recipe(inp, swap=1):
    """the nine planes the back end makes of the four input planes (dict name -> [blocks, channels, 40]), with the
    oracle's level adapter and modulation processor and the header's formulas in numpy; also `margin`, the relative
    distance of stest at from sref ar in NOISELOUD's numerator"""
    n = orc.tables(NB)["internal_noise"]
    out = {k: np.zeros_like(inp["exc_ref"]) for k in TERMS + ["adapt_ref", "adapt_test", "mod_ref", "mod_test", "margin"]}
    for c in range(inp["exc_ref"].shape[1]):
        er, et = inp["exc_ref"][:, c], inp["exc_test"][:, c]
        ar, at = orc.leveladapt(NB, er, et)
        mr, lr = orc.modproc(NB, inp["unsm_ref"][:, c])
        mt, _ = orc.modproc(NB, inp["unsm_test"][:, c])
        out["adapt_ref"][:, c], out["adapt_test"][:, c], out["mod_ref"][:, c], out["mod_test"][:, c] = ar, at, mr, mt
        out["moddiff"][:, c] = np.abs(mr - mt) / (1. + mr)                     # movs.c:224-251
        out["modwt"][:, c] = lr / (lr + np.power(n, 0.3))
        out["noiseloud"][:, c] = noise_term(n, 2.5, 0.3, mr, mt, ar, at)
        out["missing"][:, c] = noise_term(n, 1.5, 0.15, mt, mr, at, ar) if swap else noise_term(n, 1.5, 0.15, mr, mt, at, ar)
        out["lindist"][:, c] = noise_term(n, 1.5, 0.15, mr, mr if swap else mt, ar, er)
        a, b = (0.3 * mt + 1.) * at, (0.3 * mr + 1.) * ar
        out["margin"][:, c] = (a - b) / np.maximum(np.abs(a), np.abs(b))
    return out


def block_values(planes):
    """the block record's five values per channel from the five term planes -> [blocks, channels, 5], and 0.6 sum
    NOISELOUD before the 0.1 floor -> [blocks, channels]"""
    raw = 0.6 * planes["noiseloud"].sum(axis=-1)
    v = np.stack([100. / np.sqrt(NB) * planes["moddiff"].sum(axis=-1), planes["modwt"].sum(axis=-1),
                  np.where(raw < 0.1, 0., raw), 0.6 * planes["missing"].sum(axis=-1), 0.6 * planes["lindist"].sum(axis=-1)],
                 axis=-1)
    return v, raw


def filled(n_pairs, stride, channels, n_planes):
    """a row array one pair longer than the batch, full of SENTINEL; -> (the whole array, the batch's part)"""
    import torch
    whole = torch.full((n_pairs + 1, stride, channels, n_planes, NB), SENTINEL, dtype=torch.float64, device="cuda")
    return whole, whole[:n_pairs]


def run(gpu, channels, mask, uniform=False, swap=1):
    """the three pairs (uniform: the two of equal length, without per-pair lengths) as one batch with the planes of
    `mask` -> (batch_fb_bands' dict, the whole row array as numpy [pairs + 1, stride, channels, n_planes, 40]); the
    array is one block longer than the longest pair needs, one pair longer than the batch, and full of SENTINEL first.
    One run per argument set and FIR mode, shared by the tests"""
    import gstpeaq_amd
    key = (gpu.mode(), channels, mask, uniform, swap)
    if key not in _RUNS:
        pairs = pairs_of(channels)[:2] if uniform else pairs_of(channels)
        ref, test, n_ref, n_test = to_device(pairs)
        assert ref.shape[1] == N
        whole, part = filled(len(pairs), max(counts_of(channels)) + 1, channels, bin(mask).count("1"))
        ctx = gpu.ctx()
        try:
            if not swap:
                ctx.set_settings(swap_mod_patts_for_noise_loudness_movs=0)
            out = gstpeaq_amd.batch_fb_bands(ctx, ref, test, mask, None if uniform else n_ref,
                                             None if uniform else n_test, d_bands=part)
        finally:
            ctx.set_settings()
        _RUNS[key] = (out, whole.cpu().numpy())
    return _RUNS[key]


def device_recipe(gpu, channels, p, swap=1):
    """recipe() on the device's own input planes of pair p (shared per FIR mode; the inputs do not depend on the switch)"""
    key = (gpu.mode(), channels, p, swap)
    if key not in _RECIPES:
        out, _ = run(gpu, channels, ALL)
        nb = counts_of(channels)[p]
        _RECIPES[key] = recipe({k: out[k][p, :nb] for k in INPUTS}, swap)
    return _RECIPES[key]


def names_of(mask):
    return [n for n in NAMES if mask & BITS[n]]


def deviation(got, want):
    return np.abs(got - want) / (np.abs(want) + 1e-6 * np.max(np.abs(want)))


# ---- 0: the recipe itself, on the CPU oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
def test_the_recipe_reproduces_the_oracle_s_block_values_and_stays_off_the_floor(channels):
    """recipe() on the oracle's own records gives the oracle's five block values (2.2e-13 relative measured; held to
    1e-12); no block's 0.6 sum NOISELOUD lies within 1e-9 of the 0.1 floor (2.3e-3 measured), and both sides of the
    floor occur, the lower one before block 125 only"""
    for p, nb in enumerate(counts_of(channels)):
        ref, test = pairs_of(channels)[p]
        want, _ = orc.mov_trace_advanced(ref, test, nb, orc.count_frames(len(ref), len(test)))
        got, raw = block_values(recipe(oracle_inputs(channels, p)))
        for k, name in enumerate(orc.MOV_TRACE_ADV_BLOCK[:5]):
            np.testing.assert_allclose(got[:, :, k], want[name], rtol=1e-12, atol=1e-12, err_msg=f"pair {p} {name}")
        assert np.min(np.abs(raw - 0.1)) > 1e-9, (p, float(np.min(np.abs(raw - 0.1))))
        below = raw < 0.1
        assert below.any() and (~below).any() and not below[125:].any(), (p, np.argwhere(below).tolist())


# ---- 1: inputs against the oracle ----------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("channels", [1, 2])
def test_input_planes_match_the_oracle_s_block_records(gpu, channels, fir_mode):
    out, _ = run(gpu, channels, ALL)
    assert sorted(k for k in out if k in NAMES) == sorted(NAMES)
    assert np.array_equal(out["counts"], counts_of(channels)) and counts_of(channels) == [141, 141, 137]
    t = orc.tables(NB)
    np.testing.assert_allclose(out["fc"], t["fc"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(out["internal_noise"], t["internal_noise"], rtol=1e-12, atol=0)
    for p, nb in enumerate(counts_of(channels)):
        exp = oracle_inputs(channels, p)
        for name in INPUTS:
            got = out[name][p, :nb]
            assert got.shape == exp[name].shape == (nb, channels, NB)
            np.testing.assert_allclose(got, exp[name], rtol=gpu.tol("blocks"), atol=0, err_msg=f"pair {p} {name}")


# ---- 2: the back end against the recipe on the device's own inputs ---------------------------------------------------
def check_against_recipe(gpu, channels, swap, names):
    out, _ = run(gpu, channels, ALL, swap=swap)
    worst = dict.fromkeys(TERM_BOUND, 0.)
    for p, nb in enumerate(counts_of(channels)):
        exp = device_recipe(gpu, channels, p, swap)
        for name in names:
            got, want = out[name][p, :nb], exp[name]
            if name in ("adapt_ref", "adapt_test", "modwt"):
                np.testing.assert_allclose(got, want, rtol=1e-9, atol=0, err_msg=f"pair {p} {name}")
            elif name in ("mod_ref", "mod_test"):
                np.testing.assert_allclose(got, want, rtol=1e-7, atol=1e-12, err_msg=f"pair {p} {name}")
            else:
                dev = float(np.max(deviation(got, want)))
                worst[name] = max(worst[name], dev)
                print(f"fb-bands-measure mode={gpu.mode()} channels={channels} swap={swap} pair={p} {name}: "
                      f"max deviation {dev:.3e} over {got.size} values")
    print(f"fb-bands-measure mode={gpu.mode()} channels={channels} swap={swap} worst: {worst}")
    for name in names:
        if name in TERM_BOUND:
            assert worst[name] <= TERM_BOUND[name], (name, worst[name])


@gpu_test
@pytest.mark.parametrize("channels", [1, 2])
def test_back_end_planes_match_the_recipe_on_the_device_s_own_inputs(gpu, channels, fir_mode):
    check_against_recipe(gpu, channels, 1, [n for n in NAMES if n not in INPUTS])


# ---- 3: identities with the block trace, device values only -----------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("channels", [1, 2])
def test_identities_with_the_block_trace(gpu, channels):
    import gstpeaq_amd
    out, _ = run(gpu, channels, ALL)
    ref, test, n_ref, n_test = to_device(pairs_of(channels))
    trace = gstpeaq_amd.batch_trace(gpu.ctx(), 1, ref, test, n_ref, n_test)
    for p, nb in enumerate(counts_of(channels)):
        _, raw = block_values(recipe(oracle_inputs(channels, p)))
        assert np.min(np.abs(raw - 0.1)) > 1e-9                              # no block is excluded
        bl = trace["blocks"][p][:nb]
        got, draw = block_values({k: out[k][p, :nb] for k in TERMS})
        assert np.array_equal(draw < 0.1, raw < 0.1) and (draw < 0.1).any() and (draw >= 0.1).any()
        np.testing.assert_allclose(got, bl["ch"][:, :channels, :], rtol=1e-12, atol=1e-12, err_msg=f"pair {p}")
        assert (bl["ch"][:, :channels, 2][draw < 0.1] == 0.).all()
        exp = device_recipe(gpu, channels, p)
        off = exp["margin"] < -1e-9
        assert off.any() and (out["noiseloud"][p, :nb][off] == 0.).all(), p


# ---- 4: settings -------------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("channels", [1, 2])
def test_the_swap_switch_reaches_missing_and_lindist_only(gpu, channels):
    """(on the default engine, whose filter bank gives two runs the same bits: the reduced-precision bank's sums meet in
    LDS atomics in the order the waves arrive, peaq_fb.hip, and its input planes differ in the last bit run to run)"""
    check_against_recipe(gpu, channels, 0, ["missing", "lindist"])
    dflt, _ = run(gpu, channels, ALL)
    out, _ = run(gpu, channels, ALL, swap=0)
    for name in NAMES:
        same = out[name].tobytes() == dflt[name].tobytes()
        assert same == (name not in ("missing", "lindist")), name


# ---- 5: layout -----------------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("channels", [1, 2])
def test_plane_masks_write_the_same_values_at_their_slot_ranks(gpu, channels):
    every, _ = run(gpu, channels, ALL)
    cnt = counts_of(channels)
    for mask in (0x1FFF, 0x001F, 0x1FE0, 0x0004, 0x1001):
        out, whole = run(gpu, channels, mask)
        names = names_of(mask)
        assert whole.shape == (4, max(cnt) + 1, channels, len(names), NB)    # mono: channels = 1 rows only
        assert (whole[3] == SENTINEL).all(), mask
        for p, nb in enumerate(cnt):
            assert (whole[p, nb:] == SENTINEL).all(), (mask, p)
            assert not (whole[p, :nb] == SENTINEL).any(), (mask, p)
            for k, name in enumerate(names):
                assert whole[p, :nb, :, k].tobytes() == every[name][p, :nb].tobytes(), (mask, p, name)
                assert np.array_equal(out[name][p, :nb], every[name][p, :nb], equal_nan=True)
        assert out["d_results"].cpu().numpy().tobytes() == every["d_results"].cpu().numpy().tobytes(), mask


@gpu_test
@pytest.mark.parametrize("channels", [1, 2])
def test_uniform_length_equals_per_pair_lengths(gpu, channels):
    every, _ = run(gpu, channels, ALL)
    out, whole = run(gpu, channels, ALL, uniform=True)
    assert np.array_equal(out["counts"], [141, 141]) and (whole[2] == SENTINEL).all() and (whole[:2, 141:] == SENTINEL).all()
    for name in NAMES:
        assert out[name][:, :141].tobytes() == every[name][:2, :141].tobytes(), name
    assert out["d_results"].cpu().numpy().tobytes() == every["d_results"][:2].cpu().numpy().tobytes()


# ---- 6: launch seam --------------------------------------------------------------------------------------------------------------
@gpu_test
def test_rows_across_the_launch_seam(gpu):
    """two stereo pairs of 192 000 samples: 1000 blocks, two launches of the filter-bank path at 840 blocks each.  No
    row keeps the sentinel; ADAPT and MOD -- whose state the first launch hands to the second -- follow the recipe on
    the device's inputs through blocks 839 and 840; the results are peaq_batch_run's bytes; a second run is identical"""
    import gstpeaq_amd
    import torch
    ctx = gpu.ctx()
    n, names = 192000, ["noiseloud"] + NAMES[5:]
    ref, test = gstpeaq_amd.synth_fill(ctx, 700, 2, 2, n)
    nb = gstpeaq_amd.frame_count(n, n, True)
    assert nb == 1000
    d_bands = torch.full((2, nb, 2, len(names), NB), SENTINEL, dtype=torch.float64, device="cuda")
    out = gstpeaq_amd.batch_fb_bands(ctx, ref, test, names, d_bands=d_bands)
    assert ctx.last_timing()["fb_launches"] == 2, ctx.last_timing()
    assert not bool((d_bands == SENTINEL).any())
    for p in range(2):
        exp = recipe({k: out[k][p] for k in INPUTS})
        for name in ("adapt_ref", "adapt_test"):
            np.testing.assert_allclose(out[name][p], exp[name], rtol=1e-9, atol=0, err_msg=f"pair {p} {name}")
        for name in ("mod_ref", "mod_test"):
            np.testing.assert_allclose(out[name][p], exp[name], rtol=1e-7, atol=1e-12, err_msg=f"pair {p} {name}")
    plain = gstpeaq_amd.batch_run(ctx, 1, ref, test, sync=False)
    again = gstpeaq_amd.batch_fb_bands(ctx, ref, test, names, sync=False)
    torch.cuda.synchronize()
    assert plain.cpu().numpy().tobytes() == out["d_results"].cpu().numpy().tobytes()
    for k in ("d_bands", "d_results"):
        assert again[k].cpu().numpy().tobytes() == out[k].cpu().numpy().tobytes(), k


# ---- 7: results and leakage ----------------------------------------------------------------------------------------------------
@gpu_test
def test_results_are_batch_run_s_and_nothing_leaks_into_a_later_run(gpu, fir_mode):
    """d_results of a band run are peaq_batch_run's bytes, and a batch_run after a band run returns the bytes it returns on
    a fresh context, in both FIR modes; on the default engine (whose filter bank gives two runs the same bits) the
    records of a batch_trace and the rows of a batch_bands after a band run are those of a fresh context too"""
    import gstpeaq_amd
    import torch
    ref, test, n_ref, n_test = to_device(pairs_of(2))
    ctx = gpu.ctx()
    fresh_ctx = gstpeaq_amd.Context(0)
    if gpu.mode() != "default":
        fresh_ctx.set_fir_mode(gpu.mode())
    f_run = gstpeaq_amd.batch_run(fresh_ctx, 1, ref, test, n_ref, n_test, sync=False)
    first = gstpeaq_amd.batch_fb_bands(ctx, ref, test, ALL, n_ref, n_test, sync=False)
    after = gstpeaq_amd.batch_run(ctx, 1, ref, test, n_ref, n_test, sync=False)
    torch.cuda.synchronize()
    assert first["d_results"].cpu().numpy().tobytes() == f_run.cpu().numpy().tobytes()
    assert after.cpu().numpy().tobytes() == f_run.cpu().numpy().tobytes()
    if gpu.mode() == "default":
        f_trace = gstpeaq_amd.batch_trace(fresh_ctx, 1, ref, test, n_ref, n_test, sync=False)
        f_bands = gstpeaq_amd.batch_bands(fresh_ctx, 1, ref, test, 3, n_ref, n_test, sync=False)
        gstpeaq_amd.batch_fb_bands(ctx, ref, test, ALL, n_ref, n_test, sync=False)
        trace = gstpeaq_amd.batch_trace(ctx, 1, ref, test, n_ref, n_test, sync=False)
        gstpeaq_amd.batch_fb_bands(ctx, ref, test, ALL, n_ref, n_test, sync=False)
        bands = gstpeaq_amd.batch_bands(ctx, 1, ref, test, 3, n_ref, n_test, sync=False)
        torch.cuda.synchronize()
        for k in ("d_frames", "d_blocks", "d_results"):
            assert trace[k].cpu().numpy().tobytes() == f_trace[k].cpu().numpy().tobytes(), k
        for k in ("d_bands", "d_results"):
            assert bands[k].cpu().numpy().tobytes() == f_bands[k].cpu().numpy().tobytes(), k
    fresh_ctx.close()


# ---- 8: host entry and CLI -------------------------------------------------------------------------------------------------------
@gpu_test
def test_host_memory_entry_equals_the_batch_entry(gpu):
    import gstpeaq_amd
    r, t = pairs_of(2)[2]
    host = gstpeaq_amd.run_pair_fb_bands(gpu.ctx(), r, t, ALL)
    every, _ = run(gpu, 2, ALL)
    nb = counts_of(2)[2]
    for name in NAMES:
        assert host[name].shape == (nb, 2, NB)
        assert host[name].tobytes() == every[name][2, :nb].tobytes(), name
    for key in ("movs", "di", "odg", "totalsnr", "frames", "fb_blocks"):
        np.testing.assert_array_equal(host["result"][key], every["results"][2][key])


@gpu_test
@pytest.mark.parametrize("planes", [None, "lindist,moddiff,mod_test"])
def test_cli_fb_bands(gpu, planes, tmp_path):
    """`peaq --advanced --fb-bands=FILE[:PLANES]`: the CSV rows parse back to the doubles of run_pair_fb_bands (%.17g),
    one line per (block, channel, plane) in the order of the slots, the header carries the centre frequencies, the
    printed lines are those printed without the flag; the default plane is noiseloud"""
    import gstpeaq_amd
    r, t = pairs_of(2)[2]
    write_wav(tmp_path / "ref.wav", r, bits=32, fmt_float=True)
    write_wav(tmp_path / "test.wav", t, bits=32, fmt_float=True)
    csv = tmp_path / "fb_bands.csv"
    plain = subprocess.run([str(gst_env.CLI), "--advanced", tmp_path / "ref.wav", tmp_path / "test.wav"],
                           capture_output=True, text=True, timeout=300)
    out = subprocess.run([str(gst_env.CLI), "--advanced", f"--fb-bands={csv}" + (f":{planes}" if planes else ""),
                          tmp_path / "ref.wav", tmp_path / "test.wav"], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and out.returncode == 0, (plain.stderr, out.stderr, out.stdout)
    assert out.stdout == plain.stdout and "Objective Difference Grade" in out.stdout
    names = [n for n in NAMES if n in (planes.split(",") if planes else ["noiseloud"])]
    exp = gstpeaq_amd.run_pair_fb_bands(gpu.ctx(), r, t, names)
    nb = counts_of(2)[2]
    lines = csv.read_text().strip().splitlines()
    header = lines[0].split(",")
    assert header[:3] == ["block", "channel", "plane"] and len(header) == 3 + NB
    assert np.array([float(v) for v in header[3:]]).tobytes() == exp["fc"].tobytes()
    rows = [ln.split(",") for ln in lines[1:]]
    assert len(rows) == nb * 2 * len(names) and all(len(row) == 3 + NB for row in rows)
    it = iter(rows)
    for b in range(nb):
        for c in range(2):
            for name in names:
                row = next(it)
                assert (int(row[0]), int(row[1]), row[2]) == (b, c, name)
                assert np.array([float(v) for v in row[3:]]).tobytes() == exp[name][b, c].tobytes(), row[:3]

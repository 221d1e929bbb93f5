"""Stage parity of the filter-bank ear model (fb_hp_kernel + fb_bank_kernel, gstpeaq_amd/csrc/peaq_fb.hip) over whole
batches: the four input planes of batch_fb_bands (unsmeared and forward-masked excitation of reference and test, per
block, channel and band) and the block records of debug_filterbank against the CPU oracle's block records, on the
populations of tests/fb_stage_cases.py (tests/test_fb_stage_cases_host.py holds those to what they are meant to be):

  P1  every tile tail 1 .. 10 of the bank kernel, signal ends around chunk and block edges, zero-padded flush blocks
  P2  the high-pass walk's waves and workgroups: four full waves and a nearly empty one, empty / one-sample /
      reference-only / short signals at wave edges and inside a wave, a wave of 64 full-length signals, input tensors
      that end with the last pair's last sample, byte-for-byte copies of one pair in three other waves
  P3  the batch path's launch seam at block 840: pairs that end five blocks after it, one after it, on it, one before
  P4  hand-built pairs through debug_filterbank in launches of 320, 11 and 1 blocks (at 1 the window's head spans eight
      earlier launches and the history's move overlaps itself): an impulse, a drop from full scale to 1e-3 of it and
      to digital silence, DC, sines on band centres, playback levels 72 and 112 dB, the slope-filter switch

Every value is compared RELATIVELY (atol = 0: the internal noise is part of every value) at gpu.tol("blocks"): 1e-9 on
the default FP64 engine, 1e-4 on the opt-in f16x3 engine; no NaN anywhere; rows behind a pair's count and a spare pair
keep the sentinel the row array was filled with; the boundary flag (record column 160) is the oracle's exactly.
Needs an MI355X (`-m gpu`).

MEASURED on an MI355X (the largest relative error against the oracle, in the order unsm_ref, unsm_test, exc_ref,
exc_test; the module prints the table at the end of every run; DESIGN.md 30 has it too):
                     default (FP64) engine                    f16x3 engine
  P1 mono     2.3e-14  2.4e-14  2.2e-14  2.4e-14      2.8e-6   1.5e-6   2.2e-6   1.5e-6
  P1 stereo   2.8e-14  3.3e-14  2.7e-14  3.2e-14      3.3e-6   2.2e-6   1.8e-6   1.8e-6
  P2 mono     2.9e-14  3.4e-14  2.9e-14  3.2e-14      3.2e-6   3.5e-6   2.9e-6   3.3e-6
  P2 stereo   3.4e-14  4.3e-14  3.2e-14  4.1e-14      4.6e-6   2.6e-6   4.2e-6   2.5e-6
  P3          7.9e-14  9.9e-14  2.4e-14  2.2e-14      2.7e-6   1.6e-6   9.0e-7   1.2e-6
  P4 impulse  1.9e-14  8.2e-15  6.5e-15  8.0e-15      1.1e-6   1.2e-6   7.7e-7   6.5e-7
  step 1e-3   3.3e-12  2.4e-12  7.0e-13  6.2e-13      1.2e-6   1.4e-6   1.0e-6   4.8e-7
  step 0      1.3e-13  5.6e-14  9.0e-15  1.1e-14      1.1e-6   1.2e-6   1.0e-6   4.8e-7
  dc          3.9e-13  1.1e-13  1.2e-14  8.8e-15      2.4e-5   6.7e-6   1.6e-6   1.5e-6
  sine fc[0]  3.1e-12  1.8e-12  2.6e-12  1.5e-12      3.9e-4   2.2e-4   3.2e-4   1.8e-4    (f16x3: xfail, below)
  sine fc[20] 1.6e-12  8.0e-13  1.5e-12  7.5e-13      1.6e-4   1.1e-4   9.5e-5   7.6e-5    (f16x3: xfail)
  sine fc[39] 3.1e-13  2.8e-13  7.7e-14  7.0e-14      1.6e-4   6.7e-5   1.0e-4   5.6e-5    (f16x3: xfail)
  72 dB       1.1e-14  1.1e-14  5.3e-15  6.7e-15      1.1e-6   1.1e-6   5.4e-7   5.6e-7
  112 dB      1.5e-14  1.9e-14  1.5e-14  1.9e-14      2.2e-6   1.7e-6   1.5e-6   8.7e-7
  swap slope  1.2e-14  1.4e-14  7.6e-15  9.4e-15      1.3e-6   1.3e-6   7.8e-7   1.2e-6
(P4: the largest over launches of 320, 11 and 1 blocks.)  The default engine holds 1e-9 everywhere with more than two
orders of magnitude to spare; no case moved a kernel.

The three pure sines on the f16x3 engine: 416, 11 and 6 of the 12 800 values of a case lie beyond 1e-4, all of them in
channel 0 (the sine) from block 6 on, in bands away from the tone, where the band's own output is what its filter leaks
of the tone: values of 1.3 .. 13, 1.1 .. 11 times the internal noise, while the tone's own band reads 1.8e6 (50 Hz,
behind the high-pass), 1.0e9 and 1.8e5.  The absolute error there is at most 1e-9, 2e-12 and 3e-9 of the tone's band
(in amplitude under 1e-6 of the tone's) -- the rounding of FP32 sums over up to 1456 products of 22..24 bits, the
engine's documented quantisation (tests/test_gpu_fir_modes.py has the same effect at 5e-5 between the harmonics of a
sawtooth).  It is no indexing or scaling fault: the figures are the same to the last digit at 320, 11 and 1 blocks per
launch, the base signal in channel 1 of the same pairs stays below 2e-6, and the default engine -- same windows, tiles,
launches and records -- has 3e-12 on these cases.  They are strict xfails for that engine alone (F16X3_QUANTISATION)."""
import numpy as np
import pytest

import fb_stage_cases as fsc
import oracle_lib as orc

pytestmark = pytest.mark.gpu

NB = 40
PLANES = ["unsm_ref", "unsm_test", "exc_ref", "exc_test"]            # record columns 40 k .. 40 k + 39
FLAG = 160                                                           # kFbRecFlags (peaq_device.h)
SENTINEL = -777.25
WORST = {}          # (mode, population, plane) -> (largest relative error, where); printed at the end
# f16x3 only: hand-built P4 cases beyond 1e-4 whose cause is the engine's documented quantisation (22..24-bit products,
# FP32 sums; the module's docstring has the evidence) -- name -> reason with the measured figure; strict xfail for that
# engine alone, at every launch size
_LEAK = "f16x3: FP32 sums of 22..24-bit products, in bands that only see what leaks of a pure tone 45 .. 85 dB above them: "
F16X3_QUANTISATION = {"sine_fc0": _LEAK + "3.9e-4 measured (416 of 12 800 values beyond 1e-4)",
                      "sine_fc20": _LEAK + "1.6e-4 measured (11 values)",
                      "sine_fc39": _LEAK + "1.6e-4 measured (6 values)"}

_ORACLE, _RUNS = {}, {}


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback in the product)")
    import gpu_common
    yield gpu_common
    print("\nfilter-bank stage parity, largest relative error against the oracle per engine, population and plane:")
    for (mode, pop, plane), (e, where) in sorted(WORST.items()):
        print(f"  {mode:8s} {pop:14s} {plane:10s} {e:9.2e}  {where}")


def note_worst(gpu, pop, plane, err, where):
    key = (gpu.mode(), pop, plane)
    if err >= WORST.get(key, (-1., ""))[0]:
        WORST[key] = (float(err), where)


def population(pop):
    """-> (pairs, the input tensors' stride or None for the longest signal's)"""
    if pop == "p3":
        return fsc.p3_pairs(), None
    kind, ch = pop.split("-")
    ch = dict(mono=1, stereo=2)[ch]
    return (fsc.p1_pairs(ch), None) if kind == "p1" else (fsc.p2_pairs(ch), fsc.P2_FULL)


def oracle_records(pop):
    """the oracle's block records of every pair, [blocks, channels, 168] each; computed once, shared, never changed"""
    if pop not in _ORACLE:
        recs = [orc.fb_records(r, t, orc.count_blocks(len(r), len(t))) for r, t in population(pop)[0]]
        for rec in recs:
            rec.setflags(write=False)
        _ORACLE[pop] = recs
    return _ORACLE[pop]


def run_batch(gpu, pop, again=False):
    """one batch_fb_bands call of the population with the four input planes, into a row array one pair and one block
    larger than needed and full of SENTINEL -> dict(out, whole = the row array as numpy, results = d_results as numpy,
    launches); one run per population and FIR mode (again: a second one), shared by the tests"""
    import torch
    import gstpeaq_amd
    key = (gpu.mode(), pop, again)
    if key not in _RUNS:
        pairs, stride = population(pop)
        ref, test, n_ref, n_test = fsc.packed(pairs, stride)
        ch = ref.shape[2]
        cnt = [orc.count_blocks(len(r), len(t)) for r, t in pairs]
        whole = torch.full((len(pairs) + 1, max(cnt) + 1, ch, len(PLANES), NB), SENTINEL, dtype=torch.float64, device="cuda")
        ctx = gpu.ctx()
        out = gstpeaq_amd.batch_fb_bands(ctx, torch.from_numpy(ref).cuda(), torch.from_numpy(test).cuda(), PLANES, n_ref,
                                         n_test, d_bands=whole[:len(pairs)])
        _RUNS[key] = dict(out=out, whole=whole.cpu().numpy(), results=out["d_results"].cpu().numpy(),
                          launches=ctx.last_timing()["fb_launches"])
    return _RUNS[key]


def compare(gpu, pop, got, want, where):
    """got, want [blocks, channels, 40 k]: no NaN, every value within tol("blocks") of the oracle's, relatively; the
    largest error goes into WORST before anything is asserted"""
    assert got.shape == want.shape, (where, got.shape, want.shape)
    assert not np.isnan(got).any(), (where, np.argwhere(np.isnan(got))[:5].tolist())
    assert (want > 0).all()
    rel = np.abs(got - want) / want
    for k, plane in enumerate(PLANES):
        part = rel[:, :, NB * k:NB * k + NB]
        b, c, band = np.unravel_index(int(np.argmax(part)), part.shape)
        note_worst(gpu, pop, plane, part[b, c, band], f"{where} block {b} channel {c} band {band}")
    b, c, col = np.unravel_index(int(np.argmax(rel)), rel.shape)
    assert rel[b, c, col] <= gpu.tol("blocks"), \
        (f"{where}: {PLANES[col // NB]} block {b} channel {c} band {col % NB}: {got[b, c, col]!r}, the oracle "
         f"{want[b, c, col]!r}, relative error {rel[b, c, col]:.3e}; {(rel > gpu.tol('blocks')).sum()} values beyond the bound")


def check_population(gpu, pop):
    run = run_batch(gpu, pop)
    pairs, _ = population(pop)
    recs = oracle_records(pop)
    cnt = [len(r) for r in recs]
    assert np.array_equal(run["out"]["counts"], cnt)
    whole = run["whole"]
    assert whole.shape == (len(pairs) + 1, max(cnt) + 1, pairs[0][0].shape[1], len(PLANES), NB)
    assert (whole[len(pairs)] == SENTINEL).all(), "the spare pair's rows were written"
    failures = []
    for p, nb in enumerate(cnt):
        assert (whole[p, nb:] == SENTINEL).all(), f"pair {p}: rows behind its {nb} blocks were written"
        if nb == 0:                                   # an empty pair: nothing but sentinels
            continue
        got = whole[p, :nb].reshape(nb, whole.shape[2], len(PLANES) * NB)
        try:
            compare(gpu, pop, got, recs[p][:, :, :len(PLANES) * NB], f"pair {p} ({nb} blocks)")
        except AssertionError as e:                   # every pair is measured before the first failure is raised
            failures.append(str(e))
    assert not failures, f"{len(failures)} of {len(cnt)} pairs: " + " | ".join(failures[:4])
    return run


# ---- P1 .. P3: whole batches through batch_fb_bands ------------------------------------------------------------------
@pytest.mark.parametrize("channels", ["mono", "stereo"])
def test_every_tile_tail_matches_the_oracle(gpu, channels, fir_mode):
    """P1: 40 ragged pairs of 1 .. 39 blocks in one launch -- nvb = 1 .. 10 in the bank kernel's last tile, row_valid at
    every length, signal ends on, before and behind chunk and block edges in the walk's sample-by-sample blocks"""
    run = check_population(gpu, "p1-" + channels)
    assert run["launches"] == 1


@pytest.mark.parametrize("channels", ["mono", "stereo"])
def test_wave_and_workgroup_edges_match_the_oracle(gpu, channels, fir_mode):
    """P2: 258 / 260 signals -- four full waves and the second workgroup's spare-lane wave; empty, one-sample,
    reference-only and short signals beside full ones (the straight-line range [f_lo, f_hi) reduced over the lanes, the
    store rows fetched by shuffle, the loader's row mapping at one and two channels), and input tensors that end with
    the last pair's last sample (the straight-line path loads a chunk ahead)"""
    run = check_population(gpu, "p2-" + channels)
    assert run["launches"] == 1


def test_both_sides_of_the_launch_seam_match_the_oracle(gpu, fir_mode):
    """P3: pairs of 845, 841, 840 and 839 blocks, two launches of 840 and 5 blocks -- the double-buffered rows
    (hp_prev), the peak slots of the launch index, the running sums re-anchored from the history; the second launch has
    5, 1, 0 and 0 blocks of the four pairs"""
    run = check_population(gpu, "p3")
    assert run["launches"] == 2, run["launches"]


@pytest.mark.parametrize("channels", ["mono", "stereo"])
def test_copies_of_a_pair_in_other_waves_give_the_same_rows(gpu, channels, fir_mode):
    """P2's three copies of pair 1 (in waves 2 and 3 and in the second workgroup) get pair 1's rows and results: byte
    for byte on the default engine.  The f16x3 engine's partial sums of a band meet in LDS atomics in the order its
    waves arrive (fir_mfma_h3, peaq_fb.hip), so the same input gives values that differ in the last bits from
    workgroup to workgroup and from run to run: there they are held to gpu.tol("chunks"), the bound of one stream
    computed twice in different launches"""
    run = run_batch(gpu, "p2-" + channels)
    _, _, copies = fsc.p2_layout(dict(mono=1, stereo=2)[channels])
    whole, res = run["whole"], run["results"]
    assert not (whole[1, :12] == SENTINEL).any()
    for p in copies:
        same_or_close(gpu, whole[p], whole[1], res[p], res[1], f"pair {p}")


def same_or_close(gpu, rows, rows0, res, res0, where):
    if gpu.mode() == "default":
        assert rows.tobytes() == rows0.tobytes(), where
        assert res.tobytes() == res0.tobytes(), where
    else:
        assert np.array_equal(rows == SENTINEL, rows0 == SENTINEL), where
        np.testing.assert_allclose(rows, rows0, rtol=gpu.tol("chunks"), atol=0, err_msg=where)
        res, res0 = res.reshape(-1, res.shape[-1]), res0.reshape(-1, res0.shape[-1])
        np.testing.assert_allclose(res[:, :5], res0[:, :5], rtol=gpu.tol("chunks"), atol=1e-12, equal_nan=True, err_msg=where)
        np.testing.assert_allclose(res[:, 11:14], res0[:, 11:14], rtol=gpu.tol("chunks"), atol=1e-9, equal_nan=True, err_msg=where)
        assert np.array_equal(res[:, 14:], res0[:, 14:], equal_nan=True), where       # counts


@pytest.mark.parametrize("channels", ["mono", "stereo"])
def test_a_second_run_returns_the_same_rows_and_results(gpu, channels, fir_mode):
    """P2 twice on one context: the same bytes in d_bands (sentinels included) and d_results on the default engine; on
    the f16x3 engine within gpu.tol("chunks"), for the reason given above"""
    first, second = run_batch(gpu, "p2-" + channels), run_batch(gpu, "p2-" + channels, again=True)
    same_or_close(gpu, second["whole"], first["whole"], second["results"], first["results"], "second run")


# ---- P4: hand-built pairs through debug_filterbank ---------------------------------------------------------------------
@pytest.fixture
def configured(gpu):
    """the shared context and the oracle under a case's settings, both restored afterwards"""
    ctx = gpu.ctx()

    def apply(settings):
        orc.set_settings(**settings)
        ctx.set_settings(**settings)
        return ctx
    yield apply
    orc.set_settings()
    ctx.set_settings()


@pytest.mark.parametrize("bpl", [320, 11, 1])
@pytest.mark.parametrize("name", fsc.P4_NAMES)
def test_hand_built_pairs_match_the_oracle(gpu, configured, request, name, bpl, fir_mode):
    """P4: record columns 0 .. 159 within tol("blocks") of the oracle's, column 160 -- the boundary flag of the
    reference's block -- exactly.  Where the input has loud and silent blocks (the impulse, both step-downs) the
    oracle's flags differ from block to block; the constant 0.25 keeps the flag set in every block (the detector looks
    at the input, five samples of 0.25) while its excitation decays to the noise floor behind the high-pass"""
    import torch
    import gstpeaq_amd
    if gpu.mode() == "f16x3" and name in F16X3_QUANTISATION:
        request.applymarker(pytest.mark.xfail(strict=True, reason=F16X3_QUANTISATION[name]))
    c = fsc.p4_cases(orc.tables(NB)["fc"])[name]
    ctx = configured(c["settings"])
    key = ("p4", name)
    if key not in _ORACLE:
        _ORACLE[key] = orc.fb_records(c["ref"], c["test"], 40, c["level"])
        _ORACLE[key].setflags(write=False)
    want = _ORACLE[key]
    got = gstpeaq_amd.debug_filterbank(ctx, torch.from_numpy(c["ref"]).cuda(), torch.from_numpy(c["test"]).cuda(), 40,
                                       bpl, c["level"])
    assert got.shape == want.shape == (40, 2, 168)
    if name in ("impulse", "step_1e-3", "step_0"):
        assert len(set(want[:, 0, FLAG].tolist())) == 2, want[:, 0, FLAG]
    elif name == "dc":
        assert want[:, 0, FLAG].all()
    assert np.array_equal(got[:, :, FLAG], want[:, :, FLAG]), (got[:, :, FLAG].T, want[:, :, FLAG].T)
    compare(gpu, "p4 " + name, got[:, :, :160], want[:, :, :160], f"{name} at {bpl} blocks per launch")

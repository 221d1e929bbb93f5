"""The HIP back ends on the hand-built records of tests/backend_scenarios.py: every discrete decision between a
record and the result -- the accumulators' INIT / NORMAL / TENTATIVE, frame 24 / block 125, the loudness gate and its
lag of 3 frames / 13 blocks, bw_ref > 346, the 1.5 dB vote, p > 0.5, the energy flags that admit EHS, WinModDiff's
window -- placed on a chosen side of its gate (tests/test_backend_records_host.py holds each scenario to that in the
oracle).  Every scenario runs three ways, through the C ABI:
  1. the debug instantiations' per-frame / per-block values against the trace of the oracle's records back end, with
     the tolerances of tests/test_gpu_backend_stage.py (1e-9; 1e-6 on the cancellation-limited values; atol 1e-12);
  2. the result against the oracle's: frames and NaN places equal, MOVs rtol 1e-7 / atol 1e-9, DI and ODG 1e-6,
     the quotients of small integer sums (RelDistFrames, both bandwidths) rtol 1e-14, ADB's -0.5 and 0 exactly,
     totalsnr 1e-12;
  3. the SHIPPED instantiations (peaq_debug_backend_plain): in one launch the debug instantiation's result bit for
     bit, and cut into launches at every position the scenario names, their own uncut result bit for bit.
Needs an MI355X (`-m gpu`)."""
import numpy as np
import pytest

import backend_scenarios as scn
import oracle_lib as orc

pytestmark = pytest.mark.gpu

BASIC_MOVS = ["BandwidthRefB", "BandwidthTestB", "TotalNMRB", "WinModDiff1B", "ADBB", "EHSB", "AvgModDiff1B",
              "AvgModDiff2B", "RmsNoiseLoudB", "MFPDB", "RelDistFramesB"]
ADV_MOVS = ["RmsModDiffA", "RmsNoiseLoudAsymA", "SegmentalNMRB", "EHSB (55 bands)", "AvgLinDistA"]
WORST = {}          # MOV / DI / ODG / totalsnr -> (largest error over all scenarios, scenario); printed at the end


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback in the product)")
    import gpu_common
    yield gpu_common
    print("\nworst error of the result over the scenarios (relative for the MOVs, absolute for DI, ODG, totalsnr):")
    for k, (e, where) in WORST.items():
        print(f"  {k:20s} {e:9.2e}  {where}")


@pytest.fixture
def configured(gpu):
    """the shared context and the oracle under the scenario's settings, both restored afterwards"""
    ctx = gpu.ctx()

    def apply(notes):
        orc.set_settings(**notes.get("settings", {}))
        ctx.set_settings(**notes.get("settings", {}))
        return ctx
    yield apply
    orc.set_settings()
    ctx.set_settings()


def note_worst(key, err, where):
    if not np.isnan(err) and err >= WORST.get(key, (-1., ""))[0]:
        WORST[key] = (float(err), where)


def same_bits(a, b):
    return all(np.asarray(a[k], dtype=np.float64).tobytes() == np.asarray(b[k], dtype=np.float64).tobytes()
               for k in ("movs", "di", "odg", "totalsnr", "frames", "fb_blocks"))


def compare_result(name, got, exp, mov_names, exact_quotients=(), adb=None):
    n = len(mov_names)
    g, e = got["movs"][:n], exp["movs"][:n]
    assert got["frames"] == exp["frames"]
    for i in range(n):
        assert np.isnan(g[i]) == np.isnan(e[i]), (mov_names[i], g[i], e[i])
    ok = ~np.isnan(e)
    for i in np.flatnonzero(ok):
        note_worst(mov_names[i], abs(g[i] - e[i]) / abs(e[i]) if e[i] != 0. else abs(g[i]), name)
    for k in ("di", "odg"):
        if not np.isnan(exp[k]):
            note_worst(k, abs(got[k] - exp[k]), name)
    if np.isfinite(exp["totalsnr"]):
        note_worst("totalsnr", abs(got["totalsnr"] - exp["totalsnr"]), name)
    np.testing.assert_allclose(g[ok], e[ok], rtol=1e-7, atol=1e-9)
    for k in ("di", "odg"):
        if np.isnan(exp[k]):
            assert np.isnan(got[k]), (k, got[k])
        else:
            assert abs(got[k] - exp[k]) < 1e-6, (k, got[k], exp[k])
    for i in exact_quotients:
        if ok[i]:
            np.testing.assert_allclose(g[i], e[i], rtol=1e-14, atol=0., err_msg=mov_names[i])
    if adb is not None and e[adb] in (-0.5, 0.):
        assert g[adb] == e[adb], (g[adb], e[adb])
    assert abs(got["totalsnr"] - exp["totalsnr"]) <= 1e-12, (got["totalsnr"], exp["totalsnr"])


def cut_lengths(n, positions, fixed):
    """launch lengths that cut the n frames after one frame each, and so that a launch ends on, one before and one
    after each position (a launch of length L ends on frame L - 1), and on each of the fixed frames"""
    lens = {1} | {p + d for p in positions for d in (0, 1, 2)} | {p + 1 for p in fixed}
    return sorted(L for L in lens if 1 <= L < n)


@pytest.mark.parametrize("idx", range(len(scn.basic_scenarios())), ids=[s[0] for s in scn.basic_scenarios()])
def test_basic_back_end_on_the_gates(configured, idx):
    import gstpeaq_amd.capi as capi
    name, rec, notes = scn.basic_scenarios()[idx]
    ctx = configured(notes)
    n = rec.shape[0]
    exp = orc.backend_records(rec)
    d, res = capi.debug_backend(ctx, rec)
    # 1. per-frame values
    for mov in orc.MOV_TRACE:
        got, want = d["mov"][mov], exp["trace"][mov]
        if mov in ("p_detect", "steps"):
            got, want = got[:, :1], want[:, :1]
        rtol = 1e-6 if mov in ("moddiff1", "moddiff2", "nmr_mean", "nmr_max", "noiseloud") else 1e-9
        np.testing.assert_allclose(got, want, rtol=rtol, atol=1e-12, err_msg=f"{name}: {mov}")
    ev = ~np.isnan(exp["gate"])
    assert ev.any()
    np.testing.assert_allclose(d["loudness"][ev], exp["gate"][ev], rtol=1e-9, err_msg=f"{name}: gate loudness")
    # 2. result
    compare_result(name, res, exp, BASIC_MOVS, exact_quotients=(scn.RELDIST, scn.BW_REF, scn.BW_TEST), adb=scn.ADB)
    # 3. the shipped instantiation, whole and cut
    plain = capi.debug_backend_plain(ctx, rec)
    assert same_bits(plain, res), (name, plain, res)
    for L in cut_lengths(n, notes["positions"], (23, 24, 25)):
        cut = capi.debug_backend_plain(ctx, rec, L)
        assert same_bits(cut, plain), (name, L, cut, plain)


@pytest.mark.parametrize("idx", range(len(scn.advanced_scenarios())), ids=[s[0] for s in scn.advanced_scenarios()])
def test_advanced_back_ends_on_the_gates(configured, idx):
    import gstpeaq_amd.capi as capi
    name, fb, ff, notes = scn.advanced_scenarios()[idx]
    ctx = configured(notes)
    n_blocks, n_frames = fb.shape[0], ff.shape[0]
    exp = orc.backend_records_advanced(fb, ff)
    blk, frm, res = capi.debug_backend_advanced(ctx, fb, ff)
    # 1. per-block and per-frame values
    ev = ~np.isnan(exp["gate"][:, 0, 0])             # the blocks on which the oracle evaluated the gate's loudness
    assert ev.any()
    for mov in orc.MOV_TRACE_ADV_BLOCK:
        got, want = blk[mov], exp["trace_blocks"][mov]
        if mov.startswith("loudness"):
            np.testing.assert_allclose(got[ev], want[ev], rtol=1e-9, err_msg=f"{name}: {mov}")
            continue
        rtol = 1e-6 if mov in ("rmsmoddiff", "noiseloud", "missing", "lindist") else 1e-9
        np.testing.assert_allclose(got, want, rtol=rtol, atol=1e-12, err_msg=f"{name}: {mov}")
    for mov in orc.MOV_TRACE_ADV_FRAME:
        np.testing.assert_allclose(frm[mov], exp["trace_frames"][mov], rtol=1e-6, atol=1e-9, err_msg=f"{name}: {mov}")
    # 2. result
    assert res["fb_blocks"] == n_blocks
    compare_result(name, res, exp, ADV_MOVS)
    # 3. the shipped instantiations, whole and cut: the blocks with the frames whole, the frames with the blocks whole,
    # and both into single ones
    plain = capi.debug_backend_plain(ctx, ff, None, fb, None)
    assert same_bits(plain, res), (name, plain, res)
    for L in cut_lengths(n_blocks, notes["block_positions"], (124, 125, 126)):
        cut = capi.debug_backend_plain(ctx, ff, None if L > 1 else 1, fb, L)
        assert same_bits(cut, plain), (name, "blocks", L, cut, plain)
    for L in cut_lengths(n_frames, notes["positions"], ()):
        cut = capi.debug_backend_plain(ctx, ff, L, fb, None)
        assert same_bits(cut, plain), (name, "frames", L, cut, plain)

"""Traces (peaq_batch_run_trace, include/peaq_amd.h): the MOV layer's values of every FFT frame and filter-bank block of
every pair of a batch, before accumulation, with the gates that were open -- pinned here against the CPU oracle's traces
(orc.mov_trace, orc.mov_trace_advanced) at the tolerances of the stage tests (tests/test_gpu_backend_stage.py), the
flags against restatements of the gates, the records against the result of the same call (four MOVs recomputed from
them), across the batch path's launch boundaries, and through the host entry and the CLI.  Needs an MI355X (`-m gpu`)."""
import subprocess

import numpy as np
import pytest

import cases as case_defs
import gst_env
import oracle_lib as orc
from test_conformance_runner import write_wav
from test_gpu_backend_stage import ADV_STAGE_CASES
from test_gpu_trajectory import to_device

pytestmark = pytest.mark.gpu

# the seven cases of test_mov_values_match_oracle_per_frame / test_advanced_mov_values_match_oracle_per_block_and_frame
CASES = ADV_STAGE_CASES
IDS = ["mono", "stereo-ragged", "lead-silence", "quiet", "identical", "saw-triangle", "mid-gaps"]
FILL = 0xA5                                          # what the tests put into the record arrays before a run
ABOVE, MOD_OPEN, LOUD_OPEN, FLUSH = 1, 2, 4, 8
FRAME_NAMES = ["moddiff1", "moddiff2", "tempwt", "noiseloud", "nmr_mean", "nmr_max"]
BLOCK_NAMES = ["rmsmoddiff", "tempwt", "noiseloud", "missing", "lindist"]


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback in the product)")
    import gpu_common
    return gpu_common


_INPUTS, _ORACLE = {}, {}


def inputs_of(channels):
    """[(id, case, ref, test)] of the seven cases with this channel count: one ragged batch"""
    if channels not in _INPUTS:
        _INPUTS[channels] = [(i, c) + tuple(case_defs.make_inputs(c)) for i, c in zip(IDS, CASES)
                             if c.get("channels", 1) == channels]
    return _INPUTS[channels]


def counts(ref, test):
    import gstpeaq_amd
    return gstpeaq_amd.frame_count(len(ref), len(test)), gstpeaq_amd.frame_count(len(ref), len(test), True)


def oracle_trace(name, advanced, ref, test):
    """computed once per case, shared by the tests, never changed (the same for both FIR modes)"""
    key = (name, advanced)
    if key not in _ORACLE:
        nf, nb = counts(ref, test)
        _ORACLE[key] = orc.mov_trace_advanced(ref, test, nb, nf) if advanced else orc.mov_trace(ref, test, nf)
    return _ORACLE[key]


def filled(n_pairs, stride, size):
    import torch
    return torch.full((n_pairs, stride, size), FILL, dtype=torch.uint8, device="cuda")


def trace_batch(gpu, advanced, items, with_fill=True):
    """the items [(id, case, ref, test)] as one ragged batch -> batch_trace's dict; record arrays one record longer than
    the longest pair needs and filled with FILL first"""
    import gstpeaq_amd
    ref, test, n_ref, n_test = to_device([(r, t) for _, _, r, t in items])
    cnt = [counts(r, t) for _, _, r, t in items]
    d_frames = filled(len(items), max(f for f, _ in cnt) + 1, 128) if with_fill else None
    d_blocks = filled(len(items), max(b for _, b in cnt) + 1, 96) if with_fill and advanced else None
    return gstpeaq_amd.batch_trace(gpu.ctx(), advanced, ref, test, n_ref, n_test, d_frames=d_frames, d_blocks=d_blocks)


def assert_untouched_past(records, n, where):
    """the records after a pair's last one still hold the fill pattern"""
    rest = np.ascontiguousarray(records[n:]).view(np.uint8)
    assert rest.size and (rest == FILL).all(), where


# ---- 1, 2: against the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2])
def test_basic_frames_match_the_oracle_trace(gpu, channels):
    """every field of every frame of the seven cases, run as ragged batches (one per channel count), at the tolerances
    of test_mov_values_match_oracle_per_frame: 1e-6 relative on the five cancellation-limited values, 1e-9 on the
    others, 1e-12 absolute, identical signals' noise-to-mask ratios below 1e-9 on both sides"""
    items = inputs_of(channels)
    out = trace_batch(gpu, 0, items)
    assert out["blocks"] is None
    for p, (name, case, ref, test) in enumerate(items):
        nf, _ = counts(ref, test)
        assert out["n_frames"][p] == nf
        rec = out["frames"][p]
        exp = oracle_trace(name, 0, ref, test)
        assert np.array_equal(rec["frame"][:nf], np.arange(nf)), name
        assert (rec["reserved"][:nf] == 0).all(), name
        assert_untouched_past(rec, nf, name)
        if channels == 1:
            assert (rec["ch"][:nf, 1] == 0).all(), name
        for k, field in enumerate(FRAME_NAMES):
            got, want = rec["ch"][:nf, :channels, k], exp[field]
            rtol = 1e-6 if field in ("moddiff1", "moddiff2", "nmr_mean", "nmr_max", "noiseloud") else 1e-9
            if case.get("identical") and field in ("nmr_mean", "nmr_max"):
                assert np.all(np.abs(got) < 1e-9) and np.all(np.abs(want) < 1e-9), (name, field)
                continue
            np.testing.assert_allclose(got, want, rtol=rtol, atol=1e-12, err_msg=f"{name} {field}")
        for field in ("p_detect", "steps"):
            np.testing.assert_allclose(rec[field][:nf], exp[field][:, 0], rtol=1e-9, atol=1e-12, err_msg=f"{name} {field}")


@pytest.mark.parametrize("channels", [1, 2])
def test_advanced_blocks_and_frames_match_the_oracle_trace(gpu, channels, fir_mode):
    """the same for the advanced version, blocks and frames, at the tolerances of
    test_advanced_mov_values_match_oracle_per_block_and_frame, its looser column for the opt-in engine included"""
    items = inputs_of(channels)
    out = trace_batch(gpu, 1, items)
    loose = gpu.mode() != "default"
    for p, (name, case, ref, test) in enumerate(items):
        nf, nb = counts(ref, test)
        assert (out["n_frames"][p], out["n_blocks"][p]) == (nf, nb)
        frm, blk = out["frames"][p], out["blocks"][p]
        eblk, efrm = oracle_trace(name, 1, ref, test)
        assert np.array_equal(frm["frame"][:nf], np.arange(nf)) and np.array_equal(blk["block"][:nb], np.arange(nb)), name
        assert (frm["reserved"][:nf] == 0).all() and (blk["reserved"][:nb] == 0).all(), name
        assert_untouched_past(frm, nf, name)
        assert_untouched_past(blk, nb, name)
        if channels == 1:
            assert (frm["ch"][:nf, 1] == 0).all() and (blk["ch"][:nb, 1] == 0).all(), name
        for k, field in enumerate(BLOCK_NAMES):
            got, want = blk["ch"][:nb, :channels, k], eblk[field]
            rtol = 1e-6 if field in ("rmsmoddiff", "noiseloud", "missing", "lindist") else 1e-9
            if loose:
                rtol = 2e-3
            if case.get("identical") and field in ("rmsmoddiff", "noiseloud", "missing"):
                assert np.all(np.abs(got) < 1e-9) and np.all(np.abs(want) < 1e-9), (name, field)
                continue
            np.testing.assert_allclose(got, want, rtol=rtol, atol=1e-12, err_msg=f"{name} {field}")
        for k, field in enumerate(orc.MOV_TRACE_ADV_FRAME):
            got, want = frm["ch"][:nf, :channels, k], efrm[field]
            if case.get("identical"):
                assert np.all(got < -100) or np.all(np.isinf(got)) or np.allclose(got, want, rtol=1e-6, equal_nan=True), \
                    (name, field)
                continue
            np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-9, err_msg=f"{name} {field}")
        assert (frm["ch"][:nf, :, 2:] == 0).all() and (frm["p_detect"][:nf] == 0).all() and (frm["steps"][:nf] == 0).all()


# ---- 3: flags ------------------------------------------------------------------------------------------------------
THRESHOLD = 200. / 32768


def windows(x, n_units, size, hop):
    """[n_units, size, channels]: unit u is samples [u hop, u hop + size) of x, zeros beyond its end (do_flush)"""
    pad = np.zeros(((n_units - 1) * hop + size, x.shape[1]), dtype=np.float32)
    pad[:len(x)] = x[:len(pad)]
    return np.stack([pad[u * hop: u * hop + size] for u in range(n_units)])


def largest_running_sum(w):
    """is_frame_above_threshold (gstpeaq.c:1081-1099) restated: per unit and channel the largest value the FP32 running
    sum of |x| over 5 samples takes from sample 5 on.  As the C expression `sum += fabs (new) - fabs (old)` evaluates:
    the difference new - old and its sum with the running value are formed in double, the result is rounded to FP32
    once per sample.  All units at once -> [n_units, channels]"""
    a = np.abs(w).astype(np.float64)
    s = np.zeros((w.shape[0], w.shape[2]), dtype=np.float32)
    for i in range(5):
        s = (s.astype(np.float64) + a[:, i]).astype(np.float32)
    best = np.zeros_like(s)
    for i in range(5, w.shape[1]):
        s = (s.astype(np.float64) + (a[:, i] - a[:, i - 5])).astype(np.float32)
        best = np.maximum(best, s)
    return best


def expected_above(ref, n_units, size, hop, where):
    best = largest_running_sum(windows(ref, n_units, size, hop)).max(axis=1)     # any channel, reference only
    assert (np.abs(best / THRESHOLD - 1.) > 1e-3).all(), (where, best[np.abs(best / THRESHOLD - 1.) <= 1e-3])
    return best >= THRESHOLD


def loudness_reached(ref, test, n_units, advanced):
    """gstpeaq.c:841-845: the first frame (block) in which a channel's reference and test loudness both exceed 0.1"""
    size, hop = (192, 192) if advanced else (2048, 1024)
    n = (n_units - 1) * hop + size
    both = np.zeros(n_units, dtype=bool)
    for c in range(ref.shape[1]):
        sig = []
        for x in (ref, test):
            pad = np.zeros(n, dtype=np.float32)
            pad[:min(len(x), n)] = x[:n, c]
            sig.append(orc.fbear(pad, n_units)["loudness"] if advanced else orc.fftear(109, pad, n_units, hop)["loudness"])
        both |= (sig[0] > 0.1) & (sig[1] > 0.1)
    hit = np.flatnonzero(both)
    return int(hit[0]) if hit.size else None


def expected_flags(ref, test, n_units, advanced_blocks, where, gates=True):
    size, hop = (192, 192) if advanced_blocks else (2048, 1024)
    first, lag = (125, 13) if advanced_blocks else (24, 3)
    idx = np.arange(n_units)
    n_min = min(len(ref), len(test))
    full = n_min // 192 if advanced_blocks else ((n_min - 2048) // 1024 + 1 if n_min >= 2048 else 0)
    fl = np.where(expected_above(ref, n_units, size, hop, where), ABOVE, 0) | np.where(idx >= full, FLUSH, 0)
    if gates:
        reached = loudness_reached(ref, test, n_units, advanced_blocks)
        fl |= np.where(idx >= first, MOD_OPEN, 0)
        if reached is not None:
            fl |= np.where((idx >= first) & (idx - lag >= reached), LOUD_OPEN, 0)
    return fl.astype(np.uint32), full


@pytest.mark.parametrize("advanced", [0, 1])
@pytest.mark.parametrize("channels", [1, 2])
def test_flags(gpu, channels, advanced):
    """ABOVE against the detector restated in numpy (after the margin: in no frame or block the largest running sum is
    within 1e-3 of the threshold), MOD_OPEN = frame >= 24 (block >= 125), LOUD_OPEN from the oracle's ear models'
    loudness as gstpeaq.c:841-845,880-881 (996-997) uses it, FLUSH on exactly the record after the full frames; the
    advanced version's frame records carry ABOVE and FLUSH only (include/peaq_amd.h)"""
    items = inputs_of(channels)
    out = trace_batch(gpu, advanced, items)
    not_above = False
    for p, (name, _, ref, test) in enumerate(items):
        nf, nb = counts(ref, test)
        want, full = expected_flags(ref, test, nf, False, (name, "frames"), gates=not advanced)
        np.testing.assert_array_equal(out["frames"][p]["flags"][:nf], want, err_msg=f"{name} frames")
        assert full == nf - 1 and want[-1] & FLUSH and not (want[:-1] & FLUSH).any(), name   # every pair has a remainder
        not_above |= not (want & ABOVE).all()
        if advanced:
            want, full = expected_flags(ref, test, nb, True, (name, "blocks"))
            np.testing.assert_array_equal(out["blocks"][p]["flags"][:nb], want, err_msg=f"{name} blocks")
            assert nb - full in (0, 1) and np.count_nonzero(want & FLUSH) == nb - full, name   # the last record, if there is a remainder
            if nb > full:
                assert want[-1] & FLUSH
    if channels == 2:
        assert not_above                                 # lead-silence, mid-gaps: records that are not ABOVE exist


# ---- 4: closure ----------------------------------------------------------------------------------------------------
def movs_from_trace(v, tempwt_and_diffs_from=24):
    """four MOVs of the basic version from per-frame values v[name] = [frames, channels] (all frames ABOVE):
    TotalNMR (2), RelDistFrames (10), AvgModDiff1 (6), AvgModDiff2 (7)"""
    f0 = tempwt_and_diffs_from
    wt = v["tempwt"][f0:]
    return {2: np.mean(10. * np.log10(v["nmr_mean"].mean(axis=0))),
            10: np.mean((v["nmr_max"] > 10. ** 0.15).mean(axis=0)),
            6: np.mean((wt * v["moddiff1"][f0:]).sum(axis=0) / wt.sum(axis=0)),
            7: np.mean((wt * v["moddiff2"][f0:]).sum(axis=0) / wt.sum(axis=0))}


@pytest.mark.parametrize("name", ["mono", "stereo-ragged"])
def test_the_trace_explains_the_result(gpu, name):
    """for pairs whose frames are all ABOVE four MOVs are plain means of the records: recomputed from the same call's
    records they equal the same call's result at 1e-9 relative -- asserted on the oracle's trace against the oracle's
    result first, so that a failure names the side"""
    case = CASES[IDS.index(name)]
    ref, test = case_defs.make_inputs(case)
    ch = ref.shape[1]
    nf, _ = counts(ref, test)
    o_res = orc.run_pair(0, ref, test)
    o_movs = movs_from_trace(oracle_trace(name, 0, ref, test))
    for i, val in o_movs.items():
        np.testing.assert_allclose(val, o_res["movs"][i], rtol=1e-9, err_msg=f"oracle, MOV {i}")
    out = trace_batch(gpu, 0, [(name, case, ref, test)])
    rec = out["frames"][0][:nf]
    assert (rec["flags"] & ABOVE).all()
    got = movs_from_trace({f: rec["ch"][:, :ch, k] for k, f in enumerate(FRAME_NAMES)})
    for i, val in got.items():
        np.testing.assert_allclose(val, out["results"][0]["movs"][i], rtol=1e-9, err_msg=f"device, MOV {i}")


# ---- 5: seams ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("advanced", [0, 1])
def test_records_across_launch_boundaries(gpu, advanced):
    """256 stereo pairs of 5 s: 234 frames in 4 front-end launches, 1 250 blocks in 2 bank launches (the batch path
    takes a batch's frames in one launch while their records fit 256 MB: at 352 doubles per frame and channel that is
    up to 204 such pairs, so 128 of them would not meet a seam).  The index fields count without gap or repeat, the
    results are peaq_batch_run's bytes, and four pairs' records are bit for bit those of a batch of their own (whose
    frames are one launch)"""
    import gstpeaq_amd
    import torch
    ctx = gpu.ctx()
    n, pairs = 240000, 256
    ref, test = gstpeaq_amd.synth_fill(ctx, 700, pairs, 2, n)
    out = gstpeaq_amd.batch_trace(ctx, advanced, ref, test, sync=False)
    tm = ctx.last_timing()
    assert tm["frontend_launches"] == 4 and tm["backend_launches"] == 4, tm
    if advanced:
        assert tm["fb_launches"] == 2, tm
    torch.cuda.synchronize()
    nf, nb = gstpeaq_amd.frame_count(n, n), gstpeaq_amd.frame_count(n, n, True)
    assert (nf, nb) == (234, 1250)
    frames = out["d_frames"].cpu().numpy().view(gstpeaq_amd.FRAME_TRACE_DTYPE)[:, :, 0]
    assert frames.shape == (pairs, nf) and (frames["frame"] == np.arange(nf)[None, :]).all()
    blocks = None
    if advanced:
        blocks = out["d_blocks"].cpu().numpy().view(gstpeaq_amd.BLOCK_TRACE_DTYPE)[:, :, 0]
        assert blocks.shape == (pairs, nb) and (blocks["block"] == np.arange(nb)[None, :]).all()
    whole = gstpeaq_amd.batch_run(ctx, advanced, ref, test, sync=False)
    torch.cuda.synchronize()
    assert whole.cpu().numpy().tobytes() == out["d_results"].cpu().numpy().tobytes()
    own = [0, 37, 64, 127]
    sub = gstpeaq_amd.batch_trace(ctx, advanced, ref[own].contiguous(), test[own].contiguous(), sync=False)
    assert ctx.last_timing()["frontend_launches"] == 1
    torch.cuda.synchronize()
    assert sub["d_frames"].cpu().numpy().tobytes() == out["d_frames"][own].cpu().numpy().tobytes()
    if advanced:
        assert sub["d_blocks"].cpu().numpy().tobytes() == out["d_blocks"][own].cpu().numpy().tobytes()
    assert sub["d_results"].cpu().numpy().tobytes() == out["d_results"][own].cpu().numpy().tobytes()


# ---- 6: no leakage ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("advanced", [0, 1])
def test_no_leakage_into_a_later_batch(gpu, advanced):
    """a batch_run after a trace on the same context returns the bytes it returns on a fresh context, and a trace is
    bit-identical run to run"""
    import gstpeaq_amd
    import torch
    items = inputs_of(2)
    ref, test, n_ref, n_test = to_device([(r, t) for _, _, r, t in items])
    ctx = gpu.ctx()
    first = gstpeaq_amd.batch_trace(ctx, advanced, ref, test, n_ref, n_test, sync=False)
    after = gstpeaq_amd.batch_run(ctx, advanced, ref, test, n_ref, n_test, sync=False)
    again = gstpeaq_amd.batch_trace(ctx, advanced, ref, test, n_ref, n_test, sync=False)
    fresh_ctx = gstpeaq_amd.Context(0)
    fresh = gstpeaq_amd.batch_run(fresh_ctx, advanced, ref, test, n_ref, n_test, sync=False)
    torch.cuda.synchronize()
    assert after.cpu().numpy().tobytes() == fresh.cpu().numpy().tobytes()
    assert after.cpu().numpy().tobytes() == first["d_results"].cpu().numpy().tobytes()
    for k in ("d_frames", "d_results") + (("d_blocks",) if advanced else ()):
        assert first[k].cpu().numpy().tobytes() == again[k].cpu().numpy().tobytes(), k
    fresh_ctx.close()


# ---- 7: host entry and CLI ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("advanced", [0, 1])
def test_host_memory_entry_equals_the_batch_entry(gpu, advanced):
    import gstpeaq_amd
    case = dict(kind="synth", seed=21, channels=2, n=100000, test_trim=1500)
    r, t = case_defs.make_inputs(case)
    host = gstpeaq_amd.run_pair_trace(gpu.ctx(), advanced, r, t)
    ref, test, n_ref, n_test = to_device([(r, t)])
    dev = gstpeaq_amd.batch_trace(gpu.ctx(), advanced, ref, test, n_ref, n_test)
    nf, nb = counts(r, t)
    assert len(host["frames"]) == nf and host["frames"].tobytes() == dev["frames"][0][:nf].tobytes()
    if advanced:
        assert len(host["blocks"]) == nb and host["blocks"].tobytes() == dev["blocks"][0][:nb].tobytes()
    else:
        assert host["blocks"] is None
    for key in ("movs", "di", "odg", "totalsnr", "frames", "fb_blocks"):
        np.testing.assert_array_equal(host["result"][key], dev["results"][0][key])
    whole = gstpeaq_amd.run_pair(gpu.ctx(), advanced, r, t)
    np.testing.assert_array_equal(host["result"]["movs"], whole["movs"])


@pytest.mark.parametrize("advanced", [0, 1])
def test_cli_trace(gpu, advanced, tmp_path):
    """`peaq --trace=FILE`: the CSV rows parse back to the doubles of run_pair_trace, the printed lines are those
    printed without --trace"""
    import gstpeaq_amd
    r, t = case_defs.make_inputs(dict(kind="synth", seed=22, channels=2, n=60000, ref_trim=700))
    write_wav(tmp_path / "ref.wav", r, bits=32, fmt_float=True)
    write_wav(tmp_path / "test.wav", t, bits=32, fmt_float=True)
    flags = ["--advanced"] if advanced else []
    csv = tmp_path / "trace.csv"
    plain = subprocess.run([str(gst_env.CLI), *flags, tmp_path / "ref.wav", tmp_path / "test.wav"],
                           capture_output=True, text=True, timeout=300)
    out = subprocess.run([str(gst_env.CLI), *flags, f"--trace={csv}", tmp_path / "ref.wav", tmp_path / "test.wav"],
                         capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and out.returncode == 0, (plain.stderr, out.stderr, out.stdout)
    assert out.stdout == plain.stdout and "Objective Difference Grade" in out.stdout
    exp = gstpeaq_amd.run_pair_trace(gpu.ctx(), advanced, r, t)
    lines = csv.read_text().strip().splitlines()
    header = lines[0].split(",")
    assert header[:3] == ["kind", "index", "flags"] and header[-2:] == ["p_detect", "steps"] and len(header) == 17
    rows = [ln.split(",") for ln in lines[1:]]
    assert all(len(row) == 17 for row in rows)
    fr = [row for row in rows if row[0] == "frame"]
    bl = [row for row in rows if row[0] == "block"]
    assert len(fr) == len(exp["frames"]) and len(bl) == (len(exp["blocks"]) if advanced else 0) == len(rows) - len(fr)
    for row, rec in zip(fr, exp["frames"]):
        assert (int(row[1]), int(row[2])) == (rec["frame"], rec["flags"])
        got = np.array([float(v) for v in row[3:]])
        want = np.concatenate([rec["ch"].reshape(-1), [rec["p_detect"], rec["steps"]]])
        assert got.tobytes() == want.tobytes(), row[:3]
    for row, rec in zip(bl, exp["blocks"] if advanced else []):
        assert (int(row[1]), int(row[2])) == (rec["block"], rec["flags"])
        assert row[8] == row[14] == row[15] == row[16] == ""
        got = np.array([float(v) for v in row[3:8] + row[9:14]])
        assert got.tobytes() == rec["ch"].reshape(-1).tobytes(), row[:3]

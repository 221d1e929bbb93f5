"""The steps stage on the device against FP64 numpy (include/peaq_amd.h, "delay steps on the device"):
locate_steps against the statistic restated in numpy (tests/steps_common.py) on stepped pink noise and modulated tones,
cut_pieces bit for bit against cut_track, cut_drift and cut where the header says so and against the numpy sum where
lines jump, and estimate_steps end to end: a pair that the track flags through a 300-sample step alone comes out with
one accepted step at the true position and unflagged, a drift and a bend come out as the track's own segments.

Tolerances.  locate_steps: the header bounds every H by 1.3e-13 sum |h|, and sum |h| <= norm (Cauchy-Schwarz), so the
device and numpy (pairwise sums, better still) agree to far below the 1e-9 norm the comparisons allow; positions are
compared only where the model's margin over every other position exceeds that.  cut_pieces: tests/test_gpu_track.py's,
one FP32 rounding of an FP64 sum of 65 products on both sides.

The fixtures' delay is 37.5 samples before the step for the locator, whose candidates are handed to it.  The
end-to-end fixtures use 37.25: at exactly 37.5 every window's sub-sample estimate sits on the edge of its grid
(PEAQ_SUB_F_EDGE), which the drift stage's validity rule discards, so the track under this stage has no valid window
(tests/test_gpu_track.py notes the same of its own fixtures)."""
import numpy as np
import pytest

import gpu_common
import steps_common as sc
from test_gpu_drift import hiss, resampled
from test_gpu_subsample import SUM_BOUND, cuda, noise, same_bits, same_result
from test_gpu_track import bent_pair

pytestmark = pytest.mark.gpu

W = 4096
N = 48000
MAX_E = 1 / 64
TOL = 1e-9                       # x norm
STEPS = (1, 2, 300, -20, 3000)
PLACES = {"mid": 6 * W + W // 2, "behind a border": 6 * W + 5, "before a border": 7 * W - 3}   # in the pair's coordinates
# |c - true position| of the numpy model itself, measured on the CPU, the largest over both materials and the three
# places: a positive step is found within 3 outputs, the step of 1 within 5 (the half sample between 37.5 and the integer
# hypotheses blurs the edge: with an integer delay the model is exact), a step of -20 within 12, inside the 2 |step| its
# 20 ambiguous outputs allow.  The device is held to the model's own distance case by case.
MODEL_DISTANCE = {1: 5, 2: 2, 300: 3, 3000: 3, -20: 12}


def ctx():
    return gpu_common.ctx("default")


def hypotheses(step, lag0):
    """(LA, LB) around a delay of 37.5 that steps: the nearest integers, for +1 the two outer ones (38 would fit both sides)"""
    la, lb = (37, 39) if step == 1 else (38, 38 + step)
    return la - lag0, lb - lag0


def located_cases():
    """(kind, lag0, step, place, ref, test, candidate row without the pair, true c) for every material, step and place"""
    out = []
    for kind, lag0 in (("pink", 0), ("tones", 30)):
        ref = sc.material(kind, N, 2, 5)
        for step in STEPS:
            for place, c0 in PLACES.items():
                LA, LB = hypotheses(step, lag0)
                at = c0 + lag0 + LA                      # the test position where the step is: output c0 reads it first
                test = sc.stepped(ref, step, at)
                k = (c0 - W // 2) // W                   # the segment whose own outputs hold c0
                out.append((kind, lag0, step, place, ref.astype(np.float32), test.astype(np.float32), (k * W, (k + 2) * W, LA, LB), c0))
    return out


@pytest.fixture(scope="module")
def located():
    import gstpeaq_amd
    cases = located_cases()
    R = np.stack([c[4] for c in cases])
    T = np.stack([c[5] for c in cases])
    lags = np.array([c[1] for c in cases], np.int32)
    cand = [(p,) + c[6] for p, c in enumerate(cases)]
    d_ref, d_test = cuda(R), cuda(T)
    got = gstpeaq_amd.locate_steps(ctx(), d_ref, d_test, lags, cand)
    again = gstpeaq_amd.locate_steps(ctx(), d_ref, d_test, lags, cand)
    models = [sc.locate_model(c[4], c[5], c[1], *c[6]) for c in cases]
    return cases, cand, (d_ref, d_test, lags), got, again, models


def check_record(rec, model, cand, what):
    """one device record against the model of its candidate (the header's comparisons)"""
    lo, hi, LA, LB = cand
    norm = model["norm"]
    assert (rec["LA"], rec["LB"]) == (LA, LB) and lo <= rec["c"] <= hi, (what, rec)
    assert rec["flags"] == model["flags"], (what, rec, model["flags"])
    assert abs(rec["norm"] - norm) <= TOL * norm, (what, rec["norm"], norm)
    sH = model["sH"]
    best = float(sH.max())
    assert best - sH[rec["c"] - lo] <= TOL * norm, (what, rec["c"], model["c"], best - sH[rec["c"] - lo], norm)
    assert abs(rec["gain_left"] - model["gain_left"]) <= TOL * norm and abs(rec["gain_right"] - model["gain_right"]) <= TOL * norm, \
        (what, rec, model["gain_left"], model["gain_right"])
    others = np.delete(sH, model["c"] - lo)
    margin = best - float(others.max())
    if margin > TOL * norm:
        assert rec["c"] == model["c"], (what, rec["c"], model["c"], margin / norm)
    return margin > TOL * norm


# ---- (a) locate -------------------------------------------------------------------------------------------------------
def test_located_steps_are_the_models_and_at_the_true_position(located):
    import gstpeaq_amd
    cases, cand, _, got, _, models = located
    exact = 0
    for p, (kind, lag0, step, place, _, _, cd, c0) in enumerate(cases):
        what = (kind, step, place)
        exact += check_record(got[p], models[p], cd, what)
        assert got[p]["pair"] == p and got[p]["flags"] == 0
        d_model, d_dev = abs(models[p]["c"] - c0), abs(int(got[p]["c"]) - c0)
        print(what, "c", got[p]["c"], "model", models[p]["c"], "true", c0, "min gain / norm",
              min(got[p]["gain_left"], got[p]["gain_right"]) / got[p]["norm"])
        assert d_model <= MODEL_DISTANCE[step], (what, d_model)          # the model is where it was measured to be
        assert d_dev <= d_model or d_dev <= (0 if step > 0 else 2 * abs(step)), (what, d_dev, d_model)
        if step < 0:
            assert d_dev <= 2 * abs(step), (what, d_dev)
        # every true step is accepted by the default min_gain
        assert min(got[p]["gain_left"], got[p]["gain_right"]) >= gstpeaq_amd.STEP_MIN_GAIN * got[p]["norm"], (what, got[p])
    assert exact >= len(cases) - 3, exact                # (nearly every arg-max is clear of its runner-up)


def test_records_repeat_and_do_not_depend_on_the_other_candidates(located):
    import gstpeaq_amd
    cases, cand, (d_ref, d_test, lags), got, again, _ = located
    assert got.tobytes() == again.tobytes()
    pick = [3, 17, 28]
    extra = [(cand[3][0], 100, 100 + 5000, -4, 9)]       # another candidate on pair 3, a span that is no multiple of a chunk
    some = gstpeaq_amd.locate_steps(ctx(), d_ref, d_test, lags, [cand[p] for p in pick] + extra)
    for j, p in enumerate(pick):
        assert some[j].tobytes() == got[p].tobytes(), (p, some[j], got[p])
    # ... nor on where the buffers lie, nor on the batch: the pair alone, elsewhere
    import torch
    spacer = torch.zeros(4321, device="cuda")
    for p in pick:
        alone = gstpeaq_amd.locate_steps(ctx(), cuda(cases[p][4][None]), cuda(cases[p][5][None]), lags[p:p + 1], [(0,) + cases[p][6]])
        want = got[p].copy()
        want["pair"] = 0
        assert alone[0].tobytes() == want.tobytes(), (p, alone[0], got[p])
    del spacer


def test_a_pair_without_a_step_is_rejected_by_the_default_min_gain():
    import gstpeaq_amd
    rows, pairs = [], []
    for kind, lag0 in (("pink", 0), ("tones", 30)):
        ref = sc.material(kind, N, 2, 5)
        test = sc.stepped(ref, 0, 0)
        pairs.append((ref.astype(np.float32), test.astype(np.float32), lag0))
        for step in STEPS:
            for k in (3, 6):
                rows.append((len(pairs) - 1, k * W, (k + 2) * W) + hypotheses(step, lag0))
    lags = np.array([p[2] for p in pairs], np.int32)
    got = gstpeaq_amd.locate_steps(ctx(), cuda(np.stack([p[0] for p in pairs])), cuda(np.stack([p[1] for p in pairs])), lags, rows)
    worst = 0.0
    for rec, row in zip(got, rows):
        r, t, lag0 = pairs[row[0]]
        check_record(rec, sc.locate_model(r, t, lag0, *row[1:]), row[1:], row)
        worst = max(worst, min(rec["gain_left"], rec["gain_right"]) / rec["norm"])
        assert min(rec["gain_left"], rec["gain_right"]) < gstpeaq_amd.STEP_MIN_GAIN * rec["norm"], (row, rec)
    print("largest min gain / norm of a control:", worst)


def test_polarity_mono_the_signals_end_silence_and_nan():
    import gstpeaq_amd
    ref = sc.material("pink", N, 1, 8)
    c0 = 5 * W + 777
    test = sc.stepped(ref, 300, c0 + 38)
    r32, t32 = ref.astype(np.float32), test.astype(np.float32)
    rows = [(0, 4 * W, 6 * W, 38, 338),                  # mono
            (1, 4 * W, 6 * W, 38, 338),                  # the test signal inverted: the same position, s = -1
            (0, 5 * W, N - 38, 38, 338),                 # hi = n_common with LB = 338: the reads pass the signal's end; odd span
            (0, N - 3100, N - 38, 38, 3038),             # every t[i + LB] lies behind the end
            (2, 4 * W, 6 * W, 38, 338),                  # a silent reference in the interval
            (3, 4 * W, 6 * W, 38, 338),                  # a NaN in the interval
            (3, 0, 2 * W, 38, 338)]                      # ... and the same pair where there is none
    quiet, nan = r32.copy(), t32.copy()
    quiet[4 * W:6 * W] = 0
    nan[5 * W + 50] = np.nan
    R = np.stack([r32, r32, quiet, r32])
    T = np.stack([t32, -t32, t32, nan])
    lags = np.zeros(4, np.int32)
    got = gstpeaq_amd.locate_steps(ctx(), cuda(R), cuda(T), lags, rows)
    models = [sc.locate_model(R[row[0]], T[row[0]], 0, *row[1:]) for row in rows]
    for j in (0, 1, 2, 3, 6):
        check_record(got[j], models[j], rows[j][1:], rows[j])
    assert models[0]["s"] == 1 and models[1]["s"] == -1
    assert got[0]["c"] == got[1]["c"]
    for j in (0, 1, 2):
        assert abs(int(got[j]["c"]) - c0) <= abs(models[j]["c"] - c0) <= MODEL_DISTANCE[300], (j, got[j]["c"], models[j]["c"], c0)
    assert got[0]["gain_left"] == got[1]["gain_left"] and got[0]["gain_right"] == got[1]["gain_right"] and got[0]["norm"] == got[1]["norm"]
    for j in (4, 5):
        assert got[j]["flags"] == gstpeaq_amd.STEP_F_NONE and got[j]["c"] == rows[j][1], got[j]
        assert got[j]["gain_left"] == 0 and got[j]["gain_right"] == 0
    assert got[4]["norm"] == 0 and np.isnan(got[5]["norm"])


def test_the_longest_span_is_searched_and_a_longer_one_is_not():
    """one mono pair of 2^22 + 4100 samples: a candidate of exactly PEAQ_STEP_MAX_SPAN (1024 chunks, the step in chunk 700)
    against the model, and one of a sample more, which is flagged PEAQ_STEP_F_SPAN"""
    import gstpeaq_amd
    n = (1 << 22) + 4100
    rng = np.random.default_rng(77)
    r = rng.standard_normal((n, 1)).astype(np.float32)
    c0 = 700 * 4096 + 1234
    t = np.zeros_like(r)
    t[3:c0 + 3] = r[:c0]
    t[c0 + 10:] = r[c0:n - 10]
    rows = [(0, 100, 100 + (1 << 22), 3, 10), (0, 99, 100 + (1 << 22), 3, 10), (0, 4096, 8192, 3, 10)]
    got = gstpeaq_amd.locate_steps(ctx(), cuda(r[None]), cuda(t[None]), np.zeros(1, np.int32), rows)
    check_record(got[0], sc.locate_model(r, t, 0, *rows[0][1:]), rows[0][1:], "2^22")
    assert got[0]["c"] == c0 and got[0]["flags"] == 0
    assert got[1]["flags"] == gstpeaq_amd.STEP_F_SPAN and got[1]["c"] == 99 and got[1]["norm"] == 0 and got[1]["gain_left"] == 0
    check_record(got[2], sc.locate_model(r, t, 0, *rows[2][1:]), rows[2][1:], "beside it")


# ---- (b) cut ----------------------------------------------------------------------------------------------------------
def test_pieces_equal_to_a_tracks_segments_are_bit_for_bit_cut_track():
    """tests/test_gpu_track.py's three pairs of 3, 2 and 1 segments at window 5001, slopes of +-1/64 among them, and a
    one-piece pair against cut_drift"""
    import gstpeaq_amd
    import torch
    from test_gpu_track import SUM_WINDOW, segments, sum_cases
    for channels in (1, 2):
        rng = np.random.default_rng(90 + channels)
        cases = sum_cases()
        n = len(cases) + 1
        a, e, b = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3), np.uint32)
        n_seg = np.ones(n, np.uint32)
        for p, (knots, _, _, _) in enumerate(cases):
            sa, se = segments(knots, SUM_WINDOW)
            a[p, :len(sa)], e[p, :len(se)], n_seg[p] = sa, se, len(sa)
            b[p, :len(sa)] = [sc.start_of(k, SUM_WINDOW) for k in range(len(sa))]
        a[n - 1, 0], e[n - 1, 0] = 17.5, -1e-3             # one piece: cut_drift's line
        skip = np.array([c[1] for c in cases] + [3], np.uint32)
        keep = np.array([c[2] for c in cases] + [5000], np.uint32)
        n_in = (skip + keep + np.array([400, 250, 9, 30])).astype(np.uint32)
        x = rng.standard_normal((n, int(n_in.max()) + 1, channels)).astype(np.float32)
        outs = [torch.full((n, int(keep.max()) + 3, channels), -77.25, dtype=torch.float32, device="cuda") for _ in (0, 1, 2)]
        gstpeaq_amd.cut_track(ctx(), cuda(x), skip, keep, SUM_WINDOW, n_seg, a, e, n_in=n_in, out=outs[0])
        gstpeaq_amd.cut_pieces(ctx(), cuda(x), skip, keep, n_seg, b, a, e, n_in=n_in, out=outs[1])
        gstpeaq_amd.cut_drift(ctx(), cuda(x[3:]), skip[3:], keep[3:], a[3:, 0], e[3:, 0], n_in=n_in[3:], out=outs[2][3:])
        torch.cuda.synchronize()
        want, got, line = (o.cpu().numpy() for o in outs)
        for p in range(n):
            assert same_bits(got[p], want[p]), (channels, p, int(np.argmax(got[p].view(np.uint32) != want[p].view(np.uint32))))
            assert (got[p, keep[p]:] == np.float32(-77.25)).all(), p
        assert same_bits(got[n - 1], line[n - 1])        # one piece is cut_drift's line


def test_zero_pieces_move_nan_payloads():
    import gstpeaq_amd
    import torch
    rng = np.random.default_rng(13)
    keeps = np.array([3 * 1024 + 37, 1025, 63], np.uint32)
    bits = rng.integers(0, 2 ** 32, size=(3, int(keeps.max()) + 40, 2), dtype=np.uint32)
    bits[:, ::7] = 0x7FC12345
    x = bits.view(np.float32)
    skip = np.array([0, 1, 33], np.uint32)
    outs = [torch.full((3, int(keeps.max()) + 2, 2), -3.5, dtype=torch.float32, device="cuda") for _ in (0, 1)]
    gstpeaq_amd.cut(ctx(), cuda(x), skip, keeps, out=outs[0])
    zeros = np.zeros((3, 3))
    zeros[1, 1] = -0.0
    b = np.array([[0, 500, 2000], [0, 1, 0], [0, 0, 0]], np.uint32)
    # (n_in of 5: a pair that is moved does not look at it)
    gstpeaq_amd.cut_pieces(ctx(), cuda(x), skip, keeps, [3, 2, 1], b, zeros, zeros.copy(), n_in=[5, 5, 5], out=outs[1])
    torch.cuda.synchronize()
    assert same_bits(outs[0].cpu().numpy(), outs[1].cpu().numpy())


def jump_cases():
    """(b, a, e, skip, n_keep, tail): n_in = skip + n_keep + (m of the last output) + tail.
    Pair 0: a breakpoint at a tile border (1024) and in the middle of a tile (1500); three pieces inside one tile (2100,
    2101, 2106: pieces of 1, 5 and 300 outputs); jumps of +5000 and -5000; a piece at 1/64 beside one at -1/64.
    Pair 1: a first piece that reads before the signal's start (a = -59 at skip 0) and a breakpoint three outputs before
    the pair's end.  Pair 2: one piece, the signal ending inside the last outputs' taps.  Pair 3: one output short of a
    tile, breakpoints at 1 and at n_keep - 1.  Pair 4: nothing kept, beside the long pairs."""
    return [([0, 1024, 1500, 2100, 2101, 2106, 2406, 4000], [0.3, 5000.25, 0.75, -4999.5, 17.5, -3.75, 90.25, 26.25],
             [1e-3, -1e-3, 3.73e-5, 0.0, 0.0, MAX_E, MAX_E, -MAX_E], 5200, 6003, 22),
            ([0, 700, 2997], [-59.0, 12.5, 4000.0], [MAX_E, -MAX_E, 0.0], 0, 3000, 22),
            ([0], [0.3], [1e-3], 7, 2997, 9),
            ([0, 1, 1022], [0.3, 7.25, -2.5], [1e-3, 0.0, -MAX_E], 40, 1023, 22),
            ([0], [0.3], [1e-3], 40, 0, 22)]


@pytest.mark.parametrize("channels", [1, 2])
def test_cut_pieces_against_the_numpy_sum(channels):
    """every sample compared, the sentinel behind n_keep kept; the kernel's staged index, restated in numpy, stays inside
    0 .. 17 for every output"""
    import gstpeaq_amd
    import torch
    rng = np.random.default_rng(160 + channels)
    cases = jump_cases()
    n = len(cases)
    width = max(len(c[0]) for c in cases)
    b, a, e = np.zeros((n, width), np.uint32), np.zeros((n, width)), np.zeros((n, width))
    n_pc = np.zeros(n, np.uint32)
    for p, (pb, pa, pe, _, _, _) in enumerate(cases):
        b[p, :len(pb)], a[p, :len(pa)], e[p, :len(pe)], n_pc[p] = pb, pa, pe, len(pb)
    skip = np.array([c[3] for c in cases], np.uint32)
    keep = np.array([c[4] for c in cases], np.uint32)
    last_m = [int(sc.pieces_indices(b[p, :n_pc[p]], a[p, :n_pc[p]], e[p, :n_pc[p]], np.array([max(int(keep[p]), 1) - 1]))[0][0]) for p in range(n)]
    n_in = np.array([int(skip[p]) + int(keep[p]) + last_m[p] + cases[p][5] for p in range(n)], np.uint32)
    n_in[1] = 3000 + 2000                               # pair 1: its last piece, 4000 ahead, reads past the end
    x = rng.standard_normal((n, max(int(n_in.max()), int((skip + keep).max())) + 1, channels)).astype(np.float32)
    sentinel = np.float32(-77.25)
    out = torch.full((n, int(keep.max()) + 3, channels), float(sentinel), dtype=torch.float32, device="cuda")
    gstpeaq_amd.cut_pieces(ctx(), cuda(x), skip, keep, n_pc, b, a, e, n_in=n_in, out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    worst = 0.0
    for p in range(n):
        k = int(keep[p])
        if k == 0:
            assert (got[p] == sentinel).all(), p                                    # nothing kept: the sentinel stays
            continue
        pb, pa, pe = b[p, :n_pc[p]], a[p, :n_pc[p]], e[p, :n_pc[p]]
        want, m, phi, piece = sc.pieces_model(x[p], int(n_in[p]), int(skip[p]), k, pb, pa, pe)
        assert set(piece) == set(range(n_pc[p])), (p, set(piece))                   # every piece is met
        dm = sc.staged_offsets(pb, pa, pe, k)
        assert dm.min() == 0 and dm.max() < sc.SPREAD - 2, (p, dm.min(), dm.max())   # the kernel's clamp never acts
        s = int(skip[p]) + np.arange(k) + m
        if p == 0:
            d = np.diff(s)
            assert d.max() > 4900 and d.min() < -4900 and (s - sc.K).min() >= 0      # jumps both ways, none before the start
        if p == 1:
            assert s.min() < 0 and (s[-3:] - sc.K > int(n_in[p])).all()              # before the start; wholly past the end
            assert not want[-3:].any()
        if p == 2:
            assert (s + sc.K).max() >= int(n_in[p]) > s.max()                        # the signal ends inside the last taps
        tol = 2.0 ** -23 * np.abs(want) + SUM_BOUND * np.abs(x[p]).max() + 1.5e-45
        err = np.abs(got[p, :k].astype(np.float64) - want)
        assert (err <= tol).all(), (p, float((err / tol).max()), int(np.argmax((err / tol).max(axis=1))))
        worst = max(worst, float((err / tol).max()))
        assert (got[p, k:] == sentinel).all(), p
    print("channels", channels, "worst error / tolerance:", worst)


# ---- (c) end to end ---------------------------------------------------------------------------------------------------
E2E_OFFSET, E2E_LAG0, E2E_N = 37.25, 37, 2 * 48000


def stepped_pair(step=300, c0=6 * W + W // 2):
    """2 s of stereo pink noise late by 37.25 samples and, from output c0 of the pair aligned at 37 on, by `step` more"""
    ref = sc.material("pink", E2E_N, 2, 5)
    test = sc.stepped(ref, step, c0 + E2E_LAG0, offset=E2E_OFFSET)
    return ref.astype(np.float32), test.astype(np.float32), c0


def test_a_step_that_flags_the_track_is_located_and_the_pair_comes_out_unflagged():
    """The numpy model (tests/test_gpu_drift.py's stage_model, peaq_track_fit, the restatement of the candidates and the
    locator), measured on the CPU: the track is PEAQ_TRACK_F_RANGE with knots 0.25 .. 0.25, 300.25 .. 300.25, one candidate
    (segment 6, 24576 .. 32768, LA 0, LB 300), located one output behind the true position (the inserted noise's first
    sample happens to correlate), min gain / norm 0.147"""
    import gstpeaq_amd
    import torch
    ref, test, c0 = stepped_pair()
    d_ref, d_test = cuda(ref[None]), cuda(test[None])
    lags = np.array([E2E_LAG0], np.int32)
    tr = gstpeaq_amd.estimate_track(ctx(), d_ref, d_test, lags, window=W)
    assert tr["flags"][0] == gstpeaq_amd.TRACK_F_RANGE and not tr["a"].any()
    got = gstpeaq_amd.estimate_steps(ctx(), d_ref, d_test, lags, window=W)
    for k in gstpeaq_amd.TRACK_DTYPE.names:
        assert got["track"][k].tobytes() == tr[k].tobytes(), k
    assert got["knots"].tobytes() == tr["knots"].tobytes()
    assert got["n_candidates"][0] == 1 and got["n_accepted"][0] == 1 and got["flags"][0] == 0, got
    step = got["steps"][0, 0]
    print("step", step, "pieces", got["b"][0], got["a"][0], got["e"][0])
    assert (step["LA"], step["LB"], step["flags"]) == (0, 300, 0), step
    model = sc.locate_model(ref, test, E2E_LAG0, 6 * W, 8 * W, 0, 300)
    check_record(step, model, (6 * W, 8 * W, 0, 300), "end to end")
    c = int(step["c"])                                   # (the model's own: one output behind c0 on this fixture)
    assert abs(c - c0) <= abs(model["c"] - c0) <= MODEL_DISTANCE[300], (c, model["c"], c0)
    n_pc = int(got["n_pieces"][0])
    assert n_pc == tr["n_segments"][0] + 1 and c in got["b"][0, :n_pc] and got["max_abs_e"][0] < 1e-4
    j = list(got["b"][0, :n_pc]).index(c)
    # every piece's line, taken where the piece starts (a is the line's offset at output 0, not its height there)
    at_start = got["a"][0, :n_pc] + got["e"][0, :n_pc] * got["b"][0, :n_pc]
    assert np.abs(at_start[:j] - 0.25).max() < 0.02 and np.abs(at_start[j:] - 300.25).max() < 0.02, at_start
    # the cut along the pieces follows the reference on both sides of the step; the plain cut loses it behind the step
    sr, st, keep = gstpeaq_amd.pieces_lengths(E2E_LAG0, got["b"][0, :n_pc], got["a"][0, :n_pc], got["e"][0, :n_pc], E2E_N, E2E_N)
    out = gstpeaq_amd.cut_pieces(ctx(), d_test, [st], [keep], [n_pc], got["b"], got["a"], got["e"])
    torch.cuda.synchronize()
    y = out.cpu().numpy()[0, :keep].astype(np.float64)
    for lo, hi in ((1000, c0 - 100), (c0 + 100, keep - 1000)):
        resid = y[lo:hi] - ref[sr + lo:sr + hi]
        assert resid.std() < 0.02 * ref[sr + lo:sr + hi].std(), (lo, hi, resid.std())
    # the keyword paths: batch_run and run_pair are the stages one by one
    a = gstpeaq_amd.cut(ctx(), d_ref, [sr], [keep])
    want = gstpeaq_amd.batch_run(ctx(), 0, a, out, [keep], [keep])[0]
    one = gstpeaq_amd.run_pair(ctx(), 0, ref, test, align=4096, steps=W)
    lag = one["delay"]["lag"]
    print("lag", lag, "ODG along the pieces", one["odg"], "stages", want["odg"], one["pieces"], one["steps"])
    assert one["pieces"]["n_accepted"] == 1 and one["pieces"]["flags"] == 0 and one["track"]["flags"] == gstpeaq_amd.TRACK_F_RANGE
    # (whichever side the lag is taken from, lag + LA is 37 and the step is at output c0; the model was measured at 37)
    assert abs(int(one["steps"][0]["c"]) - c0) <= MODEL_DISTANCE[300], (one["steps"], lag)
    batch = gstpeaq_amd.batch_run(ctx(), 0, d_ref, d_test, align=4096, steps=W)[0]
    assert same_result(batch, one), (batch, one)
    if lag == E2E_LAG0:
        assert same_result(one, want), (one, want)
    flagged = gstpeaq_amd.run_pair(ctx(), 0, ref, test, align=4096, track=W)
    print("ODG along the flagged track", flagged["odg"])
    assert flagged["track"]["flags"] == gstpeaq_amd.TRACK_F_RANGE and one["odg"] > flagged["odg"], (one["odg"], flagged["odg"])
    with pytest.raises(gstpeaq_amd.PeaqError, match="exclude each other"):
        gstpeaq_amd.batch_run(ctx(), 0, d_ref, d_test, align=4096, steps=True, track=True)


def test_a_drift_and_a_bend_come_out_as_the_tracks_own_segments():
    """a pure drift of 1e-3 (2 s of pink noise, window 4096, lag0 85: 19 of 23 windows valid in the numpy model, every D
    between 3.5 and 4.7) and tests/test_gpu_track.py's bent pair (window 16384, lag0 48): no candidate on the CPU"""
    import gstpeaq_amd
    ref = noise("pink", E2E_N, 2, 6)
    test = resampled(ref, 1e-3, 37.5) + hiss(ref.shape, 1e-4, 3)
    bent_ref, bent_test = bent_pair()
    for r, t, lag0, window in ((ref.astype(np.float32), test.astype(np.float32), 85, W), (bent_ref, bent_test, 48, 16384)):
        d_ref, d_test = cuda(r[None]), cuda(t[None])
        lags = np.array([lag0], np.int32)
        tr = gstpeaq_amd.estimate_track(ctx(), d_ref, d_test, lags, window=window)
        got = gstpeaq_amd.estimate_steps(ctx(), d_ref, d_test, lags, window=window)
        S = int(tr["n_segments"][0])
        assert tr["flags"][0] == 0 and got["n_candidates"][0] == 0 and got["n_accepted"][0] == 0 and got["flags"][0] == 0
        assert got["n_pieces"][0] == S and list(got["b"][0, :S]) == [sc.start_of(k, window) for k in range(S)]
        assert got["a"][0, :S].tobytes() == tr["a"][0].tobytes() and got["e"][0, :S].tobytes() == tr["e"][0].tobytes()
        assert not got["a"][0, S:].any() and not got["b"][0, S:].any() and not got["steps"]["norm"].any()


# ---- (d) what it is for -----------------------------------------------------------------------------------------------
# ODGs of the CPU oracle (tests/oracle_lib.py, advanced version) for grade_pair(), measured on the CPU: unstepped; cut
# at the one integer lag (-263: the half behind the step wins the correlation); along the track, which is
# PEAQ_TRACK_F_RANGE (46 of 46 windows valid, knots 300.23 then 0.23) and therefore the same cut; along the pieces of the
# numpy models (stage_model with window 4096 -> peaq_track_fit -> candidates_model -> locate_model -> fit_model ->
# pieces_model: one candidate (segment 23, 94208 .. 102400, LA 300, LB 0), located 14 outputs behind the true position,
# inside the 300 that fit neither delay, gain 0.215, accepted; 45 pieces).  With 300 samples INSERTED instead (silence):
# 0.195, -0.144 (lag 337), the same, 0.190.
GRADE_ORACLE = (0.195, -0.744, -0.744, 0.190)
GRADE_WINDOW = 4096


def grade_pair():
    """tests/test_gpu_drift.py's clicks on digital silence at 4 s (stereo, 400 clicks of 0.5), the test signal late by
    37.25 samples (not 37.5: see the head of this file) with 300 samples dropped at its middle, hiss 80 dB below the
    reference's rms.  (ref, test, unstepped): unstepped is the reference with the same hiss"""
    from test_gpu_subsample import delayed
    rng = np.random.default_rng(4)
    n = 4 * 48000
    ref = np.zeros((n, 2))
    ref[rng.integers(100, n - 200, 400)] = 0.5
    h = ref.std() * 10 ** (-80.0 / 20) * np.random.default_rng(9).standard_normal(ref.shape)
    base = delayed(ref, E2E_OFFSET)
    at = n // 2 + 37
    test = np.concatenate([base[:at], base[at + 300:], np.zeros((300, 2))])
    return ref.astype(np.float32), (test + h).astype(np.float32), (ref + h).astype(np.float32)


def test_a_stepped_pair_scores_near_the_unstepped_one_along_the_pieces_and_not_along_the_track():
    """The oracle's ODGs for the pair are GRADE_ORACLE: 0.195 unstepped, -0.744 along the flagged track (which is the
    integer-aligned pair), 0.190 along the pieces: the track loses 0.940 ODG, the pieces 0.0055 (the 300 outputs around
    the step that fit neither delay hold one click in 160 on average).  Asserted with tests/test_gpu_drift.py's factor of
    two on each margin: the pieces-corrected pair within 2 x 0.0055 of the unstepped one, the track-corrected pair at
    least 0.940 / 2 below it."""
    import gstpeaq_amd
    und, integer, track, pieces = GRADE_ORACLE
    ref, test, unstepped = grade_pair()
    odg_und = gstpeaq_amd.run_pair(ctx(), 1, ref, unstepped)["odg"]
    by_track = gstpeaq_amd.run_pair(ctx(), 1, ref, test, align=4096, track=GRADE_WINDOW)
    got = gstpeaq_amd.run_pair(ctx(), 1, ref, test, align=4096, steps=GRADE_WINDOW)
    plain = gstpeaq_amd.run_pair(ctx(), 1, ref, test, align=4096)
    print("device ODG: unstepped", odg_und, "integer", plain["odg"], "track", by_track["odg"], by_track["track"], "pieces", got["odg"],
          got["delay"], got["pieces"], got["steps"])
    assert by_track["track"]["flags"] == gstpeaq_amd.TRACK_F_RANGE and by_track["track"]["n_windows"] == 46
    assert same_result(by_track, plain)                  # the flagged track scores what the integer lag scores
    assert got["pieces"]["flags"] == 0 and got["pieces"]["n_candidates"] == 1 and got["pieces"]["n_accepted"] == 1
    assert got["pieces"]["n_pieces"] == 45 and (got["steps"][0]["LA"], got["steps"][0]["LB"]) == (300, 0)
    assert abs(got["odg"] - odg_und) <= 2 * abs(pieces - und), (got["odg"], odg_und)
    assert by_track["odg"] <= odg_und - abs(track - und) / 2, (by_track["odg"], odg_und)

"""The track stage on the device against FP64 numpy (include/peaq_amd.h, "delay track on the device"):
cut_track bit for bit against cut_drift where every segment is the same line and against the numpy sum where they are
not (an odd window, so that knots fall inside tiles), the per-window records of estimate_track against estimate_drift's,
the recovery of a bent delay through the stage's numpy model, robustness, independence of the batch, determinism, the
keyword paths bit for bit against the stage's entry points called one by one, and what the stage is for: a pair whose
delay bends scores near the unbent pair along the track and far from it along one line.

Tolerance of cut_track: tests/test_gpu_subsample.py's, as tests/test_gpu_drift.py takes it -- both sides round an FP64
sum of 65 products to FP32 once, and the two sums differ by at most 65 x 2^-53 x sum|h| x max|x| < 1e-13 max|x|."""
import numpy as np
import pytest

import gpu_common
from test_gpu_drift import ALIGN_TIE, drift_model, hiss, index, resampled, stage_model
from test_gpu_subsample import SUM_BOUND, cuda, noise, same_bits, same_result, tables

pytestmark = pytest.mark.gpu

K, STEPS, TILE, SPREAD = 32, 256, 1024, 20
NONE, RANGE = 1, 2
WINDOW = 16384
MAX_E = 1 / 64


def ctx():
    return gpu_common.ctx("default")


def centres(n, window):
    return np.arange(n) * float(window) + window // 2


def segments(knots, window):
    """(a, e) of the header's step 4 for given knots (at least two)"""
    knots = np.asarray(knots, np.float64)
    e = (knots[1:] - knots[:-1]) / float(window)
    return knots[:-1] - e * centres(len(knots) - 1, window), e


def segment_of(i, window, n_seg):
    h = window // 2
    return np.where(i < h, 0, np.minimum((i - h) // window, n_seg - 1))


def track_indices(window, a, e, i):
    """peaq_track_index for an array of i, without the library (tests/test_gpu_drift.py's index per segment)"""
    k = segment_of(i, window, len(a))
    m, phi = np.zeros(len(i), np.int64), np.zeros(len(i), np.int64)
    for s in range(len(a)):
        sel = k == s
        if sel.any():
            m[sel], phi[sel] = index(float(a[s]), float(e[s]), i[sel])
    return m, phi, k


def track_model(x, n_in, skip, n_keep, window, a, e):
    """the header's sum in FP64, taps o = -32 .. 32 in order; x: [n, channels] float32"""
    tab = tables()[1]
    i = np.arange(n_keep)
    m, phi, k = track_indices(window, a, e, i)
    xs = x[:n_in].astype(np.float64)
    out = np.zeros((n_keep, x.shape[1]))
    for o in range(-K, K + 1):
        s = skip + i + m + o
        ok = (s >= 0) & (s < n_in)
        v = np.where(ok[:, None], xs[np.clip(s, 0, max(n_in - 1, 0))], 0.0) if n_in else np.zeros_like(out)
        out += tab[phi + STEPS // 2, o + K][:, None] * v
    return out, m, phi, k


def staged_offsets(window, a, e, n_keep):
    """the kernel's index arithmetic in numpy: for every output its position m_i - m_lo in the staged span, m_lo the
    smallest m among the tile's first output, its last output and the two outputs at a knot inside it"""
    i = np.arange(n_keep)
    m, _, k = track_indices(window, a, e, i)
    dm = np.zeros(n_keep, np.int64)
    for i0 in range(0, n_keep, TILE):
        i1 = min(i0 + TILE, n_keep) - 1
        cand = [i0, i1]
        if k[i1] != k[i0]:
            assert k[i1] == k[i0] + 1                   # a tile meets at most two segments
            knot = i0 + int(np.argmax(k[i0:i1 + 1] != k[i0]))
            cand += [knot - 1, knot]
        dm[i0:i1 + 1] = m[i0:i1 + 1] - m[cand].min()
    return dm


# ---- (a) equal segments: cut_drift bit for bit ------------------------------------------------------------------------
EQ_KEEP = 3 * TILE + 37          # several tiles and a partial one
EQ_LONG = 7000                   # ... and one pair that reaches the knot at 4097 + 2048 = 6145, one output into a tile
EQ_WINDOW = 4097
EQ_LINES = [(-0.37, 1e-3), (17.5, -1e-3), (0.49, 3.73e-5), (-3.0, -3.73e-5), (5 / 256, 0.0), (-128 / 256, 0.0), (127 / 256, 0.0)]


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("misaligned", [0, 1], ids=["aligned", "base+4"])
def test_equal_segments_are_bit_for_bit_cut_drift(channels, misaligned):
    """one call: a pair per line, 1, 2 or 3 equal segments, odd skips; the flat lines a = q / 256 are bit for bit
    cut_shifted as well; with `misaligned` both buffers one float off their allocation"""
    import gstpeaq_amd
    import torch
    rng = np.random.default_rng(30 + channels)
    cases = [(EQ_KEEP, skip, a, e, 1 + (j + skip) % 3) for j, (a, e) in enumerate(EQ_LINES) for skip in (0, 3, 40)]
    cases += [(EQ_LONG, 40, a, e, 3) for a, e in EQ_LINES[:5]]
    n = len(cases)
    in_stride = EQ_LONG + 40 + 43
    assert in_stride & 1
    x = rng.standard_normal((n, in_stride, channels)).astype(np.float32)
    skip = np.array([c[1] for c in cases], np.uint32)
    keep = np.array([c[0] for c in cases], np.uint32)
    n_in = (skip + keep + np.array([0, 40])[np.arange(n) % 2]).astype(np.uint32)
    a = np.array([c[2] for c in cases])
    e = np.array([c[3] for c in cases])
    n_seg = np.array([c[4] for c in cases], np.uint32)
    o_stride = EQ_LONG + 3
    flat = torch.zeros(x.size + 1, dtype=torch.float32, device="cuda")
    d_x = flat[misaligned:misaligned + x.size].view(x.shape)
    d_x.copy_(cuda(x))
    outs = []
    for _ in (0, 1, 2):
        o = torch.full((n * o_stride * channels + 1,), -77.25, dtype=torch.float32, device="cuda")
        outs.append(o[misaligned:misaligned + n * o_stride * channels].view(n, o_stride, channels))
    assert d_x.is_contiguous() and d_x.data_ptr() % 16 == 4 * misaligned
    gstpeaq_amd.cut_drift(ctx(), d_x, skip, keep, a, e, n_in=n_in, out=outs[0])
    gstpeaq_amd.cut_track(ctx(), d_x, skip, keep, EQ_WINDOW, n_seg, np.repeat(a[:, None], 3, 1), np.repeat(e[:, None], 3, 1),
                          n_in=n_in, out=outs[1])
    flat_q = np.array([int(round(c[2] * 256)) if c[3] == 0 else 0 for c in cases], np.int32)
    gstpeaq_amd.cut_shifted(ctx(), d_x, skip, keep, flat_q, n_in=n_in, out=outs[2])
    torch.cuda.synchronize()
    want, got, shifted = (o.cpu().numpy() for o in outs)
    for p, c in enumerate(cases):
        assert same_bits(got[p], want[p]), (p, c, int(np.argmax(got[p].view(np.uint32) != want[p].view(np.uint32))))
        assert (got[p, c[0]:] == np.float32(-77.25)).all(), (p, c)
        if c[3] == 0:
            assert same_bits(got[p], shifted[p]), (p, c)


def test_zero_segments_move_nan_payloads():
    import gstpeaq_amd
    import torch
    rng = np.random.default_rng(12)
    bits = rng.integers(0, 2 ** 32, size=(3, EQ_KEEP + 40, 2), dtype=np.uint32)
    bits[:, ::7] = 0x7FC12345
    x = bits.view(np.float32)
    skip, keep = np.array([0, 1, 33], np.uint32), np.array([EQ_KEEP, 1025, 63], np.uint32)
    outs = [torch.full((3, EQ_KEEP + 2, 2), -3.5, dtype=torch.float32, device="cuda") for _ in (0, 1)]
    gstpeaq_amd.cut(ctx(), cuda(x), skip, keep, out=outs[0])
    zeros = np.zeros((3, 3))
    zeros[1, 1] = -0.0
    # (n_in of 5: a pair that is moved does not look at it)
    gstpeaq_amd.cut_track(ctx(), cuda(x), skip, keep, 4096, [3, 2, 1], zeros, zeros.copy(), n_in=[5, 5, 5], out=outs[1])
    torch.cuda.synchronize()
    assert same_bits(outs[0].cpu().numpy(), outs[1].cpu().numpy())


# ---- (b) against the FP64 numpy sum ---------------------------------------------------------------------------------
SUM_WINDOW = 5001                # odd, no multiple of the tile: the knots 7501 and 12502 fall inside tiles


def sum_cases():
    """(knots, skip, n_keep, tail): n_in = skip + n_keep + (m of the last output) + tail"""
    rise = SUM_WINDOW / 64                              # a knot-to-knot rise of exactly 1/64 per sample
    return [([90.25, 90.25 - rise, 90.25, 90.25 - 0.4 * rise], 40, 13000, 22),    # -1/64, +1/64, a gentler one: 3 segments
            ([-20.0, -20.0 + rise, -20.0 + 0.3 * rise], 0, 11003, 22),             # a = -59: taps before the start; up, then down
            ([0.3, 0.3 + 1e-3 * SUM_WINDOW], 7, 10997, 9)]                         # 1 segment; the signal ends inside the last taps


def edge_cases():
    """as sum_cases, for the numpy sum alone: the tests that chain the cuts bit for bit keep sum_cases' three pairs"""
    return [([17.5, 17.5 - 1e-3 * SUM_WINDOW], 40, 1023, 22),                      # one output short of a tile
            ([0.3, 0.3 + 1e-3 * SUM_WINDOW], 40, 0, 22)]                           # nothing kept, beside the long pairs


@pytest.mark.parametrize("channels", [1, 2])
def test_cut_track_against_the_numpy_sum(channels):
    """one call of pairs of 3, 2 and 1 segments, window 5001; slopes +1/64 and -1/64 on the two sides of one knot, a
    negative a with skip = 0, an n_in that ends inside the last outputs' taps, a pair of 1023 outputs and one of none;
    every sample compared, the sentinel behind n_keep kept.  The kernel's staged index, restated in numpy, stays inside
    0 .. 19 for every output."""
    import gstpeaq_amd
    import torch
    rng = np.random.default_rng(60 + channels)
    cases = sum_cases() + edge_cases()
    n = len(cases)
    a, e = np.zeros((n, 3)), np.zeros((n, 3))
    n_seg = np.zeros(n, np.uint32)
    for p, (knots, _, _, _) in enumerate(cases):
        sa, se = segments(knots, SUM_WINDOW)
        a[p, :len(sa)], e[p, :len(se)], n_seg[p] = sa, se, len(sa)
        assert np.abs(se).max() <= MAX_E
    assert e[0, 0] == -MAX_E and e[0, 1] == MAX_E and e[1, 0] == MAX_E and e[1, 1] < 0 and a[1, 0] < -50
    skip = np.array([c[1] for c in cases], np.uint32)
    keep = np.array([c[2] for c in cases], np.uint32)
    last_m = [int(track_indices(SUM_WINDOW, a[p, :n_seg[p]], e[p, :n_seg[p]], np.array([max(int(keep[p]), 1) - 1]))[0][0]) for p in range(n)]
    n_in = np.array([int(skip[p]) + int(keep[p]) + last_m[p] + cases[p][3] for p in range(n)], np.uint32)
    in_stride = int(n_in.max()) + 1
    x = rng.standard_normal((n, in_stride, channels)).astype(np.float32)
    sentinel = np.float32(-77.25)
    out = torch.full((n, int(keep.max()) + 3, channels), float(sentinel), dtype=torch.float32, device="cuda")
    gstpeaq_amd.cut_track(ctx(), cuda(x), skip, keep, SUM_WINDOW, n_seg, a, e, n_in=n_in, out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    worst = 0.0
    for p in range(n):
        k = int(keep[p])
        if k == 0:
            assert (got[p] == sentinel).all(), p                                    # nothing kept: the sentinel stays
            continue
        pa, pe = a[p, :n_seg[p]], e[p, :n_seg[p]]
        want, m, phi, seg = track_model(x[p], int(n_in[p]), int(skip[p]), k, SUM_WINDOW, pa, pe)
        assert set(seg) == set(range(n_seg[p])), (p, set(seg))                      # every segment is met
        dm = staged_offsets(SUM_WINDOW, pa, pe, k)
        assert dm.min() == 0 and dm.max() < SPREAD - 2, (p, dm.min(), dm.max())      # the kernel's clamp never acts
        s = int(skip[p]) + np.arange(k) + m
        if p == 1:
            assert s.min() < 0 and (s - K).min() < -K                               # outputs centred before the signal's start
        if p == 2:
            assert (s + K).max() >= int(n_in[p]) > s.max()                          # the signal ends inside the last taps
        tol = 2.0 ** -23 * np.abs(want) + SUM_BOUND * np.abs(x[p]).max() + 1.5e-45
        err = np.abs(got[p, :k].astype(np.float64) - want)
        assert (err <= tol).all(), (p, float((err / tol).max()), int(np.argmax((err / tol).max(axis=1))))
        worst = max(worst, float((err / tol).max()))
        assert (got[p, k:] == sentinel).all(), p
    print("channels", channels, "worst error / tolerance:", worst)


# ---- the bent pair ------------------------------------------------------------------------------------------------------
BENT_SECONDS, BENT_OFFSET, BENT_E, BENT_SEED = 4, 37.5, 2e-4, 900
BENT_HALF = BENT_SECONDS * 48000 // 2        # the reference position at which the second clock takes over


def bent_delay(u, e=BENT_E, half=BENT_HALF):
    """the delay of the test signal at reference position u: it grows by e per sample up to `half`, then falls by e"""
    u = np.asarray(u, np.float64)
    return BENT_OFFSET + e * np.minimum(u, half) - e * np.maximum(u - half, 0.0)


def bent(ref, e=BENT_E, half=BENT_HALF):
    """The reference through two clocks one after the other, in FP64: test[j] = ref(u) with j = u + bent_delay(u).  The
    position function is linear on either side of `half`, so its inverse is: u = (j - 37.5) / (1 + e) up to j_half =
    half + bent_delay(half), and u = (j - 37.5 - 2 e half) / (1 - e) behind it -- tests/test_gpu_drift.py's interpolator
    with each side's clock and offset, joined at j_half."""
    j_half = int(np.ceil(half + float(bent_delay(half, e, half))))
    first = resampled(ref, e, BENT_OFFSET)
    second = resampled(ref, -e, BENT_OFFSET + 2 * e * half)
    u = np.where(np.arange(len(ref)) < j_half, (np.arange(len(ref)) - BENT_OFFSET) / (1 + e),
                 (np.arange(len(ref)) - BENT_OFFSET - 2 * e * half) / (1 - e))
    assert np.abs(u + bent_delay(u, e, half) - np.arange(len(ref))).max() < 1e-6     # the inverse is the inverse
    return np.where((np.arange(len(ref)) < j_half)[:, None], first, second)


def bent_pair(seed=BENT_SEED):
    """4 s of stereo pink noise (rms 0.1, tests/test_gpu_drift.py's material), delay 37.5, clock +2e-4 for the first half
    and -2e-4 for the second, hiss 60 dB down: (ref, test) in FP32"""
    ref = noise("pink", BENT_SECONDS * 48000, 2, seed)
    test = bent(ref) + hiss(ref.shape, 1e-4, seed + 10)
    return ref.astype(np.float32), test.astype(np.float32)


def model_track(ref, test, lag0, window=WINDOW, R=1024):
    """the stage in numpy: tests/test_gpu_drift.py's stage_model for the windows, then the host fit (no device in it):
    (rows, fit)"""
    import gstpeaq_amd
    rows = stage_model(ref, test, lag0, window, R)
    d = [lag + q / 256.0 for lag, q, _, _, _, _ in rows]
    return rows, gstpeaq_amd.track_fit(d, [ok for _, _, ok, _, _, _ in rows], window=window)


@pytest.fixture(scope="module")
def bent_fixture():
    return bent_pair()


def track_of(ctx_, ref, test, lag0, **kw):
    """estimate_track of one pair"""
    import gstpeaq_amd
    return gstpeaq_amd.estimate_track(ctx_, cuda(ref[None]), cuda(test[None]), np.array([lag0], np.int32), **kw)


# ---- (c) the per-window records are the drift stage's ------------------------------------------------------------------
def test_window_records_are_estimate_drifts_and_the_track_is_their_fit():
    """tests/test_gpu_drift.py's shapes: 3 pairs, window 4096, W = 5, 4 and 5 of unequal lengths, a negative lag among
    them; one pair's clock bends"""
    import gstpeaq_amd
    W, R = 4096, 512
    lens = [(5 * W + 700, 5 * W + 300), (4 * W + 4000, 5 * W + 9), (6 * W, 5 * W + 133)]
    lag0 = np.array([9, -3, 40], np.int32)
    stride = 6 * W + 1
    ref = np.zeros((3, stride, 2), np.float32)
    test = np.zeros_like(ref)
    for p, (nr, nt) in enumerate(lens):
        r = noise("pink", max(nr, nt) + 200, 2, 700 + p)
        ref[p, :nr] = r[:nr]
        t = bent(r, 2e-4, 3 * W) if p == 2 else resampled(r, 1e-4 * (p - 1), float(lag0[p]) + 0.3)
        test[p, :nt] = (t + hiss(r.shape, 1e-4, 710 + p))[:nt]
    n_ref = np.array([a for a, _ in lens], np.uint32)
    n_test = np.array([b for _, b in lens], np.uint32)
    d_ref, d_test = cuda(ref), cuda(test)
    line = gstpeaq_amd.estimate_drift(ctx(), d_ref, d_test, lag0, n_ref, n_test, window=W, R=R)
    got = gstpeaq_amd.estimate_track(ctx(), d_ref, d_test, lag0, n_ref, n_test, window=W, R=R)
    assert list(got["n_windows"]) == [5, 4, 5] and list(got["n_segments"]) == [4, 3, 4] and list(got["lag0"]) == list(lag0)
    for k in line["windows"]:
        assert got["windows"][k].tobytes() == line["windows"][k].tobytes(), k
    for k in gstpeaq_amd.DRIFT_DTYPE.names:
        assert got["drift"][k].tobytes() == line[k].tobytes(), k
    win = got["windows"]
    assert got["knots"].shape == (3, 5) and got["a"].shape == (3, 4)
    for p in range(3):
        nw = int(got["n_windows"][p])
        d = win["lag"][p, :nw] + win["q"][p, :nw] / 256.0
        valid = np.isfinite(win["norm"][p, :nw]) & (win["norm"][p, :nw] > 0) & (win["sub_flags"][p, :nw] == 0) & \
            (np.abs(win["peak"][p, :nw]) >= 0.5 * win["norm"][p, :nw])
        fit = gstpeaq_amd.track_fit(d, valid, window=W)
        assert fit["n_valid"] >= 3 and fit["flags"] == 0
        for k in ("flags", "n_valid", "n_filled", "n_segments", "d_min", "d_max", "max_abs_e"):
            assert np.array([fit[k]]).astype(got[k].dtype).tobytes() == got[k][p:p + 1].tobytes(), (p, k, fit[k], got[k][p])
        assert got["knots"][p, :nw].tobytes() == fit["knots"].tobytes() and not got["knots"][p, nw:].any(), p
        ns = fit["n_segments"]
        assert got["a"][p, :ns].tobytes() == fit["a"].tobytes() and got["e"][p, :ns].tobytes() == fit["e"].tobytes(), p
        assert not got["a"][p, ns:].any() and not got["e"][p, ns:].any(), p


# ---- (d) a bent delay comes back --------------------------------------------------------------------------------------
# What the numpy model itself (model_track: stage_model, then the host fit) makes of bent_pair(), measured on the CPU:
# lag0 = 48, all 11 windows valid, no window's arg-max margin below ALIGN_TIE / 1e-9 (none exempt, so the cap of 2 is
# met by the model alone with this seed), and |knot_w - true delay at x_w| per window as below.  Window 5 holds the
# bend (at 96000 of 81920 .. 98304): it measures 7.63 against 7.52 at its centre, the largest of the eleven, and the
# running median takes the apex down to its larger neighbour, 6.59 -- the stage's own error, 0.94 samples at that
# knot and nowhere else (DESIGN.md 18 "Not done").  Each knot is held to twice its own figure.
BENT_LAG0 = 48
BENT_KNOT_ERR = (0.0413, 0.0285, 0.0189, 0.0079, 0.0229, 0.9365, 0.0149, 0.0354, 0.0075, 0.0048, 0.0170)
BENT_EXEMPT_CAP = 2


def test_a_bent_delay_comes_back_and_is_the_models(bent_fixture):
    """The device's lag_w and q_w equal the numpy model's wherever the model's arg-max margins clear ALIGN_TIE / 1e-9
    (at most 2 windows may be exempt for that reason; on the CPU the model exempts none with this seed), knots and
    segments are peaq_track_fit of them, and every knot lies within twice the model's own error of the true delay at
    x_w (BENT_KNOT_ERR above)."""
    import gstpeaq_amd
    ref, test = bent_fixture
    d_ref, d_test = cuda(ref[None]), cuda(test[None])
    lag0 = int(gstpeaq_amd.estimate_delay(ctx(), d_ref, d_test, 4096)["lag"][0])
    assert lag0 == BENT_LAG0, lag0
    got = gstpeaq_amd.estimate_track(ctx(), d_ref, d_test, np.array([lag0], np.int32), window=WINDOW)
    rows, fit = model_track(ref, test, lag0)
    assert got["n_windows"][0] == len(rows) == 11 and got["flags"][0] == 0
    win = got["windows"]
    exempt = 0
    for w, (lag, q, ok, margin, qmargin, xc) in enumerate(rows):
        if margin > ALIGN_TIE and qmargin > 1e-9:
            assert win["lag"][0, w] == lag and win["q"][0, w] == q, (w, lag, q, win["lag"][0, w], win["q"][0, w])
        else:
            exempt += 1
    assert exempt <= BENT_EXEMPT_CAP, exempt
    if exempt == 0:
        assert got["knots"][0].tobytes() == fit["knots"].tobytes() and got["a"][0].tobytes() == fit["a"].tobytes()
    true = bent_delay(centres(11, WINDOW)) - lag0
    err = np.abs(got["knots"][0] - true)
    print("lag0", lag0, "exempt", exempt, "knots", got["knots"][0], "errors", err)
    assert (err <= 2 * np.array(BENT_KNOT_ERR)).all(), err
    assert got["n_valid"][0] == 11 and got["n_filled"][0] == 0 and got["max_abs_e"][0] < 2.2e-4
    # the line the drift stage makes of the same windows is flat: the bend is lost on it
    assert abs(got["drift"]["e"][0]) < 5e-5 and got["drift"]["flags"][0] == 0


# ---- (e) robustness ---------------------------------------------------------------------------------------------------
def test_a_silent_a_foreign_and_a_nan_window_are_filled_from_their_neighbours(bent_fixture):
    """Windows 3 and 7: on the straight stretches, two windows from either end and not beside the bend's window 5, so
    that the medians of the other windows keep their three values' middle one -- the other knots stay bit-identical.
    The filled knot lies on the line between its neighbours' knots; the delay is straight there, so it is off the clean
    run's knot by at most the mean of the neighbours' model errors plus the window's own (BENT_KNOT_ERR)."""
    import gstpeaq_amd
    ref, test = bent_fixture
    lag0 = BENT_LAG0
    clean = track_of(ctx(), ref, test, lag0, window=WINDOW)
    assert clean["flags"][0] == 0 and clean["n_valid"][0] == 11
    hurt = test.copy()
    hurt[lag0 + 3 * WINDOW:lag0 + 4 * WINDOW] = 0                                     # window 3 of A_test: silence
    hurt[lag0 + 7 * WINDOW:lag0 + 8 * WINDOW] = noise("white", WINDOW, 2, 77).astype(np.float32)   # window 7: unrelated
    nan = test.copy()
    nan[lag0 + 7 * WINDOW + 99, 1] = np.nan
    for signal, bad in ((hurt, (3, 7)), (nan, (7,))):
        got = track_of(ctx(), ref, signal, lag0, window=WINDOW)
        win = got["windows"]
        assert got["flags"][0] == 0 and got["n_valid"][0] == 11 - len(bad) and got["n_filled"][0] == len(bad), got
        if signal is hurt:
            assert win["norm"][0, 3] == 0 and abs(win["peak"][0, 7]) < 0.5 * win["norm"][0, 7]
        else:
            assert np.isnan(win["norm"][0, 7])
        keep = np.array([w not in bad for w in range(11)])
        assert got["knots"][0, keep].tobytes() == clean["knots"][0, keep].tobytes(), (bad, got["knots"][0], clean["knots"][0])
        for w in bad:
            between = (clean["knots"][0, w - 1] + clean["knots"][0, w + 1]) / 2
            assert abs(got["knots"][0, w] - between) < 1e-12, (w, got["knots"][0, w], between)
            bound = (BENT_KNOT_ERR[w - 1] + BENT_KNOT_ERR[w + 1]) / 2 + BENT_KNOT_ERR[w]
            assert abs(got["knots"][0, w] - clean["knots"][0, w]) <= bound, (w, got["knots"][0, w], clean["knots"][0, w])


def test_no_valid_window_is_no_track_and_the_cut_is_the_plain_one(bent_fixture):
    import gstpeaq_amd
    import torch
    ref, test = bent_fixture
    n = 3 * WINDOW + 5000
    quiet = np.zeros_like(test[:n])
    quiet[100] = np.nan                                                               # (window 0: a NaN norm; the others: 0)
    got = track_of(ctx(), ref[:n], quiet, 47, window=WINDOW)
    assert got["flags"][0] == NONE and got["n_valid"][0] == 0 and got["n_filled"][0] == 3 and got["n_segments"][0] == 2
    assert not got["knots"].any() and not got["a"].any() and not got["e"].any()
    assert got["drift"]["flags"][0] == NONE
    sr, st, keep = gstpeaq_amd.track_lengths(47, WINDOW, got["a"][0], got["e"][0], n, n)
    assert (sr, st, keep) == gstpeaq_amd.aligned_lengths(47, n, n)
    src = test[:n].copy()
    a = gstpeaq_amd.cut(ctx(), cuda(src[None]), [st], [keep])
    b = gstpeaq_amd.cut_track(ctx(), cuda(src[None]), [st], [keep], WINDOW, got["n_segments"], got["a"], got["e"])
    torch.cuda.synchronize()
    assert same_bits(a.cpu().numpy(), b.cpu().numpy())
    # a slope beyond max_e is flagged, its segments are zeroed and its knots stay
    far = track_of(ctx(), ref, test, BENT_LAG0, window=WINDOW, max_e=1e-4)
    assert far["flags"][0] == RANGE and not far["a"].any() and not far["e"].any() and far["max_abs_e"][0] > 1e-4
    assert far["knots"][0].tobytes() == track_of(ctx(), ref, test, BENT_LAG0, window=WINDOW)["knots"][0].tobytes()


# ---- (f) independence and determinism ---------------------------------------------------------------------------------
def test_record_and_cut_are_the_same_alone_in_a_batch_elsewhere_and_again():
    import gstpeaq_amd
    import torch
    W = 4096
    pairs = []
    for i in range(5):
        n = 5 * W + 300 * i + 17
        r = noise("pink", n, 2, 800 + i)
        t = bent(r, (i - 2.5) * 1.2e-4, n // 2 + 500 * i) + hiss(r.shape, 1e-4, 820 + i)     # (never 0: 37.5 would sit on q's edge)
        pairs.append((r.astype(np.float32), t.astype(np.float32), 37 + (i & 1)))
    stride = max(len(r) for r, _, _ in pairs) + 1
    R = np.zeros((5, stride, 2), np.float32)
    T = np.zeros_like(R)
    for p, (r, t, _) in enumerate(pairs):
        R[p, :len(r)], T[p, :len(t)] = r, t
    n = np.array([len(r) for r, _, _ in pairs], np.uint32)
    lags = np.array([l for _, _, l in pairs], np.int32)

    def run(d_ref, d_test, lags, n):
        rec = gstpeaq_amd.estimate_track(ctx(), d_ref, d_test, lags, n, n, window=W)
        ns = rec["n_segments"]
        cuts = np.array([gstpeaq_amd.track_lengths(int(lags[p]), W, rec["a"][p, :ns[p]], rec["e"][p, :ns[p]], int(n[p]), int(n[p]))
                         for p in range(len(n))], np.uint32).reshape(-1, 3)
        out = gstpeaq_amd.cut_track(ctx(), d_test, cuts[:, 1], cuts[:, 2], W, ns, rec["a"], rec["e"], n_in=n)
        torch.cuda.synchronize()
        return rec, cuts, out.cpu().numpy()

    names = gstpeaq_amd.TRACK_DTYPE.names + ("knots", "a", "e")
    batch = run(cuda(R), cuda(T), lags, n)
    again = run(cuda(R), cuda(T), lags, n)
    assert (batch[0]["flags"] == 0).all() and (batch[0]["max_abs_e"] > 5e-5).sum() >= 4, batch[0]
    for k in names:
        assert batch[0][k].tobytes() == again[0][k].tobytes(), k
    assert same_bits(batch[2], again[2])
    spacer = torch.zeros(12345, device="cuda")                                        # (another address for the copies)
    for p in (0, 2, 4):
        r, t, _ = pairs[p]
        alone = run(cuda(r[None]), cuda(t[None]), lags[p:p + 1], n[p:p + 1])
        for k in names:                                                               # (rows of the batch are as wide as its longest pair)
            mine, theirs = alone[0][k][0], batch[0][k][p]
            width = np.size(mine)
            assert np.ravel(mine).tobytes() == np.ravel(theirs)[:width].tobytes() and not np.ravel(theirs)[width:].any(), (p, k, mine, theirs)
        keep = int(batch[1][p, 2])
        assert (alone[1][0] == batch[1][p]).all() and same_bits(alone[2][0, :keep], batch[2][p, :keep]), p
    del spacer


# ---- (g) the keywords equal the stages called one by one ----------------------------------------------------------------
@pytest.mark.parametrize("gain", [None, "lsq"])
def test_keywords_are_the_stages_one_by_one(bent_fixture, gain, tmp_path):
    import subprocess
    import gst_env
    import gstpeaq_amd
    from test_gpu_subsample import write_wav
    ref, test = bent_fixture
    n0 = 48000 + 60000
    # row 0 holds the bend (at 56000 of it); row 1 ends before it, at half the level
    rows = [(ref[40000:40000 + n0], test[40000:40000 + n0]), (ref[3000:88000], 0.5 * test[3000:88000])]
    R = np.zeros((2, n0, 2), np.float32)
    T = np.zeros_like(R)
    for p, (r, t) in enumerate(rows):
        R[p, :len(r)], T[p, :len(t)] = r, t
    n = np.array([len(r) for r, _ in rows], np.uint32)
    d_ref, d_test = cuda(R), cuda(T)
    kw = {} if gain is None else dict(gain=gain)
    got = gstpeaq_amd.batch_run(ctx(), 0, d_ref, d_test, n, n, align=4096, track=WINDOW, **kw)
    last = gstpeaq_amd.align.last_track
    lags = gstpeaq_amd.estimate_delay(ctx(), d_ref, d_test, 4096, n, n)["lag"]
    rec = gstpeaq_amd.estimate_track(ctx(), d_ref, d_test, lags, n, n, window=WINDOW)
    assert (rec["flags"] == 0).all() and list(rec["n_windows"]) == [6, 5] and (rec["d_max"] - rec["d_min"] > 2).all(), rec
    for k in gstpeaq_amd.TRACK_DTYPE.names + ("knots", "a", "e"):
        assert last[k].tobytes() == rec[k].tobytes(), k
    ns = rec["n_segments"]
    cuts = np.array([gstpeaq_amd.track_lengths(int(lags[p]), WINDOW, rec["a"][p, :ns[p]], rec["e"][p, :ns[p]], int(n[p]), int(n[p]))
                     for p in range(2)], np.uint32)
    a = gstpeaq_amd.cut(ctx(), d_ref, cuts[:, 0], cuts[:, 2])
    b = gstpeaq_amd.cut_track(ctx(), d_test, cuts[:, 1], cuts[:, 2], WINDOW, ns, rec["a"], rec["e"], n_in=n)
    if gain is not None:
        grec, _ = gstpeaq_amd.measure_gain(ctx(), a, b, gain, n=cuts[:, 2])
        b = gstpeaq_amd.cut_scaled(ctx(), b, np.zeros(2, np.uint32), cuts[:, 2], grec)
    want = gstpeaq_amd.batch_run(ctx(), 0, a, b, cuts[:, 2], cuts[:, 2])
    for p in range(2):
        assert same_result(got[p], want[p]), (p, got[p], want[p])
        one = gstpeaq_amd.run_pair(ctx(), 0, rows[p][0], rows[p][1], align=4096, track=WINDOW, **kw)
        assert same_result(one, want[p]), (p, one, want[p])
        assert one["delay"]["lag"] == lags[p]
        for k in gstpeaq_amd.TRACK_DTYPE.names:
            assert one["track"][k] == rec[k][p], (p, k, one["track"][k], rec[k][p])
        if gain is not None and p == 1:
            assert abs(one["gain"]["gain"][0] - 2.0) < 0.02, one["gain"]      # (the numpy model's cut gives 1.9992)
    if gain is None and gst_env.CLI.exists():
        # 32-bit float files hand the CLI the samples as they are
        write_wav(tmp_path / "r.wav", rows[0][0])
        write_wav(tmp_path / "t.wav", rows[0][1])
        run = subprocess.run([str(gst_env.CLI), "--align-track=%d" % WINDOW, str(tmp_path / "r.wav"), str(tmp_path / "t.wav")],
                             capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout + run.stderr
        lines = run.stdout.strip().splitlines()
        assert lines[0] == "Delay: %d samples, track %+.4f .. %+.4f (6 of 6 windows)" % (lags[0], rec["d_min"][0], rec["d_max"][0]), run.stdout
        assert lines[1] == "Objective Difference Grade: %.3f" % want[0]["odg"], run.stdout
        assert lines[2] == "Distortion Index: %.3f" % want[0]["di"], run.stdout
    with pytest.raises(gstpeaq_amd.PeaqError, match="exclude each other"):
        gstpeaq_amd.batch_run(ctx(), 0, d_ref, d_test, n, n, align=4096, track=True, drift=True)
    with pytest.raises(gstpeaq_amd.PeaqError, match="exclude each other"):
        gstpeaq_amd.batch_run(ctx(), 0, d_ref, d_test, n, n, align=4096, track=True, subsample=True)
    with pytest.raises(gstpeaq_amd.PeaqError, match="requires align="):
        gstpeaq_amd.batch_run(ctx(), 0, d_ref, d_test, n, n, track=True)


# ---- (h) what it is for -----------------------------------------------------------------------------------------------
PURPOSE_E, PURPOSE_SNR_DB, PURPOSE_WINDOW = 6e-4, 80.0, 4096
# ODGs of the CPU oracle (tests/oracle_lib.py, advanced version) for purpose_pair(), measured on the CPU: unbent;
# corrected along ONE line by the numpy model of tests/test_gpu_drift.py (stage_model with window 4096 -> peaq_drift_fit
# -> drift_model: lag0 = 80, a = -6.376, e = -1.3e-5: the two halves cancel); corrected along the track by the numpy
# model of this file (model_track -> peaq_track_lengths -> track_model: 29 of 46 windows valid, the others filled).
# The same three at other bends (the integer-aligned pair beside them), which is why the bend is 6e-4:
#   bend    unbent   integer   line     track
#   3e-4    0.195    -0.735    -0.471   -0.195      (the line still helps: it loses too little to tell the two apart)
#   6e-4    0.195    -0.757    -0.790   -0.080
#   1e-3    0.195    -1.385    -3.210   -0.333      (9 of 46 windows valid)
PURPOSE_ORACLE = (0.195, -0.790, -0.080)


def purpose_pair():
    """tests/test_gpu_drift.py's clicks on digital silence at 4 s (stereo, 400 clicks of 0.5), the test signal late by
    37.5 samples through a clock fast by 6e-4 for the first half and slow by 6e-4 for the second (the delay peaks 57.6
    samples up), hiss 80 dB below the reference's rms.  (ref, test, unbent): unbent is the reference with the same hiss"""
    rng = np.random.default_rng(4)
    n = 4 * 48000
    ref = np.zeros((n, 2))
    ref[rng.integers(100, n - 200, 400)] = 0.5
    h = ref.std() * 10 ** (-PURPOSE_SNR_DB / 20) * np.random.default_rng(9).standard_normal(ref.shape)
    return ref.astype(np.float32), (bent(ref, PURPOSE_E) + h).astype(np.float32), (ref + h).astype(np.float32)


def test_a_bent_pair_scores_near_the_unbent_one_along_the_track_and_not_along_a_line():
    """The oracle's three ODGs for the pair are PURPOSE_ORACLE: 0.195 unbent, -0.790 along one line, -0.080 along the
    track: the line loses 0.985 ODG, the track 0.275 (what resampling clicks through 65 taps leaves against digital
    silence, and the bend's own window).  Asserted with tests/test_gpu_drift.py's factor of two on each
    margin: the track-corrected pair within 2 x 0.275 of the unbent one, the line-corrected pair at least 0.985 / 2
    below it."""
    import gstpeaq_amd
    und, line, track = PURPOSE_ORACLE
    ref, test, unbent = purpose_pair()
    odg_und = gstpeaq_amd.run_pair(ctx(), 1, ref, unbent)["odg"]
    by_line = gstpeaq_amd.run_pair(ctx(), 1, ref, test, align=4096, drift=PURPOSE_WINDOW)
    got = gstpeaq_amd.run_pair(ctx(), 1, ref, test, align=4096, track=PURPOSE_WINDOW)
    print("device ODG: unbent", odg_und, "line", by_line["odg"], by_line["drift"], "track", got["odg"], got["delay"], got["track"])
    assert got["track"]["flags"] == 0 and got["track"]["n_windows"] == 46 and got["track"]["n_segments"] == 45
    assert by_line["drift"]["flags"] == 0
    assert abs(got["odg"] - odg_und) <= 2 * abs(track - und), (got["odg"], odg_und)
    assert odg_und - by_line["odg"] >= (und - line) / 2, (odg_und, by_line["odg"])

"""What the tests of the steps stage share (include/peaq_amd.h, "delay steps on the device"): the stepped
fixtures, and the stage restated in numpy -- the locator's statistic in FP64, the host fit, the pieces' index
arithmetic and the cut's sum.  No device and no test in here."""
import math

import numpy as np

from test_gpu_drift import hiss, index
from test_gpu_subsample import delayed, noise, tables

K, STEPS, TILE, SPREAD = 32, 256, 1024, 20
F_NONE, F_SPAN, F_WEAK, P_RANGE = 1, 2, 4, 2
MAX_SPAN = 1 << 22
OFFSET = 37.5                    # the fixtures' delay before the step


# ---- fixtures ---------------------------------------------------------------------------------------------------------
def tones(n, channels, seed):
    """two amplitude-modulated tones (997 Hz and 3163 Hz, modulated at 3 and 7 Hz) with 2 % noise, FP64 [n, channels],
    rms about 0.1"""
    t = np.arange(n) / 48000.0
    rng = np.random.default_rng(seed)
    y = np.zeros((n, channels))
    for c in range(channels):
        y[:, c] = (1 + 0.5 * np.sin(2 * np.pi * 3 * t + c)) * np.sin(2 * np.pi * 997 * t + 0.3 * c) + \
            0.6 * (1 + 0.5 * np.sin(2 * np.pi * 7 * t)) * np.sin(2 * np.pi * 3163 * t + 1.1 * c)
    y += 0.02 * np.std(y) * rng.standard_normal(y.shape)
    return 0.1 * y / np.std(y)


def material(kind, n, channels, seed):
    return tones(n, channels, seed) if kind == "tones" else noise(kind, n, channels, seed)


def stepped(ref, step, at, offset=OFFSET, level=1e-4, seed=1):
    """The reference late by `offset` samples, and from test position `at` on by `step` more: a positive step inserts
    `step` samples of unrelated white noise at the material's level there (an edit; a block played twice would be right
    at either copy), a negative one drops -step samples.  Hiss at `level` (60 dB below the material's 0.1).  FP64, the
    reference's length."""
    base = delayed(ref, offset)
    if step > 0:
        fill = 0.1 * np.random.default_rng(seed + 200).standard_normal((step,) + base.shape[1:])
        out = np.concatenate([base[:at], fill, base[at:]])[:len(ref)]
    elif step < 0:
        out = np.concatenate([base[:at], base[at - step:], np.zeros((-step,) + base.shape[1:])])
    else:
        out = base
    return out + hiss(out.shape, level, seed + 100)


# ---- the locator ------------------------------------------------------------------------------------------------------
def mono(x):
    return x.astype(np.float64).sum(axis=1)


def locate_model(ref, test, lag0, lo, hi, LA, LB):
    """The header's statistic for one candidate in FP64 (numpy's own summation order: the comparisons with the device
    carry the header's accuracy).  ref, test: FP32 [n, channels].  A dict: c, gain_left, gain_right, norm, s, and sH, the
    array of s H[c] for c = lo .. hi."""
    sr, st = max(-lag0, 0), max(lag0, 0)
    r, t = mono(ref), mono(test)
    i = np.arange(lo, hi)

    def at(L):
        j = st + i + L
        ok = (j >= 0) & (j < len(t))
        return np.where(ok, t[np.clip(j, 0, len(t) - 1)], 0.0)
    rr, ta, tb = r[sr + i], at(LA), at(LB)
    d = ta - tb
    h = rr * d
    H = np.concatenate([[0.0], np.cumsum(h)])
    s = -1.0 if float((rr * (ta + tb)).sum()) < 0 else 1.0
    norm = math.sqrt(float((rr * rr).sum()) * float((d * d).sum()))
    sH = s * H
    if not (np.isfinite(norm) and norm > 0):
        return dict(c=lo, gain_left=0.0, gain_right=0.0, norm=norm, s=s, sH=sH, flags=F_NONE, sum_abs=float(np.abs(h).sum()))
    c = int(np.argmax(sH))
    return dict(c=lo + c, gain_left=float(sH[c]), gain_right=float(sH[c] - sH[-1]), norm=norm, s=s, sH=sH, flags=0,
                sum_abs=float(np.abs(h).sum()))


# ---- the host fit -----------------------------------------------------------------------------------------------------
def segment_line(knots, window, k):
    """(a_k, e_k) of the track's item 4, the same FP64 operations"""
    if len(knots) < 2:
        return (float(knots[0]) if len(knots) else 0.0), 0.0
    e = (knots[k + 1] - knots[k]) / float(window)
    return float(knots[k] - e * (float(k) * window + float(window // 2))), float(e)


def start_of(k, window):
    return window // 2 + k * window if k else 0


def candidates_model(knots, window, n_common, min_step=0.75, ratio=3.0):
    """rows (k, lo, hi, LA, LB)"""
    W = len(knots)
    out = []
    for k in range(max(W - 1, 0)):
        D = abs(knots[k + 1] - knots[k])
        Dl = abs(knots[k] - knots[k - 1]) if k else 0.0
        Dr = abs(knots[k + 2] - knots[k + 1]) if k + 2 < W else 0.0
        if not (D >= min_step and D >= ratio * max(Dl, Dr)):
            continue
        LA, LB = int(np.rint(knots[k])), int(np.rint(knots[k + 1]))
        lo, hi = k * window, min((k + 2) * window, n_common)
        if LA != LB and lo < hi:
            out.append((k, lo, hi, LA, LB))
    return out


def fit_model(knots, window, n_common, records, min_step=0.75, ratio=3.0, min_gain=0.0021, max_e=1 / 64):
    """peaq_steps_fit restated: records are dicts (c, flags, gain_left, gain_right, norm) in the candidates' order.
    Returns (flags, accepted, b, a, e, record flags)."""
    W = len(knots)
    S = max(W - 1, 1)
    cand = candidates_model(knots, window, n_common, min_step, ratio)
    assert len(cand) == len(records)
    at, rflags = {}, []
    for (k, lo, hi, _, _), rec in zip(cand, records):
        ok = rec["flags"] == 0 and min(rec["gain_left"], rec["gain_right"]) >= min_gain * rec["norm"]
        rflags.append(rec["flags"] | (0 if ok else F_WEAK))
        if ok:
            at[k] = min(max(rec["c"], lo), hi)
    END = 1 << 62
    b, a, e = [], [], []

    def put(lo, hi, line):
        if lo < hi:
            b.append(lo)
            a.append(line[0])
            e.append(line[1])
    for k in range(S):
        start, end = start_of(k, window), (start_of(k + 1, window) if k + 1 < S else END)
        left, right = k - 1 in at, k + 1 in at
        if k not in at:
            put(max(start, at[k - 1]) if left else start, min(end, at[k + 1]) if right else end, segment_line(knots, window, k))
            continue
        c, lo, hi = at[k], start, end
        if c < start:
            if left:
                c = start
            else:
                lo = c
        if c > end:
            if right:
                c = end
            else:
                hi = c
        ll = segment_line(knots, window, k - 1) if k and not left else (float(knots[k]), 0.0)
        rl = segment_line(knots, window, k + 1) if k + 1 < S and not right else (float(knots[k + 1]), 0.0)
        put(lo, c, ll)
        put(c, hi, rl)
    flags = 0
    if max(abs(x) for x in e) > max_e:
        flags = P_RANGE
        a, e = [0.0] * len(a), [0.0] * len(e)
    return flags, len(at), np.array(b, np.uint32), np.array(a), np.array(e), rflags


# ---- the pieces' index arithmetic and the cut -----------------------------------------------------------------------------
def piece_of(b, i):
    return np.searchsorted(np.asarray(b, np.int64), i, side="right") - 1


def pieces_indices(b, a, e, i):
    """peaq_pieces_index for an array of i, without the library (tests/test_gpu_drift.py's index per piece)"""
    j = piece_of(b, i)
    m, phi = np.zeros(len(i), np.int64), np.zeros(len(i), np.int64)
    for s in range(len(b)):
        sel = j == s
        if sel.any():
            m[sel], phi[sel] = index(float(a[s]), float(e[s]), i[sel])
    return m, phi, j


def pieces_model(x, n_in, skip, n_keep, b, a, e):
    """the header's sum in FP64, taps o = -32 .. 32 in order; x: [n, channels] float32"""
    tab = tables()[1]
    i = np.arange(n_keep)
    m, phi, j = pieces_indices(b, a, e, i)
    xs = x[:n_in].astype(np.float64)
    out = np.zeros((n_keep, x.shape[1]))
    for o in range(-K, K + 1):
        s = skip + i + m + o
        ok = (s >= 0) & (s < n_in)
        v = np.where(ok[:, None], xs[np.clip(s, 0, max(n_in - 1, 0))], 0.0) if n_in else np.zeros_like(out)
        out += tab[phi + STEPS // 2, o + K][:, None] * v
    return out, m, phi, j


def keep_brute(b, a, e, skip_test, n_common, n_test):
    """peaq_pieces_lengths' count by looking at every output"""
    if n_common == 0:
        return 0
    i = np.arange(n_common)
    m, _, _ = pieces_indices(b, a, e, i)
    bad = np.nonzero(skip_test + i + m >= n_test)[0]
    return int(bad[0]) if len(bad) else n_common


def staged_offsets(b, a, e, n_keep):
    """the kernel's index arithmetic in numpy: for every output its position m_i - m_lo in its pass's staged span, m_lo
    the smaller m of the pass's first and last output (a pass: the outputs of one tile inside one piece)"""
    i = np.arange(n_keep)
    m, _, j = pieces_indices(b, a, e, i)
    dm = np.zeros(n_keep, np.int64)
    for i0 in range(0, n_keep, TILE):
        i1 = min(i0 + TILE, n_keep)
        for piece in np.unique(j[i0:i1]):
            sel = i0 + np.nonzero(j[i0:i1] == piece)[0]
            dm[sel] = m[sel] - min(m[sel[0]], m[sel[-1]])
    return dm

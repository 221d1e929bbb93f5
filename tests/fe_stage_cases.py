"""Input populations of the FFT front end's stage tests (tests/test_fe_stage_cases_host.py holds them to what they are
meant to be with the CPU oracle alone, tests/test_gpu_fe_stage_batches.py runs them on the device).  numpy and synth_np
only.

Every pair is "foreign": the reference is synth_np.pair(s, ch, n)[0], the test signal synth_np.pair(s + 100, ch, n)[0],
each cut to its own length.  (A seed's own test signal follows its reference so closely that the noise in bands,
Pr - 2 sqrt(Pr Pt) + Pt, is cancellation-limited in many bands of a short frame: about 40 % of the oracle's own values
move beyond 2.5e-7 when 1 % of the samples move by an ulp, by up to 9.5e-5; with foreign pairs 0.3 % do, by at most
1.1e-6.)  Only seeds s are used for which neither s nor s + 100 has leading or trailing silence (usable_seed): otherwise a
short signal is digital silence throughout.

A "every end"    39 pairs, 55 frames (orc.count_frames), mono and stereo, one batch.  (n_ref, n_test):
                   (2500, t) and (t, 2500), t in ENDS = 0, 1, 2, 3, 127, 128, 129, 1023, 1024, 1025, 2045, 2046, 2047:
                       one flush frame at sample 0 in which one signal has t samples and the other a full frame
                   (2048 + k, 2048 + k), k in 0, 1, 2, 3, 127, 129, 1021, 1023: a full frame and a flush frame at sample
                       1024 with 1024 + k samples left (k = 0: the last hop alone)
                   (3077, 3076), (3203, 3139), (4073, 3073): the two signals end at different samples of the flush frame,
                       one and many rows of 128 samples apart
                   (4096, 4096): three full frames and the last hop as a flush frame
                   (0, 0): no frame
B "grids"        pairs of 4 frames (4099 samples) at 3 frames per launch -- a second launch of ONE frame with frame0 = 3:
                   mono batches of 3 .. 10 pairs (first launch: 9 .. 30 items, every remainder modulo 8), stereo batches of
                   3 .. 6 pairs (18 .. 36 items: 2, 0, 6, 4); pair 1 of every batch has (2051, 2051) = 2 frames
                 and 10 pairs of 8 frames (8195 samples) at 7 frames per launch, 70 / 140 items (above the prefetch
                   distance of 64; a reciprocal of 7); pair 1 has (2051, 2051), pair 4 (8195, 5000), pair 7 (3000, 8195)

Layout (packed): a flat float32 buffer full of NaN; the [pairs, stride, ch] tensor is the contiguous view that starts ONE
float into it; stride is the smallest odd number that holds the longest signal.  Mono pair bases are then 4-byte but
not 8-byte aligned at even pair indices and 8-byte aligned at odd ones; everything behind a signal's own length, and a
spare pair behind the batch, keeps the NaN."""
import functools

import numpy as np

import synth_np

FRAME, HOP = 2048, 1024
ENDS = (0, 1, 2, 3, 127, 128, 129, 1023, 1024, 1025, 2045, 2046, 2047)
A_FULL = 2500
A_EQUAL_K = (0, 1, 2, 3, 127, 129, 1021, 1023)
A_RAGGED = ((3077, 3076), (3203, 3139), (4073, 3073))
A_LENGTHS = ([(A_FULL, t) for t in ENDS] + [(t, A_FULL) for t in ENDS] + [(FRAME + k, FRAME + k) for k in A_EQUAL_K] +
             list(A_RAGGED) + [(4096, 4096), (0, 0)])
# the pairs of A that are also run as batches of one, and through the 55-band kernel one pair per call
A_SINGLES = ((2500, 1), (129, 2500), (2051, 2051), (4073, 3073), (4096, 4096))
A_SEED0, B_SEED0, B_BIG_SEED0 = 101, 232, 262        # the first usable seed at or above these

B_N, B_FPL = 4099, 3                                 # 4 frames; a second launch of one
B_SHORT = (2051, 2051)                               # pair 1 of every batch: 2 frames
B_MONO_SIZES, B_STEREO_SIZES = tuple(range(3, 11)), tuple(range(3, 7))
B_BIG_N, B_BIG_FPL, B_BIG_PAIRS = 8195, 7, 10        # 8 frames
B_BIG_DEVIANTS = {1: B_SHORT, 4: (8195, 5000), 7: (3000, 8195)}
PREFETCH_ITEMS = 64                                  # kPrefetchItems (gstpeaq_amd/csrc/peaq_frontend.hip)


def count_frames(n_ref, n_test):
    """oracle_lib.count_frames (asserted equal in the host file; here so that this module needs no oracle)"""
    n = min(n_ref, n_test)
    full = (n - FRAME) // HOP + 1 if n >= FRAME else 0
    return full + (1 if max(n_ref, n_test) > full * HOP else 0)


def flush_left(n_ref, n_test):
    """-> (samples of the reference, of the test signal) inside the pair's flush frame, 0 .. 2048 each; None without one"""
    n = min(n_ref, n_test)
    full = (n - FRAME) // HOP + 1 if n >= FRAME else 0
    if max(n_ref, n_test) <= full * HOP:
        return None
    return tuple(int(np.clip(x - full * HOP, 0, FRAME)) for x in (n_ref, n_test))


def usable_seed(s):
    return all(synth_np.params(x)[k] == 0 for x in (s, s + 100) for k in ("lead_silence", "tail_silence"))


def seeds_from(s0, count):
    out, s = [], s0
    while len(out) < count:
        if usable_seed(s):
            out.append(s)
        s += 1
    return out


@functools.lru_cache(maxsize=None)
def _signal(seed, ch, n):
    x = synth_np.pair(seed, ch, n)[0]
    x.setflags(write=False)
    return x


def foreign_pair(seed, ch, n_ref, n_test):
    """(ref, test) float32 [n_ref, ch], [n_test, ch]"""
    n = max(n_ref, n_test, 1)
    return _signal(seed, ch, n)[:n_ref].copy(), _signal(seed + 100, ch, n)[:n_test].copy()


def a_specs():
    """[(seed, n_ref, n_test)] of population A"""
    return [(s, a, b) for s, (a, b) in zip(seeds_from(A_SEED0, len(A_LENGTHS)), A_LENGTHS)]


def b_specs(n_pairs):
    """one batch of the remainder series: pair i has the i-th seed of B in every batch"""
    return [(s, *(B_SHORT if i == 1 else (B_N, B_N))) for i, s in enumerate(seeds_from(B_SEED0, n_pairs))]


def b_big_specs():
    return [(s, *B_BIG_DEVIANTS.get(i, (B_BIG_N, B_BIG_N))) for i, s in enumerate(seeds_from(B_BIG_SEED0, B_BIG_PAIRS))]


def b_sizes(ch):
    return B_MONO_SIZES if ch == 1 else B_STEREO_SIZES


def grid_items(n_pairs, frames_per_launch, ch):
    return n_pairs * frames_per_launch * ch


def odd_stride(specs):
    return max(max(a, b) for _, a, b in specs) | 1


def view(flat, n_pairs, stride, ch):
    """the [pairs, stride, ch] tensor inside a packed buffer (numpy or torch): contiguous, one float into it"""
    return flat[1:1 + n_pairs * stride * ch].reshape(n_pairs, stride, ch)


def packed(specs, ch, stride=None):
    """-> (flat_ref, flat_test, n_ref, n_test, stride): the two NaN-filled float32 buffers of 1 + (pairs + 1) * stride * ch
    floats (the signals written through view(); one spare pair of NaN behind the batch) and the uint32 lengths"""
    stride = odd_stride(specs) if stride is None else stride
    assert stride & 1 and stride >= max(max(a, b) for _, a, b in specs)
    flats = [np.full(1 + (len(specs) + 1) * stride * ch, np.nan, dtype=np.float32) for _ in range(2)]
    vr, vt = (view(f, len(specs), stride, ch) for f in flats)
    for i, (s, a, b) in enumerate(specs):
        vr[i, :a], vt[i, :b] = foreign_pair(s, ch, a, b)
    return (flats[0], flats[1], np.array([a for _, a, _ in specs], dtype=np.uint32),
            np.array([b for _, _, b in specs], dtype=np.uint32), stride)


def planes_from_records(bands, rec, tab):
    """The band planes of one pair in numpy from the oracle's front-end records rec [frames, channels, 576] (unsmeared
    excitations at 0 and 112, noise at 448) and tab = orc.tables(bands): dict name -> [frames, channels, bands] with
    exc_ref, exc_test, noise, nmr and (109 bands) detect, steps, e_db"""
    nf, channels = rec.shape[:2]
    a = tab["ear_tc"]
    sm = np.zeros((2, channels, bands))
    e = np.zeros((2, nf, channels, bands))
    for f in range(nf):                              # fftearmodel.c:496-504
        for i, off in enumerate((0, 112)):
            u = rec[f, :, off:off + bands]
            sm[i] = a * sm[i] + (1 - a) * u
            e[i, f] = np.maximum(sm[i], u)
    out = dict(exc_ref=e[0], exc_test=e[1], noise=rec[:, :, 448:448 + bands])
    out["nmr"] = out["noise"] * tab["mask_diff"] / e[0]              # movs.c:1002-1022
    if bands == 109:                                 # movs.c:1239-1260 as prob_detect_of_frame (oracle/peaq_oracle.c)
        er, et = 10. * np.log10(e[0]), 10. * np.log10(e[1])
        lv = 0.3 * np.maximum(er, et) + 0.7 * et
        pos = np.where(lv > 0., lv, 1.)
        sd = np.where(lv > 0., 5.95072 * np.power(6.39468 / pos, 1.71332) + 9.01033e-11 * np.power(pos, 4.) +
                      5.05622e-6 * np.power(pos, 3.) - 0.00102438 * pos * pos + 0.0550197 * pos - 0.198719, 1e30)
        d = er - et
        out["detect"] = np.power(d / sd, np.where(er > et, 4., 6.))
        out["steps"] = np.abs(np.trunc(d)) / sd
        out["e_db"] = d
    return out

"""Input populations of the filter-bank stage tests (tests/test_fb_stage_cases_host.py holds them to what they are meant
to be with the CPU oracle alone, tests/test_gpu_fb_stage_batches.py runs them on the device).  numpy only.

The base signal of a pair p is white noise, 0.25 * default_rng(seed + p).standard_normal((n, ch)) clipped to +-1,
float32; the test signal is the reference plus an independent noise (the same generator's next draw) at 0.01.

P1 "every tail"     40 pairs, one launch: n_ref = 192 p + TAILS[p % 6]; for odd p the test signal is (37 p) % 400 samples
                    shorter.  The counts are orc.count_blocks' (p + 1 for even p, fewer where the test signal is short):
                    every tile tail 1 .. 10 of fb_bank_kernel occurs, signal ends fall on, one sample before and one
                    after a 16-sample chunk and a block, and flush blocks are zero-padded.
P2 "wave edges"     65 stereo pairs (260 signals) or 129 mono pairs (258): fb_hp_kernel's first workgroup of four full
                    waves and a second one with one nearly empty wave.  Full pairs have 2304 samples = 12 blocks, and
                    the tensors are [pairs, 2304, ch] with no padding: the last pair is full, so a read past its row's
                    end is a read past the allocation.  At stereo pair indices (mono: twice that)
                      0 both signals empty   15 a single sample   16 reference only   31 3 blocks   40 11 blocks + 100
                      33, 63, 64 byte-for-byte copies of pair 1
                    so waves 0 and 1 hold an empty signal and mixed lengths at both edges, wave 2 mixes lengths inside,
                    wave 3 is all full-length (every interior block on the straight-line path) with a copy of pair 1 as
                    its last pair, and the copy at the last index is the second workgroup's only pair.
P3 "the seam"       mono, 4 pairs of 845, 841, 840 and 839 blocks: two launches at 840 blocks per launch, the second with
                    5, 1, 0 and 0 blocks.
P4 "hand-built"     one pair each, 40 blocks, for debug_filterbank: see p4_cases()."""
import numpy as np

FRAME = 192                                          # samples per filter-bank block
TAILS = [192, 1, 15, 16, 17, 191]
P1_PAIRS, P1_SEED = 40, 1000
P2_FULL, P2_SEED = 12 * FRAME, 2300
P2_STEREO_DEVIANTS = {0: "empty", 15: "one_sample", 16: "ref_only", 31: "blocks3", 40: "blocks11_100"}
P2_STEREO_COPIES = (33, 63, 64)                      # of pair 1
P3_LENGTHS = [FRAME * 844 + 50, FRAME * 840 + 1, FRAME * 840, FRAME * 839]
P3_SEED = 3000
P4_N, P4_SEED = 40 * FRAME, 4000
P4_IMPULSE_AT, P4_STEP_AT = 1000, 3840


def base_pair(seed, p, n, ch):
    """(ref, test) float32 [n, ch] of pair p"""
    rng = np.random.default_rng(seed + p)
    ref = np.clip(0.25 * rng.standard_normal((n, ch)), -1., 1.).astype(np.float32)
    test = (ref + np.float32(0.01) * rng.standard_normal((n, ch)).astype(np.float32)).astype(np.float32)
    return ref, test


def p1_pairs(ch):
    out = []
    for p in range(P1_PAIRS):
        n = FRAME * p + TAILS[p % 6]
        ref, test = base_pair(P1_SEED, p, n, ch)
        if p & 1:
            test = np.ascontiguousarray(test[:n - (37 * p) % 400])
        out.append((ref, test))
    return out


def p2_layout(ch):
    """-> (n_pairs, {pair index: deviant kind}, the indices of the copies of pair 1)"""
    k = 2 // ch                                      # mono: the corresponding positions x 2
    return 64 * k + 1, {k * i: kind for i, kind in P2_STEREO_DEVIANTS.items()}, tuple(k * i for i in P2_STEREO_COPIES)


def p2_pairs(ch):
    n_pairs, deviants, copies = p2_layout(ch)
    out = []
    for p in range(n_pairs):
        ref, test = base_pair(P2_SEED, p, P2_FULL, ch)
        kind = deviants.get(p)
        if kind == "empty":
            ref, test = ref[:0], test[:0]
        elif kind == "one_sample":
            ref, test = ref[:1], test[:1]
        elif kind == "ref_only":
            test = test[:0]
        elif kind == "blocks3":
            ref, test = ref[:3 * FRAME], test[:3 * FRAME]
        elif kind == "blocks11_100":
            ref, test = ref[:11 * FRAME + 100], test[:11 * FRAME + 100]
        out.append((np.ascontiguousarray(ref), np.ascontiguousarray(test)))
    for p in copies:
        out[p] = (out[1][0].copy(), out[1][1].copy())
    return out


def p3_pairs():
    return [base_pair(P3_SEED, p, n, 1) for p, n in enumerate(P3_LENGTHS)]


def packed(pairs, stride=None):
    """(ref, test, n_ref, n_test): float32 [pairs, stride, ch] zero-filled behind every signal's end, uint32 lengths;
    stride: the longest signal's length, made even (the FFT path loads sample pairs), unless given"""
    ch = pairs[0][0].shape[1]
    if stride is None:
        stride = max(max(len(r), len(t)) for r, t in pairs)
        stride += stride & 1
    ref = np.zeros((len(pairs), stride, ch), dtype=np.float32)
    test = np.zeros_like(ref)
    for i, (r, t) in enumerate(pairs):
        ref[i, :len(r)] = r
        test[i, :len(t)] = t
    return (ref, test, np.array([len(r) for r, _ in pairs], dtype=np.uint32),
            np.array([len(t) for _, t in pairs], dtype=np.uint32))


def wave_map(n_pairs, ch):
    """fb_hp_kernel's grouping (gstpeaq_amd/csrc/peaq_fb.hip: one thread per signal in the order pair, channel, ref/test;
    64 lanes per wave; kHpWaves = 4 waves per workgroup) -> int arrays [n_pairs, ch, 2]: wave (counted over the whole
    launch) and workgroup of every signal"""
    g = np.arange(n_pairs * ch * 2).reshape(n_pairs, ch, 2)
    return g // 64, g // (64 * 4)


# ---- P4 ------------------------------------------------------------------------------------------------------------------
def _with_base(sig, p):
    """a stereo pair: the hand-built signal in channel 0 (its test signal: the same at half the level), pair p's base
    signal in channel 1 -- the two channels of the pair differ in kind"""
    ref, test = base_pair(P4_SEED, p, P4_N, 2)
    ref[:, 0] = sig
    test[:, 0] = np.float32(0.5) * sig.astype(np.float32)
    return ref, test


def impulse(at=P4_IMPULSE_AT):
    x = np.zeros(P4_N, np.float32)
    x[at] = 0.5
    return x


def step_down(q):
    """pair 1's base signal (channel 0) normalised to peak 1.0, times q from sample P4_STEP_AT on"""
    x = base_pair(P4_SEED, 1, P4_N, 1)[0][:, 0].astype(np.float64)
    x /= np.max(np.abs(x))
    x[P4_STEP_AT:] *= q
    return x.astype(np.float32)


def sine(f):
    return (0.5 * np.sin(2 * np.pi * f * np.arange(P4_N) / 48000.)).astype(np.float32)


def p4_cases(fc):
    """fc: the 40 centre frequencies.  -> dict name -> dict(ref, test, level, settings)"""
    def case(ref, test, level=92.0, **settings):
        return dict(ref=np.ascontiguousarray(ref), test=np.ascontiguousarray(test), level=level, settings=settings)

    out = {"impulse": case(*_with_base(impulse(), 0)),
           "step_1e-3": case(*_with_base(step_down(1e-3), 1)),
           "step_0": case(*_with_base(step_down(0.), 1)),
           "dc": case(*_with_base(np.full(P4_N, 0.25, np.float32), 2))}
    for k, name in ((0, "sine_fc0"), (20, "sine_fc20"), (39, "sine_fc39")):
        out[name] = case(*_with_base(sine(float(fc[k])), 3 + k))
    base = base_pair(P4_SEED, 50, P4_N, 2)
    out["level_72"] = case(*base, level=72.0)
    out["level_112"] = case(*base, level=112.0)
    out["swap_slope"] = case(*base, swap_slope_filter_coefficients=1)
    return out


P4_NAMES = ["impulse", "step_1e-3", "step_0", "dc", "sine_fc0", "sine_fc20", "sine_fc39", "level_72", "level_112",
            "swap_slope"]

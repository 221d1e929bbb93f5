"""The host side of the steps stage without a GPU (include/peaq_amd.h, "delay steps on the device"):
peaq_steps_candidates and peaq_steps_fit against a restatement in numpy doubles (tests/steps_common.py), bit for bit;
peaq_pieces_index and peaq_pieces_lengths against brute force, negative jumps where i + m_i falls across a breakpoint
among them (which is also the check of peaq_steps_math.h's argument for the piece-by-piece search); the records' sizes
and constants; and the argument checks of peaq_batch_locate_steps, peaq_batch_cut_pieces, peaq_batch_estimate_steps and
peaq_run_pair_steps, which return PEAQ_ERR_ARG with the offending value in the message before any device is touched (a
NULL context is the last thing they look at)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import gstpeaq_amd
import steps_common as sc
from test_track_host import FIT_CASES

PEAQ_ERR_ARG = -1
ROOT = Path(__file__).resolve().parent.parent
WEAK, RANGE = 4, 2
MAX_E = 1 / 64


@pytest.fixture(scope="module")
def lib():
    if not gstpeaq_amd.library_path().exists():
        gstpeaq_amd.build_library()
    return gstpeaq_amd.load_library()


def err(lib):
    return lib.peaq_last_error().decode()


def u32(*v):
    return (C.c_uint32 * len(v))(*v)


def i32(*v):
    return (C.c_int32 * len(v))(*v)


def f64(*v):
    return (C.c_double * len(v))(*v)


def header_define(name):
    text = (ROOT / "include" / "peaq_amd.h").read_text()
    return re.search(r"^#define\s+%s\s+(.+?)\s*(/\*.*)?$" % name, text, flags=re.M).group(1)


def records(cand, found):
    """STEP_DTYPE records for the candidates: found[j] = (c, gain_left, gain_right, norm, flags)"""
    st = np.zeros(len(cand), gstpeaq_amd.STEP_DTYPE)
    for j, (cd, f) in enumerate(zip(cand, found)):
        st[j]["LA"], st[j]["LB"] = cd["LA"], cd["LB"]
        st[j]["c"], st[j]["gain_left"], st[j]["gain_right"], st[j]["norm"], st[j]["flags"] = f
    return st


def run_fit(knots, window, found, n_common=None, **kw):
    """(the library's fit, the restatement's) for the records found[j] = (c, gain_left, gain_right, norm, flags)"""
    knots = np.asarray(knots, np.float64)
    n_common = len(knots) * window + 777 if n_common is None else n_common
    ckw = {k: v for k, v in kw.items() if k in ("min_step", "ratio")}
    cand = gstpeaq_amd.steps_candidates(knots, window, n_common, **ckw)
    want_cand = sc.candidates_model(knots, window, n_common, **ckw)
    assert [(int(c["lo"]), int(c["hi"]), int(c["LA"]), int(c["LB"])) for c in cand] == [c[1:] for c in want_cand]
    assert len(found) == len(cand), (len(found), cand)
    got = gstpeaq_amd.steps_fit(knots, window, n_common, records(cand, found), **kw)
    recs = [dict(c=f[0], gain_left=f[1], gain_right=f[2], norm=f[3], flags=f[4]) for f in found]
    want = sc.fit_model(knots, window, n_common, recs, **kw)
    return got, want, want_cand


def same_pieces(got, want):
    flags, accepted, b, a, e, rflags = want
    assert got["flags"] == flags and got["n_accepted"] == accepted and got["n_pieces"] == len(b), (got, want)
    assert got["b"].tobytes() == b.tobytes(), (got["b"], b)
    assert got["a"].tobytes() == a.tobytes() and got["e"].tobytes() == e.tobytes(), (got["a"], a, got["e"], e)
    assert list(got["steps"]["flags"]) == rflags
    assert got["b"][0] == 0 and (np.diff(got["b"].astype(np.int64)) > 0).all()


GOOD = (1.0, 1.0, 2.0, 0)        # gains, norm, flags of a record that is accepted


# ---- candidates and fit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["line up", "line down, odd window", "gridded line", "constant", "bend", "W = 1", "W = 0", "W = 2"])
def test_a_drift_and_a_bend_give_no_candidate_and_the_tracks_own_pieces(lib, name):
    d, valid, window = FIT_CASES[name]
    tr = gstpeaq_amd.track_fit(d, valid, window=window)
    if name == "W = 2":                                 # (one segment with no neighbour: any D >= min_step is a candidate)
        assert len(gstpeaq_amd.steps_candidates(tr["knots"], window, 2 * window)) == 1
        return
    got, want, cand = run_fit(tr["knots"], window, [])
    assert cand == [] and got["n_candidates"] == 0 and got["n_accepted"] == 0
    same_pieces(got, want)
    # the pieces are the track's segments: its boundaries, its (a, e) to the bit
    S = max(len(d) - 1, 1)
    assert got["n_pieces"] == S and list(got["b"]) == [sc.start_of(k, window) for k in range(S)]
    assert got["a"].tobytes() == tr["a"].tobytes() and got["e"].tobytes() == tr["e"].tobytes()


@pytest.mark.parametrize("k", [0, 3, 6], ids=["first", "middle", "last"])
def test_one_step_replaces_its_segment_by_two_flat_pieces(lib, k):
    window = 4096
    knots = np.full(8, 37.5)
    knots[k + 1:] += 9.0
    c = sc.start_of(k, window) + 1000
    got, want, cand = run_fit(knots, window, [(c,) + GOOD])
    assert [x[0] for x in cand] == [k] and cand[0][3:] == (38, 46)
    same_pieces(got, want)
    assert got["flags"] == 0 and got["n_accepted"] == 1 and got["n_pieces"] == 8 and c in got["b"]
    assert not got["e"].any() and set(got["a"]) == {37.5, 46.5}
    j = list(got["b"]).index(c)
    assert (got["a"][:j] == 37.5).all() and (got["a"][j:] == 46.5).all()


def test_a_step_on_a_drift_continues_the_neighbours_slopes(lib):
    window = 5001
    knots = 3.0 + 0.25 * np.arange(9)
    knots[5:] += 40.0
    c = 4 * window + 3000
    got, want, cand = run_fit(knots, window, [(c,) + GOOD])
    assert [x[0] for x in cand] == [4]
    same_pieces(got, want)
    j = list(got["b"]).index(c)
    tr = gstpeaq_amd.track_fit(knots, window=window, max_e=MAX_E)
    assert tr["flags"] == 0
    assert (got["a"][j - 1], got["e"][j - 1]) == (tr["a"][3], tr["e"][3]) and (got["a"][j], got["e"][j]) == (tr["a"][5], tr["e"][5])
    assert got["n_pieces"] == 9


@pytest.mark.parametrize("where", ["before", "behind", "at lo", "at hi", "at its start"])
def test_a_c_outside_its_segments_own_outputs_moves_the_neighbours_border(lib, where):
    window, k = 4096, 3
    knots = np.full(8, -2.25)
    knots[k + 1:] -= 20.0
    start, end = sc.start_of(k, window), sc.start_of(k + 1, window)
    c = {"before": start - 700, "behind": end + 900, "at lo": k * window, "at hi": (k + 2) * window, "at its start": start}[where]
    got, want, _ = run_fit(knots, window, [(c,) + GOOD])
    same_pieces(got, want)
    # one of the segment's two pieces is empty and left out; its own border on that side is no breakpoint any more
    assert got["n_accepted"] == 1 and c in got["b"] and got["n_pieces"] == 7
    assert (start in got["b"]) == (c >= start) and (end in got["b"]) == (c < end or c == end)
    j = list(got["b"]).index(c)
    assert (got["a"][:j] == -2.25).all() and (got["a"][j:] == -22.25).all()
    # both neighbours keep at least window / 2 outputs
    assert (np.diff(got["b"].astype(np.int64)) >= window // 2).all()


def test_a_weak_record_keeps_the_segment(lib):
    window = 4096
    knots = np.full(6, 1.0)
    knots[3:] = 4.0
    tr = gstpeaq_amd.track_fit(knots, window=window)
    for found in [(9000, 1.0, 0.001, 2.0, 0), (9000, 0.0, 0.0, 0.0, 1), (9000, 0.0, 0.0, 0.0, 2)]:
        got, want, cand = run_fit(knots, window, [found])
        same_pieces(got, want)
        assert got["n_candidates"] == 1 and got["n_accepted"] == 0 and got["steps"]["flags"][0] == found[4] | WEAK
        assert got["a"].tobytes() == tr["a"].tobytes() and got["e"].tobytes() == tr["e"].tobytes() and got["flags"] == 0
    # min_gain is the caller's: the same record is accepted at a lower one
    got, want, _ = run_fit(knots, window, [(9000, 1.0, 0.001, 2.0, 0)], min_gain=0.0004)
    same_pieces(got, want)
    assert got["n_accepted"] == 1


def test_steps_in_adjacent_segments_fall_back_to_flat_lines(lib):
    """with ratio 3 two neighbours cannot both be candidates, so this runs at ratio 1"""
    window = 4096
    knots = np.array([0.0, 0.0, 0.0, 6.0, 12.0, 12.0, 12.0])
    for c2, c3, levels in [(2 * window + 3000, 3 * window + 3500, [0.0, 6.0, 12.0]),
                           (4 * window - 5, 3 * window + 5, [0.0, 12.0]),      # each c is taken as the border between the two
                           (2 * window, 5 * window, [0.0, 6.0, 12.0])]:        # ... and reaches into a neighbour that is no step
        got, want, cand = run_fit(knots, window, [(c2,) + GOOD, (c3,) + GOOD], ratio=1.0)
        assert [x[0] for x in cand] == [2, 3]
        same_pieces(got, want)
        assert got["n_accepted"] == 2 and not got["e"].any()
        assert [v for j, v in enumerate(got["a"]) if j == 0 or v != got["a"][j - 1]] == levels


def test_a_pair_flagged_through_a_step_alone_comes_out_unflagged(lib):
    window = 16384
    knots = np.full(11, 0.25)
    knots[6:] += 300.0
    tr = gstpeaq_amd.track_fit(knots, window=window)
    assert tr["flags"] == RANGE and not tr["a"].any() and np.array_equal(tr["knots"], knots)
    c = 5 * window + window // 2 + 4321
    got, want, cand = run_fit(knots, window, [(c,) + GOOD])
    assert [x[0] for x in cand] == [5] and cand[0][3:] == (0, 300)
    same_pieces(got, want)
    assert got["flags"] == 0 and got["n_accepted"] == 1 and got["max_abs_e"] == 0 and got["n_pieces"] == 11
    # not accepted: the steep segment stays, the pieces are flagged and zeroed as the track is
    got, want, _ = run_fit(knots, window, [(c, 0.0, 0.0, 1.0, 0)])
    same_pieces(got, want)
    assert got["flags"] == RANGE and not got["a"].any() and not got["e"].any() and got["max_abs_e"] > MAX_E
    assert got["n_pieces"] == 10


def test_fit_on_random_tracks(lib):
    rng = np.random.default_rng(19)
    seen = 0
    for trial in range(300):
        W = int(rng.integers(2, 14))
        window = int(rng.choice([4096, 5001, 16384]))
        knots = np.round(np.cumsum(rng.normal(0, 0.3, W)) * 256) / 256
        for _ in range(int(rng.integers(0, 4))):
            knots[int(rng.integers(1, W)):] += float(rng.choice([-300, -20, -3, 2, 7, 300]))
        ratio = float(rng.choice([1.0, 3.0]))
        n_common = W * window + int(rng.integers(0, window))
        cand = sc.candidates_model(knots, window, n_common, ratio=ratio)
        found = []
        for (k, lo, hi, _, _) in cand:
            good = rng.random() < 0.7
            found.append((int(rng.integers(lo, hi + 1)), 1.0, 1.0 if good else 0.0, 2.0, 0))
        got, want, _ = run_fit(knots, window, found, n_common=n_common, ratio=ratio)
        same_pieces(got, want)
        seen += got["n_accepted"]
    assert seen > 100


# ---- index and lengths -------------------------------------------------------------------------------------------------
PIECES = {
    "jumps up and down": ([0, 1000, 1001, 1006, 1306, 5000], [0.3, 5000.25, -5000.0, 17.5, -3.75, 2.0],
                          [1e-3, -1 / 64, 1 / 64, 0.0, 3e-4, -2e-3]),
    "one piece": ([0], [12.3], [-1e-3]),
    "a negative jump near the end": ([0, 9000], [40.0, -4000.5], [0.0, 1e-3]),
    "a positive jump past the end": ([0, 3000, 6000], [0.0, 8000.0, -10.0], [0.0, 0.0, 0.0]),
}


@pytest.mark.parametrize("name", sorted(PIECES))
def test_index_and_lengths_against_brute_force(lib, name):
    b, a, e = (np.asarray(v) for v in PIECES[name])
    i = np.arange(12000)
    m, phi, _ = sc.pieces_indices(b, a, e, i)
    for at in list(range(0, 12000, 997)) + [int(x) + d for x in b for d in (-1, 0, 1) if int(x) + d >= 0]:
        assert gstpeaq_amd.pieces_index(b, a, e, at) == (int(m[at]), int(phi[at])), at
    if name == "jumps up and down":
        assert ((i + m)[1:] < (i + m)[:-1]).any()       # i + m_i falls across a breakpoint
    for lag0 in (0, 37, -12):
        for n_ref, n_test in [(12000, 12000), (12000, 9500), (9000, 12000), (10500, 10450), (12000, 6100)]:
            sr, st, common = gstpeaq_amd.aligned_lengths(lag0, n_ref, n_test)
            want = sc.keep_brute(b, a, e, st, common, n_test)
            assert gstpeaq_amd.pieces_lengths(lag0, b, a, e, n_ref, n_test) == (sr, st, want), (lag0, n_ref, n_test)


def test_lengths_on_random_pieces(lib):
    """the argument of peaq_steps_math.h by brute force: random breakpoints, slopes up to 1/64, jumps either way"""
    rng = np.random.default_rng(5)
    cut_short = 0
    for trial in range(200):
        n = int(rng.integers(1, 7))
        b = np.concatenate([[0], np.sort(rng.choice(np.arange(1, 6000), n - 1, replace=False))]).astype(np.uint32)
        a = np.round(rng.uniform(-300, 300, n) * 256) / 256
        e = rng.uniform(-MAX_E, MAX_E, n)
        n_ref, n_test = int(rng.integers(5000, 6500)), int(rng.integers(5000, 6500))
        lag0 = int(rng.integers(-50, 50))
        sr, st, common = gstpeaq_amd.aligned_lengths(lag0, n_ref, n_test)
        want = sc.keep_brute(b, a, e, st, common, n_test)
        assert gstpeaq_amd.pieces_lengths(lag0, b, a, e, n_ref, n_test) == (sr, st, want), trial
        cut_short += want < common
    assert 20 < cut_short < 200


def test_pieces_equal_to_a_tracks_segments_have_the_tracks_index_and_lengths(lib):
    d, valid, window = FIT_CASES["bend"]
    tr = gstpeaq_amd.track_fit(d, valid, window=window)
    S = tr["n_segments"]
    b = np.array([sc.start_of(k, window) for k in range(S)], np.uint32)
    for i in list(range(0, 12 * window, 4999)) + [int(x) + dd for x in b[1:] for dd in (-1, 0)]:
        assert gstpeaq_amd.pieces_index(b, tr["a"], tr["e"], i) == gstpeaq_amd.track_index(window, tr["a"], tr["e"], i), i
    n = 12 * window + 100
    assert gstpeaq_amd.pieces_lengths(5, b, tr["a"], tr["e"], n, n) == gstpeaq_amd.track_lengths(5, window, tr["a"], tr["e"], n, n)


# ---- sizes and constants ------------------------------------------------------------------------------------------------
def test_record_sizes_and_constants(lib):
    assert lib.peaq_step_size() == C.sizeof(gstpeaq_amd.Step) == gstpeaq_amd.STEP_DTYPE.itemsize == 48
    assert lib.peaq_step_candidate_size() == C.sizeof(gstpeaq_amd.StepCandidate) == gstpeaq_amd.STEP_CANDIDATE_DTYPE.itemsize == 20
    assert lib.peaq_pieces_size() == C.sizeof(gstpeaq_amd.Pieces) == gstpeaq_amd.PIECES_DTYPE.itemsize == 24
    assert int(header_define("PEAQ_STEP_F_NONE")) == gstpeaq_amd.STEP_F_NONE == 1
    assert int(header_define("PEAQ_STEP_F_SPAN")) == gstpeaq_amd.STEP_F_SPAN == 2
    assert int(header_define("PEAQ_STEP_F_WEAK")) == gstpeaq_amd.STEP_F_WEAK == 4
    assert int(header_define("PEAQ_PIECES_F_RANGE")) == gstpeaq_amd.PIECES_F_RANGE == 2
    assert int(header_define("PEAQ_STEP_MAX_L")) == gstpeaq_amd.STEP_MAX_L == 2 ** 20 + 16384
    assert header_define("PEAQ_STEP_MAX_SPAN") == "(1u << 22)" and gstpeaq_amd.STEP_MAX_SPAN == 1 << 22
    assert float(header_define("PEAQ_STEP_MIN_STEP")) == gstpeaq_amd.STEP_MIN_STEP == 0.75
    assert float(header_define("PEAQ_STEP_RATIO")) == gstpeaq_amd.STEP_RATIO == 3.0
    assert float(header_define("PEAQ_STEP_MIN_GAIN")) == gstpeaq_amd.STEP_MIN_GAIN
    assert gstpeaq_amd.PIECES_MAX_PER_PAIR == 2 * gstpeaq_amd.DRIFT_MAX_WINDOWS and gstpeaq_amd.PIECES_MAX_PER_CALL == 1 << 20
    assert gstpeaq_amd.steps_workspace_bytes(0, 8192) == 0
    assert gstpeaq_amd.steps_workspace_bytes(3, 8192) == 3 * 2 * 64 and gstpeaq_amd.steps_workspace_bytes(1, 1) == 64
    assert gstpeaq_amd.steps_workspace_bytes(2, 1 << 30) == 2 * 1024 * 64
    assert gstpeaq_amd.steps_workspace_bytes(65535, 1 << 22) == 256 << 20


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_candidates_and_fit_refuse(lib):
    knots = f64(*([0.0] * 4 + [9.0] * 4))
    out = (gstpeaq_amd.StepCandidate * 8)()
    n = C.c_uint32(0)

    def cand(**kw):
        a = dict(knots=knots, W=8, window=4096, n_common=8 * 4096, pair=0, min_step=0.75, ratio=3.0, out=out, n=C.byref(n))
        a.update(kw)
        return lib.peaq_steps_candidates(a["knots"], a["W"], a["window"], a["n_common"], a["pair"], a["min_step"], a["ratio"],
                                         a["out"], a["n"])
    assert cand() == 0 and n.value == 1 and (out[0].pair, out[0].lo, out[0].hi, out[0].LA, out[0].LB) == (0, 3 * 4096, 5 * 4096, 0, 9)
    assert cand(pair=7) == 0 and out[0].pair == 7
    for kw, text in [(dict(window=4095), "window 4095"), (dict(window=(1 << 20) + 1), "window 1048577"), (dict(W=4097), "4097 windows"),
                     (dict(n_common=8 * 4096 - 1), "n_common 32767"), (dict(min_step=-1.0), "min_step -1.0"),
                     (dict(ratio=float("nan")), "ratio nan"), (dict(knots=None), "NULL"), (dict(out=None), "NULL"), (dict(n=None), "NULL")]:
        assert cand(**kw) == PEAQ_ERR_ARG and text in err(lib), (kw, err(lib))
    steps = (gstpeaq_amd.Step * 2)()
    steps[0].LA, steps[0].LB, steps[0].c = 0, 9, 14000
    rec = gstpeaq_amd.Pieces()
    b, a, e = u32(*[0] * 9), f64(*[0.0] * 9), f64(*[0.0] * 9)

    def fit(**kw):
        x = dict(knots=knots, W=8, window=4096, n_common=8 * 4096, min_step=0.75, ratio=3.0, min_gain=0.002, max_e=MAX_E,
                 steps=steps, n_steps=1, out=C.byref(rec), b=b, a=a, e=e)
        x.update(kw)
        return lib.peaq_steps_fit(x["knots"], x["W"], x["window"], x["n_common"], x["min_step"], x["ratio"], x["min_gain"],
                                  x["max_e"], x["steps"], x["n_steps"], x["out"], x["b"], x["a"], x["e"])
    assert fit() == 0 and rec.n_candidates == 1
    for kw, text in [(dict(n_steps=2), "n_steps 2 is not the number of candidates, 1"), (dict(n_steps=0), "n_steps 0"),
                     (dict(min_gain=-0.5), "min_gain -0.5"), (dict(max_e=0.02), "max_e 0.02"), (dict(max_e=0.0), "max_e 0.0"),
                     (dict(window=100), "window 100"), (dict(b=None), "NULL"), (dict(out=None), "NULL"), (dict(steps=None), "NULL")]:
        assert fit(**kw) == PEAQ_ERR_ARG and text in err(lib), (kw, err(lib))
    steps[0].LB = 8
    assert fit() == PEAQ_ERR_ARG and "LA 0, LB 8 are not the candidate's 0, 9" in err(lib), err(lib)


def test_locate_steps_checks_its_arguments_before_any_device(lib):
    buf = C.c_void_p(0x1000)                           # never dereferenced: every call below is refused first

    def call(**kw):
        a = dict(ctx=None, channels=2, n_pairs=2, ref=buf, test=buf, stride=50000, n_ref=u32(50000, 40000), n_test=u32(50000, 45000),
                 n_uniform=0, lag0=i32(37, -5), cand=[(0, 100, 8292, 38, 338)], out=buf)
        a.update(kw)
        cd = a["cand"]
        arr = None
        if cd is not None:
            arr = (gstpeaq_amd.StepCandidate * max(len(cd), 1))()
            for j, row in enumerate(cd):
                arr[j].pair, arr[j].lo, arr[j].hi, arr[j].LA, arr[j].LB = row
        n_cand = a.get("n_cand", len(cd) if cd is not None else 1)
        return lib.peaq_batch_locate_steps(a["ctx"], a["channels"], a["n_pairs"], a["ref"], a["test"], a["stride"], a["n_ref"],
                                           a["n_test"], a["n_uniform"], a["lag0"], n_cand, arr, a["out"], None)
    assert call() == PEAQ_ERR_ARG and "ctx is NULL" in err(lib)       # the last thing looked at
    common1 = 40000 - 5
    for kw, text in [(dict(channels=3), "channels must be 1 or 2, not 3"), (dict(n_pairs=70000), "70000 pairs"),
                     (dict(ref=None), "NULL buffer"), (dict(lag0=None), "NULL lag0"), (dict(n_test=None), "both"),
                     (dict(n_ref=u32(50001, 1)), "n_ref 50001 passes pair_stride 50000"),
                     (dict(cand=None), "NULL cand"), (dict(out=None), "NULL cand or d_out"),
                     (dict(cand=[(2, 0, 10, 1, 2)]), "candidate 0: pair 2 is not below n_pairs 2"),
                     (dict(cand=[(0, 0, 10, 1, 2), (1, 500, 500, 1, 2)]), "candidate 1: lo 500 is not below hi 500"),
                     (dict(cand=[(1, 0, common1 + 1, 1, 2)]), "hi %d passes the pair's n_common %d" % (common1 + 1, common1)),
                     (dict(cand=[(0, 0, 10, 7, 7)]), "LA and LB are both 7"),
                     (dict(cand=[(0, 0, 10, 1064961, 7)]), "a delay of 1064961"), (dict(cand=[(0, 0, 10, 7, -1064961)]), "a delay of -1064961"),
                     (dict(cand=[(0, 0, 10, 1, 2)] * 2, n_cand=65536), "65536 candidates"), (dict(n_cand=-1), "n_cand -1")]:
        assert call(**kw) == PEAQ_ERR_ARG and text in err(lib), (kw, err(lib))
    assert call(cand=[(1, 0, common1, 1064960, -1064960)]) == PEAQ_ERR_ARG and "ctx is NULL" in err(lib)   # the limits themselves pass


def test_cut_pieces_checks_its_arguments_before_any_device(lib):
    buf, buf2 = C.c_void_p(0x100000), C.c_void_p(0x40000000)

    def call(**kw):
        a = dict(ctx=None, channels=2, n_pairs=2, d_in=buf, in_stride=9000, n_in=u32(9000, 8000), skip=u32(10, 0), n_keep=u32(8000, 7000),
                 n_pieces=u32(3, 1), piece_stride=3, b=u32(0, 100, 105, 0, 0, 0), a=f64(0.5, 5000.0, -5000.0, 0.0, 0.0, 0.0),
                 e=f64(MAX_E, -MAX_E, 0.0, 0.0, 0.0, 0.0), d_out=buf2, out_stride=8000)
        a.update(kw)
        return lib.peaq_batch_cut_pieces(a["ctx"], a["channels"], a["n_pairs"], a["d_in"], a["in_stride"], a["n_in"], a["skip"],
                                         a["n_keep"], a["n_pieces"], a["piece_stride"], a["b"], a["a"], a["e"], a["d_out"],
                                         a["out_stride"], None)
    assert call() == PEAQ_ERR_ARG and "ctx is NULL" in err(lib)       # lines that do not meet and jumps of 5000 pass
    for kw, text in [(dict(channels=0), "channels must be 1 or 2, not 0"), (dict(n_pairs=65536), "65536 pairs"),
                     (dict(b=None), "NULL n_in, skip, n_keep, n_pieces, b, a or e"), (dict(d_out=None), "NULL buffer"),
                     (dict(skip=u32(1001, 0)), "skip 1001 + n_keep 8000 passes in_stride 9000"), (dict(out_stride=7999), "out_stride 7999"),
                     (dict(n_in=u32(9001, 1)), "n_in 9001 passes in_stride 9000"), (dict(d_out=buf), "overlaps"),
                     (dict(n_pieces=u32(0, 1)), "pair 0: n_pieces 0"), (dict(n_pieces=u32(3, 4)), "pair 1: n_pieces 4"),
                     (dict(b=u32(1, 100, 105, 0, 0, 0)), "pair 0, piece 0: b 1 is not 0"),
                     (dict(b=u32(0, 100, 100, 0, 0, 0)), "pair 0, piece 2: b 100 is not above the piece before it at 100"),
                     (dict(b=u32(0, 100, 99, 0, 0, 0)), "piece 2: b 99 is not above"),
                     (dict(a=f64(0.5, 1048577.0, 0.0, 0.0, 0.0, 0.0)), "piece 1: a 1048577"),
                     (dict(a=f64(float("nan"), 0.0, 0.0, 0.0, 0.0, 0.0)), "piece 0: a nan"),
                     (dict(e=f64(0.0, 0.0, 0.0157, 0.0, 0.0, 0.0)), "piece 2: e 0.0157"),
                     (dict(e=f64(0.0, 0.0, 0.0, float("inf"), 0.0, 0.0)), "pair 1, piece 0: e inf")]:
        assert call(**kw) == PEAQ_ERR_ARG and text in err(lib), (kw, err(lib))
    many = 8193
    assert call(n_pairs=1, n_pieces=u32(many), piece_stride=many, b=u32(*range(many)), a=f64(*[0.0] * many), e=f64(*[0.0] * many)) == \
        PEAQ_ERR_ARG and "n_pieces 8193" in err(lib)


def test_estimate_steps_and_run_pair_steps_check_their_arguments_before_any_device(lib):
    buf = C.c_void_p(0x1000)

    def call(**kw):
        a = dict(window=4096, R=1024, min_corr=0.5, max_e=MAX_E, min_step=0.75, ratio=3.0, min_gain=0.002, w_max=7, steps_stride=6,
                 piece_stride=12, steps=buf, pieces=buf, b=buf)
        a.update(kw)
        return lib.peaq_batch_estimate_steps(None, 2, 1, buf, buf, 30000, None, None, 30000, i32(3), a["window"], a["R"], a["min_corr"],
                                             a["max_e"], a["min_step"], a["ratio"], a["min_gain"], a["w_max"], buf, buf, None,
                                             C.cast(buf, C.POINTER(gstpeaq_amd.Track)), C.cast(buf, C.POINTER(C.c_double)),
                                             a["steps_stride"], C.cast(a["steps"], C.POINTER(gstpeaq_amd.Step)),
                                             C.cast(a["pieces"], C.POINTER(gstpeaq_amd.Pieces)), a["piece_stride"],
                                             C.cast(a["b"], C.POINTER(C.c_uint32)), C.cast(buf, C.POINTER(C.c_double)),
                                             C.cast(buf, C.POINTER(C.c_double)), None)
    assert call() == PEAQ_ERR_ARG and "ctx is NULL" in err(lib)
    for kw, text in [(dict(min_step=-1.0), "min_step -1.0"), (dict(ratio=-3.0), "ratio -3.0"), (dict(min_gain=float("inf")), "min_gain inf"),
                     (dict(max_e=0.1), "max_e 0.1"), (dict(steps_stride=5), "steps_stride 5 is below"), (dict(piece_stride=11), "piece_stride 11 is below"),
                     (dict(steps=None), "NULL steps, pieces, b, a or e"), (dict(window=100), "window 100"), (dict(w_max=0), "w_max")]:
        assert call(**kw) == PEAQ_ERR_ARG and text in err(lib), (kw, err(lib))
    x = np.zeros((9000, 2), np.float32)
    fp = x.ctypes.data_as(C.POINTER(C.c_float))
    out = f64(*[0.0] * 64)

    def pair(**kw):
        a = dict(ctx=None, channels=2, level=92.0, rate=48000, max_lag=4096, window=4096, mode=0, max_gain_db=40.0)
        a.update(kw)
        return lib.peaq_run_pair_steps(a["ctx"], 0, a["channels"], a["level"], a["rate"], a["max_lag"], a["window"], a["mode"],
                                       a["max_gain_db"], fp, 9000, fp, 9000, None, None, None, None, 0, None, out)
    assert pair() == PEAQ_ERR_ARG and "NULL" in err(lib)
    for kw, text in [(dict(window=4095), "window 4095"), (dict(max_lag=0), "max_lag"), (dict(level=131.0), "playback level"),
                     (dict(channels=3), "channels"), (dict(mode=99), "mode")]:
        assert pair(**kw) == PEAQ_ERR_ARG and text in err(lib), (kw, err(lib))


def test_python_keywords():
    """steps= excludes track=, drift= and subsample= and needs align=, with a message, before anything runs"""
    for kw, text in [(dict(align=4096, steps=True, track=True), "steps= and track= exclude each other"),
                     (dict(align=4096, steps=True, drift=True), "steps= and drift= exclude each other"),
                     (dict(align=4096, steps=4096, subsample=True), "steps= and subsample=True exclude each other"),
                     (dict(steps=True), "steps= requires align=")]:
        with pytest.raises(gstpeaq_amd.PeaqError, match=text):
            gstpeaq_amd.run_pair(None, 0, np.zeros((10, 2), np.float32), np.zeros((10, 2), np.float32), **kw)
        with pytest.raises(gstpeaq_amd.PeaqError, match=text):
            gstpeaq_amd.capi._need_align(kw.get("subsample", False), kw.get("align"), kw.get("drift", False), kw.get("track", False),
                                         kw.get("steps", False))

"""-m gpu: live alignment of a session (peaq_session_set_align / peaq_session_align_read / peaq_session_watch_read,
include/peaq_amd.h "live alignment").

Acquisition: a session whose test pad is the reference pad's programme L samples late (or early) holds its stream until
the probe is there, reads the delay the batch aligner reads from the same samples -- the record bit for bit -- and then
IS a plain session fed the streams as scored, ref[skip_ref:] and test[skip_test:]: bit for bit in the basic version, to
the project's tolerance for one stream cut into other launches in the advanced version.  Watch: every window's sums
against math.fsum over the header's rule B, and records that do not depend on how the stream was pushed.

The streams are synthetic cases of tests/cases.py of 5000 to 31700 samples whose first 4096 samples are not silent (the
stereo cases of tests/test_gpu_meter.py begin with silence: a probe over them reads the aligner's lag 0 with norm 0,
which is the silent-probe test's subject and nobody else's).

The case that fails without the feature: LATE (seed 75 mono, seed 76 stereo, 31700 samples), advanced version, L = +37.
On the CPU oracle the aligned pair reads ODG +0.154 (mono) / +0.156 (stereo) and the pair with the test signal 37 samples
late -3.611 / -3.610: a gap of 3.7, asserted here as "at least 1"."""
import math

import numpy as np
import pytest

import cases as case_defs
import gpu_common as gpu
from test_gpu_broker import _same
from test_gpu_meter import feed, same_bits

pytestmark = pytest.mark.gpu

CASES = {
    "late_mono": dict(name="late_mono", kind="synth", seed=75, channels=1, n=31700),
    "late_stereo": dict(name="late_stereo", kind="synth", seed=76, channels=2, n=31700),
    "short_stereo": dict(name="short_stereo", kind="synth", seed=69, channels=2, n=5000),
    "ragged_mono": dict(name="ragged_mono", kind="synth", seed=83, channels=1, n=20000, test_trim=700),
}
MAX_LAG, PROBE = 256, 4096
LAGS = (0, 37, -113, 256)
_INPUTS, _PLAIN = {}, {}


def inputs(name):
    if name not in _INPUTS:
        ref, test = case_defs.make_inputs(CASES[name])
        assert np.abs(ref[:PROBE]).max() > 0.01 and np.abs(test[:PROBE]).max() > 0.01
        _INPUTS[name] = (ref, test)
    return _INPUTS[name]


def delayed(ref, test, L):
    """the pair with the test pad L samples late (L < 0: the reference pad -L samples late): digital silence first"""
    late = np.zeros((abs(L), ref.shape[1]), dtype=np.float32)
    return (ref, np.concatenate([late, test])) if L >= 0 else (np.concatenate([late, ref]), test)


def run_session(ref, test, advanced, how="whole", setup=None):
    """-> (result, session) of a session fed the pair: "whole" (one pad whole, then the other) or "feed" (uneven pushes)"""
    import gstpeaq_amd
    s = gstpeaq_amd.Session(gpu.ctx(), advanced, ref.shape[1])
    if setup:
        setup(s)
    if how == "whole":
        s.push(0, ref)
        s.push(1, test)
    else:
        feed(s, ref, test)
    s.flush()
    return s.results(), s


def plain_result(name, advanced):
    """the plain session on the case's own pair -- the streams as scored of every delayed version of it --, once"""
    key = (name, advanced, gpu.mode() if advanced else "default")
    if key not in _PLAIN:
        res, s = run_session(*inputs(name), advanced)
        s.close()
        _PLAIN[key] = res
    return _PLAIN[key]


def batch_record(ref, test, n_ref, n_test, max_lag=MAX_LAG):
    """estimate_delay over the leading n_ref / n_test samples"""
    import torch
    import gstpeaq_amd
    n = max(n_ref, n_test)
    pad = [np.zeros((1, n, ref.shape[1]), dtype=np.float32) for _ in range(2)]
    pad[0][0, :n_ref] = ref[:n_ref]
    pad[1][0, :n_test] = test[:n_test]
    d = gstpeaq_amd.estimate_delay(gpu.ctx(), torch.from_numpy(pad[0]).cuda(), torch.from_numpy(pad[1]).cuda(), max_lag,
                                   n_ref=[n_ref], n_test=[n_test])
    return {k: v[0].item() for k, v in d.items()}


def check_record(got, ref, test, L, probe=PROBE):
    import gstpeaq_amd
    assert got["acquired"] is True
    want = gstpeaq_amd.live_align_plan(MAX_LAG, len(ref), len(test), got["lag"], probe=probe)
    assert (got["probe_ref"], got["probe_test"], got["skip_ref"], got["skip_test"]) == want, (got, want)
    rec = batch_record(ref, test, got["probe_ref"], got["probe_test"])
    for k in ("lag", "peak", "runner_up", "norm"):
        assert got[k] == rec[k] or (got[k] != got[k] and rec[k] != rec[k]), (k, got, rec)
    if L is not None:
        assert got["lag"] == L, got


def check_result(res, want, advanced, where):
    if advanced:
        _same(res, want, where, rtol=gpu.tol("chunks"))
        assert (res["frames"], res["fb_blocks"]) == (want["frames"], want["fb_blocks"]), where
    else:
        assert same_bits(res, want), (where, res, want)


def align(probe=PROBE, watch=None, max_lag=MAX_LAG):
    return lambda s: s.set_align(max_lag, probe=probe, watch=watch)


@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
@pytest.mark.parametrize("L", LAGS)
@pytest.mark.parametrize("name", ["late_mono", "late_stereo", "ragged_mono"])
def test_record_and_result_are_the_aligners_and_the_plain_sessions(name, L, advanced, fir_mode):
    ref, test = delayed(*inputs(name), L)
    want = plain_result(name, advanced)
    for how in ("whole", "feed"):
        res, s = run_session(ref, test, advanced, how, align())
        got = s.align_read()
        s.close()
        check_record(got, ref, test, L)
        assert (got["skip_ref"], got["skip_test"]) == (max(-L, 0), max(L, 0))
        check_result(res, want, advanced, (name, L, how))


@pytest.mark.parametrize("name", ["late_mono", "late_stereo"])
def test_without_the_alignment_the_late_pair_reads_an_odg_at_least_1_lower(name):
    ref, test = delayed(*inputs(name), 37)
    late, s = run_session(ref, test, True)
    s.close()
    aligned, s = run_session(ref, test, True, setup=align())
    assert s.align_read()["lag"] == 37
    s.close()
    print(name, "aligned", aligned["odg"], "late", late["odg"])
    assert late["odg"] <= aligned["odg"] - 1.0, (late["odg"], aligned["odg"])
    assert late["odg"] < -3.0 < 0.0 < aligned["odg"] + 0.5


def test_the_stream_holds_until_the_probe_is_there():
    ref, test = delayed(*inputs("late_stereo"), 37)
    import gstpeaq_amd
    s = gstpeaq_amd.Session(gpu.ctx(), False, 2)
    s.set_align(MAX_LAG, probe=PROBE)
    nothing = dict(acquired=False, probe_ref=0, probe_test=0, skip_ref=0, skip_test=0, lag=0, peak=0.0, runner_up=0.0,
                   norm=0.0)
    assert s.align_read() == nothing
    s.push(0, ref)                                          # one pad whole: nothing can be estimated
    assert s.align_read() == nothing and s.results()["frames"] == 0
    s.push(1, test[:PROBE - 1])
    assert s.align_read() == nothing and s.results()["frames"] == 0
    s.push(1, test[PROBE - 1:PROBE])                        # the sample that completes the probe
    got = s.align_read()
    assert got["acquired"] and got["lag"] == 37 and (got["probe_ref"], got["probe_test"]) == (PROBE, PROBE)
    assert s.results()["frames"] == (PROBE - 37 - 2048) // 1024 + 1
    s.push(1, test[PROBE:])
    s.flush()
    assert s.align_read() == got
    assert same_bits(s.results(), plain_result("late_stereo", False))
    s.close()


@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
def test_a_flush_before_the_probe_is_full_acquires_over_what_is_there(advanced):
    ref, test = delayed(*inputs("short_stereo"), 37)
    res, s = run_session(ref, test, advanced, "feed", align(probe=8192))
    got = s.align_read()
    s.close()
    assert (got["probe_ref"], got["probe_test"]) == (5000, 5037)
    check_record(got, ref, test, 37, probe=8192)
    check_result(res, plain_result("short_stereo", advanced), advanced, "short")


def test_a_silent_probe_leaves_the_stream_unaligned_and_says_why():
    ref, test = inputs("late_mono")
    quiet = np.zeros((PROBE, 1), dtype=np.float32)
    ref, test = np.concatenate([quiet, ref]), np.concatenate([quiet, test[37:]])
    res, s = run_session(ref, test, False, "feed", align())
    got = s.align_read()
    s.close()
    assert got["acquired"] and (got["lag"], got["norm"], got["peak"], got["skip_ref"], got["skip_test"]) == (0, 0.0, 0.0, 0, 0)
    plain, s = run_session(ref, test, False)
    s.close()
    assert same_bits(res, plain)


def test_a_probe_that_is_not_a_number_reads_norm_nan():
    ref, test = (x.copy() for x in inputs("late_mono"))
    test[100] = np.nan
    _, s = run_session(ref, test, False, setup=align())
    got = s.align_read()
    s.close()
    assert got["acquired"] and got["lag"] == 0 and math.isnan(got["norm"]) and got["skip_test"] == 0


def test_lifecycle_set_align_only_before_the_stream_and_reset_arms_again():
    import gstpeaq_amd
    ref, test = inputs("late_mono")
    s = gstpeaq_amd.Session(gpu.ctx(), False, 1)
    with pytest.raises(gstpeaq_amd.PeaqError, match="peaq_session_align_read: no acquisition is set"):
        s.align_read()
    with pytest.raises(gstpeaq_amd.PeaqError, match="peaq_session_watch_read: the watch is off"):
        s.watch_read()
    s.set_align(0, watch=4)
    with pytest.raises(gstpeaq_amd.PeaqError, match="peaq_session_align_read: no acquisition is set"):
        s.align_read()
    assert s.watch_read() is None
    s.set_align(MAX_LAG, probe=PROBE)
    with pytest.raises(gstpeaq_amd.PeaqError, match="peaq_session_watch_read: the watch is off"):
        s.watch_read()
    with pytest.raises(gstpeaq_amd.PeaqError, match="peaq_session_set_align: max_lag 16385 is outside"):
        s.set_align(16385)
    first = delayed(ref, test, 37)
    s.push(0, first[0][:100])
    with pytest.raises(gstpeaq_amd.PeaqError, match=r"peaq_session_set_align: the stream has begun \(100 samples pushed\)"):
        s.set_align(MAX_LAG, probe=PROBE)
    with pytest.raises(gstpeaq_amd.PeaqError, match="the stream has begun"):
        s.set_align(0)
    s.push(0, first[0][100:])
    s.push(1, first[1])
    s.flush()
    assert s.align_read()["lag"] == 37
    assert same_bits(s.results(), plain_result("late_mono", False))
    s.reset()                                               # holds again, for another delay
    assert s.align_read()["acquired"] is False
    second = delayed(ref, test, -113)
    feed(s, *second)
    s.flush()
    got = s.align_read()
    assert got["lag"] == -113 and got["skip_ref"] == 113
    assert same_bits(s.results(), plain_result("late_mono", False))
    s.reset()
    s.set_align(0)                                          # right after a reset it is accepted again: off
    s.push(0, first[0])
    s.push(1, first[1])
    s.flush()
    late, p = run_session(*first, False)
    p.close()
    assert same_bits(s.results(), late)
    s.close()


@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
@pytest.mark.parametrize("L", [37, -113])
def test_with_the_meter_the_readings_are_those_of_the_stream_as_scored(L, advanced):
    name, W, H = "late_stereo", 4, 2
    ref, test = delayed(*inputs(name), L)

    def metered(pair, setup):
        res, s = run_session(*pair, advanced, "feed", setup)
        rows, dropped = s.meter_read()
        assert dropped == 0
        s.close()
        return rows, res

    got, res = metered((ref, test), lambda s: (s.set_meter(W, H, 256), s.set_align(MAX_LAG, probe=PROBE)))
    want, plain = metered(inputs(name), lambda s: s.set_meter(W, H, 256))
    fields = ("index", "start", "length", "first_frame", "n_frames", "first_block", "n_blocks", "frames", "fb_blocks")
    assert len(got) == len(want) > 10
    assert [{k: g[k] for k in fields} for g in got] == [{k: w[k] for k in fields} for w in want]
    for g, w in zip(got, want):
        _same(g, w, (L, advanced, g["index"]), rtol=gpu.tol("chunks") if advanced else 1e-12)
    check_result(res, plain, advanced, ("metered", L))


# ---- the watch --------------------------------------------------------------------------------------------------------
W = 4


def rule_b(ref, test, k, W=W):
    """window k of rule B by math.fsum: (c[63], e_ref, e_test)"""
    r, t = ref.astype(np.float64).sum(axis=1), test.astype(np.float64).sum(axis=1)
    n = np.arange(1024 * k * W + 512, 1024 * (k + 1) * W + 512)
    c = np.array([math.fsum(r[n] * t[n + d]) for d in range(-31, 32)])
    return c, math.fsum(r[n] * r[n]), math.fsum(t[n] * t[n])


def watched(ref, test, how, advanced=False, W=W, flush=True, max_lag=0):
    """-> {index: window} of every window read after each push (how: samples per push on both pads, or "feed" / "whole")"""
    import gstpeaq_amd
    s = gstpeaq_amd.Session(gpu.ctx(), advanced, ref.shape[1])
    s.set_align(max_lag, probe=PROBE if max_lag else None, watch=W)
    seen = {}

    def read(*_):
        w = s.watch_read()
        if w is not None:
            again = s.watch_read()
            assert same_window(w, again)
            assert seen.setdefault(w["index"], w) is w or same_window(seen[w["index"]], w)

    if how == "feed":
        feed(s, ref, test, on_push=read)
    elif how == "whole":
        s.push(0, ref)
        s.push(1, test)
        read()
    else:
        for at in range(0, max(len(ref), len(test)), how):
            s.push(0, ref[at:at + how])
            s.push(1, test[at:at + how])
            read()
    if flush:
        s.flush()
        read()
    s.close()
    return seen


def same_window(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a) and a.keys() == b.keys()


@pytest.mark.parametrize("delta", [0, 5, -31])
@pytest.mark.parametrize("name", ["late_mono", "late_stereo"])
def test_watch_values_against_rule_b(name, delta):
    import gstpeaq_amd
    ref = inputs(name)[0]
    ref, test = delayed(ref, ref.copy(), delta)
    seen = watched(ref, test, 1024 * W)                     # a window per push: every window is read
    whole = (min(len(ref), len(test)) - 2048) // 1024 + 1
    assert sorted(seen) == list(range(whole // W)) and len(seen) >= 7
    for k, w in seen.items():
        c, e_ref, e_test = rule_b(ref, test, k)
        norm = math.sqrt(e_ref * e_test)
        assert (w["first_frame"], w["n_frames"]) == (k * W, W)
        assert np.abs(w["c"] - c).max() <= 1e-9 * norm, (k, np.abs(w["c"] - c).max() / norm)
        assert abs(w["e_ref"] - e_ref) <= 1e-9 * norm and abs(w["e_test"] - e_test) <= 1e-9 * norm, k
        assert w["offset"] == delta, (k, w["offset"])
        pick = gstpeaq_amd.delay_watch_pick(w["c"], w["e_ref"], w["e_test"])
        assert {f: w[f] for f in pick} == pick
        assert w["norm"] == math.sqrt(w["e_ref"] * w["e_test"]) and w["peak"] == w["c"][delta + 31] > 0.9 * w["norm"]


def test_watch_sees_a_delay_that_steps_in_mid_stream():
    ref = inputs("late_stereo")[0]
    step = 20480                                            # 5 windows of 4 frames
    test = np.concatenate([ref[:step], ref[step - 3:-3]])   # 3 samples late from there on
    seen = watched(ref, test, 1024 * W)
    assert len(seen) >= 7
    for k, w in seen.items():
        if 1024 * (k + 1) * W + 512 + 31 <= step:
            assert w["offset"] == 0, (k, w["offset"])
        elif 1024 * k * W + 512 - 31 >= step:
            assert w["offset"] == 3, (k, w["offset"])
        c, e_ref, e_test = rule_b(ref, test, k)
        assert np.abs(w["c"] - c).max() <= 1e-9 * math.sqrt(e_ref * e_test)
    assert [w["offset"] for _, w in sorted(seen.items())][:4] == [0] * 4 and seen[max(seen)]["offset"] == 3


def test_watch_counts_whole_frames_only_and_reads_none_before_a_window_is_complete():
    ref = inputs("late_stereo")[0]
    assert watched(ref[:3072], ref[:3072], "whole") == {}   # two frames (and the flush frame)
    assert watched(ref[:4096 + 500], ref[:4096 + 500], "whole") == {}   # three whole frames and the flush frame
    n = 5 * 1024 + 500                                      # four whole frames: one window; the flush frame is not a fifth
    before = watched(ref[:n], ref[:n], "whole", flush=False)
    after = watched(ref[:n], ref[:n], "whole")
    assert list(before) == list(after) == [0] and same_window(before[0], after[0])
    assert (after[0]["first_frame"], after[0]["n_frames"]) == (0, 4)
    # an incomplete last window is discarded: 29 whole frames are three windows of 8, the last five frames are none
    assert sorted(watched(ref, ref, "whole", W=8)) == [2]
    assert sorted(watched(ref, ref, 8192, W=8)) == [0, 1, 2]


@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
def test_watch_records_do_not_depend_on_the_pushes_or_the_run(advanced):
    ref, test = delayed(*inputs("late_stereo"), 5)
    runs = [watched(ref, test, how, advanced) for how in (1024 * W, 1024 * W, "feed", 1000, "whole")]
    assert sorted(runs[0]) == list(range(7))
    for other in runs[1:]:
        assert other and set(other) <= set(runs[0])
        for k, w in other.items():
            assert same_window(w, runs[0][k]), k
    assert sorted(runs[3]) == sorted(runs[0])               # pushes of 1000 samples: at most one new frame each
    assert max(runs[4]) == 6


def test_watch_behind_an_acquisition_sees_the_aligned_stream():
    ref = inputs("late_mono")[0]
    ref, test = delayed(ref, ref.copy(), 37)
    seen = watched(ref, test, 1024 * W, max_lag=MAX_LAG)
    assert len(seen) >= 6 and all(w["offset"] == 0 for w in seen.values())
    c, e_ref, e_test = rule_b(ref, test[37:], 0)
    assert np.abs(seen[0]["c"] - c).max() <= 1e-9 * math.sqrt(e_ref * e_test)


# ---- the broker -------------------------------------------------------------------------------------------------------
BROKER_LAGS = (0, 37, -113, 256, -256, 5, -1, 100, -200, 64, 181)      # eleven slots: more than a tick's eight estimates
BROKER_PROBE = 36864                                                    # above the back-pressure limit of 32768 samples
CASES["long_stereo"] = dict(name="long_stereo", kind="synth", seed=76, channels=2, n=50000)


def whole_frames(n):
    return (n - 2048) // 1024 + 1 if n >= 2048 else 0


@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
def test_broker_slots_acquire_eight_a_tick_and_equal_the_aligned_sessions(advanced):
    """Eleven slots opened over three ticks, then fed in step in buffers of 4096: all eleven probes are complete in the
    same tick.  That tick enqueues eight estimates, the next reads them, releases those eight and enqueues the other
    three.  The watch with windows of one frame counts the frames a slot has run: a released slot advances by what a
    tick takes (eight frames, or what is there) in every tick, whatever the others wait for.  A held slot's samples pass
    the back-pressure limit before its probe is there: the pushes return all the same."""
    import gstpeaq_amd
    ref0, test0 = inputs("long_stereo")
    pairs = [delayed(ref0, test0, L) for L in BROKER_LAGS]
    b = gstpeaq_amd.Broker(gpu.ctx(), 2, max_sessions=12, advanced=advanced)
    b.set_align(MAX_LAG, probe=BROKER_PROBE, watch=1)
    sids = []
    for n_open in (4, 4, 3):
        sids += [b.open() for _ in range(n_open)]
        b.tick()
    done = {sid: 0 for sid in sids}

    def frames_run(sid):
        w = b.watch_read(sid)
        return 0 if w is None else w["index"] + 1

    acquired_after_tick, pos, flushed = [], 0, set()
    while len(flushed) < len(sids) or any(b.align_read(sid)["acquired"] is False for sid in sids):
        for sid, (ref, test) in zip(sids, pairs):
            b.push(sid, 0, ref[pos:pos + 4096])
            b.push(sid, 1, test[pos:pos + 4096])
            if pos + 4096 >= max(len(ref), len(test)) and sid not in flushed:
                b.flush(sid)
                flushed.add(sid)
        pos += 4096
        before = {sid: b.align_read(sid) for sid in sids if sid not in flushed}   # (a read of a flushed slot would tick)
        b.tick()
        acquired_after_tick.append(sum(b.align_read(sid)["acquired"] for sid in sids if sid not in flushed))
        for sid, (ref, test) in zip(sids, pairs):
            if sid in flushed or not before[sid]["acquired"]:
                continue
            there = whole_frames(min(min(pos, len(ref)) - before[sid]["skip_ref"], min(pos, len(test)) - before[sid]["skip_test"]))
            # (at least: a push that finds more than the back-pressure limit waiting ticks by itself)
            now = frames_run(sid)
            assert min(done[sid] + 8, there) <= now <= there and now > done[sid], (sid, pos, done[sid], now, there)
            done[sid] = now
    # 36864 samples are there after nine pushes: nothing yet after that tick, eight slots after the next, all after the third
    assert acquired_after_tick[:8] == [0] * 8 and acquired_after_tick[8:11] == [0, 8, 11], acquired_after_tick
    for sid, (ref, test), L in zip(sids, pairs, BROKER_LAGS):
        res = b.results(sid)
        got = b.align_read(sid)
        want_res, s = run_session(ref, test, advanced, "whole", align(probe=BROKER_PROBE))
        want = s.align_read()
        s.close()
        assert got == want and got["lag"] == L and (got["probe_ref"], got["probe_test"]) == (BROKER_PROBE, BROKER_PROBE), (L, got, want)
        check_result(res, want_res, advanced, ("broker", L))
    b.close()


def test_broker_slot_that_is_flushed_before_its_probe_is_full_and_a_reopened_slot():
    import gstpeaq_amd
    ref, test = delayed(*inputs("short_stereo"), 37)
    b = gstpeaq_amd.Broker(gpu.ctx(), 2, max_sessions=2)
    b.set_align(MAX_LAG, probe=8192)
    sid = b.open()
    b.push(sid, 0, ref)
    b.push(sid, 1, test)
    assert b.tick() == 0 and b.align_read(sid)["acquired"] is False      # held: 5000 samples are no probe
    assert b.results(sid)["frames"] == 0                                  # (and no reason to tick)
    b.flush(sid)
    got = b.align_read(sid)                                               # drives the held, flushed slot to its delay
    assert got["acquired"] and got["lag"] == 37 and (got["probe_ref"], got["probe_test"]) == (5000, 5037)
    check_record(got, ref, test, 37, probe=8192)
    assert same_bits(b.results(sid), plain_result("short_stereo", False))
    b.close_session(sid)
    assert b.open() == sid                                                # the slot again: it holds again
    assert b.align_read(sid)["acquired"] is False
    ref, test = delayed(*inputs("short_stereo"), -113)
    b.push(sid, 0, ref)
    b.push(sid, 1, test)
    b.flush(sid)
    assert same_bits(b.results(sid), plain_result("short_stereo", False))  # results drives it as well
    assert b.align_read(sid)["lag"] == -113
    other = b.open()                                                      # a flush with nothing pushed: nothing to estimate
    b.flush(other)
    assert b.align_read(other) == dict(acquired=True, probe_ref=0, probe_test=0, skip_ref=0, skip_test=0, lag=0, peak=0.0,
                                       runner_up=0.0, norm=0.0)
    b.close()


@pytest.mark.parametrize("how", ["manual", "thread", "multi"])
def test_broker_watch_is_the_sessions_bit_for_bit(how):
    import gstpeaq_amd
    ref, test = delayed(*inputs("late_stereo"), 5)
    want = watched(ref, test, 1024 * W)
    b = gstpeaq_amd.Broker(gpu.ctx(), 2, max_sessions=4, devices=[0, 0] if how == "multi" else None)
    b.set_align(0, watch=W)
    if how == "thread":
        b.start(500)
    sid = b.open()
    seen = {}
    for at in range(0, len(test), 4096):
        b.push(sid, 0, ref[at:at + 4096])
        b.push(sid, 1, test[at:at + 4096])
        if how != "thread":
            b.tick()
            w = b.watch_read(sid)
            if w is not None:
                seen[w["index"]] = w
                assert same_window(w, b.watch_read(sid))
    b.flush(sid)
    b.results(sid)
    w = b.watch_read(sid)
    seen[w["index"]] = w
    if how == "thread":
        b.stop()
    b.close()
    assert max(seen) == max(want) == 6 and (how == "thread" or sorted(seen) == sorted(want))
    for k, w in seen.items():
        assert same_window(w, want[k]), k


def test_what_a_broker_refuses_of_the_alignment():
    import gstpeaq_amd
    b = gstpeaq_amd.Broker(gpu.ctx(), 1, max_sessions=2)
    with pytest.raises(gstpeaq_amd.PeaqError, match="peaq_broker_align_read: no acquisition is set"):
        b.align_read(0)
    with pytest.raises(gstpeaq_amd.PeaqError, match="peaq_broker_watch_read: the watch is off"):
        b.watch_read(0)
    with pytest.raises(gstpeaq_amd.PeaqError, match="peaq_broker_set_align: probe 2303 is outside"):
        b.set_align(256, probe=2303)
    b.set_align(MAX_LAG, probe=PROBE, watch=4)
    with pytest.raises(gstpeaq_amd.PeaqError, match="peaq_broker_align_read: session is not open"):
        b.align_read(1)
    sid = b.open()
    assert b.align_read(sid)["acquired"] is False and b.watch_read(sid) is None
    with pytest.raises(gstpeaq_amd.PeaqError, match="peaq_broker_set_align: session 0 is open"):
        b.set_align(0)
    b.close_session(sid)
    b.set_align(0)                                                        # off again
    with pytest.raises(gstpeaq_amd.PeaqError, match="peaq_broker_align_read: no acquisition is set"):
        b.align_read(0)
    b.start(1000)
    with pytest.raises(gstpeaq_amd.PeaqError, match="set the alignment before peaq_broker_start"):
        b.set_align(MAX_LAG)
    b.stop()
    b.close()

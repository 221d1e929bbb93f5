"""-m gpu: the band rows of the live meter (peaq_session_set_meter_bands / peaq_session_meter_read_bands and the
broker's, include/peaq_amd.h "meter: band rows").

With the band meter on every reading carries rows 0 .. 3 of the band summary over the window's counted frames.  The
expected rows are a NumPy restatement of the definition: the planes NMR and EXC_REF of peaq_batch_run_bands reduced over
each reading's frames [first_frame, first_frame + n_frames), with the above-boundary flags of peaq_batch_run_trace --
first .. last frame above the boundary, sums in frame order.  Sums and maxima hold to the tolerance
tests/test_gpu_meter.py holds its scores to (1e-12 relative in the basic version, the "chunks" tolerance in the advanced
one), the counts exactly."""
import numpy as np
import pytest

import cases as case_defs
import gpu_common as gpu
from test_gpu_broker import _same
from test_gpu_meter import feed, same_bits

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in case_defs.e2e_cases() if c["advanced"] == 0}
INPUTS = ("gap3_stereo", "gap1_mono", "synth_ragged_test_short", "synth_sub_frame")
THRESHOLD = 1.41253754462275                            # 1.5 dB: the disturbed count's
CORNERS = ("gap3_stereo", 4, 2)                         # the input and geometry that must cover the rule's corners
_BATCH, _SESSION = {}, {}


def inputs(name):
    return case_defs.make_inputs(CASES[name])


def rtol(advanced):
    return gpu.tol("chunks") if advanced else 1e-12


def batch_planes(name, advanced):
    """(nmr [T, channels, nb], exc_ref [T, channels, nb], above [T]) of the whole pair, once per (stream, version)"""
    import gstpeaq_amd
    key = (name, advanced)
    if key not in _BATCH:
        ref, test = inputs(name)
        b = gstpeaq_amd.run_pair_bands(gpu.ctx(), advanced, ref, test, planes=("nmr", "exc_ref"))
        t = gstpeaq_amd.run_pair_trace(gpu.ctx(), advanced, ref, test)
        above = (t["frames"]["flags"] & 1) != 0         # PEAQ_TRACE_ABOVE
        assert len(above) == len(b["nmr"]) == gstpeaq_amd.frame_count(len(ref), len(test))
        # an exact disturbed count must not test rounding
        near = np.abs(b["nmr"] - THRESHOLD) <= 1e-9 * THRESHOLD
        print(name, "advanced" if advanced else "basic", "frames", len(above), "above", int(above.sum()),
              "closest NMR to the threshold, relative:", float(np.abs(b["nmr"] / THRESHOLD - 1).min()))
        assert not near.any(), (name, advanced, np.argwhere(near))
        _BATCH[key] = (b["nmr"], b["exc_ref"], above)
    return _BATCH[key]


def counted(above, a, n):
    """the counted frames [lo, hi] of the window [a, a + n), or None"""
    idx = np.flatnonzero(above[a:a + n])
    return (a + idx[0], a + idx[-1]) if len(idx) else None


def expected_rows(name, advanced, a, n):
    """the definition, restated: -> [channels, 4, row]"""
    nmr, exc, above = batch_planes(name, advanced)
    channels, nb = nmr.shape[1], nmr.shape[2]
    out = np.zeros((channels, 4, (nb + 2) & ~1))
    span = counted(above, a, n)
    if span is None:
        return out
    for f in range(span[0], span[1] + 1):               # FP64, in frame order
        out[:, 0, :nb] += nmr[f]
        out[:, 1, :nb] = np.where(nmr[f] > out[:, 1, :nb], nmr[f], out[:, 1, :nb])
        out[:, 2, :nb] += nmr[f] > THRESHOLD
        out[:, 3, :nb] += exc[f]
    out[:, :, nb] = span[1] - span[0] + 1
    return out


def corners(name, advanced, W, H):
    """how many of the stream's readings sit in each corner of the counting rule"""
    import gstpeaq_amd
    ref, test = inputs(name)
    _, _, above = batch_planes(name, advanced)
    rows = gstpeaq_amd.meter_windows(len(ref), len(test), W, H)
    spans = [(r["first_frame"], r["n_frames"], counted(above, r["first_frame"], r["n_frames"])) for r in rows]
    return dict(empty=sum(1 for _, _, c in spans if c is None),
                leading=sum(1 for a, _, c in spans if c is not None and c[0] > a),
                trailing=sum(1 for a, n, c in spans if c is not None and c[1] < a + n - 1))


def check_rows(got, name, advanced, where):
    """every reading's rows against the restatement"""
    nb = 55 if advanced else 109
    for g in got:
        want = expected_rows(name, advanced, g["first_frame"], g["n_frames"])
        at = (where, g["index"])
        assert g["bands"].shape == want.shape, at
        for k in (0, 1, 3):                             # the sums and the maximum
            np.testing.assert_allclose(g["bands"][:, k, :nb], want[:, k, :nb], rtol=rtol(advanced), atol=0, err_msg=str(at))
        assert np.array_equal(g["bands"][:, 2, :nb], want[:, 2, :nb]), at           # the disturbed counts
        assert np.array_equal(g["bands"][:, :, nb:], want[:, :, nb:]), at           # the counted frames, in every row
        assert np.array_equal(g["counted"], want[:, 0, nb].astype(np.int64)), at
        for k, key in enumerate(("nmr_sum", "nmr_max", "nmr_disturbed", "exc_ref_sum")):
            assert np.array_equal(g[key], g["bands"][:, k, :nb]), (at, key)


def same_rows(a, b):
    return a["index"] == b["index"] and np.array_equal(a["bands"], b["bands"])


def metered_run(name, advanced, W, H, depth=256, whole=False, bands=True, read_early=True):
    """-> (all readings in the order they were read, the session's own end result)"""
    import gstpeaq_amd
    ref, test = inputs(name)
    s = gstpeaq_amd.Session(gpu.ctx(), advanced, ref.shape[1])
    s.set_meter(W, H, depth, bands=bands)
    got = []

    def read(_n_both=None):
        rows, dropped = s.meter_read(bands=bands)
        assert dropped == 0
        got.extend(rows)

    if whole:
        s.push(0, ref)
        s.push(1, test)
    else:
        feed(s, ref, test, on_push=read if read_early else None)
    s.flush()
    read()
    assert s.meter_read(bands=bands) == ([], 0)
    res = s.results()
    s.close()
    return got, res


def session_rows(name, advanced, W, H):
    """the uneven, out-of-step pushes, read after every push: once per (stream, version, geometry)"""
    key = (name, advanced, W, H)
    if key not in _SESSION:
        _SESSION[key] = metered_run(name, advanced, W, H)
    return _SESSION[key]


# ---- 1. rows against the batch traces ---------------------------------------------------------------------------------
@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
def test_the_chosen_input_covers_the_corners_of_the_counting_rule(advanced):
    c = corners(*CORNERS[:1], advanced, *CORNERS[1:])
    print(CORNERS, "advanced" if advanced else "basic", c)
    assert c["empty"] >= 1, c                           # a window without a counted frame
    assert c["leading"] >= 1, c                         # a window whose first frame is not above the boundary
    assert c["trailing"] >= 1, c                        # a window that ends on a dropped trailing run


@pytest.mark.parametrize("W,H", [(16, 4), (4, 2)])
@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
@pytest.mark.parametrize("name", INPUTS)
def test_session_rows_equal_the_reduced_batch_planes(name, advanced, W, H):
    import gstpeaq_amd
    if (name, W, H) == CORNERS:
        c = corners(name, advanced, W, H)
        assert c["empty"] >= 1 and c["leading"] >= 1 and c["trailing"] >= 1, c
    got, _ = session_rows(name, advanced, W, H)
    ref, test = inputs(name)
    rows = gstpeaq_amd.meter_windows(len(ref), len(test), W, H)
    assert [{k: g[k] for k in rows[0]} for g in got] == rows
    check_rows(got, name, advanced, (name, advanced, W, H))


# ---- 2. a window with W >= T ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
@pytest.mark.parametrize("name", ["gap3_stereo", "synth_sub_frame"])
def test_a_window_over_the_whole_stream_has_the_rows_of_the_band_summary(name, advanced):
    import gstpeaq_amd
    got, _ = metered_run(name, advanced, 200, 200)
    assert len(got) == 1 and got[0]["index"] == 0 and got[0]["first_frame"] == 0
    ref, test = inputs(name)
    want = gstpeaq_amd.run_pair_band_summary(gpu.ctx(), advanced, ref, test)["rows"][:, :4, :]
    nb = 55 if advanced else 109
    g = got[0]["bands"]
    print(name, "advanced" if advanced else "basic", "bit for bit:", bool(np.array_equal(g, want)))
    for k in (0, 1, 3):
        np.testing.assert_allclose(g[:, k, :nb], want[:, k, :nb], rtol=rtol(advanced), atol=0)
    assert np.array_equal(g[:, 2, :nb], want[:, 2, :nb]) and np.array_equal(g[:, :, nb:], want[:, :, nb:])
    check_rows(got, name, advanced, (name, advanced, "whole"))


# ---- 3. one push of the whole stream ----------------------------------------------------------------------------------
@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
@pytest.mark.parametrize("name", ["gap3_stereo", "synth_ragged_test_short"])
def test_one_push_of_the_whole_stream_gives_the_same_rows(name, advanced):
    """crosses the 64-frame launches of a session"""
    whole, _ = metered_run(name, advanced, 16, 4, whole=True)
    uneven, _ = session_rows(name, advanced, 16, 4)
    assert len(whole) == len(uneven) > 20
    check_rows(whole, name, advanced, (name, advanced, "one push"))
    if not advanced:                                    # (the basic version's launches are the same arithmetic however cut)
        assert all(same_rows(a, b) for a, b in zip(whole, uneven))


def test_rows_read_early_are_the_rows_read_after_the_flush():
    early, _ = session_rows("gap3_stereo", False, 16, 4)
    late, _ = metered_run("gap3_stereo", False, 16, 4, read_early=False)
    assert len(late) == len(early) > 20
    assert all(same_rows(a, b) and same_bits(a, b) for a, b in zip(early, late))


# ---- 4. bands on and off ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
def test_the_band_meter_does_not_change_the_scores(advanced):
    import gstpeaq_amd
    on, res_on = session_rows("gap3_stereo", advanced, 16, 4)
    off, res_off = metered_run("gap3_stereo", advanced, 16, 4, bands=False)
    assert len(on) == len(off) > 20 and "bands" not in off[0]
    for a, b in zip(on, off):
        assert a["index"] == b["index"]
        if advanced:
            _same(a, b, a["index"], rtol=gpu.tol("chunks"))
        else:
            assert same_bits(a, b), (a, b)
    if advanced:
        _same(res_on, res_off, "end result", rtol=gpu.tol("chunks"))
    else:
        assert same_bits(res_on, res_off), (res_on, res_off)
    # with bands off the rows cannot be read; the plain read goes on working with bands on
    s = gstpeaq_amd.Session(gpu.ctx(), advanced, 2)
    s.set_meter(16, 4)
    with pytest.raises(gstpeaq_amd.PeaqError, match=r"peaq_session_meter_read_bands: the band meter is off"):
        s.meter_read(bands=True)
    s.set_meter_bands(True)
    ref, test = inputs("synth_ragged_test_short")
    s.push(0, ref[:30000])
    s.push(1, test[:30000])
    plain, dropped = s.meter_read()
    assert dropped == 0 and len(plain) == 4 and "bands" not in plain[0]      # 28 frames: windows 0 .. 3 of 16 / 4
    s.close()


# ---- 5. ring and refusals ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
def test_a_reader_that_falls_behind_loses_the_oldest_rows(advanced):
    import gstpeaq_amd
    name = "synth_ragged_test_short"
    ref, test = inputs(name)
    n_rows = len(gstpeaq_amd.meter_windows(len(ref), len(test), 16, 4))
    s = gstpeaq_amd.Session(gpu.ctx(), advanced, 2)
    s.set_meter(16, 4, depth=2, bands=True)
    feed(s, ref, test)
    s.flush()
    got, dropped = s.meter_read(bands=True)
    assert dropped == n_rows - 2 and [g["index"] for g in got] == [n_rows - 2, n_rows - 1]
    check_rows(got, name, advanced, (name, advanced, "depth 2"))
    assert s.meter_read(bands=True) == ([], 0)
    s.close()


def test_reset_starts_the_rows_over():
    import gstpeaq_amd
    first, second = inputs("gap3_stereo"), inputs("synth_ragged_test_short")
    s = gstpeaq_amd.Session(gpu.ctx(), False, 2)
    s.set_meter(4, 2, 256, bands=True)
    feed(s, *first)                                     # (neither flushed nor read: the rows are gone with the reset)
    s.reset()                                           # (the meter and its bands stay set)
    feed(s, *second)
    s.flush()
    got, dropped = s.meter_read(bands=True)
    s.close()
    assert dropped == 0 and got[0]["index"] == 0
    assert len(got) == len(gstpeaq_amd.meter_windows(len(second[0]), len(second[1]), 4, 2))
    check_rows(got, "synth_ragged_test_short", False, "after reset")


def test_what_a_session_refuses():
    import gstpeaq_amd
    s = gstpeaq_amd.Session(gpu.ctx(), False, 1)
    with pytest.raises(gstpeaq_amd.PeaqError, match=r"peaq_session_set_meter_bands: the meter is off"):
        s.set_meter_bands(True)
    s.set_meter(17, 1)                                  # K = 17: fine for the meter, too many for its bands
    with pytest.raises(gstpeaq_amd.PeaqError, match=r"peaq_session_set_meter_bands: .*keeps 17 windows open at once"):
        s.set_meter_bands(True)
    with pytest.raises(gstpeaq_amd.PeaqError, match=r"keeps 17 windows open at once"):
        s.set_meter(17, 1, bands=True)
    s.set_meter(16, 4, 257)
    with pytest.raises(gstpeaq_amd.PeaqError, match=r"peaq_session_set_meter_bands: depth 257"):
        s.set_meter_bands(True)
    s.set_meter(16, 4, bands=True)
    assert s.meter_read(bands=True) == ([], 0)
    s.set_meter(16, 4)                                  # a new set_meter: the bands are off again
    with pytest.raises(gstpeaq_amd.PeaqError, match=r"the band meter is off"):
        s.meter_read(bands=True)
    s.push(0, np.zeros((100, 1), dtype=np.float32))
    with pytest.raises(gstpeaq_amd.PeaqError,
                       match=r"peaq_session_set_meter_bands: the stream has begun \(100 samples pushed\)"):
        s.set_meter_bands(True)
    s.reset()
    s.set_meter_bands(True)                             # right after a reset it is accepted again
    s.close()


# ---- 6. the broker ----------------------------------------------------------------------------------------------------
BROKER_STREAMS = ("gap3_stereo", "synth_ragged_test_short", "synth_s0_stereo", "synth_sub_frame", "synth_frame_and_hop")
BROKER_REOPENED = "synth_swapped"                       # takes the slot of synth_sub_frame in mid-run


def broker_run(advanced, multi):
    """five sessions opened at different ticks, fed in 4096-sample buffers, tick() after every round and a read after
    every tick, one slot closed and opened again for a sixth stream (the walk of tests/test_gpu_meter.py)"""
    import gstpeaq_amd
    b = gstpeaq_amd.Broker(gpu.ctx(), 2, max_sessions=8, advanced=advanced, devices=[0, 0] if multi else None)
    b.set_meter(16, 4, 256, bands=True)
    live, got = {}, {}                                  # name -> [sid, position], readings

    def read(name):
        rows, dropped = b.meter_read(live[name][0], bands=True)
        assert dropped == 0
        got.setdefault(name, []).extend(rows)

    pending = list(BROKER_STREAMS)
    rounds = 0
    while pending or live:
        if pending and rounds % 2 == 0:                 # a new session every other tick
            live[pending.pop(0)] = [b.open(), 0]
        for name in list(live):
            sid, pos = live[name]
            ref, test = inputs(name)
            b.push(sid, 0, ref[pos:pos + 4096])
            b.push(sid, 1, test[pos:pos + 4096])
            live[name][1] = pos + 4096
            if live[name][1] >= max(len(ref), len(test)):
                b.flush(sid)
                b.results(sid)                          # (drains the session: its flush has run)
                read(name)
                assert b.meter_read(sid, bands=True) == ([], 0)
                b.close_session(sid)
                del live[name]
                if name == "synth_sub_frame":           # its slot again, for another stream, in mid-run
                    again = b.open()
                    assert again == sid or multi        # (two shards: the emptier one takes it)
                    live[BROKER_REOPENED] = [again, 0]
        b.tick()
        for name in live:
            read(name)
        rounds += 1
    b.close()
    return got


@pytest.mark.parametrize("multi", [False, True], ids=["one_device", "two_shards"])
@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
def test_broker_rows_equal_a_session_s(advanced, multi):
    got = broker_run(advanced, multi)
    assert sorted(got) == sorted(BROKER_STREAMS + (BROKER_REOPENED,))
    nb = 55 if advanced else 109
    for name, rows in got.items():
        want, _ = session_rows(name, advanced, 16, 4)
        assert [g["index"] for g in rows] == [w["index"] for w in want], name
        for g, w in zip(rows, want):
            at = (name, advanced, multi, g["index"])
            assert (g["first_frame"], g["n_frames"]) == (w["first_frame"], w["n_frames"]), at
            for k in (0, 1, 3):
                np.testing.assert_allclose(g["bands"][:, k, :nb], w["bands"][:, k, :nb], rtol=rtol(advanced), atol=0,
                                           err_msg=str(at))
            assert np.array_equal(g["bands"][:, 2, :nb], w["bands"][:, 2, :nb]), at
            assert np.array_equal(g["counted"], w["counted"]) and np.array_equal(g["bands"][:, :, nb:], w["bands"][:, :, nb:]), at


def test_what_a_broker_refuses():
    import gstpeaq_amd
    b = gstpeaq_amd.Broker(gpu.ctx(), 1, max_sessions=2)
    with pytest.raises(gstpeaq_amd.PeaqError, match=r"peaq_broker_set_meter_bands: the meter is off"):
        b.set_meter_bands(True)
    b.set_meter(17, 1)
    with pytest.raises(gstpeaq_amd.PeaqError, match=r"peaq_broker_set_meter_bands: .*keeps 17 windows open at once"):
        b.set_meter_bands(True)
    b.set_meter(16, 4)
    sid = b.open()
    with pytest.raises(gstpeaq_amd.PeaqError, match=r"peaq_broker_meter_read_bands: the band meter is off"):
        b.meter_read(sid, bands=True)
    with pytest.raises(gstpeaq_amd.PeaqError, match=r"peaq_broker_set_meter_bands: session 0 is open"):
        b.set_meter_bands(True)
    b.close_session(sid)
    b.set_meter_bands(True)
    sid = b.open()
    assert b.meter_read(sid, bands=True) == ([], 0)
    b.close()

"""-m gpu: the live meter of a session (peaq_session_set_meter / peaq_session_meter_read, include/peaq_amd.h "meter";
DESIGN.md 29).

A metered session delivers, while it streams and at its flush, the readings that peaq_meter_readings lists for its
stream, and every reading is the batch side's window (basic version) or span (advanced version) of the row's {start,
length} -- to the project's tolerance for one stream cut into launches in different ways, `frames` and `fb_blocks`
exactly.  tests/test_meter_host.py asserts that every row of the lengths and geometries used here has such a window, so
the comparison leaves no reading out.  The meter does not disturb the stream, keeps the `depth` newest readings, and
starts over with peaq_session_reset."""
import numpy as np
import pytest

import cases as case_defs
import gpu_common as gpu
from test_gpu_broker import _same

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in case_defs.e2e_cases() if c["advanced"] == 0}
# 30 frames, the last the flush frame, and the whole blocks reach e_k / 192 of the window that ends on it before the
# flush: the filter-bank path finishes that window while the stream runs and has to take the flush block into it after all
CASES["blocks_end_early"] = dict(name="blocks_end_early", kind="synth", seed=77, channels=2, n=31700)
CASES["short_stereo"] = dict(name="short_stereo", kind="synth", seed=78, channels=2, n=5000)   # four frames
CHUNKS = (1000, 7777, 300, 20000, 4096, 1, 2500, 12345)
_BATCH = {}


def inputs(name):
    return case_defs.make_inputs(CASES[name])


def batch_readings(name, advanced, W, H):
    """the batch side's reading of every row of the stream's list, computed once per (stream, version, geometry, engine)"""
    import gstpeaq_amd
    key = (name, advanced, W, H, gpu.mode() if advanced else "default")
    if key not in _BATCH:
        ref, test = inputs(name)
        rows = gstpeaq_amd.meter_windows(len(ref), len(test), W, H)
        assert rows and all(r["length"] for r in rows)
        spans = np.array([[r["start"], r["length"]] for r in rows], dtype=np.uint32)
        run = gstpeaq_amd.run_pair_adv_spans if advanced else gstpeaq_amd.run_pair_windows
        _BATCH[key] = (rows, run(gpu.ctx(), ref, test, spans)["spans" if advanced else "windows"])
    return _BATCH[key]


def complete_windows(n_both, W, H):
    """windows delivered once n_both samples are present on both pads"""
    frames = (n_both - 2048) // 1024 + 1 if n_both >= 2048 else 0
    return (frames - W) // H + 1 if frames >= W else 0


def feed(s, ref, test, on_push=None):
    """uneven pushes, the two pads out of step (the test pad a few chunks behind, then ahead)"""
    pos, i = [0, 0], 0
    sig = (ref, test)
    while pos[0] < len(ref) or pos[1] < len(test):
        pad = 0 if i % 5 in (0, 1, 3) else 1
        if pos[pad] >= len(sig[pad]):
            pad = 1 - pad
        k = CHUNKS[i % len(CHUNKS)]
        s.push(pad, sig[pad][pos[pad]:pos[pad] + k])
        pos[pad] = min(pos[pad] + k, len(sig[pad]))
        i += 1
        if on_push:
            on_push(min(pos))


def check_against_batch(got, name, advanced, W, H):
    rows, want = batch_readings(name, advanced, W, H)
    assert [{k: g[k] for k in rows[0]} for g in got] == rows
    for g, row, w in zip(got, rows, want):
        where = (name, advanced, W, H, row["index"])
        _same(g, w, where, rtol=gpu.tol("chunks") if advanced else 1e-12)
        assert g["frames"] == row["n_frames"] and g["fb_blocks"] == w["fb_blocks"], where
        assert g["fb_blocks"] == (row["n_blocks"] if advanced else 0), where


def same_bits(a, b):
    return (np.array_equal(a["movs"], b["movs"], equal_nan=True) and
            all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in ("di", "odg", "totalsnr", "frames", "fb_blocks")))


def metered_run(name, advanced, W, H, depth=256, whole=False):
    """-> (all readings in the order they were read, the session's own end result)"""
    import gstpeaq_amd
    ref, test = inputs(name)
    s = gstpeaq_amd.Session(gpu.ctx(), advanced, ref.shape[1])
    s.set_meter(W, H, depth)
    got = []

    def read(n_both):
        rows, dropped = s.meter_read()
        assert dropped == 0
        got.extend(rows)
        assert len(got) == complete_windows(n_both, W, H), (name, n_both)

    if whole:
        s.push(0, ref)
        s.push(1, test)
    else:
        feed(s, ref, test, on_push=read)
    s.flush()
    rows, dropped = s.meter_read()
    assert dropped == 0
    got.extend(rows)
    assert s.meter_read() == ([], 0)
    res = s.results()
    s.close()
    return got, res


@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
@pytest.mark.parametrize("name", ["gap3_stereo", "gap1_mono", "synth_ragged_test_short", "synth_sub_frame"])
def test_session_readings_equal_the_batch_windows(name, advanced, fir_mode):
    got, _ = metered_run(name, advanced, 16, 4)
    check_against_batch(got, name, advanced, 16, 4)


def test_a_reading_read_early_is_the_reading_read_after_the_flush():
    """a delivered reading never changes: the same pushes, read after every push and read once at the end (basic
    version, whose launches are the same arithmetic from run to run), bit for bit"""
    import gstpeaq_amd
    early, _ = metered_run("gap3_stereo", False, 16, 4)
    ref, test = inputs("gap3_stereo")
    s = gstpeaq_amd.Session(gpu.ctx(), False, 2)
    s.set_meter(16, 4, 256)
    feed(s, ref, test)
    s.flush()
    late, dropped = s.meter_read()
    s.close()
    assert dropped == 0 and len(late) == len(early) > 20
    assert all(same_bits(a, b) and a["index"] == b["index"] for a, b in zip(early, late))


@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
@pytest.mark.parametrize("name", ["gap3_stereo", "synth_ragged_test_short"])
def test_one_push_of_the_whole_stream_reads_the_same(name, advanced, fir_mode):
    """crosses the 64-frame / 120-block launches of a session; in the advanced version the FFT path is the whole stream
    ahead of the filter-bank path while the push runs"""
    got, _ = metered_run(name, advanced, 16, 4, whole=True)
    check_against_batch(got, name, advanced, 16, 4)


@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
@pytest.mark.parametrize("W,H", [(1, 1), (64, 1), (5, 9)])
@pytest.mark.parametrize("name", ["gap3_stereo", "synth_ragged_test_short"])
def test_geometries(name, W, H, advanced):
    got, _ = metered_run(name, advanced, W, H)
    check_against_batch(got, name, advanced, W, H)
    if (W, H) == (5, 9) and name == "gap3_stereo":      # 117 frames: the flush falls into the gap [113, 117), no cut reading
        assert got[-1]["first_frame"] == 108 and got[-1]["n_frames"] == 5, got[-1]


@pytest.mark.parametrize("W,H", [(1, 1), (4, 2)])
def test_a_window_whose_blocks_end_before_its_flush_frame_takes_the_flush_block(W, H):
    n, T = 31700, 30
    e = 1024 * (T + 1)                                  # of the window that ends on the flush frame
    assert 192 * (e // 192) <= n < e and (T - W) % H == 0
    got, _ = metered_run("blocks_end_early", True, W, H)
    (g,) = [g for g in got if g["first_frame"] + W == T]   # the complete window that ends on the flush frame
    assert g["n_frames"] == W and g["first_block"] + g["n_blocks"] == n // 192 + 1 == g["first_block"] + g["fb_blocks"]
    check_against_batch(got, "blocks_end_early", True, W, H)


@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
@pytest.mark.parametrize("name", ["gap3_stereo", "synth_sub_frame"])
def test_a_window_over_the_whole_stream_is_the_end_result_bit_for_bit(name, advanced):
    got, res = metered_run(name, advanced, 200, 200)
    assert len(got) == 1 and got[0]["index"] == 0 and got[0]["first_frame"] == 0
    assert same_bits(got[0], res), (got[0], res)
    check_against_batch(got, name, advanced, 200, 200)


@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
def test_the_meter_does_not_disturb_the_stream(advanced):
    import gstpeaq_amd
    ref, test = inputs("gap3_stereo")
    _, metered = metered_run("gap3_stereo", advanced, 16, 4)
    s = gstpeaq_amd.Session(gpu.ctx(), advanced, 2)
    feed(s, ref, test)
    s.flush()
    plain = s.results()
    s.close()
    assert same_bits(metered, plain), (metered, plain)


@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
def test_a_reader_that_falls_behind_loses_the_oldest_readings(advanced):
    import gstpeaq_amd
    name = "synth_ragged_test_short"
    ref, test = inputs(name)
    rows, want = batch_readings(name, advanced, 16, 4)
    s = gstpeaq_amd.Session(gpu.ctx(), advanced, 2)
    s.set_meter(16, 4, depth=2)
    feed(s, ref, test)
    s.flush()
    got, dropped = s.meter_read()
    assert dropped == len(rows) - 2 and [g["index"] for g in got] == [len(rows) - 2, len(rows) - 1]
    for g, w in zip(got, want[-2:]):
        _same(g, w, (advanced, g["index"]), rtol=gpu.tol("chunks") if advanced else 1e-12)
    assert s.meter_read() == ([], 0)
    s.close()


@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
def test_reset_starts_the_meter_over(advanced):
    import gstpeaq_amd
    first, second = inputs("gap3_stereo"), inputs("synth_ragged_test_short")
    s = gstpeaq_amd.Session(gpu.ctx(), advanced, 2)
    s.set_meter(16, 4, 256)
    feed(s, *first)                                     # (neither flushed nor read: the readings are gone with the reset)
    s.reset()
    s.set_meter(16, 4, 256)
    feed(s, *second)
    s.flush()
    got, dropped = s.meter_read()
    s.close()
    assert dropped == 0
    check_against_batch(got, "synth_ragged_test_short", advanced, 16, 4)


def test_an_advanced_reading_read_early_does_not_change():
    """the advanced version, where a window's two halves come from two kernels and one window is stored a second time at
    the flush: the readings handed out while the stream runs are those a second session of the same pushes holds in its
    ring after the flush, nothing read before."""
    import gstpeaq_amd
    ref, test = inputs("blocks_end_early")
    runs = []
    for read_early in (True, False):
        s = gstpeaq_amd.Session(gpu.ctx(), True, 2)
        s.set_meter(4, 2, depth=64)
        got = []
        feed(s, ref, test, on_push=(lambda _n: got.extend(s.meter_read()[0])) if read_early else None)
        s.flush()
        rows, dropped = s.meter_read()
        got.extend(rows)
        s.close()
        runs.append((got, dropped))
    (early, d0), (late, d1) = runs
    assert d0 == 0 and d1 == 0 and [g["index"] for g in late] == [g["index"] for g in early]
    check_against_batch(early, "blocks_end_early", True, 4, 2)
    check_against_batch(late, "blocks_end_early", True, 4, 2)
    # (two runs of the advanced version agree to the chunks tolerance, not to the bit: the bank adds with LDS atomics)
    for a, b in zip(early, late):
        _same(a, b, a["index"], rtol=gpu.tol("chunks"))


# ---- the broker -------------------------------------------------------------------------------------------------------
BROKER_STREAMS = ("gap3_stereo", "synth_ragged_test_short", "blocks_end_early", "synth_sub_frame", "short_stereo")
BROKER_REOPENED = "synth_swapped"                       # takes the slot of synth_sub_frame in mid-run


def broker_run(advanced, how):
    """five sessions opened at different ticks, fed in 4096-sample buffers, one slot closed and opened again for a sixth
    stream; how = "manual" (tick() after every round, the meter read as it goes), "multi" (the same through
    peaq_broker_create_multi on devices {0, 0}) or "thread" (the broker's own tick thread, read after the flush only)"""
    import gstpeaq_amd
    b = gstpeaq_amd.Broker(gpu.ctx(), 2, max_sessions=8, advanced=advanced, devices=[0, 0] if how == "multi" else None)
    b.set_meter(16, 4, 256)
    if how == "thread":
        b.start(500)
    live, got, done = {}, {}, {}                        # name -> [sid, position], readings, finished

    def read(name):
        rows, dropped = b.meter_read(live[name][0])
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
                done[name] = b.results(sid)             # (drains the session: its flush has run)
                read(name)
                assert b.meter_read(sid) == ([], 0)
                b.close_session(sid)
                del live[name]
                if name == "synth_sub_frame":           # its slot again, for another stream, in mid-run
                    again = b.open()
                    assert again == sid or how == "multi"   # (two shards: the emptier one takes it)
                    live[BROKER_REOPENED] = [again, 0]
        if how != "thread":
            b.tick()
            for name in live:
                read(name)
        rounds += 1
    if how == "thread":
        b.stop()
    b.close()
    return got, done


@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
def test_broker_of_two_shards_reads_the_batch_windows(advanced):
    """(the shards' contexts are their own, on the default engine)"""
    got, _ = broker_run(advanced, "multi")
    assert sorted(got) == sorted(BROKER_STREAMS + (BROKER_REOPENED,))
    for name, rows in got.items():
        check_against_batch(rows, name, advanced, 16, 4)


@pytest.mark.parametrize("how", ["manual", "thread"])
@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
def test_broker_sessions_read_the_batch_windows(advanced, how, fir_mode):
    got, done = broker_run(advanced, how)
    assert sorted(got) == sorted(BROKER_STREAMS + (BROKER_REOPENED,))
    for name, rows in got.items():
        check_against_batch(rows, name, advanced, 16, 4)
    if how == "manual":                                 # the metered stream's own end result is still the batch's
        whole = gpu.run_batch([inputs(n) for n in done], advanced, 2)
        for w, (name, res) in zip(whole, done.items()):
            _same(res, w, name, rtol=gpu.tol("chunks") if advanced else 1e-12)


def test_a_flush_with_a_backlog_keeps_the_two_halves_of_a_reading_together():
    """advanced version, every frame its own window, depth 1 (a ring of three slots), the flush asked for while four
    ticks' worth of frames wait: through the ticks that work the backlog off the blocks must not run ahead of the
    frames, or a reading's filter-bank half would be a later window's.  Read after every tick."""
    import gstpeaq_amd
    name = "blocks_end_early"
    ref, test = inputs(name)
    rows, want = batch_readings(name, True, 1, 1)
    b = gstpeaq_amd.Broker(gpu.ctx(), 2, max_sessions=2, advanced=True)
    b.set_meter(1, 1, depth=1)
    sid = b.open()
    b.push(sid, 0, ref)
    b.push(sid, 1, test)                                # (ticks by itself until no more than the backlog waits)
    b.flush(sid)
    got, ticks = [], 0
    idle = 0
    while idle < 2:
        idle = idle + 1 if b.tick() == 0 else 0
        ticks += 1
        got.extend(b.meter_read(sid)[0])
    b.close()
    assert ticks >= 5 and len(got) >= 4 and got[-1]["index"] == rows[-1]["index"]
    for g in got:
        k = g["index"]
        assert {f: g[f] for f in rows[k]} == rows[k]
        _same(g, want[k], (name, k), rtol=gpu.tol("chunks"))
        assert g["fb_blocks"] == want[k]["fb_blocks"] == rows[k]["n_blocks"]


def test_what_a_broker_refuses():
    import gstpeaq_amd
    b = gstpeaq_amd.Broker(gpu.ctx(), 1, max_sessions=2)
    with pytest.raises(gstpeaq_amd.PeaqError, match="peaq_broker_meter_read: the meter is off"):
        b.meter_read(0)
    with pytest.raises(gstpeaq_amd.PeaqError, match="depth 4097 is outside"):
        b.set_meter(16, 4, 4097)
    b.set_meter(16, 4)
    with pytest.raises(gstpeaq_amd.PeaqError, match="peaq_broker_meter_read: session is not open"):
        b.meter_read(1)
    sid = b.open()
    assert b.meter_read(sid) == ([], 0)
    with pytest.raises(gstpeaq_amd.PeaqError, match="peaq_broker_set_meter: session 0 is open"):
        b.set_meter(8, 8)
    b.close_session(sid)
    b.start(1000)
    with pytest.raises(gstpeaq_amd.PeaqError, match="set the meter before peaq_broker_start"):
        b.set_meter(8, 8)
    b.stop()
    b.close()


def test_what_a_session_refuses():
    import gstpeaq_amd
    s = gstpeaq_amd.Session(gpu.ctx(), False, 1)
    with pytest.raises(gstpeaq_amd.PeaqError, match="peaq_session_meter_read: the meter is off"):
        s.meter_read()
    s.set_meter(0)
    with pytest.raises(gstpeaq_amd.PeaqError, match="peaq_session_meter_read: the meter is off"):
        s.meter_read()
    with pytest.raises(gstpeaq_amd.PeaqError, match="keeps 65 windows open at once"):
        s.set_meter(65, 1)
    s.set_meter(16, 4)
    assert s.meter_read() == ([], 0)
    s.push(0, np.zeros((100, 1), dtype=np.float32))
    with pytest.raises(gstpeaq_amd.PeaqError, match=r"peaq_session_set_meter: the stream has begun \(100 samples pushed\)"):
        s.set_meter(8, 8)
    with pytest.raises(gstpeaq_amd.PeaqError, match="the stream has begun"):
        s.set_meter(0)
    s.reset()
    s.set_meter(8, 8)                                   # right after a reset it is accepted again
    s.close()

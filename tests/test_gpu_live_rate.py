"""-m gpu: live rate conversion (include/peaq_amd.h "live rate conversion").

The primitive: slices of resample(x) of a whole signal, bit for bit, from peaq_batch_resample_range over segments that
begin at 0, hold exactly their span, run to the stream's end, are empty, pass the kernel's tile by one, and travel
several to a call; positions past 2^33; rows that miss a sample.  The streams: a session or a broker slot with rates IS
the plain one fed the resample()d signals -- bit for bit in the basic version, to the project's tolerance for one stream
cut into other launches in the advanced version --, with the meter and with live alignment as well.

Rates: one of each class, 44100 (L = 160, tiled in the batch converter), 32000 (L = 3), 11025 (L = 640, the batch's
`any` kernel), 96000 (L = 1, down).  Signals: synthetic cases of tests/cases.py, 5000 to 31700 raw samples.

The case that shows the point: BOX (seed 76 stereo, 31700 samples at 44.1 kHz, the test signal the reference through
one 8-tap mean), basic version.  On the CPU oracle the pair pushed as it is reads ODG -1.920, the pair converted to
48 kHz first -1.053: a gap of 0.87, asserted here as "at least 0.4"."""
import numpy as np
import pytest

import cases as case_defs
import gpu_common as gpu
from test_gpu_broker import _same
from test_gpu_live_align import batch_record, check_result
from test_gpu_meter import feed, same_bits

pytestmark = pytest.mark.gpu

RATES = (44100, 32000, 11025, 96000)
CASES = {
    "mono": dict(name="mono", kind="synth", seed=75, channels=1, n=31700),
    "stereo": dict(name="stereo", kind="synth", seed=76, channels=2, n=31700),
    "short_stereo": dict(name="short_stereo", kind="synth", seed=69, channels=2, n=5000),
    "ragged_mono": dict(name="ragged_mono", kind="synth", seed=83, channels=1, n=20000, test_trim=700),
    "box": dict(name="box", kind="synth", seed=76, channels=2, n=31700, from_ref=1, box8_test=1),
}
_INPUTS, _CONVERTED, _PLAIN = {}, {}, {}


def inputs(name):
    if name not in _INPUTS:
        _INPUTS[name] = case_defs.make_inputs(CASES[name])
    return _INPUTS[name]


def converted(x, rate, key=None):
    """resample() of the whole signal, on the host (kept per key)"""
    import torch
    import gstpeaq_amd
    if rate == 48000:
        return x
    if key is None or (key, rate) not in _CONVERTED:
        y, n = gstpeaq_amd.resample(gpu.ctx(), torch.from_numpy(np.ascontiguousarray(x[None])).cuda(), rate)
        y = y[0, :int(n[0])].cpu().numpy().copy()
        if key is None:
            return y
        _CONVERTED[(key, rate)] = y
    return _CONVERTED[(key, rate)]


def pair_48k(name, rates):
    ref, test = inputs(name)
    return converted(ref, rates[0], (name, 0)), converted(test, rates[1], (name, 1))


# ---- the primitive ---------------------------------------------------------------------------------------------

def segments_of(g, rate, n, n_out):
    """(out_first, out_count, in_base, in_have, in_total) of the slices the issue lists"""
    segs = []
    lo, hi = g.live_rate_span(rate, 0, 700)
    segs.append((0, 700, 0, hi, None))                                   # begins at m = 0
    first = n_out // 3
    lo, hi = g.live_rate_span(rate, first, 300)
    assert lo > 0
    segs.append((first, 300, lo, hi - lo, None))                         # the row holds exactly the span
    first = n_out - 500
    lo, hi = g.live_rate_span(rate, first, 500)
    assert hi > n                                                        # (its taps pass the end)
    segs.append((first, 500, lo, n - lo, n))                             # to the stream's end, in_total set
    segs.append((n_out // 2, 0, 0, 0, None))                             # nothing
    first = n_out // 5 + 3
    lo, hi = g.live_rate_span(rate, first, g.RANGE_TILE + 1)
    segs.append((first, g.RANGE_TILE + 1, lo - min(lo, 11), hi - lo + min(lo, 11) + 5, None))   # the tile and one; a wider row
    return segs


def run_segments(g, x, rate, segs, shift=0):
    """the segments' rows cut from x -> the rows of outputs (numpy); shift = (outputs, inputs) moves every position"""
    import torch
    so, si = shift if shift else (0, 0)
    stride = max([s[3] for s in segs] + [1])
    rows = np.zeros((len(segs), stride, x.shape[1]), dtype=np.float32)
    for i, (_, _, base, have, _) in enumerate(segs):
        rows[i, :have] = x[base:base + have]
    out = torch.full((len(segs), max(s[1] for s in segs) + 3, x.shape[1]), 7.0, dtype=torch.float32, device="cuda")
    moved = [(f + so, c, b + si, h, None if t is None else t + si) for f, c, b, h, t in segs]
    g.resample_range(gpu.ctx(), torch.from_numpy(rows).cuda(), rate, moved, out=out)
    return out.cpu().numpy()


@pytest.mark.parametrize("name", ["mono", "stereo"])
@pytest.mark.parametrize("rate", RATES)
def test_slices_of_the_whole_conversion_bit_for_bit(rate, name):
    import gstpeaq_amd as g
    x = inputs(name)[0]
    y = converted(x, rate, (name, 0))
    assert len(y) == g.resampled_length(len(x), rate) == g.live_rate_ready(rate, len(x), ended=True)
    segs = segments_of(g, rate, len(x), len(y))
    got = run_segments(g, x, rate, segs)                                 # several in one call, of different lengths
    for row, (first, count, *_) in zip(got, segs):
        assert np.array_equal(row[:count].view(np.uint32), y[first:first + count].view(np.uint32)), (rate, first, count)
        assert (row[count:] == 7.0).all()                                # nothing behind out_count is touched
    alone = run_segments(g, x, rate, segs[:1])                           # and one alone
    assert np.array_equal(alone[0, :700].view(np.uint32), y[:700].view(np.uint32))


@pytest.mark.parametrize("rate", RATES)
def test_positions_past_2_to_33_convert_like_the_same_phase_near_zero(rate):
    import gstpeaq_amd as g
    x = inputs("stereo")[0]
    plan = g.resample_plan(rate)
    L, M = plan["L"], plan["M"]
    segs = [s for s in segments_of(g, rate, len(x), g.resampled_length(len(x), rate)) if s[2] > 0 and s[4] is None]
    assert len(segs) == 2
    k = 2 ** 33 // L + 1
    assert segs[0][0] + k * L > 2 ** 33
    near, far = run_segments(g, x, rate, segs), run_segments(g, x, rate, segs, shift=(k * L, k * M))
    assert np.array_equal(near.view(np.uint32), far.view(np.uint32))
    assert np.abs(near[0, :300]).max() > 0.01


def test_a_row_that_misses_a_sample_is_refused_and_the_context_goes_on():
    import torch
    import gstpeaq_amd as g
    x = inputs("mono")[0]
    y = converted(x, 44100, ("mono", 0))
    first, count = 1000, 300
    lo, hi = g.live_rate_span(44100, first, count)
    rows = torch.from_numpy(np.ascontiguousarray(x[None, lo:hi])).cuda()
    for seg, what in (((first, count, lo, hi - lo - 1, None), "the row holds"),       # the last sample is not there
                      ((first, count, lo + 1, hi - lo - 1, None), "the row holds"),   # nor the first
                      ((first, count, lo, hi - lo - 2, hi - 1), "the row holds"),     # inside the stream that ended at hi - 1
                      ((len(y) - 10, 11, lo, hi - lo, len(x)), "pass the"),           # an output past the ended stream's
                      ((first, count, lo, hi - lo + 1, None), "passes in_stride")):
        with pytest.raises(g.PeaqError, match="peaq_batch_resample_range: segment 0: .*" + what):
            g.resample_range(gpu.ctx(), rows, 44100, [seg])
    for rate in (48000, 12347):
        with pytest.raises(g.PeaqError, match="peaq_batch_resample_range: rate %d" % rate):
            g.resample_range(gpu.ctx(), rows, rate, [(first, count, lo, hi - lo, None)])
    with pytest.raises(g.PeaqError, match="channels must be 1 or 2"):
        g.resample_range(gpu.ctx(), rows.reshape(1, -1, 1).expand(1, -1, 3).contiguous(), 44100, [(first, count, lo, hi - lo, None)])
    got = g.resample_range(gpu.ctx(), rows, 44100, [(first, count, lo, hi - lo, None)]).cpu().numpy()
    assert np.array_equal(got[0, :count].view(np.uint32), y[first:first + count].view(np.uint32))


# ---- sessions ----------------------------------------------------------------------------------------------------

def run_session(ref, test, advanced, how="whole", rates=(48000, 48000), setup=None):
    import gstpeaq_amd
    s = gstpeaq_amd.Session(gpu.ctx(), advanced, ref.shape[1], rates=rates)
    if setup:
        setup(s)
    if how == "whole":
        s.push(0, ref)
        s.push(1, test)
    else:
        feed(s, ref, test)
    s.flush()
    return s.results(), s


def plain_result(name, rates, advanced):
    """the plain session over the resample()d pair, once"""
    key = (name, rates, advanced, gpu.mode() if advanced else "default")
    if key not in _PLAIN:
        res, s = run_session(*pair_48k(name, rates), advanced)
        s.close()
        _PLAIN[key] = res
    return _PLAIN[key]


@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
@pytest.mark.parametrize("name", ["mono", "stereo"])
@pytest.mark.parametrize("rate", RATES)
def test_a_rated_session_is_the_plain_session_over_the_converted_streams(rate, name, advanced, fir_mode):
    ref, test = inputs(name)
    want = plain_result(name, (rate, rate), advanced)
    assert want["frames"] >= 14
    for how in ("whole", "feed"):
        res, s = run_session(ref, test, advanced, how, rates=(rate, rate))
        s.close()
        check_result(res, want, advanced, (rate, name, how))


@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
@pytest.mark.parametrize("rates", [(44100, 48000), (48000, 32000)])
@pytest.mark.parametrize("name", ["stereo", "ragged_mono"])
def test_pads_at_different_rates(name, rates, advanced):
    ref, test = inputs(name)
    want = plain_result(name, rates, advanced)
    for how in ("whole", "feed"):
        res, s = run_session(ref, test, advanced, how, rates=rates)
        s.close()
        check_result(res, want, advanced, (rates, name, how))


def test_reset_keeps_the_rates_and_a_push_after_the_flush_is_refused():
    import gstpeaq_amd
    ref, test = inputs("short_stereo")
    want = plain_result("short_stereo", (44100, 44100), False)
    res, s = run_session(ref, test, False, "feed", rates=(44100, 44100))
    assert same_bits(res, want)
    with pytest.raises(gstpeaq_amd.PeaqError, match="peaq_session_push: the stream of a pad at 44100 Hz ended"):
        s.push(0, ref[:100])
    with pytest.raises(gstpeaq_amd.PeaqError, match="peaq_session_set_rates: the stream has begun"):
        s.set_rates(32000)
    s.reset()
    s.push(1, test)
    s.push(0, ref)
    s.flush()
    assert same_bits(s.results(), want)
    s.reset()
    with pytest.raises(gstpeaq_amd.PeaqError, match="peaq_session_set_rates: rate 12347"):
        s.set_rates(44100, 12347)
    s.set_rates(48000)                                                   # plain again
    s.push(0, ref)
    s.push(1, test)
    s.flush()
    assert same_bits(s.results(), plain_result("short_stereo", (48000, 48000), False))
    s.close()


@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
def test_with_the_meter_the_readings_are_the_plain_sessions(advanced):
    ref, test = inputs("stereo")
    meter = lambda s: s.set_meter(4, 2, depth=64)
    _, s = run_session(*pair_48k("stereo", (44100, 44100)), advanced, setup=meter)
    want, _ = s.meter_read()
    s.close()
    res, s = run_session(ref, test, advanced, "feed", rates=(44100, 44100), setup=meter)
    got, dropped = s.meter_read()
    s.close()
    assert dropped == 0 and len(got) == len(want) >= 10
    fields = ("index", "start", "length", "first_frame", "n_frames", "first_block", "n_blocks")
    for a, b in zip(got, want):
        assert [a[k] for k in fields] == [b[k] for k in fields]
        check_result(a, b, advanced, ("meter", a["index"]))


@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
@pytest.mark.parametrize("name", ["mono", "stereo"])
def test_alignment_counts_converted_samples(name, advanced):
    """the test pad 147 raw samples late at 44.1 kHz: 160 converted ones"""
    import gstpeaq_amd
    ref, test = inputs(name)
    late = np.concatenate([np.zeros((147, test.shape[1]), dtype=np.float32), test])
    want = plain_result(name, (44100, 44100), advanced)
    ref48, late48 = converted(ref, 44100, (name, 0)), converted(late, 44100)
    assert len(late48) == len(converted(test, 44100, (name, 1))) + 160
    for how in ("whole", "feed"):
        res, s = run_session(ref, late, advanced, how, rates=(44100, 44100), setup=lambda s: s.set_align(256, probe=4096))
        got = s.align_read()
        s.close()
        assert got["acquired"] is True and got["lag"] == 160, got
        assert (got["probe_ref"], got["probe_test"], got["skip_ref"], got["skip_test"]) == (4096, 4096, 0, 160)
        rec = batch_record(ref48, late48, 4096, 4096, 256)
        for k in ("lag", "peak", "runner_up", "norm"):
            assert got[k] == rec[k], (k, got, rec)
        check_result(res, want, advanced, ("align", name, how))


def test_a_pair_pushed_unconverted_reads_an_odg_at_least_0_4_lower():
    """(the module's docstring has the oracle's values)"""
    ref, test = inputs("box")
    plain, s = run_session(ref, test, False)
    s.close()
    rated, s = run_session(ref, test, False, rates=(44100, 44100))
    s.close()
    print("unconverted", plain["odg"], "converted", rated["odg"])
    assert plain["odg"] <= rated["odg"] - 0.4, (plain["odg"], rated["odg"])
    assert abs(rated["odg"] - -1.053) < 0.2 and abs(plain["odg"] - -1.920) < 0.2


# ---- broker ------------------------------------------------------------------------------------------------------

BROKER_STREAMS = ("stereo", "short_stereo", "box", "stereo", "short_stereo", "box", "stereo", "box")
BROKER_FLUSHED_EARLY, BROKER_REOPENED = 3, 4        # indices into BROKER_STREAMS


def broker_run(advanced, rates, set_rates=True):
    """eight slots opened over three ticks and fed 4096 raw samples a pad and tick; one is flushed after 12288 samples,
    one is closed in mid-stream and opened again for its whole stream -> [(stream, raw samples pushed, result)]"""
    import gstpeaq_amd
    b = gstpeaq_amd.Broker(gpu.ctx(), 2, max_sessions=8, advanced=advanced, rates=rates if set_rates else None)
    sids, pos, ends, out = [], {}, {}, []
    step = 0
    while len(out) < len(BROKER_STREAMS):
        if len(sids) < len(BROKER_STREAMS) and step % 2 == 0:          # staggered starts
            for _ in range(3):
                if len(sids) < len(BROKER_STREAMS):
                    sids.append(b.open())
                    pos[len(sids) - 1] = 0
        for i, sid in enumerate(sids):
            if i in ends:
                continue
            ref, test = inputs(BROKER_STREAMS[i])
            at = pos[i]
            b.push(sid, 0, ref[at:at + 4096])
            b.push(sid, 1, test[at:at + 4096])
            pos[i] = at + 4096
            if i == BROKER_REOPENED and pos[i] == 4096 and "reopened" not in ends:
                b.close_session(sid)
                assert b.open() == sid
                ends["reopened"] = True
                pos[i] = 0
                continue
            cut = 12288 if i == BROKER_FLUSHED_EARLY else len(ref)
            if pos[i] >= cut:
                b.flush(sid)
                ends[i] = min(pos[i], len(ref))
        b.tick()
        step += 1
        for i in list(ends):
            if i != "reopened" and i not in [o[0] for o in out]:
                out.append((i, ends[i], b.results(sids[i])))
    b.close()
    return sorted(out)


@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
def test_every_broker_slot_is_its_rated_session(advanced):
    rates = (44100, 44100)
    runs = broker_run(advanced, rates)
    assert [r[1] for r in runs][BROKER_FLUSHED_EARLY] == 12288
    for i, n, res in runs:
        ref, test = inputs(BROKER_STREAMS[i])
        want, s = run_session(ref[:n], test[:n], advanced, "whole", rates=rates)
        s.close()
        check_result(res, want, advanced, ("broker", i, BROKER_STREAMS[i]))
        if n == len(ref):
            check_result(res, plain_result(BROKER_STREAMS[i], rates, advanced), advanced, ("broker, plain", i))


def test_a_broker_with_pads_at_different_rates():
    rates = (48000, 32000)
    for i, n, res in broker_run(False, rates):
        if n == len(inputs(BROKER_STREAMS[i])[0]):
            assert same_bits(res, plain_result(BROKER_STREAMS[i], rates, False)), i


@pytest.mark.parametrize("advanced", [False, True], ids=["basic", "advanced"])
def test_rates_of_48000_are_no_rates(advanced):
    a, b = broker_run(advanced, (48000, 48000)), broker_run(advanced, None, set_rates=False)
    assert len(a) == len(b) == len(BROKER_STREAMS)
    for (i, n, x), (j, m, y) in zip(a, b):
        assert (i, n) == (j, m) and same_bits(x, y), i


def test_a_broker_slot_aligns_in_converted_samples():
    import gstpeaq_amd
    ref, test = inputs("stereo")
    late = np.concatenate([np.zeros((147, 2), dtype=np.float32), test])
    want, s = run_session(ref, late, False, "whole", rates=(44100, 44100), setup=lambda s: s.set_align(256, probe=4096))
    want_rec = s.align_read()
    s.close()
    b = gstpeaq_amd.Broker(gpu.ctx(), 2, max_sessions=2, rates=(44100, 44100))
    b.set_align(256, probe=4096)
    sid = b.open()
    for at in range(0, len(late), 4096):
        b.push(sid, 0, ref[at:at + 4096])
        b.push(sid, 1, late[at:at + 4096])
        b.tick()
    b.flush(sid)
    res = b.results(sid)
    got = b.align_read(sid)
    b.close()
    assert got == want_rec and got["lag"] == 160, (got, want_rec)
    assert same_bits(res, want)


def test_what_a_broker_refuses_of_the_rates():
    import gstpeaq_amd
    b = gstpeaq_amd.Broker(gpu.ctx(), 1, max_sessions=2)
    for rate in (7000, 12347):
        with pytest.raises(gstpeaq_amd.PeaqError, match="peaq_broker_set_rates: rate %d" % rate):
            b.set_rates(44100, rate)
    b.set_rates(44100)
    sid = b.open()
    with pytest.raises(gstpeaq_amd.PeaqError, match="peaq_broker_set_rates: session 0 is open"):
        b.set_rates(48000)
    b.push(sid, 0, np.zeros((100, 1), dtype=np.float32))
    b.flush(sid)
    with pytest.raises(gstpeaq_amd.PeaqError, match="peaq_broker_push: the stream of a pad at 44100 Hz ended"):
        b.push(sid, 0, np.zeros((100, 1), dtype=np.float32))
    b.close_session(sid)
    b.set_rates(48000, 48000)
    b.start(1000)
    with pytest.raises(gstpeaq_amd.PeaqError, match="set the rates before peaq_broker_start"):
        b.set_rates(44100)
    b.stop()
    b.close()
    multi = gstpeaq_amd.Broker(gpu.ctx(), 1, max_sessions=2, devices=[0, 0], rates=(32000, 32000))
    x = inputs("mono")[0][:5000]
    sid = multi.open()
    multi.push(sid, 0, x)
    multi.push(sid, 1, x)
    multi.flush(sid)
    got = multi.results(sid)
    multi.close()
    want, s = run_session(x, x, False, rates=(32000, 32000))
    s.close()
    assert same_bits(got, want)

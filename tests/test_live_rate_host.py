"""Host side of live rate conversion (include/peaq_amd.h "live rate conversion": peaq_live_rate_ready,
peaq_live_rate_inputs, peaq_rate_segment_size), without a GPU: the closed form against a direct count over the header's
n_first / last, the converted length as the ended count, the spans, the refusals, header and exports."""
import ctypes as C
import re
from math import gcd
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
RATES = (8000, 11025, 32000, 44100, 88200, 96000, 192000)
HELD_BACK = {44100: 36, 32000: 50, 96000: 32, 11025: 144, 8000: 198}   # the header's figures, at most
LARGE = (1000, 4410, 31700, 100003, 2 ** 33 + 12345)
NEW = ("peaq_live_rate_ready", "peaq_live_rate_inputs", "peaq_rate_segment_size", "peaq_batch_resample_range",
       "peaq_session_set_rates", "peaq_broker_set_rates")


@pytest.fixture(scope="module")
def g():
    import gstpeaq_amd
    if not gstpeaq_amd.library_path().exists():
        gstpeaq_amd.build_library()
    gstpeaq_amd.load_library()
    return gstpeaq_amd


def geometry(g, rate):
    """(L, M, K) of the header's notation"""
    d = gcd(48000, rate)
    return 48000 // d, rate // d, g.resample_plan(rate)["taps"] // 2


def n_first(geo, m):
    L, M, K = geo
    p = (m * M) % L
    return (m * M) // L + (-1 if 8 * p < L else 0) - K + 1


def last(geo, m):
    return n_first(geo, m) + 2 * geo[2] - 1


def direct_count(geo, n, start=0):
    """outputs m with last(m) < n, counted one by one from a known lower bound"""
    m = start
    while last(geo, m) < n:
        m += 1
    return m


@pytest.mark.parametrize("rate", RATES)
def test_ready_is_the_direct_count_and_never_passes_the_converted_length(g, rate):
    geo = geometry(g, rate)
    prev = 0
    for n in range(0, 401):
        got = g.live_rate_ready(rate, n)
        assert got == direct_count(geo, n, prev), (rate, n)
        assert got >= prev                                           # non-decreasing
        ended = g.live_rate_ready(rate, n, ended=True)
        assert got <= ended == g.resampled_length(n, rate), (rate, n)
        prev = got
    for n in LARGE:
        got = g.live_rate_ready(rate, n)
        assert got >= 1 and last(geo, got - 1) < n <= last(geo, got), (rate, n)   # (a prefix: last is non-decreasing)
        ended = g.live_rate_ready(rate, n, ended=True)
        assert got <= ended
        if n < 2 ** 32:
            assert ended == g.resampled_length(n, rate)
        else:
            assert ended == (n - 1) * 48000 // rate + 1              # (no limit of 32 bits)
        assert g.live_rate_ready(rate, n + 1) >= got


@pytest.mark.parametrize("rate", sorted(HELD_BACK))
def test_what_is_held_back_stays_under_the_figures_of_the_header(g, rate):
    worst = max(g.live_rate_ready(rate, n, ended=True) - g.live_rate_ready(rate, n) for n in range(400, 1700))
    assert 0 < worst <= HELD_BACK[rate], (rate, worst)
    assert worst / 48000.0 < 5e-3


@pytest.mark.parametrize("rate", RATES)
def test_span_is_n_first_to_last(g, rate):
    geo = geometry(g, rate)
    for first in (0, 1, 7, 160, 1023, 31700, 2 ** 33 + 5):
        for count in (1, 2, 256, 257, 3072):
            lo, hi = g.live_rate_span(rate, first, count)
            assert lo == max(0, n_first(geo, first)) and hi == last(geo, first + count - 1) + 1, (rate, first, count)
        lo, hi = g.live_rate_span(rate, first, 0)
        assert lo == hi == max(0, n_first(geo, first))
    # what is ready reads only what is there
    for n in (100, 401, 31700):
        ready = g.live_rate_ready(rate, n)
        if ready:
            assert g.live_rate_span(rate, 0, ready)[1] <= n < g.live_rate_span(rate, 0, ready + 1)[1]


@pytest.mark.parametrize("rate", [48000, 7000, 12347, 400000])
def test_refusals_name_the_rate(g, rate):
    for call in (lambda: g.live_rate_ready(rate, 1000), lambda: g.live_rate_span(rate, 0, 10)):
        with pytest.raises(g.PeaqError) as e:
            call()
        assert str(rate) in str(e.value)


def test_positions_past_the_arithmetic_are_refused(g):
    with pytest.raises(g.PeaqError, match="n_have"):
        g.live_rate_ready(44100, 2 ** 62)
    with pytest.raises(g.PeaqError, match="out_first"):
        g.live_rate_span(44100, 2 ** 62, 1)


def test_segment_mirror_header_and_exports(g):
    assert g.load_library().peaq_rate_segment_size() == C.sizeof(g.RateSegment) == 32
    header = (ROOT / "include" / "peaq_amd.h").read_text()
    assert "live rate conversion" in header
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(g.load_library(), name), name
    for name in ("live_rate_ready", "live_rate_span", "resample_range", "RateSegment"):
        assert name in g.__all__
    assert "rates" in g.Session.__init__.__code__.co_varnames and "rates" in g.Broker.__init__.__code__.co_varnames
    assert "peaq_live_rate.hip" in (ROOT / "gstpeaq_amd" / "csrc" / "Makefile").read_text()

"""CPU-side checks of what one slot of the broker contributes to a tick (csrc/peaq_host.h, take_slot_windows), run
without a device through peaq_debug_broker_plan: the same units as the stream framer cuts on its own, one window of a
kind a tick, and with the meter on the rule that holds the blocks back behind the frames, the flush block after the
last frame, and the closing entry of a stream whose blocks end without a flush block."""
import ctypes as C
import json

import numpy as np
import pytest

from test_stream_framing import BROKER_CAPS, ROOT, check_windows, partitions, stream_plan, unit_sequence

FRAME, HOP, BLOCK = 2048, 1024, 192
TICK, FLUSH = (-2, 0), (-1, 0)
AHEAD = 1024 * 2 // 192                              # blocks the meter lets the filter-bank path run ahead of the frames


@pytest.fixture(scope="module")
def lib():
    import gstpeaq_amd
    if not gstpeaq_amd.library_path().exists():
        gstpeaq_amd.build_library()
    L = gstpeaq_amd.load_library()
    L.peaq_debug_stream_plan.restype = C.c_int
    L.peaq_debug_stream_plan.argtypes = [C.c_int, C.c_uint, C.c_uint, C.c_int, C.c_size_t, C.POINTER(C.c_int),
                                         C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_size_t)]
    L.peaq_debug_broker_plan.restype = C.c_int
    L.peaq_debug_broker_plan.argtypes = [C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_uint64),
                                         C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)]
    return L


def broker_plan(lib, advanced, metered, events):
    """-> rows [n][6] = (tick, kind, first, count, valid on ref, valid on test) for events [(pad, n_samples)]"""
    pads = np.ascontiguousarray([p for p, _ in events], dtype=np.intc)
    ns = np.ascontiguousarray([n for _, n in events], dtype=np.uint64)
    args = (int(advanced), int(metered), len(events), pads.ctypes.data_as(C.POINTER(C.c_int)),
            ns.ctypes.data_as(C.POINTER(C.c_uint64)))
    n = C.c_size_t(0)
    assert lib.peaq_debug_broker_plan(*args, 0, None, C.byref(n)) == 0, lib.peaq_last_error()
    out = np.zeros((n.value, 6), dtype=np.uint64)
    assert lib.peaq_debug_broker_plan(*args, n.value, out.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n)) == 0
    assert n.value == len(out)
    return out.astype(np.int64)


def windows_of(rows, kinds=(0, 1)):
    """the rows of `kinds` without the tick column, as stream_plan gives its windows"""
    return [tuple(int(v) for v in r[1:]) for r in rows if r[1] in kinds]


def ticked(pushes, every):
    """a tick after every `every`-th push"""
    out = []
    for i, p in enumerate(pushes):
        out.append(p)
        if (i + 1) % every == 0:
            out.append(TICK)
    return out


def golden_streams():
    """every golden case and every partition of its lengths, identical ones once:
    (what, advanced, n_ref, n_test, frames, blocks, pushes)"""
    recs = json.loads((ROOT / "tests" / "golden" / "ref_e2e.json").read_text())
    seen = set()
    for k, r in enumerate(recs):
        c = r["case"]
        n_ref, n_test = c["n"] - c.get("ref_trim", 0), c["n"] - c.get("test_trim", 0)
        for name, pushes in partitions(n_ref, n_test, seed=k).items():
            key = (c["advanced"], n_ref, n_test, name, k if name == "random" else None)
            if key not in seen:                      # (the plan is a function of these alone)
                seen.add(key)
                yield (c["name"], name), c["advanced"], n_ref, n_test, r["frames"], r["fb_frames"], pushes


def per_tick(rows, events, n_ref, n_test):
    """-> F, B (frames and blocks handed out through each tick), have (samples present on both pads at each tick),
    n_before (ticks before the first flush request; all of them if the events have none)"""
    pads = np.array([p for p, _ in events], dtype=np.int64)
    ns = np.array([n for _, n in events], dtype=np.int64)
    n_explicit = int((pads == -2).sum())
    n_ticks = max(n_explicit, int(rows[:, 0].max()) + 1 if len(rows) else 0)
    at_tick = np.flatnonzero(pads == -2)
    have = np.full(n_ticks, min(n_ref, n_test), dtype=np.int64)      # (the ticks behind the last event: everything)
    pushed = [np.cumsum(np.where(pads == p, ns, 0)) for p in (0, 1)]
    have[:n_explicit] = np.minimum(pushed[0][at_tick], pushed[1][at_tick])
    done = []
    for kind in (0, 1):
        mine = rows[rows[:, 1] == kind]
        done.append(np.cumsum(np.bincount(mine[:, 0], weights=mine[:, 3], minlength=n_ticks).astype(np.int64)))
    flushes = np.flatnonzero(pads == -1)
    n_before = int((at_tick < flushes[0]).sum()) if len(flushes) else n_explicit
    return done[0], done[1], have, n_before


def check_unmetered(lib, what, advanced, n_ref, n_test, frames, blocks, pushes, events):
    rows = broker_plan(lib, advanced, 0, events)
    assert not (rows[:, 1] == 2).any(), what
    windows = windows_of(rows)
    units = check_windows(windows, BROKER_CAPS, n_ref, n_test, advanced)
    assert units[0] == frames, what
    if advanced:
        assert units[1] == blocks, what
    assert sorted(unit_sequence(windows)) == sorted(unit_sequence(stream_plan(lib, advanced, BROKER_CAPS, pushes))), what
    _, per_tick_and_kind = np.unique(rows[:, :2], axis=0, return_counts=True)
    assert (per_tick_and_kind == 1).all(), what         # at most one window of a kind a tick
    return windows


def check_metered(lib, what, advanced, n_ref, n_test, T, TB, events, like):
    """`like`: the windows of the same events without the meter"""
    rows = broker_plan(lib, advanced, 1, events)
    for kind in (0, 1):
        assert unit_sequence(windows_of(rows, (kind,))) == unit_sequence([w for w in like if w[0] == kind]), (what, kind)
    F, B, have, n_before = per_tick(rows, events, n_ref, n_test)
    t = np.arange(len(F))
    # the blocks stay behind the frame after the last one taken: before the flush request, and until the last frame
    held = (t < n_before) | (F < T)
    assert (B[held] <= 1024 * (F[held] + 2) // BLOCK).all(), what
    # the flush block: only in a tick that has the stream's last frame
    for r in rows[(rows[:, 1] == 1) & ((rows[:, 4] != rows[:, 3] * BLOCK) | (rows[:, 5] != rows[:, 3] * BLOCK))]:
        assert F[r[0]] == T, (what, r)
    # a whole frame waiting on both pads is taken
    F_before = np.concatenate(([0], F[:-1]))
    waiting = have - HOP * F_before >= FRAME
    assert (F[waiting] > F_before[waiting]).all(), what
    # the closing entry: once, for an advanced stream with frames whose blocks ended without a flush block
    closing = rows[rows[:, 1] == 2]
    no_flush_block = max(n_ref, n_test) == BLOCK * (min(n_ref, n_test) // BLOCK)
    assert len(closing) == (1 if advanced and T > 0 and no_flush_block else 0), (what, closing)
    for r in closing:
        assert tuple(r[2:]) == (TB, 0, 0, 0), (what, r)
        assert r[0] >= rows[rows[:, 1] == 0][-1, 0], (what, r)
    return F, B


def test_a_slot_hands_out_the_framer_s_units_one_window_of_a_kind_a_tick(lib):
    for what, advanced, n_ref, n_test, frames, blocks, pushes in golden_streams():
        for every in (1, 7):
            check_unmetered(lib, (what, every), advanced, n_ref, n_test, frames, blocks, pushes, ticked(pushes, every))


def test_the_meter_holds_the_blocks_behind_the_frames_and_closes_a_stream_without_a_flush_block(lib):
    for what, advanced, n_ref, n_test, frames, blocks, pushes in golden_streams():
        for every in (1, 7):
            events = ticked(pushes, every)
            like = windows_of(broker_plan(lib, advanced, 0, events))
            check_metered(lib, (what, every), advanced, n_ref, n_test, frames, blocks, events, like)


def test_a_flush_s_backlog_keeps_the_two_paths_together_tick_by_tick(lib):
    """Everything pushed, then the flush, then ticks only: 8 frames a tick, and the blocks with them."""
    for what, advanced, n_ref, n_test, frames, blocks, pushes in golden_streams():
        events = pushes + [FLUSH]
        like = check_unmetered(lib, what, advanced, n_ref, n_test, frames, blocks, pushes, events)
        F, B = check_metered(lib, what, advanced, n_ref, n_test, frames, blocks, events, like)
        if advanced:
            # the blocks cover the frames' windows (as far as the stream has whole blocks) and at most AHEAD more
            whole = min(n_ref, n_test) // BLOCK
            assert (BLOCK * B >= np.minimum(HOP * (F + 1), BLOCK * whole)).all(), what
            assert (B <= -(-HOP * (F + 1) // BLOCK) + AHEAD).all(), what


def test_a_stream_goes_on_after_a_flush_and_flushes_twice(lib):
    """the event lists of test_stream_edge_cases that continue after a flush or flush twice, a tick after each flush"""
    for pushes in ([(0, 100), FLUSH, (0, 2048), (1, 2048)], [(0, 3000), (1, 10), FLUSH, FLUSH]):
        events = []
        for e in pushes:
            events += [e, TICK] if e == FLUSH else [e]
        assert windows_of(broker_plan(lib, 0, 0, events)) == stream_plan(lib, 0, BROKER_CAPS, pushes)
    assert windows_of(broker_plan(lib, 0, 0, [(0, 100), FLUSH, TICK, (0, 2048), (1, 2048)])) == \
        [(0, 0, 1, 100, 0), (0, 1, 1, 2048, 2048), (0, 2, 1, 1024, 1024)]
    assert windows_of(broker_plan(lib, 0, 0, [(0, 3000), (1, 10), FLUSH, TICK, FLUSH, TICK])) == \
        [(0, 0, 1, 2048, 10), (0, 1, 1, 952, 0)]


def test_broker_plan_checks_its_arguments(lib):
    n = C.c_size_t(0)
    ns = (C.c_uint64 * 1)(10)
    assert lib.peaq_debug_broker_plan(0, 0, 0, None, None, 0, None, None) == -1                 # PEAQ_ERR_ARG
    assert lib.peaq_debug_broker_plan(0, 0, 1, None, ns, 0, None, C.byref(n)) == -1
    assert lib.peaq_debug_broker_plan(0, 0, 1, (C.c_int * 1)(0), None, 0, None, C.byref(n)) == -1
    assert lib.peaq_debug_broker_plan(0, 0, 1, (C.c_int * 1)(0), ns, 1, None, C.byref(n)) == -1
    for bad in (2, -3):
        assert lib.peaq_debug_broker_plan(0, 0, 1, (C.c_int * 1)(bad), ns, 0, None, C.byref(n)) == -1
    assert lib.peaq_debug_broker_plan(0, 0, 0, None, None, 0, None, C.byref(n)) == 0 and n.value == 0

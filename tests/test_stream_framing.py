"""CPU-side checks of the code that cuts a session's two streams into launches (csrc/peaq_host.h, StreamFramer),
run without a device through peaq_debug_stream_plan: the unit counts the real element recorded, the shape of every
launch window, the one zero-padded unit of the flush, and that the per-launch caps only group the units."""
import ctypes as C
import json
import random
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
FRAME, HOP, BLOCK = 2048, 1024, 192
SESSION_CAPS, BROKER_CAPS = (64, 120), (8, 48)       # kSessionMax* / kBrokerMax* (frames, blocks per launch)
UNIT = {0: (FRAME, HOP), 1: (BLOCK, BLOCK)}          # kind -> (unit, hop)


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
    return L


def stream_plan(lib, advanced, caps, pushes, drain_every_push=True):
    """-> [(kind, first unit, units, valid on ref, valid on test)] for pushes [(pad, n_samples)] and a flush;
    pad -1 is a flush in mid-stream; drain_every_push=False: windows are taken at the flushes only"""
    pads = np.ascontiguousarray([p for p, _ in pushes], dtype=np.intc)
    ns = np.ascontiguousarray([n for _, n in pushes], dtype=np.uint64)
    args = (int(advanced), caps[0], caps[1], int(drain_every_push), len(pushes), pads.ctypes.data_as(C.POINTER(C.c_int)),
            ns.ctypes.data_as(C.POINTER(C.c_uint64)))
    n = C.c_size_t(0)
    assert lib.peaq_debug_stream_plan(*args, 0, None, C.byref(n)) == 0, lib.peaq_last_error()
    out = np.zeros((n.value, 5), dtype=np.uint64)
    assert lib.peaq_debug_stream_plan(*args, n.value, out.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n)) == 0
    assert n.value == len(out)
    return [tuple(int(v) for v in row) for row in out]


def partitions(n_ref, n_test, seed):
    """name -> pushes: the same two streams handed over in different buffers"""
    def deal(next_size, pick):
        left, out = [n_ref, n_test], []
        while left[0] or left[1]:
            p = pick(left, len(out))
            k = min(next_size(), left[p])
            out.append((p, k))
            left[p] -= k
        return out

    def alternate(left, i):
        return i % 2 if left[i % 2] else 1 - i % 2

    rng = random.Random(seed)
    parts = {"4096 alternating": deal(lambda: 4096, alternate),
             "ref first": [(0, n_ref), (1, n_test)],
             "random": deal(lambda: rng.randint(1, 10000),
                            lambda left, i: rng.choice([p for p in (0, 1) if left[p]]))}
    if max(n_ref, n_test) <= 50000:
        parts["one sample at a time"] = deal(lambda: 1, alternate)
    return parts


def check_windows(windows, caps, n_ref, n_test, advanced):
    """the shape of every window; -> units per kind"""
    n = (n_ref, n_test)
    units = {}
    for kind in (0, 1):
        unit, hop = UNIT[kind]
        mine = [w for w in windows if w[0] == kind]
        if kind == 1 and not advanced:
            assert not mine
            continue
        nxt, whole, flushes = 0, 0, []
        for i, (_, first, count, v_ref, v_test) in enumerate(mine):
            assert first == nxt and 1 <= count <= caps[kind], (kind, i, mine[i])       # contiguous from 0, within the cap
            nxt = first + count
            if (v_ref, v_test) == ((count - 1) * hop + unit,) * 2:
                assert not flushes, "a whole window after the flush unit"
                whole += count
            else:
                flushes.append(mine[i])
        left = [n[p] - whole * hop for p in (0, 1)]
        assert min(left) < unit, "a whole unit was left behind"
        assert len(flushes) == (1 if max(left) else 0)
        for (_, _, count, v_ref, v_test) in flushes:       # (the last of its kind: nothing whole follows, see above)
            assert count == 1 and (v_ref, v_test) == (min(left[0], unit), min(left[1], unit)), (kind, flushes, left)
        units[kind] = nxt
    assert set(w[0] for w in windows) <= {0, 1}
    return units


def unit_sequence(windows):
    """every window spelled out as its units: (kind, index, valid on ref, valid on test)"""
    seq = []
    for kind, first, count, v_ref, v_test in windows:
        unit, hop = UNIT[kind]
        for i in range(count):
            seq.append((kind, first + i, min(unit, v_ref - i * hop), min(unit, v_test - i * hop)))
    return seq


def test_streams_are_cut_into_the_reference_element_s_units(lib):
    """Every golden case's lengths, handed over in several partitions, under the session's and the broker's caps:
    as many FFT frames and filter-bank blocks as the real element recorded, well-formed windows, and the same
    sequence of units whatever the caps."""
    recs = json.loads((ROOT / "tests" / "golden" / "ref_e2e.json").read_text())
    for k, r in enumerate(recs):
        c = r["case"]
        n_ref = c["n"] - c.get("ref_trim", 0)
        n_test = c["n"] - c.get("test_trim", 0)
        for name, pushes in partitions(n_ref, n_test, seed=k).items():
            seqs = []
            for caps in (SESSION_CAPS, BROKER_CAPS):
                windows = stream_plan(lib, c["advanced"], caps, pushes)
                units = check_windows(windows, caps, n_ref, n_test, c["advanced"])
                assert units[0] == r["frames"], (c["name"], name, caps)
                if c["advanced"]:
                    assert units[1] == r["fb_frames"], (c["name"], name, caps)
                seqs.append(unit_sequence(windows))
                # the flush requested with everything still waiting (a broker whose ticks come late): whole units
                # first, then the one flush unit -- the same units, kind by kind
                late = stream_plan(lib, c["advanced"], caps, pushes, drain_every_push=False)
                assert check_windows(late, caps, n_ref, n_test, c["advanced"]) == units
                assert sorted(unit_sequence(late)) == sorted(seqs[-1]), (c["name"], name, caps)
            assert seqs[0] == seqs[1], (c["name"], name)


def test_stream_edge_cases(lib):
    for caps in (SESSION_CAPS, BROKER_CAPS):
        assert stream_plan(lib, 0, caps, []) == []                                       # (0, 0): nothing, also at the flush
        assert stream_plan(lib, 1, caps, [(0, 0), (1, 0)]) == []
        assert stream_plan(lib, 0, caps, [(0, 1)]) == [(0, 0, 1, 1, 0)]                   # leftover on one side only still flushes
        assert stream_plan(lib, 0, caps, [(0, 5000), (1, 2048)]) == [(0, 0, 1, 2048, 2048), (0, 1, 1, 2048, 1024)]
        # whole blocks and nothing left on either side: no flush block (the frames keep their overlap: one flush frame)
        assert stream_plan(lib, 1, caps, [(0, 384), (1, 384)]) == [(1, 0, 2, 384, 384), (0, 0, 1, 384, 384)]
    # a stream that goes on after a flush starts where the flush unit ended: min(left, unit) further on each pad
    assert stream_plan(lib, 0, SESSION_CAPS, [(0, 100), (-1, 0), (0, 2048), (1, 2048)]) == \
        [(0, 0, 1, 100, 0), (0, 1, 1, 2048, 2048), (0, 2, 1, 1024, 1024)]
    assert stream_plan(lib, 0, SESSION_CAPS, [(0, 3000), (1, 10), (-1, 0), (-1, 0)]) == \
        [(0, 0, 1, 2048, 10), (0, 1, 1, 952, 0)]                                      # (each flush has its own unit)
    # 10 s at 48 kHz: 467 whole frames + the flush frame, 2500 whole blocks
    w = stream_plan(lib, 1, SESSION_CAPS, [(0, 480000), (1, 480000)])
    assert check_windows(w, SESSION_CAPS, 480000, 480000, 1) == {0: 468, 1: 2500}
    assert [x for x in w if x[0] == 0][-1] == (0, 467, 1, 1792, 1792) and all(x[3] == x[2] * 192 for x in w if x[0] == 1)


def test_stream_plan_checks_its_arguments(lib):
    n = C.c_size_t(0)
    pad = (C.c_int * 1)(2)
    ns = (C.c_uint64 * 1)(10)
    assert lib.peaq_debug_stream_plan(0, 64, 120, 1, 0, None, None, 0, None, None) == -1       # PEAQ_ERR_ARG
    assert lib.peaq_debug_stream_plan(0, 64, 120, 1, 1, None, ns, 0, None, C.byref(n)) == -1
    assert lib.peaq_debug_stream_plan(0, 0, 120, 1, 0, None, None, 0, None, C.byref(n)) == -1
    assert lib.peaq_debug_stream_plan(0, 64, 120, 1, 1, pad, ns, 0, None, C.byref(n)) == -1

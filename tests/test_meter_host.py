"""CPU-side tests of the live meter (peaq_session_set_meter, include/peaq_amd.h "meter"): the list of a
finished stream's readings (peaq_meter_readings) held against the batch rules it refers to (peaq_window_frames,
peaq_span_blocks), the seconds-to-frames helper, the refusals that need no session, and the size of the public struct.
No GPU.  (A session exists only on a device: what one refuses once it has been pushed to, or reads with its meter off, is
in tests/test_gpu_meter.py.)"""
import ctypes as C

import pytest

U32P = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def lib():
    import gstpeaq_amd
    if not gstpeaq_amd.library_path().exists():
        gstpeaq_amd.build_library()
    L = gstpeaq_amd.load_library()
    L.peaq_last_error.restype = C.c_char_p
    return L


def rows_of(lib, n_ref, n_test, W, H):
    import gstpeaq_amd
    cfg = gstpeaq_amd.MeterConfig(W, H, 1)
    n = C.c_int(-1)
    assert lib.peaq_meter_readings(n_ref, n_test, C.byref(cfg), None, 0, C.byref(n)) == 0
    buf = (gstpeaq_amd.MeterReading * max(n.value, 1))()
    for i in range(len(buf)):
        buf[i].r[0] = 12345.0                           # (`r` is left alone)
    m = C.c_int(-1)
    assert lib.peaq_meter_readings(n_ref, n_test, C.byref(cfg), buf, n.value, C.byref(m)) == 0 and m.value == n.value
    assert all(buf[i].r[0] == 12345.0 for i in range(n.value))
    return [buf[i] for i in range(n.value)]


def batch_frames(lib, n_ref, n_test, start, length):
    first, count = C.c_uint32(0xdead), C.c_uint32(0xdead)
    assert lib.peaq_window_frames(n_ref, n_test, start, length, C.byref(first), C.byref(count)) == 0
    return first.value, count.value


def batch_blocks(lib, n_ref, n_test, start, length):
    first, count = C.c_uint32(0xdead), C.c_uint32(0xdead)
    assert lib.peaq_span_blocks(n_ref, n_test, start, length, C.byref(first), C.byref(count)) == 0
    return first.value, count.value


def grid_lengths():
    base = {0, 1, 1500, 2047, 2048, 2049, 3071, 3072, 9000}
    base |= {192 * j for j in range(1, 47, 5)} | {1024 * j + d for j in range(1, 9) for d in (-1, 0, 1)}
    base = sorted(x for x in base if 0 <= x <= 9000)
    pairs = {(x, x) for x in base}
    pairs |= {(x, y) for x in base for y in (0, 1, 1500, 2048, 3072, 4097, 6144, 8191, 9000)}
    pairs |= {(y, x) for x, y in pairs}
    return sorted(pairs)


def test_the_list_of_readings_against_the_batch_rules_on_a_grid(lib):
    corner_e_is_m = corner_flush_only = partial_rows = mapped = 0
    for n_ref, n_test in grid_lengths():
        n, m = min(n_ref, n_test), max(n_ref, n_test)
        T, TB = lib.peaq_frame_count(n_ref, n_test, 0), lib.peaq_frame_count(n_ref, n_test, 1)
        for W in (1, 2, 3, 7):
            for H in (1, 2, 3, 9):
                rows = rows_of(lib, n_ref, n_test, W, H)
                where = (n_ref, n_test, W, H)
                # the count: every complete window, and the oldest one that the end cuts short
                complete = (T - W) // H + 1 if T >= W else 0
                assert len(rows) == complete + (1 if complete * H < T else 0), where
                for k, row in enumerate(rows):
                    a, b = k * H, min(k * H + W, T)
                    assert row.index == k and (row.first_frame, row.n_frames) == (a, b - a), (where, k)
                    assert row.n_frames >= 1, (where, k)
                    partial = row.n_frames < W
                    assert not partial or k == len(rows) - 1, (where, k)      # at most one, and the last
                    partial_rows += partial
                    start, e = (1024 * (a + 1) if a else 0), 1024 * (k * H + W + 1)
                    assert row.start == start, (where, k)
                    reaches_end = k * H + W >= T
                    want_blocks = (start // 192, (TB if reaches_end else e // 192) - start // 192)
                    assert (row.first_block, row.n_blocks) == want_blocks, (where, k)
                    if row.length:
                        assert row.length == (m - start if reaches_end else e - start), (where, k)
                        assert batch_frames(lib, n_ref, n_test, row.start, row.length) == (a, b - a), (where, k)
                        assert batch_blocks(lib, n_ref, n_test, row.start, row.length) == want_blocks, (where, k)
                        mapped += 1
                    else:                                   # the two corners, and nothing else
                        if reaches_end:
                            assert start >= m and (a, b) == (T - 1, T), (where, k)
                            corner_flush_only += 1
                        else:
                            assert e == m and b == T - 1, (where, k)
                            corner_e_is_m += 1
                    # (a window that does not reach the end lies in whole frames of both signals)
                    assert reaches_end or e <= n, (where, k)
    assert corner_e_is_m and corner_flush_only and partial_rows and mapped > 10000


GPU_CASES = [(120000, 120000), (98500, 100000), (100000, 98500), (1500, 1500), (31700, 31700), (5000, 5000),
             (96000, 96000)]                            # tests/test_gpu_meter.py's lengths
GPU_GEOMETRIES = [(16, 4), (1, 1), (64, 1), (5, 9), (200, 200), (4, 2)]


def test_every_reading_of_the_gpu_cases_has_a_batch_window(lib):
    for n_ref, n_test in GPU_CASES:
        for W, H in GPU_GEOMETRIES:
            rows = rows_of(lib, n_ref, n_test, W, H)
            assert rows and all(r.length for r in rows), (n_ref, n_test, W, H)


def test_meter_frames_rounds_and_never_gives_zero(lib):
    import gstpeaq_amd
    f = C.c_uint32(0xdead)
    for seconds, want in ((0.0, 1), (0.001, 1), (1024 / 48000, 1), (1.5 * 1024 / 48000, 2), (1.0, 47), (0.5, 23), (3.0, 141),
                          (0.25, 12), (0.1, 5), (5.0, 234), (600.0, 28125)):
        assert lib.peaq_meter_frames(seconds, C.byref(f)) == 0 and f.value == want, (seconds, f.value)
        assert gstpeaq_amd.meter_frames(seconds) == want
        assert want == max(1, int(seconds * 48000 / 1024 + 0.5))
    assert lib.peaq_meter_frames(1.0, None) == -1
    assert lib.peaq_last_error().decode() == "peaq_meter_frames: frames is NULL"
    for bad in (-1.0, float("nan"), float("inf"), 1e7):
        assert lib.peaq_meter_frames(bad, C.byref(f)) == -1
        assert lib.peaq_last_error().decode().startswith("peaq_meter_frames: seconds "), bad


def test_the_entries_refuse_what_needs_no_device(lib):
    import gstpeaq_amd
    cfg = gstpeaq_amd.MeterConfig(16, 4, 8)
    n, dropped = C.c_int(7), C.c_uint64(7)
    row = gstpeaq_amd.MeterReading()
    assert lib.peaq_session_set_meter(None, C.byref(cfg)) == -1
    assert lib.peaq_last_error().decode() == "peaq_session_set_meter: session is NULL"
    assert lib.peaq_session_meter_read(None, C.byref(row), 1, C.byref(n), C.byref(dropped)) == -1
    assert lib.peaq_last_error().decode() == "peaq_session_meter_read: NULL argument"
    s = C.c_void_p(0x5000)                                  # never dereferenced: the checks below come first
    assert lib.peaq_session_meter_read(s, C.byref(row), 1, None, None) == -1
    assert lib.peaq_session_meter_read(s, None, 1, C.byref(n), None) == -1 and n.value == 0
    assert lib.peaq_last_error().decode() == "peaq_session_meter_read: cap 1 with out NULL"
    for W, H, D, words in ((65, 1, 8, "keeps 65 windows open at once, more than 64"),
                           (1000, 10, 8, "keeps 100 windows open at once, more than 64"),
                           (16, 0, 8, "window_frames 16 and hop_frames 0 must both be at least 1"),
                           (16, 4, 0, "depth 0 is outside 1 .. 4096"), (16, 4, 4097, "depth 4097 is outside 1 .. 4096")):
        bad = gstpeaq_amd.MeterConfig(W, H, D)
        assert lib.peaq_session_set_meter(s, C.byref(bad)) == -1, (W, H, D)
        msg = lib.peaq_last_error().decode()
        assert msg.startswith("peaq_session_set_meter: ") and words in msg, msg
    assert lib.peaq_meter_readings(48000, 48000, None, None, 0, C.byref(n)) == -1
    assert lib.peaq_meter_readings(48000, 48000, C.byref(cfg), None, 0, None) == -1
    assert lib.peaq_meter_readings(48000, 48000, C.byref(cfg), None, 3, C.byref(n)) == -1
    zero = gstpeaq_amd.MeterConfig(0, 4, 8)
    assert lib.peaq_meter_readings(48000, 48000, C.byref(zero), None, 0, C.byref(n)) == -1
    assert "window_frames 0" in lib.peaq_last_error().decode()


def test_the_list_fills_no_more_rows_than_it_is_given(lib):
    import gstpeaq_amd
    cfg = gstpeaq_amd.MeterConfig(16, 4, 1)
    buf = (gstpeaq_amd.MeterReading * 4)()
    buf[3].index = 99
    n = C.c_int(0)
    assert lib.peaq_meter_readings(120000, 120000, C.byref(cfg), buf, 3, C.byref(n)) == 0
    assert n.value == len(gstpeaq_amd.meter_windows(120000, 120000, 16, 4)) > 3
    assert [buf[i].index for i in range(4)] == [0, 1, 2, 99]


def test_the_reading_has_the_size_the_library_says(lib):
    import gstpeaq_amd
    lib.peaq_meter_reading_size.restype = C.c_size_t
    assert lib.peaq_meter_reading_size() == C.sizeof(gstpeaq_amd.MeterReading) == 3 * 8 + 4 * 4 + 16 * 8
    assert C.sizeof(gstpeaq_amd.MeterConfig) == 12


def test_python_binding_exports_the_meter():
    import gstpeaq_amd
    for name in ("meter_frames", "meter_windows", "MeterConfig", "MeterReading", "METER_MAX_OPEN", "METER_MAX_DEPTH"):
        assert hasattr(gstpeaq_amd, name) and name in gstpeaq_amd.__all__, name
    for name in ("set_meter", "meter_read", "reset"):
        assert hasattr(gstpeaq_amd.Session, name), name
    rows = gstpeaq_amd.meter_windows(120000, 120000, 16, 4)
    assert [r["index"] for r in rows] == list(range(len(rows)))
    assert rows[0] == dict(index=0, start=0, length=1024 * 17, first_frame=0, n_frames=16, first_block=0,
                           n_blocks=1024 * 17 // 192)

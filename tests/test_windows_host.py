"""CPU-side tests of the scores of time windows (peaq_batch_run_windows, include/peaq_amd.h): the rule that
says which frames a window covers, what the entries refuse before a context or a device is touched, the names the
header, the library and the Python package agree on, and the CLI's usage errors.  No GPU."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import gst_env

ROOT = Path(__file__).resolve().parent.parent
U32P = C.POINTER(C.c_uint32)
WINDOWS_MAX = 4096


@pytest.fixture(scope="module")
def lib():
    import gstpeaq_amd
    if not gstpeaq_amd.library_path().exists():
        gstpeaq_amd.build_library()
    L = gstpeaq_amd.load_library()
    L.peaq_last_error.restype = C.c_char_p
    return L


# ---- the frame rule ---------------------------------------------------------------------------------------------------
def F(a):
    return (a - 2048) // 1024 + 1 if a >= 2048 else 0


def rule(lib, n_ref, n_test, start, length):
    """the header's rule, restated: (first, count)"""
    n, m, total = min(n_ref, n_test), max(n_ref, n_test), lib.peaq_frame_count(n_ref, n_test, 0)
    e = start + length                                 # (Python integers: no wrap at 2^32)
    first = total if start >= m else F(min(start, n))
    end = total if e >= m else F(min(e, n))
    return first, end - first


def frames(lib, n_ref, n_test, start, length):
    first, count = C.c_uint32(0xdead), C.c_uint32(0xdead)
    assert lib.peaq_window_frames(n_ref, n_test, start, length, C.byref(first), C.byref(count)) == 0
    return first.value, count.value


LENGTHS = [(48000, 48000), (100000, 98500), (98500, 100000), (5000, 2047), (2047, 5000), (2048, 2048), (2049, 2048),
           (3072, 3071), (1500, 1500), (1, 0), (0, 1), (0, 0), (2000, 9000), (4096, 4097)]


def test_window_frames_follows_the_rule_on_a_grid(lib):
    seen_flush = seen_empty = 0
    for n_ref, n_test in LENGTHS:
        n, m = min(n_ref, n_test), max(n_ref, n_test)
        starts = sorted({s for s in (0, 1, 1023, 1024, 2047, 2048, 2049, 3071, 3072, n - 1, n, n + 1, m - 1, m, m + 1,
                                     0xFFFFFFFF) if 0 <= s <= 0xFFFFFFFF})
        for start in starts:
            lengths = {1, 2, 1024, 2048, 2049, 0xFFFFFFFF, 0xFFFFFFFF - start, 0x100000000 - start}
            lengths |= {m - 1 - start, m - start, m + 1 - start, n - 1 - start, n - start, n + 1 - start}
            for length in sorted(x for x in lengths if 1 <= x <= 0xFFFFFFFF):
                want = rule(lib, n_ref, n_test, start, length)
                assert frames(lib, n_ref, n_test, start, length) == want, (n_ref, n_test, start, length)
                total = lib.peaq_frame_count(n_ref, n_test, 0)
                assert want[0] + want[1] <= total
                seen_flush += want[1] > 0 and want[0] + want[1] == total and total > F(n)
                seen_empty += want[1] == 0
    assert seen_flush and seen_empty


def test_a_window_that_ends_one_sample_short_of_the_longer_signal_leaves_the_flush_frame(lib):
    for n_ref, n_test in ((48000, 48000), (100000, 98500), (98500, 100000), (5000, 2047)):
        m, total = max(n_ref, n_test), lib.peaq_frame_count(n_ref, n_test, 0)
        assert frames(lib, n_ref, n_test, 0, m) == (0, total)
        assert frames(lib, n_ref, n_test, 0, m - 1) == (0, F(min(m - 1, n_ref, n_test)))
        assert F(min(m - 1, n_ref, n_test)) == total - 1   # (these pairs have a flush frame)


def test_start_plus_length_beyond_32_bits_does_not_wrap(lib):
    assert frames(lib, 48000, 48000, 0xFFFFFFFF, 0xFFFFFFFF) == (46, 0)
    assert frames(lib, 48000, 48000, 4096, 0xFFFFFFFF) == (F(4096), 46 - F(4096))
    assert frames(lib, 48000, 48000, 47000, 0xFFFFF000) == (F(47000), 46 - F(47000))
    # (wrapped, 47000 + 0xFFFFF000 would be 42904: a window that ends before it starts)


def test_windows_from_zero_agree_with_the_frame_count_and_the_trajectorys_f(lib):
    for n_ref, n_test in LENGTHS:
        n, m = min(n_ref, n_test), max(n_ref, n_test)
        if m:
            assert frames(lib, n_ref, n_test, 0, m) == (0, lib.peaq_frame_count(n_ref, n_test, 0))
        for L in (1, 100, 1000, 2047, 2048, 3071, 3072, 4096, 47999, 98499, 98500, 98501, 99999):
            if L < m:
                assert frames(lib, n_ref, n_test, 0, L) == (0, F(min(L, n))), (n_ref, n_test, L)


def test_window_frames_takes_either_output_alone(lib):
    first, count = C.c_uint32(0), C.c_uint32(0)
    assert lib.peaq_window_frames(48000, 48000, 24000, 12000, C.byref(first), None) == 0 and first.value == F(24000)
    assert lib.peaq_window_frames(48000, 48000, 24000, 12000, None, C.byref(count)) == 0
    assert count.value == F(36000) - F(24000)
    assert lib.peaq_window_frames(48000, 48000, 0, 1, None, None) == -1
    assert lib.peaq_last_error().decode().startswith("peaq_window_frames: ")


# ---- refusals ---------------------------------------------------------------------------------------------------------
def batch_windows(lib, windows=((0, 48000), (24000, 12000)), n_windows=None, d_windows=0x1000, ctx=None, channels=2,
                  n_pairs=2, ref=0x100000, test=0x200000, pair_stride=48000, n_ref=None, n_test=None, n_uniform=48000):
    """peaq_batch_run_windows with made-up device addresses: nothing may get as far as reading them"""
    w = None if windows is None else np.ascontiguousarray(windows, dtype=np.uint32).reshape(-1, 2)
    a = None if n_ref is None else np.ascontiguousarray(n_ref, dtype=np.uint32)
    b = None if n_test is None else np.ascontiguousarray(n_test, dtype=np.uint32)
    rc = lib.peaq_batch_run_windows(ctx, channels, 92.0, n_pairs, C.c_void_p(ref) if ref else None,
                                    C.c_void_p(test) if test else None, pair_stride,
                                    None if a is None else a.ctypes.data_as(U32P),
                                    None if b is None else b.ctypes.data_as(U32P), n_uniform,
                                    None if w is None else C.c_void_p(w.ctypes.data),
                                    (0 if w is None else len(w)) if n_windows is None else n_windows,
                                    C.c_void_p(d_windows) if d_windows else None, C.c_void_p(0x3000), None)
    return rc, lib.peaq_last_error().decode()


def test_batch_entry_refuses_its_own_arguments_by_name_and_value(lib):
    rc, msg = batch_windows(lib, windows=None, n_windows=2)
    assert rc == -1 and msg == "peaq_batch_run_windows: windows is NULL", msg
    many = np.zeros((WINDOWS_MAX + 1, 2), dtype=np.uint32)
    many[:, 1] = 1
    for n in (0, -1, WINDOWS_MAX + 1):
        rc, msg = batch_windows(lib, windows=many, n_windows=n)
        assert rc == -1 and msg == "peaq_batch_run_windows: n_windows %d is outside 1 .. %d" % (n, WINDOWS_MAX), msg
    rc, msg = batch_windows(lib, windows=many[:WINDOWS_MAX])
    assert rc == -1 and msg == "peaq_batch_run_windows: ctx is NULL", msg
    rc, msg = batch_windows(lib, windows=((0, 5), (7, 1), (9, 0), (0, 0)))
    assert rc == -1 and msg == "peaq_batch_run_windows: window 2 has length 0", msg
    rc, msg = batch_windows(lib, d_windows=0)
    assert rc == -1 and msg == "peaq_batch_run_windows: d_windows is NULL", msg
    for addr in (0x1008, 0x1004, 0x100f):
        rc, msg = batch_windows(lib, d_windows=addr)
        assert rc == -1 and msg == "peaq_batch_run_windows: d_windows is not 16-byte aligned", msg
    # (the windows come before the output pointer)
    rc, msg = batch_windows(lib, windows=((0, 0),), d_windows=0)
    assert rc == -1 and "window 0 has length 0" in msg, msg


def test_what_peaq_batch_run_refuses_is_refused_here_too(lib):
    rc, msg = batch_windows(lib)
    assert rc == -1 and msg == "peaq_batch_run_windows: ctx is NULL", msg
    ctx = C.c_void_p(0x5000)                            # never dereferenced: the checks below come first
    rc, msg = batch_windows(lib, ctx=ctx, channels=3)
    assert rc == -1 and msg == "peaq_batch_run_windows: channels must be 1 or 2, not 3", msg
    rc, msg = batch_windows(lib, ctx=ctx, n_pairs=-1)
    assert rc == -1 and msg == "peaq_batch_run_windows: n_pairs < 0", msg
    rc, msg = batch_windows(lib, ctx=ctx, ref=0)
    assert rc == -1 and msg == "peaq_batch_run_windows: NULL buffer", msg
    rc, msg = batch_windows(lib, ctx=ctx, test=0)
    assert rc == -1 and msg == "peaq_batch_run_windows: NULL buffer", msg
    rc, msg = batch_windows(lib, ctx=ctx, n_ref=[10, 10])
    assert rc == -1 and msg == "peaq_batch_run_windows: give both n_ref and n_test or neither", msg
    rc, _ = batch_windows(lib, ctx=ctx, n_pairs=0)
    assert rc == 0                                      # no pairs: nothing to do, as peaq_batch_run


def test_host_pair_entry_checks_its_arguments(lib):
    x = np.zeros(4096, dtype=np.float32)
    px = x.ctypes.data_as(C.POINTER(C.c_float))
    w = np.array([[0, 2048], [1024, 0]], dtype=np.uint32)

    def call(windows=w, n_windows=1, out=0x1000, channels=1, rate=48000, max_lag=0):
        rc = lib.peaq_run_pair_windows(None, channels, 92.0, rate, max_lag, px, 4096, px, 4096,
                                       None if windows is None else C.c_void_p(windows.ctypes.data), n_windows,
                                       C.c_void_p(out) if out else None, None, None)
        return rc, lib.peaq_last_error().decode()

    rc, msg = call(windows=None)
    assert rc == -1 and msg == "peaq_run_pair_windows: windows is NULL", msg
    rc, msg = call(n_windows=0)
    assert rc == -1 and msg == "peaq_run_pair_windows: n_windows 0 is outside 1 .. %d" % WINDOWS_MAX, msg
    rc, msg = call(n_windows=2)
    assert rc == -1 and msg == "peaq_run_pair_windows: window 1 has length 0", msg
    rc, msg = call(out=0)
    assert rc == -1 and msg == "peaq_run_pair_windows: out_windows is NULL", msg
    rc, msg = call(out=0, max_lag=20000)                # (the entry's own arguments come before max_lag)
    assert rc == -1 and msg == "peaq_run_pair_windows: out_windows is NULL", msg
    rc, msg = call(max_lag=20000)
    assert rc == -1 and msg.startswith("peaq_run_pair_windows: max_lag 20000 is outside 1 .. "), msg
    rc, msg = call(channels=5)
    assert rc == -1 and "channels must be 1 or 2" in msg, msg
    rc, msg = call()
    assert rc == -1 and msg == "peaq_run_pair_windows: NULL argument: ctx is NULL", msg


# ---- names ------------------------------------------------------------------------------------------------------------
NAME = r"peaq_[a-z_0-9]*window[a-z_0-9]*"


def test_the_header_declares_what_the_library_exports(lib):
    import gstpeaq_amd
    header = (ROOT / "include" / "peaq_amd.h").read_text()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)       # (comments speak of the entries as `name (...)` too)
    declared = set(re.findall(r"\b(" + NAME + r")\s*\(", code))
    # the dynamic symbol table's strings: names between two NULs
    exported = {m.decode() for m in re.findall(rb"\x00(" + NAME.encode() + rb")(?=\x00)",
                                               gstpeaq_amd.library_path().read_bytes())}
    exported = {n for n in exported if hasattr(lib, n)}
    want = {"peaq_window_frames", "peaq_batch_run_windows", "peaq_batch_windows_workspace_bytes", "peaq_run_pair_windows",
            "peaq_drift_windows"}
    assert declared == want, declared
    assert exported == want, exported
    assert "#define PEAQ_WINDOWS_MAX 4096" in header
    assert re.search(r"typedef struct \{ uint32_t start, length; \} peaq_window;", header)
    # what the definition promises its readers
    for phrase in ("NOT a cold-start score", "pair_stride view", "no `advanced`"):
        assert phrase in header, phrase


def test_workspace_bytes_adds_the_trace_and_the_snapshots(lib):
    lib.peaq_batch_windows_workspace_bytes.restype = C.c_size_t
    lib.peaq_batch_windows_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_int]
    lib.peaq_batch_workspace_bytes.restype = C.c_size_t
    plain = lib.peaq_batch_workspace_bytes(0, 2, 64, 480000)
    got = lib.peaq_batch_windows_workspace_bytes(2, 64, 480000, 19)
    assert got - plain == 64 * (lib.peaq_frame_count(480000, 480000, 0) * 128 + 19 * 2184) + 19 * 8


def test_python_binding_exports_the_windows():
    import gstpeaq_amd
    names = ("WINDOWS_MAX", "window_frames", "sliding_windows", "batch_windows", "run_pair_windows")
    for name in names:
        assert hasattr(gstpeaq_amd, name) and name in gstpeaq_amd.__all__, name
    assert gstpeaq_amd.WINDOWS_MAX == WINDOWS_MAX
    assert gstpeaq_amd.window_frames(100000, 98500, 24000, 12000) == (F(24000), F(36000) - F(24000))


def test_sliding_windows_cover_the_signal_and_the_last_reaches_its_end():
    import gstpeaq_amd
    for n, length, hop in ((480000, 240000, 48000), (480000, 48000, 24000), (100000, 48000, 24000), (100000, 24000, None),
                           (3000, 1000, 1000), (1000, 5000, 100), (48000, 48000, 1), (48001, 48000, 7)):
        w = gstpeaq_amd.sliding_windows(n, length, hop)
        assert w.dtype == np.uint32 and w.ndim == 2 and w.shape[1] == 2
        start, size = w[:, 0].astype(np.int64), w[:, 1].astype(np.int64)
        step = length if hop is None else hop
        assert start[0] == 0 and (np.diff(start) == step).all()
        assert (size >= 1).all() and (size[:-1] == length).all() and start[-1] + size[-1] == n
        assert (start[:-1] + size[:-1] < n).all()       # only the last reaches the end
        if step <= length:                              # no sample between two windows is left out
            assert (start[1:] <= start[:-1] + size[:-1]).all()
    assert gstpeaq_amd.sliding_windows(480000, 240000, 48000).tolist() == [[k * 48000, 240000] for k in range(6)]


# ---- the CLI ----------------------------------------------------------------------------------------------------------
def cli(*args):
    if not gst_env.CLI.exists():
        subprocess.run(["make", "-C", str(gst_env.CLI.parent)], check=True, capture_output=True)
    return subprocess.run([str(gst_env.CLI), *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("flag", ["--windows", "--windows="])
def test_cli_windows_without_a_value_is_a_usage_error(flag):
    out = cli(flag, "ref.wav", "test.wav")
    assert out.returncode == 1 and "--windows needs a length in seconds" in out.stderr, (out.returncode, out.stderr)


def test_cli_windows_usage_errors_and_help():
    out = cli("--windows=1", "--advanced", "ref.wav", "test.wav")
    assert out.returncode == 1 and "--windows is for the basic version" in out.stderr, out.stderr
    out = cli("--windows=1", "--interval=1", "ref.wav", "test.wav")
    assert out.returncode == 1 and "--windows belongs to the plain one-call mode" in out.stderr, out.stderr
    out = cli("--windows=1:0.5", "--list=pairs.txt")
    assert out.returncode == 1 and "--windows belongs to the plain one-call mode" in out.stderr, out.stderr
    for other in ("--trace=y.csv", "--bands=y.csv", "--pattern-bands=y.csv", "--band-summary=y.csv", "--match-gain",
                  "--align-subsample", "--align-drift", "--align-track", "--align-steps"):
        out = cli("--windows=1", other, "ref.wav", "test.wav")
        assert out.returncode == 1 and "--windows is a run of its own" in out.stderr, (other, out.stderr)
    for bad in ("--windows=x", "--windows=0", "--windows=1:0", "--windows=1:", "--windows=1:x", "--windows=-1"):
        out = cli(bad, "ref.wav", "test.wav")
        assert out.returncode == 1 and "invalid windows" in out.stderr, (bad, out.stderr)
    out = cli("--help")
    assert out.returncode == 0 and "--windows=S[:HOP]" in out.stdout and "window START_S END_S FRAMES ODG DI" in out.stdout

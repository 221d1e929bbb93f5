"""CPU-side tests of the scores of time spans in the advanced version (peaq_batch_run_adv_spans, include/peaq_amd.h;
DESIGN.md 28): the rule that says which filter-bank blocks a span covers, what the entries refuse before a context or a
device is touched, the names the header, the library and the Python package agree on, the workspace formula and the
CLI's usage errors.  No GPU."""
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
M32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib():
    import gstpeaq_amd
    if not gstpeaq_amd.library_path().exists():
        gstpeaq_amd.build_library()
    L = gstpeaq_amd.load_library()
    L.peaq_last_error.restype = C.c_char_p
    return L


# ---- the block rule ---------------------------------------------------------------------------------------------------
def B(a):
    return a // 192


def rule(lib, n_ref, n_test, start, length):
    """the header's block rule, restated: (first_b, count_b)"""
    n, m, total = min(n_ref, n_test), max(n_ref, n_test), lib.peaq_frame_count(n_ref, n_test, 1)
    e = start + length                                 # (Python integers: no wrap at 2^32)
    first = total if start >= m else B(min(start, n))
    end = total if e >= m else B(min(e, n))
    return first, end - first


def blocks(lib, n_ref, n_test, start, length):
    first, count = C.c_uint32(0xdead), C.c_uint32(0xdead)
    assert lib.peaq_span_blocks(n_ref, n_test, start, length, C.byref(first), C.byref(count)) == 0
    return first.value, count.value


SIZES = (0, 1, 191, 192, 193, 2047, 2048, 100000)


def test_span_blocks_follows_the_rule_on_a_grid(lib):
    seen_flush = seen_empty = 0
    for n_ref in SIZES:
        for n_test in SIZES:                           # (ragged both ways)
            n, m, total = min(n_ref, n_test), max(n_ref, n_test), lib.peaq_frame_count(n_ref, n_test, 1)
            assert total == B(n) + (m > B(n) * 192)
            starts = {0, 1, 191, 192, 193, 383, 384, 385, n - 1, n, n + 1, m - 1, m, m + 1, M32}
            starts |= {192 * (n // 192) + d for d in (-1, 0, 1)}
            for start in sorted(s for s in starts if 0 <= s <= M32):
                lengths = {1, 2, 191, 192, 193, 384, M32, M32 - start, 0x100000000 - start}
                lengths |= {m - 1 - start, m - start, m + 1 - start, n - 1 - start, n - start, n + 1 - start}
                lengths |= {192 * k - start + d for k in (1, 2, n // 192, n // 192 + 1) for d in (-1, 0, 1)}
                for length in sorted(x for x in lengths if 1 <= x <= M32):
                    want = rule(lib, n_ref, n_test, start, length)
                    assert blocks(lib, n_ref, n_test, start, length) == want, (n_ref, n_test, start, length)
                    assert want[0] + want[1] <= total
                    seen_flush += want[1] > 0 and want[0] + want[1] == total and total > B(n)
                    seen_empty += want[1] == 0
    assert seen_flush and seen_empty


def test_start_plus_length_beyond_32_bits_does_not_wrap(lib):
    assert blocks(lib, 48000, 48000, M32, M32) == (250, 0)
    assert blocks(lib, 48000, 48000, 4096, M32) == (B(4096), 250 - B(4096))
    assert blocks(lib, 48000, 48000, 47000, 0xFFFFF000) == (B(47000), 250 - B(47000))
    assert blocks(lib, 100000, 98500, 1000, M32) == (B(1000), lib.peaq_frame_count(100000, 98500, 1) - B(1000))


def test_spans_from_zero_agree_with_the_block_count_and_the_trajectorys_b(lib):
    for n_ref in SIZES:
        for n_test in SIZES:
            n, m = min(n_ref, n_test), max(n_ref, n_test)
            total = lib.peaq_frame_count(n_ref, n_test, 1)
            for L in (1, 100, 191, 192, 193, 1000, 2047, 2048, 2049, 99999, 100000, 100001, M32):
                if L < m:
                    assert blocks(lib, n_ref, n_test, 0, L) == (0, min(L, n) // 192), (n_ref, n_test, L)
                else:
                    assert blocks(lib, n_ref, n_test, 0, L) == (0, total), (n_ref, n_test, L)


def test_span_blocks_takes_either_output_alone(lib):
    first, count = C.c_uint32(0), C.c_uint32(0)
    assert lib.peaq_span_blocks(48000, 48000, 24000, 12000, C.byref(first), None) == 0 and first.value == B(24000)
    assert lib.peaq_span_blocks(48000, 48000, 24000, 12000, None, C.byref(count)) == 0
    assert count.value == B(36000) - B(24000)
    assert lib.peaq_span_blocks(48000, 48000, 0, 1, None, None) == -1
    assert lib.peaq_last_error().decode().startswith("peaq_span_blocks: ")


# ---- refusals ---------------------------------------------------------------------------------------------------------
def batch_spans(lib, spans=((0, 48000), (24000, 12000)), n_spans=None, d_spans=0x1000, ctx=None, channels=2, n_pairs=2,
                ref=0x100000, test=0x200000, pair_stride=48000, n_ref=None, n_test=None, n_uniform=48000):
    """peaq_batch_run_adv_spans with made-up device addresses: nothing may get as far as reading them"""
    w = None if spans is None else np.ascontiguousarray(spans, dtype=np.uint32).reshape(-1, 2)
    a = None if n_ref is None else np.ascontiguousarray(n_ref, dtype=np.uint32)
    b = None if n_test is None else np.ascontiguousarray(n_test, dtype=np.uint32)
    rc = lib.peaq_batch_run_adv_spans(ctx, channels, 92.0, n_pairs, C.c_void_p(ref) if ref else None,
                                      C.c_void_p(test) if test else None, pair_stride,
                                      None if a is None else a.ctypes.data_as(U32P),
                                      None if b is None else b.ctypes.data_as(U32P), n_uniform,
                                      None if w is None else C.c_void_p(w.ctypes.data),
                                      (0 if w is None else len(w)) if n_spans is None else n_spans,
                                      C.c_void_p(d_spans) if d_spans else None, C.c_void_p(0x3000), None)
    return rc, lib.peaq_last_error().decode()


def test_batch_entry_refuses_its_own_arguments_by_name_and_value(lib):
    rc, msg = batch_spans(lib, spans=None, n_spans=2)
    assert rc == -1 and msg == "peaq_batch_run_adv_spans: spans is NULL", msg
    many = np.zeros((WINDOWS_MAX + 1, 2), dtype=np.uint32)
    many[:, 1] = 1
    for n in (0, -1, WINDOWS_MAX + 1):
        rc, msg = batch_spans(lib, spans=many, n_spans=n)
        assert rc == -1 and msg == "peaq_batch_run_adv_spans: n_spans %d is outside 1 .. %d" % (n, WINDOWS_MAX), msg
    rc, msg = batch_spans(lib, spans=many[:WINDOWS_MAX])
    assert rc == -1 and msg == "peaq_batch_run_adv_spans: ctx is NULL", msg
    rc, msg = batch_spans(lib, spans=((0, 5), (7, 1), (9, 0), (0, 0)))
    assert rc == -1 and msg == "peaq_batch_run_adv_spans: span 2 has length 0", msg
    rc, msg = batch_spans(lib, d_spans=0)
    assert rc == -1 and msg == "peaq_batch_run_adv_spans: d_spans is NULL", msg
    for addr in (0x1008, 0x1004, 0x100f):
        rc, msg = batch_spans(lib, d_spans=addr)
        assert rc == -1 and msg == "peaq_batch_run_adv_spans: d_spans is not 16-byte aligned", msg
    # (the spans come before the output pointer)
    rc, msg = batch_spans(lib, spans=((0, 0),), d_spans=0)
    assert rc == -1 and "span 0 has length 0" in msg, msg


def test_what_peaq_batch_run_refuses_is_refused_here_too(lib):
    rc, msg = batch_spans(lib)                          # a valid call ends at the missing context
    assert rc == -1 and msg == "peaq_batch_run_adv_spans: ctx is NULL", msg
    ctx = C.c_void_p(0x5000)                            # never dereferenced: the checks below come first
    rc, msg = batch_spans(lib, ctx=ctx, channels=3)
    assert rc == -1 and msg == "peaq_batch_run_adv_spans: channels must be 1 or 2, not 3", msg
    rc, msg = batch_spans(lib, ctx=ctx, n_pairs=-1)
    assert rc == -1 and msg == "peaq_batch_run_adv_spans: n_pairs < 0", msg
    rc, msg = batch_spans(lib, ctx=ctx, ref=0)
    assert rc == -1 and msg == "peaq_batch_run_adv_spans: NULL buffer", msg
    rc, msg = batch_spans(lib, ctx=ctx, test=0)
    assert rc == -1 and msg == "peaq_batch_run_adv_spans: NULL buffer", msg
    rc, msg = batch_spans(lib, ctx=ctx, n_ref=[10, 10])
    assert rc == -1 and msg == "peaq_batch_run_adv_spans: give both n_ref and n_test or neither", msg
    rc, _ = batch_spans(lib, ctx=ctx, n_pairs=0)
    assert rc == 0                                      # no pairs: nothing to do, as peaq_batch_run


def test_host_pair_entry_checks_its_arguments(lib):
    x = np.zeros(4096, dtype=np.float32)
    px = x.ctypes.data_as(C.POINTER(C.c_float))
    w = np.array([[0, 2048], [1024, 0]], dtype=np.uint32)

    def call(spans=w, n_spans=1, out=0x1000, channels=1, rate=48000, max_lag=0):
        rc = lib.peaq_run_pair_adv_spans(None, channels, 92.0, rate, max_lag, px, 4096, px, 4096,
                                         None if spans is None else C.c_void_p(spans.ctypes.data), n_spans,
                                         C.c_void_p(out) if out else None, None, None)
        return rc, lib.peaq_last_error().decode()

    rc, msg = call(spans=None)
    assert rc == -1 and msg == "peaq_run_pair_adv_spans: spans is NULL", msg
    for n in (0, -3, WINDOWS_MAX + 1):
        rc, msg = call(n_spans=n)
        assert rc == -1 and msg == "peaq_run_pair_adv_spans: n_spans %d is outside 1 .. %d" % (n, WINDOWS_MAX), msg
    rc, msg = call(n_spans=2)
    assert rc == -1 and msg == "peaq_run_pair_adv_spans: span 1 has length 0", msg
    rc, msg = call(out=0)
    assert rc == -1 and msg == "peaq_run_pair_adv_spans: out_spans is NULL", msg
    rc, msg = call(out=0, max_lag=20000)                # (the entry's own arguments come before max_lag)
    assert rc == -1 and msg == "peaq_run_pair_adv_spans: out_spans is NULL", msg
    rc, msg = call(max_lag=20000)
    assert rc == -1 and msg.startswith("peaq_run_pair_adv_spans: max_lag 20000 is outside 1 .. "), msg
    rc, msg = call(channels=5)
    assert rc == -1 and "channels must be 1 or 2" in msg, msg
    rc, msg = call()                                    # a valid call ends at the missing context
    assert rc == -1 and msg == "peaq_run_pair_adv_spans: NULL argument: ctx is NULL", msg


# ---- names ------------------------------------------------------------------------------------------------------------
NAME = r"peaq_[a-z_0-9]*span[a-z_0-9]*"


def test_the_header_declares_what_the_library_exports(lib):
    import gstpeaq_amd
    header = (ROOT / "include" / "peaq_amd.h").read_text()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)       # (comments speak of the entries as `name (...)` too)
    declared = set(re.findall(r"\b(" + NAME + r")\s*\(", code))
    exported = {m.decode() for m in re.findall(rb"\x00(" + NAME.encode() + rb")(?=\x00)",
                                               gstpeaq_amd.library_path().read_bytes())}
    exported = {n for n in exported if hasattr(lib, n)}
    want = {"peaq_span_blocks", "peaq_batch_run_adv_spans", "peaq_batch_adv_spans_workspace_bytes",
            "peaq_run_pair_adv_spans"}
    assert declared == want, declared
    assert exported == want, exported
    # what the definition promises its readers, as the basic section does
    section = header[header.index("---- spans:"):header.index("peaq_batch_adv_spans_workspace_bytes (int")]
    for phrase in ("NOT a cold-start", "pair_stride view", "first_b = start >= m ? TB : B (min (start, n))",
                   "end_b = e >= m ? TB : B (min (e, n))", "peaq_frame_count (n_ref, n_test, 1)"):
        assert phrase in " ".join(section.replace(" * ", " ").split()), phrase


def test_workspace_bytes_adds_both_traces_and_the_snapshots(lib):
    lib.peaq_batch_adv_spans_workspace_bytes.restype = C.c_size_t
    lib.peaq_batch_adv_spans_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_int]
    lib.peaq_batch_workspace_bytes.restype = C.c_size_t
    for channels, n_pairs, n_max, n_spans in ((2, 64, 480000, 19), (1, 3, 100001, 1), (2, 1, 0, 4096)):
        plain = lib.peaq_batch_workspace_bytes(1, channels, n_pairs, n_max)
        got = lib.peaq_batch_adv_spans_workspace_bytes(channels, n_pairs, n_max, n_spans)
        frames = max(lib.peaq_frame_count(n_max, n_max, 0), 1)    # (a pair without frames keeps one record of scratch)
        blocks_ = max(lib.peaq_frame_count(n_max, n_max, 1), 1)
        assert got - plain == n_pairs * (frames * 128 + blocks_ * 96 + n_spans * 2184) + n_spans * 8


def test_python_binding_exports_the_spans():
    import gstpeaq_amd
    for name in ("span_blocks", "batch_adv_spans", "run_pair_adv_spans", "sliding_windows", "WINDOWS_MAX"):
        assert hasattr(gstpeaq_amd, name) and name in gstpeaq_amd.__all__, name
    assert gstpeaq_amd.span_blocks(100000, 98500, 24000, 12000) == (B(24000), B(36000) - B(24000))
    assert gstpeaq_amd.span_blocks(100000, 98500, 0, 100000) == (0, 514)


# ---- the CLI ----------------------------------------------------------------------------------------------------------
def cli(*args):
    if not gst_env.CLI.exists():
        subprocess.run(["make", "-C", str(gst_env.CLI.parent)], check=True, capture_output=True)
    return subprocess.run([str(gst_env.CLI), *args], capture_output=True, text=True, timeout=60)


def failed(out, text):
    return out.returncode == 1 and "Failed to initialize:" in out.stderr and text in out.stderr


@pytest.mark.parametrize("flag", ["--spans", "--spans="])
def test_cli_spans_without_a_value_is_a_usage_error(flag):
    out = cli("--advanced", flag, "ref.wav", "test.wav")
    assert failed(out, "--spans needs a length in seconds"), (out.returncode, out.stderr)


def test_cli_spans_usage_errors_and_help():
    out = cli("--spans=1", "ref.wav", "test.wav")
    assert failed(out, "--spans is for the advanced version"), out.stderr
    out = cli("--windows=1", "--advanced", "ref.wav", "test.wav")      # (the basic option still says where it belongs)
    assert failed(out, "--windows is for the basic version") and "--spans" in out.stderr, out.stderr
    out = cli("--advanced", "--spans=1", "--interval=1", "ref.wav", "test.wav")
    assert failed(out, "--spans belongs to the plain one-call mode"), out.stderr
    out = cli("--advanced", "--spans=1:0.5", "--list=pairs.txt")
    assert failed(out, "--spans belongs to the plain one-call mode"), out.stderr
    for other in ("--trace=y.csv", "--bands=y.csv", "--fb-bands=y.csv", "--band-summary=y.csv", "--fb-band-summary=y.csv",
                  "--match-gain", "--align-subsample", "--align-drift", "--align-track", "--align-steps"):
        out = cli("--advanced", "--spans=1", other, "ref.wav", "test.wav")
        assert failed(out, "--spans is a run of its own"), (other, out.stderr)
    out = cli("--advanced", "--spans=1", "--pattern-bands=y.csv", "ref.wav", "test.wav")
    assert failed(out, ""), out.stderr                  # (the basic version's output says so itself)
    for bad in ("--spans=x", "--spans=0", "--spans=1:0", "--spans=1:", "--spans=1:x", "--spans=-1"):
        out = cli("--advanced", bad, "ref.wav", "test.wav")
        assert failed(out, "invalid spans"), (bad, out.stderr)
    out = cli("--help")
    assert out.returncode == 0 and "--spans=S[:HOP]" in out.stdout
    assert "span START_S END_S FRAMES BLOCKS" in out.stdout and "window START_S END_S FRAMES ODG DI" in out.stdout


def test_cli_refuses_more_spans_than_a_call_takes(tmp_path):
    """4097 spans: 0.01 s every 0.01 s over 41 s of silence (a usage error before anything is scored)"""
    import wave
    path = tmp_path / "silence.wav"
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(48000)
        f.writeframes(bytes(2 * 48000 * 41))
    out = cli("--advanced", "--spans=0.01", str(path), str(path))
    assert failed(out, "--spans makes 4100 spans of these files, more than 4096"), (out.returncode, out.stdout, out.stderr)
    out = cli("--spans=0.01", str(path), str(path))     # (the missing --advanced comes first)
    assert failed(out, "--spans is for the advanced version"), out.stderr

"""CPU-side checks of the trace entry points (peaq_batch_run_trace, peaq_trace_sizes, peaq_run_pair_trace,
`peaq --trace`; include/peaq_amd.h): every argument the header says is refused is refused with PEAQ_ERR_ARG before a
context or a device is touched -- the calls below pass no context at all -- and the message names the value."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import gst_env


@pytest.fixture(scope="module")
def lib():
    import gstpeaq_amd
    if not gstpeaq_amd.library_path().exists():
        gstpeaq_amd.build_library()
    L = gstpeaq_amd.load_library()
    L.peaq_last_error.restype = C.c_char_p
    return L


def batch_trace(lib, advanced=0, channels=2, n_pairs=2, pair_stride=48000, n_ref=None, n_test=None, n_uniform=48000,
                frames=0x1000, frame_stride=46, blocks=None, block_stride=0, ctx=None, ref=0x100000, test=0x200000):
    """peaq_batch_run_trace with made-up device addresses: nothing may get as far as reading them"""
    u32p = C.POINTER(C.c_uint32)
    a = None if n_ref is None else np.ascontiguousarray(n_ref, dtype=np.uint32)
    b = None if n_test is None else np.ascontiguousarray(n_test, dtype=np.uint32)
    rc = lib.peaq_batch_run_trace(ctx, advanced, channels, 92.0, n_pairs, C.c_void_p(ref), C.c_void_p(test), pair_stride,
                                  None if a is None else a.ctypes.data_as(u32p),
                                  None if b is None else b.ctypes.data_as(u32p), n_uniform,
                                  C.c_void_p(frames) if frames else None, frame_stride,
                                  C.c_void_p(blocks) if blocks else None, block_stride, C.c_void_p(0x3000), None)
    return rc, lib.peaq_last_error().decode()


def test_record_sizes(lib):
    from gstpeaq_amd.capi import BLOCK_TRACE_DTYPE, FRAME_TRACE_DTYPE, BlockTrace, FrameTrace
    fb, bb = C.c_size_t(0), C.c_size_t(0)
    assert lib.peaq_trace_sizes(C.byref(fb), C.byref(bb)) == 128
    assert (fb.value, bb.value) == (128, 96) == (C.sizeof(FrameTrace), C.sizeof(BlockTrace))
    assert (FRAME_TRACE_DTYPE.itemsize, BLOCK_TRACE_DTYPE.itemsize) == (128, 96)
    assert lib.peaq_trace_sizes(None, None) == 128
    for ct, dt in ((FrameTrace, FRAME_TRACE_DTYPE), (BlockTrace, BLOCK_TRACE_DTYPE)):
        for name, _ in ct._fields_:
            assert getattr(ct, name).offset == dt.fields[name][1], name
    assert FrameTrace.flags.offset == 112 and BlockTrace.flags.offset == 80


def test_the_trace_s_own_arguments_are_refused_without_a_context(lib):
    rc, msg = batch_trace(lib, frames=0)
    assert rc == -1 and "d_frames is NULL" in msg
    rc, msg = batch_trace(lib, advanced=1)
    assert rc == -1 and "d_blocks is NULL" in msg
    rc, msg = batch_trace(lib, advanced=0, blocks=0x4000, block_stride=250)
    assert rc == -1 and "d_blocks must be NULL in the basic version" in msg
    rc, msg = batch_trace(lib, frames=0x1008)
    assert rc == -1 and "d_frames is not 16-byte aligned" in msg
    rc, msg = batch_trace(lib, advanced=1, blocks=0x4008, block_stride=250)
    assert rc == -1 and "d_blocks is not 16-byte aligned" in msg


def test_strides_below_the_longest_pair_s_count_are_refused_by_name(lib):
    # 48 000 samples: 45 full frames + the flush frame, 250 blocks
    assert lib.peaq_frame_count(48000, 48000, 0) == 46 and lib.peaq_frame_count(48000, 48000, 1) == 250
    rc, msg = batch_trace(lib, frame_stride=45)
    assert rc == -1 and "frame_stride 45 is below the longest pair's 46 frames" in msg
    rc, msg = batch_trace(lib, advanced=1, blocks=0x4000, block_stride=249)
    assert rc == -1 and "block_stride 249 is below the longest pair's 250 blocks" in msg
    # ragged: the longest pair counts, whichever side is the longer one (the flush frame takes what is left of either)
    rc, msg = batch_trace(lib, n_ref=[3000, 2048], n_test=[2048, 9000], frame_stride=8)
    assert rc == -1 and "frame_stride 8 is below the longest pair's 2 frames" not in msg and "9000" not in msg
    assert lib.peaq_frame_count(2048, 9000, 0) == 2
    rc, msg = batch_trace(lib, n_ref=[3000, 2048], n_test=[2048, 9000], frame_stride=1)
    assert rc == -1 and "frame_stride 1 is below the longest pair's 2 frames" in msg
    rc, msg = batch_trace(lib, advanced=1, n_ref=[3000, 193], n_test=[2048, 100], frame_stride=2, blocks=0x4000,
                          block_stride=10)
    assert rc == -1 and "block_stride 10 is below the longest pair's 11 blocks" in msg


def test_what_peaq_batch_run_refuses_is_refused_here_too(lib):
    """with strides that are large enough the call reaches the common driver's checks, still without a device"""
    rc, msg = batch_trace(lib)
    assert rc == -1 and "peaq_batch_run_trace: ctx is NULL" in msg
    ctx = C.c_void_p(0x5000)                            # never dereferenced: the checks below come first
    rc, msg = batch_trace(lib, ctx=ctx, channels=3)
    assert rc == -1 and "peaq_batch_run_trace: channels must be 1 or 2" in msg
    rc, msg = batch_trace(lib, ctx=ctx, n_pairs=-1)
    assert rc == -1 and "n_pairs < 0" in msg
    rc, msg = batch_trace(lib, ctx=ctx, ref=0)
    assert rc == -1 and "NULL buffer" in msg
    rc, msg = batch_trace(lib, ctx=ctx, n_ref=[10, 10])
    assert rc == -1 and "both n_ref and n_test or neither" in msg
    rc, _ = batch_trace(lib, ctx=ctx, n_pairs=0)
    assert rc == 0                                      # no pairs: nothing to do, as peaq_batch_run


def test_host_pair_entry_checks_its_arguments(lib):
    fp = C.POINTER(C.c_float)
    x = np.zeros(4096, dtype=np.float32)
    px = x.ctypes.data_as(fp)
    buf = C.c_void_p(0x1000)

    def call(advanced=0, channels=1, level=92.0, rate=48000, max_lag=0, frames=buf, blocks=None, ctx=None):
        rc = lib.peaq_run_pair_trace(ctx, advanced, channels, level, rate, max_lag, px, 4096, px, 4096, frames, 8, None,
                                     blocks, 0, None, None, None)
        return rc, lib.peaq_last_error().decode()

    rc, msg = call(frames=None)
    assert rc == -1 and "frames is NULL" in msg
    rc, msg = call(advanced=1)
    assert rc == -1 and "blocks is NULL" in msg
    rc, msg = call(blocks=buf)
    assert rc == -1 and "blocks must be NULL in the basic version" in msg
    rc, msg = call(max_lag=20000)
    assert rc == -1 and "20000" in msg
    rc, msg = call(rate=7000)
    assert rc == -1 and "7000" in msg
    rc, msg = call(channels=5)
    assert rc == -1 and "channels must be 1 or 2" in msg
    rc, msg = call()
    assert rc == -1 and "ctx is NULL" in msg


def test_python_binding_exports_the_trace(lib):
    import gstpeaq_amd
    assert callable(gstpeaq_amd.batch_trace) and callable(gstpeaq_amd.run_pair_trace)
    assert (gstpeaq_amd.TRACE_ABOVE, gstpeaq_amd.TRACE_MOD_OPEN, gstpeaq_amd.TRACE_LOUD_OPEN,
            gstpeaq_amd.TRACE_FLUSH) == (1, 2, 4, 8)
    assert gstpeaq_amd.frame_count(480000, 480000) == 468 and gstpeaq_amd.frame_count(480000, 480000, True) == 2500


@pytest.mark.parametrize("flag", ["--trace", "--trace="])
def test_cli_trace_without_a_file_name_is_a_usage_error(flag):
    if not gst_env.CLI.exists():
        subprocess.run(["make", "-C", str(gst_env.CLI.parent)], check=True, capture_output=True)
    out = subprocess.run([str(gst_env.CLI), flag, "ref.wav", "test.wav"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and "--trace needs a file name" in out.stderr, (out.returncode, out.stderr)
    out = subprocess.run([str(gst_env.CLI), "--trace=x.csv", "--interval=1", "ref.wav", "test.wav"], capture_output=True,
                         text=True, timeout=60)
    assert out.returncode == 1 and "--trace belongs to the plain one-call mode" in out.stderr
    out = subprocess.run([str(gst_env.CLI), "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "--trace=FILE" in out.stdout

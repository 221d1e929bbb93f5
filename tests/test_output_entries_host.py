"""CPU-side table of what the ten entries of the batch run's optional outputs refuse (peaq_batch_run_trace, _bands,
_fb_bands, _pattern_bands, _band_summary and their peaq_run_pair_* forms; include/peaq_amd.h): every entry's own
arguments are held against the same rules with the same words, before a context or a device is touched -- the calls
below pass no context at all -- and a call that has nothing wrong with it ends at the common driver's "ctx is NULL",
which names the entry.  The per-feature host tests pin parts of this; the table holds all ten against one list."""
import ctypes as C

import numpy as np
import pytest

N = 48000                      # 45 full frames + the flush frame, 250 blocks (test_trace_host.py)
FRAMES, BLOCKS = 46, 250
U32P = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def lib():
    import gstpeaq_amd
    if not gstpeaq_amd.library_path().exists():
        gstpeaq_amd.build_library()
    L = gstpeaq_amd.load_library()
    L.peaq_last_error.restype = C.c_char_p
    assert L.peaq_frame_count(N, N, 0) == FRAMES and L.peaq_frame_count(N, N, 1) == BLOCKS
    return L


def _ptr(addr):
    return C.c_void_p(addr) if addr else None


# ---- the batch entries: made-up device addresses, nothing may get as far as reading them --------------------------
# Each takes the arguments that differ between the rows of the table and returns the entry's own argument list (what
# follows n_uniform in the header); `stride` is the frame stride, or the block stride where the entry counts blocks.
def _trace_frames(advanced, out, stride, planes):
    return [_ptr(out), C.c_size_t(stride), _ptr(0x8000) if advanced else None, C.c_size_t(BLOCKS if advanced else 0)]


def _trace_blocks(advanced, out, stride, planes):
    return [_ptr(0x8000), C.c_size_t(FRAMES), _ptr(out), C.c_size_t(stride)]


def _rows(advanced, out, stride, planes):
    return [C.c_uint32(planes), _ptr(out), C.c_size_t(stride)]


def _summary(advanced, out, stride, planes):
    return [_ptr(out)]


# name, takes `advanced`, versions it runs in, own arguments, output's name, stride's name, count, unit, a valid mask,
# the mask's top bit and its name (None: the entry has no planes)
BATCH = {
    "trace/frames": ("peaq_batch_run_trace", True, (0, 1), _trace_frames, "d_frames", "frame_stride", FRAMES, "frames", None, None),
    "trace/blocks": ("peaq_batch_run_trace", True, (1,), _trace_blocks, "d_blocks", "block_stride", BLOCKS, "blocks", None, None),
    "bands": ("peaq_batch_run_bands", True, (0, 1), _rows, "d_bands", "frame_stride", FRAMES, "frames", 1, (16, "PEAQ_BAND_STEPS")),
    "fb_bands": ("peaq_batch_run_fb_bands", False, (1,), _rows, "d_bands", "block_stride", BLOCKS, "blocks", 4,
                 (4096, "PEAQ_FB_BAND_MOD_TEST")),
    "pattern_bands": ("peaq_batch_run_pattern_bands", False, (0,), _rows, "d_bands", "frame_stride", FRAMES, "frames", 8,
                      (4096, "PEAQ_PAT_BAND_AVGLOUD_REF")),
    "band_summary": ("peaq_batch_run_band_summary", True, (0, 1), _summary, "d_summary", None, None, None, None, None),
}
BATCH_CASES = [(k, adv) for k, row in BATCH.items() for adv in row[2]]


def batch_call(lib, key, advanced, out=0x1000, stride=None, planes=None, lengths=None, n_uniform=N):
    name, takes_adv, _, own, _, _, count, _, mask, _ = BATCH[key]
    a = b = None
    if lengths is not None:
        a = np.ascontiguousarray(lengths[0], dtype=np.uint32)
        b = np.ascontiguousarray(lengths[1], dtype=np.uint32)
    args = [None] + ([advanced] if takes_adv else []) + [
        2, C.c_double(92.0), 2, C.c_void_p(0x100000), C.c_void_p(0x200000), C.c_size_t(N),
        None if a is None else a.ctypes.data_as(U32P), None if b is None else b.ctypes.data_as(U32P), C.c_uint32(n_uniform)]
    args += own(advanced, out, count if stride is None else stride, mask if planes is None else planes)
    rc = getattr(lib, name)(*args, C.c_void_p(0x3000), None)
    return rc, lib.peaq_last_error().decode()


@pytest.mark.parametrize("key,advanced", BATCH_CASES)
def test_batch_entry_refuses_a_null_or_misaligned_output(lib, key, advanced):
    name, out_name = BATCH[key][0], BATCH[key][4]
    rc, msg = batch_call(lib, key, advanced, out=0)
    assert rc == -1 and msg.startswith(name + ": ") and out_name + " is NULL" in msg, msg
    rc, msg = batch_call(lib, key, advanced, out=0x1008)
    assert rc == -1 and msg.startswith(name + ": ") and "is not 16-byte aligned" in msg, msg
    if key == "band_summary":                           # (this one prints the address)
        assert "d_summary 0x1008 is not 16-byte aligned" in msg, msg
    else:
        assert out_name + " is not 16-byte aligned" in msg, msg


@pytest.mark.parametrize("key,advanced", [c for c in BATCH_CASES if BATCH[c[0]][5]])
def test_batch_entry_refuses_a_stride_one_below_the_longest_pair(lib, key, advanced):
    name, _, _, _, _, stride_name, count, unit, _, _ = BATCH[key]
    want = "%s: %s %d is below the longest pair's %d %s" % (name, stride_name, count - 1, count, unit)
    rc, msg = batch_call(lib, key, advanced, stride=count - 1)                      # n_uniform
    assert rc == -1 and want in msg, msg
    # per-pair lengths: the longest pair counts, wherever it stands (n_uniform is not read)
    for lengths in (([3000, N], [2048, N]), ([N, 100], [N, 2048])):
        rc, msg = batch_call(lib, key, advanced, stride=count - 1, lengths=lengths, n_uniform=7)
        assert rc == -1 and want in msg, msg
        rc, msg = batch_call(lib, key, advanced, stride=count, lengths=lengths, n_uniform=7)
        assert rc == -1 and msg == name + ": ctx is NULL", msg


@pytest.mark.parametrize("key,advanced", [c for c in BATCH_CASES if BATCH[c[0]][8]])
def test_batch_entry_refuses_planes_it_does_not_have(lib, key, advanced):
    name, (top, top_name) = BATCH[key][0], BATCH[key][9]
    rc, msg = batch_call(lib, key, advanced, planes=0)
    assert rc == -1 and msg == name + ": planes is 0 (no plane requested)", msg
    rc, msg = batch_call(lib, key, advanced, planes=2 * top | 1)
    assert rc == -1 and msg == "%s: planes %d has a bit above %d (%s)" % (name, 2 * top | 1, top, top_name), msg
    # (the planes come before the output pointer)
    rc, msg = batch_call(lib, key, advanced, planes=0, out=0)
    assert rc == -1 and "planes is 0" in msg, msg


def test_batch_bands_refuses_the_planes_the_advanced_version_lacks(lib):
    rc, msg = batch_call(lib, "bands", 1, planes=1 | 8)
    assert rc == -1 and msg == ("peaq_batch_run_bands: planes 9 asks for a plane the advanced version does not have "
                                "(8: its 55-band path has PEAQ_BAND_NMR and PEAQ_BAND_EXC_REF only)"), msg
    rc, msg = batch_call(lib, "bands", 1, planes=3)
    assert rc == -1 and msg == "peaq_batch_run_bands: ctx is NULL", msg
    rc, msg = batch_call(lib, "bands", 0, planes=31)
    assert rc == -1 and msg == "peaq_batch_run_bands: ctx is NULL", msg


@pytest.mark.parametrize("key,advanced", BATCH_CASES)
def test_valid_batch_call_ends_at_the_missing_context(lib, key, advanced):
    rc, msg = batch_call(lib, key, advanced)
    assert rc == -1 and msg == BATCH[key][0] + ": ctx is NULL", msg


# ---- the one-pair entries: host arrays; what comes after prepare_pair (the capacities) needs a device ---------------
# name, takes `advanced`, versions, the output's name, a valid mask, top bit and its name
PAIR = {
    "trace": ("peaq_run_pair_trace", True, (0, 1), "frames", None, None),
    "bands": ("peaq_run_pair_bands", True, (0, 1), "bands", 1, (16, "PEAQ_BAND_STEPS")),
    "fb_bands": ("peaq_run_pair_fb_bands", False, (1,), "bands", 4, (4096, "PEAQ_FB_BAND_MOD_TEST")),
    "pattern_bands": ("peaq_run_pair_pattern_bands", False, (0,), "bands", 8, (4096, "PEAQ_PAT_BAND_AVGLOUD_REF")),
    "band_summary": ("peaq_run_pair_band_summary", True, (0, 1), "summary", None, None),
}
PAIR_CASES = [(k, adv) for k, row in PAIR.items() for adv in row[2]]


def pair_call(lib, key, advanced, out=0x1000, planes=None, max_lag=0, blocks="as the version needs"):
    name, takes_adv, _, _, mask, _ = PAIR[key]
    x = np.zeros(4096, dtype=np.float32)
    px = x.ctypes.data_as(C.POINTER(C.c_float))
    args = [None] + ([advanced] if takes_adv else []) + [
        1, C.c_double(92.0), C.c_uint32(48000), C.c_uint32(max_lag), px, C.c_size_t(4096), px, C.c_size_t(4096)]
    if key == "trace":
        if blocks == "as the version needs":
            blocks = 0x8000 if advanced else 0
        args += [_ptr(out), C.c_size_t(8), None, _ptr(blocks), C.c_size_t(64 if advanced else 0), None]
    elif key == "band_summary":
        args += [_ptr(out)]
    else:
        args += [C.c_uint32(mask if planes is None else planes), _ptr(out), C.c_size_t(64), None]
    rc = getattr(lib, name)(*args, None, None)
    return rc, lib.peaq_last_error().decode()


@pytest.mark.parametrize("key,advanced", PAIR_CASES)
def test_pair_entry_refuses_a_null_output(lib, key, advanced):
    name, out_name = PAIR[key][0], PAIR[key][3]
    rc, msg = pair_call(lib, key, advanced, out=0)
    assert rc == -1 and msg == "%s: %s is NULL" % (name, out_name), msg
    # (the entry's own arguments come before max_lag)
    rc, msg = pair_call(lib, key, advanced, out=0, max_lag=20000)
    assert rc == -1 and msg == "%s: %s is NULL" % (name, out_name), msg
    rc, msg = pair_call(lib, key, advanced, max_lag=20000)
    assert rc == -1 and msg.startswith(name + ": max_lag 20000 is outside 1 .. "), msg


def test_pair_trace_refuses_block_records_the_version_does_not_write(lib):
    rc, msg = pair_call(lib, "trace", 1, blocks=0)
    assert rc == -1 and msg == "peaq_run_pair_trace: blocks is NULL (the advanced version writes block records)", msg
    rc, msg = pair_call(lib, "trace", 0, blocks=0x8000)
    assert rc == -1 and msg == ("peaq_run_pair_trace: blocks must be NULL in the basic version (it has no filter-bank "
                                "blocks)"), msg


@pytest.mark.parametrize("key,advanced", [c for c in PAIR_CASES if PAIR[c[0]][4]])
def test_pair_entry_refuses_planes_it_does_not_have(lib, key, advanced):
    name, (top, top_name) = PAIR[key][0], PAIR[key][5]
    rc, msg = pair_call(lib, key, advanced, planes=0)
    assert rc == -1 and msg == name + ": planes is 0 (no plane requested)", msg
    rc, msg = pair_call(lib, key, advanced, planes=2 * top | 1)
    assert rc == -1 and msg == "%s: planes %d has a bit above %d (%s)" % (name, 2 * top | 1, top, top_name), msg
    rc, msg = pair_call(lib, key, advanced, planes=0, out=0)
    assert rc == -1 and "planes is 0" in msg, msg


def test_pair_bands_refuses_the_planes_the_advanced_version_lacks(lib):
    rc, msg = pair_call(lib, "bands", 1, planes=1 | 4)
    assert rc == -1 and msg == ("peaq_run_pair_bands: planes 5 asks for a plane the advanced version does not have "
                                "(4: its 55-band path has PEAQ_BAND_NMR and PEAQ_BAND_EXC_REF only)"), msg


@pytest.mark.parametrize("key,advanced", PAIR_CASES)
def test_valid_pair_call_ends_at_the_missing_context(lib, key, advanced):
    rc, msg = pair_call(lib, key, advanced)
    assert rc == -1 and msg == PAIR[key][0] + ": NULL argument: ctx is NULL", msg

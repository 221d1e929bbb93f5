"""The host side of the shared-reference feed without a GPU (include/peaq_amd.h, "one reference, many tests"): the
argument checks of peaq_batch_gather and peaq_batch_run_host_refs, which return PEAQ_ERR_ARG with the offending value in
the message before any device is touched (a NULL context is the last thing they look at), and
peaq_feed_refs_workspace_bytes against peaq_feed_workspace_bytes."""
import ctypes as C

import numpy as np
import pytest

import gstpeaq_amd

PEAQ_ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    if not gstpeaq_amd.library_path().exists():
        gstpeaq_amd.build_library()
    return gstpeaq_amd.load_library()


def err(lib):
    return lib.peaq_last_error().decode()


def u32(*v):
    return (C.c_uint32 * len(v))(*v)


def test_gather_checks_its_arguments_before_any_device(lib):
    buf = (C.c_float * 256)()
    out = (C.c_float * 256)()
    p, q = C.cast(buf, C.c_void_p), C.cast(out, C.c_void_p)

    def call(channels=2, n_rows=2, n_out=3, d_in=p, in_stride=16, src=u32(0, 1, 1), skip=u32(0, 2, 3), n_keep=u32(16, 14, 5),
             d_out=q, out_stride=16):
        return lib.peaq_batch_gather(None, channels, n_rows, n_out, d_in, in_stride, src, skip, n_keep, d_out, out_stride, None)

    assert call(src=u32(0, 2, 1)) == PEAQ_ERR_ARG and "output 1" in err(lib) and "row 2 of 2" in err(lib), err(lib)
    assert call(src=u32(0, 1, 0xFFFFFFFF)) == PEAQ_ERR_ARG and "4294967295" in err(lib), err(lib)
    assert call(skip=u32(0, 3, 3)) == PEAQ_ERR_ARG and "skip 3" in err(lib) and "n_keep 14" in err(lib) \
        and "in_stride 16" in err(lib), err(lib)
    assert call(skip=u32(0, 2, 0xFFFFFFFF)) == PEAQ_ERR_ARG and "4294967295" in err(lib), err(lib)   # (no wrap-around)
    assert call(out_stride=15) == PEAQ_ERR_ARG and "out_stride 15" in err(lib) and "16" in err(lib), err(lib)
    for name in ("d_in", "d_out"):
        assert call(**{name: None}) == PEAQ_ERR_ARG and "NULL buffer" in err(lib), err(lib)
    for name in ("src", "skip", "n_keep"):
        assert call(**{name: None}) == PEAQ_ERR_ARG and "NULL src, skip or n_keep" in err(lib), err(lib)
    for bad in (0, 3):
        assert call(channels=bad) == PEAQ_ERR_ARG and "channels" in err(lib) and str(bad) in err(lib), err(lib)
    assert call(n_out=65536) == PEAQ_ERR_ARG and "65536 outputs" in err(lib) and "65535" in err(lib), err(lib)
    assert call(n_rows=65536) == PEAQ_ERR_ARG and "65536 rows" in err(lib) and "65535" in err(lib), err(lib)
    assert call(n_out=-1) == PEAQ_ERR_ARG and "-1" in err(lib), err(lib)
    # d_out inside d_in, and d_in inside d_out: 2 rows of 16 stereo samples are 64 floats, 3 outputs 96
    assert call(d_out=C.c_void_p(p.value + 63 * 4)) == PEAQ_ERR_ARG and "overlaps" in err(lib), err(lib)
    assert call(d_in=C.c_void_p(q.value + 95 * 4)) == PEAQ_ERR_ARG and "overlaps" in err(lib), err(lib)
    assert call(d_out=C.c_void_p(p.value + 64 * 4)) == PEAQ_ERR_ARG and "ctx is NULL" in err(lib), err(lib)
    # everything in order: the context is looked at last
    assert call() == PEAQ_ERR_ARG and "ctx is NULL" in err(lib)
    assert call(n_out=0, src=None, skip=None, n_keep=None, d_in=None, d_out=None) == PEAQ_ERR_ARG and "ctx is NULL" in err(lib)


def test_run_host_refs_checks_its_arguments_before_any_device(lib, monkeypatch):
    monkeypatch.delenv("PEAQ_AMD_FEED_THREADS", raising=False)
    x = np.zeros(64, np.int16)
    refs = (gstpeaq_amd.HostSignal * 3)()
    tests = (gstpeaq_amd.HostTest * 2)()
    for r in refs[:2]:
        r.data, r.n = x.ctypes.data, 32
    refs[2].data, refs[2].n = None, 77                   # nobody names it: never looked at
    for t, ref in zip(tests, (1, 0)):
        t.data, t.n, t.ref = x.ctypes.data, 32, ref
    out = (C.c_double * 32)()

    def call(level=92., refs=refs, n_refs=3, tests=tests, n_tests=2, results=out, feed=True, **changed):
        f = gstpeaq_amd.make_feed("s16", 2)
        for k, v in changed.items():
            setattr(f, k, v)
        return lib.peaq_batch_run_host_refs(None, 0, level, C.byref(f) if feed else None, n_refs, refs, n_tests, tests, results,
                                            None)

    # what peaq_batch_run_host refuses
    assert call(feed=False) == PEAQ_ERR_ARG and "feed is NULL" in err(lib)
    for bad in (0, 20, 28):
        assert call(struct_size=bad) == PEAQ_ERR_ARG and "struct_size %d" % bad in err(lib) and "24" in err(lib), err(lib)
    for bad in (-1, 6):
        assert call(format=bad) == PEAQ_ERR_ARG and "format %d" % bad in err(lib), err(lib)
    for bad in (0, 3):
        assert call(channels=bad) == PEAQ_ERR_ARG and "channels" in err(lib) and str(bad) in err(lib), err(lib)
    for bad in (0, 7999, 47999, 400000):
        assert call(rate=bad) == PEAQ_ERR_ARG and "rate %d" % bad in err(lib), err(lib)
    assert call(align_max_lag=16385) == PEAQ_ERR_ARG and "align_max_lag 16385" in err(lib), err(lib)
    assert call(chunk_pairs=65536) == PEAQ_ERR_ARG and "chunk_pairs 65536" in err(lib), err(lib)
    assert call(level=131.) == PEAQ_ERR_ARG and "playback level" in err(lib)
    assert call(tests=None) == PEAQ_ERR_ARG and "NULL" in err(lib)
    assert call(results=None) == PEAQ_ERR_ARG and "NULL" in err(lib)
    assert call(refs=None) == PEAQ_ERR_ARG and "NULL refs" in err(lib)
    tests[1].data = None
    assert call() == PEAQ_ERR_ARG and "test 1" in err(lib) and "32 samples" in err(lib) and "NULL buffer" in err(lib), err(lib)
    tests[1].data = x.ctypes.data
    tests[0].n = 1 << 32
    assert call() == PEAQ_ERR_ARG and "test 0" in err(lib) and str(1 << 32) in err(lib), err(lib)
    tests[0].n = 0xFFFFFFFF                              # fits at 44.1 kHz, not after the conversion to 48 kHz
    assert call(rate=44100) == PEAQ_ERR_ARG and "44100" in err(lib), err(lib)
    tests[0].n = 32
    refs[1].n = 1 << 32
    assert call() == PEAQ_ERR_ARG and "reference 1" in err(lib) and str(1 << 32) in err(lib), err(lib)
    refs[1].n = 32
    for bad in ("0", "17", "4x", ""):
        monkeypatch.setenv("PEAQ_AMD_FEED_THREADS", bad)
        assert call() == PEAQ_ERR_ARG and "PEAQ_AMD_FEED_THREADS" in err(lib) and '"%s"' % bad in err(lib), (bad, err(lib))
    monkeypatch.delenv("PEAQ_AMD_FEED_THREADS")
    # its own: an index that names no reference, a named reference with samples but no buffer
    for t, bad in ((0, 3), (1, 4), (1, 0xFFFFFFFF)):
        keep, tests[t].ref = tests[t].ref, bad
        assert call() == PEAQ_ERR_ARG and "test %d" % t in err(lib) and "reference %d of 3" % bad in err(lib), err(lib)
        tests[t].ref = keep
    assert call(n_refs=0) == PEAQ_ERR_ARG and "test 0" in err(lib) and "reference 1 of 0" in err(lib), err(lib)
    tests[0].ref = 2
    assert call() == PEAQ_ERR_ARG and "reference 2" in err(lib) and "77 samples" in err(lib) and "NULL buffer" in err(lib), err(lib)
    tests[0].ref = 1
    # everything in order (the unnamed reference with no buffer among it): the context is looked at last
    assert call() == PEAQ_ERR_ARG and "ctx is NULL" in err(lib), err(lib)
    assert call(rate=44100, align_max_lag=16384, chunk_pairs=65535) == PEAQ_ERR_ARG and "ctx is NULL" in err(lib)
    assert call(n_tests=0, tests=None, results=None) == PEAQ_ERR_ARG and "ctx is NULL" in err(lib)


def test_refs_workspace_counts_a_reference_once(lib):
    ws, ws_refs = gstpeaq_amd.feed_workspace_bytes, gstpeaq_amd.feed_refs_workspace_bytes
    n = 480000
    for feed in (gstpeaq_amd.make_feed("s16", 2), gstpeaq_amd.make_feed("s24", 2, rate=44100, align=4096),
                 gstpeaq_amd.make_feed("f32", 1, chunk_pairs=4)):
        for advanced in (0, 1):
            shared = ws_refs(feed, advanced, 1, 8, n)
            assert 0 < shared < ws(feed, advanced, 8, n), (feed.format, advanced)
            assert shared >= ws(feed, advanced, 1, n), (feed.format, advanced)
            assert ws_refs(feed, advanced, 8, 8, n) > ws_refs(feed, advanced, 2, 8, n) > shared    # more references, more bytes
    feed = gstpeaq_amd.make_feed("s16", 2)
    # one reference of a chunk: its raw bytes four times, decoded once; a test: its raw bytes four times, the two
    # signals of the pair layout, a result and a delay record
    raw, f32 = n * 2 * 2, n * 2 * 4
    per_ref, per_test = 4 * raw + f32, 4 * raw + 2 * f32 + 2 * (128 + 32)
    assert ws_refs(feed, 0, 1, 8, n) == 8 * per_test + per_ref + lib.peaq_batch_workspace_bytes(0, 2, 8, n)
    assert ws_refs(feed, 0, 3, 8, n) == 8 * per_test + 3 * per_ref + lib.peaq_batch_workspace_bytes(0, 2, 8, n)
    # the staging and device buffers stop at the budget, references counted once per chunk
    budget = 4 << 30
    last = 0
    for n_tests in (1, 8, 64, 1000, 4096, 1 << 20):
        v = ws_refs(feed, 0, 16, n_tests, n)
        assert v >= last, (n_tests, v, last)
        last = v
    chunk = (budget - 16 * per_ref) // per_test
    assert ws_refs(feed, 0, 16, 1 << 20, n) == ws_refs(feed, 0, 16, chunk, n)
    assert chunk * per_test + 16 * per_ref <= budget < (chunk + 1) * per_test + 16 * per_ref
    # 0: a feed peaq_batch_run_host would refuse, no tests, no references, a length beyond 2^32 - 1
    bad = gstpeaq_amd.make_feed("s16", 2)
    bad.struct_size = 20
    assert ws_refs(bad, 0, 1, 8, 48000) == 0 == ws(bad, 0, 8, 48000)
    for k, v in (("format", 6), ("channels", 3), ("rate", 47999), ("align_max_lag", 16385), ("chunk_pairs", 65536)):
        bad = gstpeaq_amd.make_feed("s16", 2)
        setattr(bad, k, v)
        assert ws_refs(bad, 0, 1, 8, 48000) == 0, k
    assert ws_refs(feed, 0, 1, 0, 48000) == 0 and ws_refs(feed, 0, 0, 8, 48000) == 0 and ws_refs(feed, 0, 1, 8, 1 << 32) == 0

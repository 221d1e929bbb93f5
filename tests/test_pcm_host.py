"""The PCM decoder's and the host feed's host side without a GPU (include/peaq_amd.h, "PCM from host memory"):
peaq_pcm_sample_bytes, peaq_feed_size, the argument checks of peaq_batch_decode_pcm and peaq_batch_run_host, which
return PEAQ_ERR_ARG with the offending value in the message before any device is touched (a NULL context is the last
thing they look at), peaq_feed_workspace_bytes, and wavio.read_wav_raw against wavio.read_wav."""
import ctypes as C
import struct
from pathlib import Path

import numpy as np
import pytest

import gstpeaq_amd
from gstpeaq_amd import wavio

PEAQ_ERR_ARG = -1
SAMPLE_BYTES = (1, 2, 3, 4, 4, 8)


@pytest.fixture(scope="module")
def lib():
    if not gstpeaq_amd.library_path().exists():
        gstpeaq_amd.build_library()
    return gstpeaq_amd.load_library()


def err(lib):
    return lib.peaq_last_error().decode()


def test_sample_bytes_and_feed_size(lib):
    assert [lib.peaq_pcm_sample_bytes(f) for f in range(6)] == list(SAMPLE_BYTES)
    for unknown in (-1, 6, 100):
        assert lib.peaq_pcm_sample_bytes(unknown) == 0
    assert [gstpeaq_amd.pcm_sample_bytes(k) for k in ("u8", "s16", "s24", "s32", "f32", "f64")] == list(SAMPLE_BYTES)
    assert lib.peaq_feed_size() == C.sizeof(gstpeaq_amd.Feed) == 24


def test_decode_checks_its_arguments_before_any_device(lib):
    buf = (C.c_uint32 * 64)()
    out = (C.c_float * 64)()
    p, q = C.cast(buf, C.c_void_p), C.cast(out, C.c_void_p)

    def call(fmt=1, channels=2, n_pairs=1, d_in=p, in_stride=16, n_in=None, n_uniform=16, d_out=q, out_stride=16):
        return lib.peaq_batch_decode_pcm(None, fmt, channels, n_pairs, d_in, in_stride, n_in, n_uniform, d_out, out_stride,
                                         None)

    for bad in (-1, 6, 77):
        assert call(fmt=bad) == PEAQ_ERR_ARG and "format %d" % bad in err(lib), err(lib)
    for bad in (0, 3):
        assert call(channels=bad) == PEAQ_ERR_ARG and "channels" in err(lib) and str(bad) in err(lib), err(lib)
    assert call(n_pairs=65536) == PEAQ_ERR_ARG and "65536" in err(lib) and "65535" in err(lib), err(lib)
    assert call(n_pairs=-1) == PEAQ_ERR_ARG
    assert call(d_in=None) == PEAQ_ERR_ARG and "NULL buffer" in err(lib)
    assert call(d_out=None) == PEAQ_ERR_ARG and "NULL buffer" in err(lib)
    assert call(d_in=C.c_void_p(p.value + 2)) == PEAQ_ERR_ARG and "4-byte aligned" in err(lib), err(lib)
    assert call(n_uniform=17) == PEAQ_ERR_ARG and "17" in err(lib) and "in_stride 16" in err(lib), err(lib)
    n = (C.c_uint32 * 2)(3, 19)
    assert call(n_pairs=2, n_in=n) == PEAQ_ERR_ARG and "19" in err(lib) and "in_stride 16" in err(lib), err(lib)
    assert call(out_stride=15) == PEAQ_ERR_ARG and "out_stride 15" in err(lib) and "16" in err(lib), err(lib)
    n = (C.c_uint32 * 2)(3, 9)
    assert call(n_pairs=2, n_in=n, out_stride=8) == PEAQ_ERR_ARG and "out_stride 8" in err(lib) and "9" in err(lib)
    # everything in order: the context is looked at last
    assert call() == PEAQ_ERR_ARG and "ctx is NULL" in err(lib)


def test_run_host_checks_its_arguments_before_any_device(lib, monkeypatch):
    monkeypatch.delenv("PEAQ_AMD_FEED_THREADS", raising=False)
    x = np.zeros(64, np.int16)
    rows = (gstpeaq_amd.HostPair * 1)()
    rows[0].ref = rows[0].test = x.ctypes.data
    rows[0].n_ref = rows[0].n_test = 32
    out = (C.c_double * 16)()

    def call(level=92., pairs=rows, n_pairs=1, results=out, feed=True, **changed):
        f = gstpeaq_amd.make_feed("s16", 2)
        for k, v in changed.items():
            setattr(f, k, v)
        return lib.peaq_batch_run_host(None, 0, level, C.byref(f) if feed else None, n_pairs, pairs, results, None)

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
    assert call(pairs=None) == PEAQ_ERR_ARG and "NULL" in err(lib)
    assert call(results=None) == PEAQ_ERR_ARG and "NULL" in err(lib)
    rows[0].test = None
    assert call() == PEAQ_ERR_ARG and "pair 0" in err(lib) and "32 samples" in err(lib) and "NULL buffer" in err(lib), err(lib)
    rows[0].test = x.ctypes.data
    rows[0].n_ref = 1 << 32
    assert call() == PEAQ_ERR_ARG and str(1 << 32) in err(lib), err(lib)
    rows[0].n_ref = 0xFFFFFFFF                           # fits at 44.1 kHz, not after the conversion to 48 kHz
    assert call(rate=44100) == PEAQ_ERR_ARG and "44100" in err(lib), err(lib)
    rows[0].n_ref = 32
    for bad in ("0", "17", "4x", "", " 4", "-1", "100"):
        monkeypatch.setenv("PEAQ_AMD_FEED_THREADS", bad)
        assert call() == PEAQ_ERR_ARG and "PEAQ_AMD_FEED_THREADS" in err(lib) and '"%s"' % bad in err(lib), (bad, err(lib))
    for good in ("1", "8", "16"):
        monkeypatch.setenv("PEAQ_AMD_FEED_THREADS", good)
        assert call() == PEAQ_ERR_ARG and "ctx is NULL" in err(lib), (good, err(lib))
    monkeypatch.delenv("PEAQ_AMD_FEED_THREADS")
    # everything in order (alignment, another rate, a chunk size): the context is looked at last
    assert call(rate=44100, align_max_lag=16384, chunk_pairs=65535) == PEAQ_ERR_ARG and "ctx is NULL" in err(lib)


def test_feed_workspace_follows_the_budget(lib):
    ws = gstpeaq_amd.feed_workspace_bytes
    budget = 4 << 30
    feed = gstpeaq_amd.make_feed("s16", 2)
    assert ws(feed, 0, 0, 480000) == 0
    one = ws(feed, 0, 1, 480000)
    # one pair: four raw signals pinned, four on the device, two decoded ones -- and the batch workspace
    raw, f32 = 480000 * 2 * 2, 480000 * 2 * 4
    assert one >= 8 * raw + 2 * f32 + lib.peaq_batch_workspace_bytes(0, 2, 1, 480000)
    last = 0
    for n_pairs in (1, 2, 64, 1000, 4096, 65535, 1 << 20):
        v = ws(feed, 0, n_pairs, 480000)
        assert v >= last, (n_pairs, v, last)
        last = v
    # the staging and device buffers stop growing at the budget: from there on a call takes chunks
    chunk = budget // (8 * raw + 2 * f32 + 2 * (128 + 32))
    assert ws(feed, 0, 1 << 20, 480000) == ws(feed, 0, chunk, 480000)
    assert ws(feed, 0, chunk, 480000) - lib.peaq_batch_workspace_bytes(0, 2, chunk, 480000) <= budget
    wide = gstpeaq_amd.make_feed("s16", 2, rate=44100, align=4096)
    assert ws(wide, 0, 8, 441000) > ws(gstpeaq_amd.make_feed("s16", 2, rate=44100), 0, 8, 441000) > ws(feed, 0, 8, 441000)
    assert ws(gstpeaq_amd.make_feed("s16", 2, chunk_pairs=3), 1, 100, 48000) == ws(feed, 1, 3, 48000)
    bad = gstpeaq_amd.make_feed("s16", 2)
    bad.struct_size = 20
    assert ws(bad, 0, 8, 48000) == 0


# ---- read_wav_raw -------------------------------------------------------------------------------------------------
def wav_bytes(tag, bits, channels, rate, body, extensible=False, junk=False):
    block = bits // 8 * channels
    if extensible:
        fmt = struct.pack("<HHIIHHHHIH", 0xFFFE, channels, rate, rate * block, block, bits, 22, bits, 3, tag) + bytes(14)
    else:
        fmt = struct.pack("<HHIIHH", tag, channels, rate, rate * block, block, bits)
    chunks = b"fmt " + struct.pack("<I", len(fmt)) + fmt
    if junk:
        chunks += b"LIST" + struct.pack("<I", 5) + b"abcde" + b"\0"        # an odd-sized chunk and its pad byte
    chunks += b"data" + struct.pack("<I", len(body)) + body
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


def numpy_decode(raw, fmt):
    """the six formats as the header defines them: the value in double, divided, one rounding to FP32"""
    raw = np.frombuffer(raw, np.uint8)
    if fmt == 0:
        return ((raw.astype(np.float64) - 128.) / 128.).astype(np.float32)
    if fmt == 1:
        return (raw.view("<i2").astype(np.float64) / 32768.).astype(np.float32)
    if fmt == 2:
        b = raw.reshape(-1, 3).astype(np.int64)
        v = b[:, 0] | b[:, 1] << 8 | b[:, 2] << 16
        return ((v - ((v & 0x800000) << 1)).astype(np.float64) / 8388608.).astype(np.float32)
    if fmt == 3:
        return (raw.view("<i4").astype(np.float64) / 2147483648.).astype(np.float32)
    if fmt == 4:
        return raw.view("<f4").copy()
    with np.errstate(over="ignore"):
        return raw.view("<f8").astype(np.float32)


FILES = [(0, 1, 8), (1, 1, 16), (2, 1, 24), (3, 1, 32), (4, 3, 32), (5, 3, 64)]      # PEAQ_PCM_*, fmt tag, bits


@pytest.mark.parametrize("fmt,tag,bits", FILES, ids=["u8", "s16", "s24", "s32", "f32", "f64"])
@pytest.mark.parametrize("channels", [1, 2])
def test_read_wav_raw_then_numpy_decode_equals_read_wav(tmp_path, fmt, tag, bits, channels):
    rng = np.random.default_rng(100 * fmt + channels)
    n = 1001
    if tag == 3:
        x = rng.standard_normal(n * channels)
        x[:4] = [0., -0., 1e39, -1e39] if bits == 64 else [0., -0., 1., -1.]
        body = x.astype("<f8" if bits == 64 else "<f4").tobytes()
    else:
        body = rng.integers(0, 256, n * channels * (bits // 8), dtype=np.uint8).tobytes()
    for k, kw in enumerate((dict(), dict(extensible=True), dict(junk=True))):
        path = tmp_path / f"x{k}.wav"
        data = body + b"\x01" * k                             # k stray bytes at the end: less than a sample, or one more
        path.write_bytes(wav_bytes(tag, bits, channels, 44100 + k, data, **kw))
        raw, got_fmt, got_ch, rate, got_n = wavio.read_wav_raw(path)
        with np.errstate(over="ignore"):
            exp, exp_rate = wavio.read_wav(path)
        assert (got_fmt, got_ch, rate, got_n) == (fmt, channels, exp_rate, len(exp)) and rate == 44100 + k
        assert len(raw) == got_n * channels * (bits // 8) and bytes(raw) == data[:len(raw)]
        got = numpy_decode(raw, fmt).reshape(-1, channels)
        assert got.view(np.uint32).tobytes() == exp.view(np.uint32).tobytes()


def test_read_wav_raw_refuses_what_read_wav_refuses(tmp_path):
    cases = {"notriff.wav": b"RIFX" + bytes(40), "nodata.wav": wav_bytes(1, 16, 1, 48000, b"")[:36],
             "adpcm.wav": wav_bytes(2, 16, 1, 48000, bytes(64)), "s12.wav": wav_bytes(1, 12, 1, 48000, bytes(64))}
    for name, content in cases.items():
        path = Path(tmp_path / name)
        path.write_bytes(content)
        with pytest.raises(ValueError, match=name):
            wavio.read_wav_raw(path)
        with pytest.raises(ValueError, match=name):
            wavio.read_wav(path)

"""PCM decoder and host-fed batch on the MI355X (peaq_batch_decode_pcm, peaq_batch_run_host; Python decode_pcm /
run_host / run_files; the CLI's --list).

Yardstick for the decoder: numpy -- the value in double, divided, one rounding to FP32 (what wavio.read_wav and the
CLI's reader do).  Yardstick for the feed: the existing entry points on the numpy-decoded floats, batch_run(..., rate=,
align=).  Every comparison is bit for bit (bytes of the FP32 samples, bytes of the 16 doubles of a result, so NaN
payloads and NaN results count); there is no tolerance anywhere in this file."""
import functools
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import gpu_common
import gst_env
import synth_np

pytestmark = pytest.mark.gpu

FORMATS = ("u8", "s16", "s24", "s32", "f32", "f64")
SAMPLE_BYTES = dict(u8=1, s16=2, s24=3, s32=4, f32=4, f64=8)
LENGTHS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4099)
IN_STRIDE, OUT_STRIDE = 4101, 4103                   # odd: with S24 mono the pair bases walk through every byte phase
SENTINEL = 0xDEADBEEF


def ctx():
    return gpu_common.ctx("default")


def numpy_decode(raw, fmt):
    """bytes -> float32, flat"""
    raw = np.ascontiguousarray(np.frombuffer(raw, np.uint8))
    if fmt == "u8":
        return ((raw.astype(np.float64) - 128.) / 128.).astype(np.float32)
    if fmt == "s16":
        return (raw.view("<i2").astype(np.float64) / 32768.).astype(np.float32)
    if fmt == "s24":
        b = raw.reshape(-1, 3).astype(np.int64)
        v = b[:, 0] | b[:, 1] << 8 | b[:, 2] << 16
        return ((v - ((v & 0x800000) << 1)).astype(np.float64) / 8388608.).astype(np.float32)
    if fmt == "s32":
        return (raw.view("<i4").astype(np.float64) / 2147483648.).astype(np.float32)
    if fmt == "f32":
        return raw.view("<f4").copy()
    with np.errstate(over="ignore"):
        return raw.view("<f8").astype(np.float32)


def pack_s24(v):
    """int array -> uint8 [..., 3], little endian"""
    v = np.asarray(v, np.int64) & 0xFFFFFF
    return np.stack([v & 255, v >> 8 & 255, v >> 16 & 255], axis=-1).astype(np.uint8)


def specials(fmt):
    """each format's extremes, 0 and +-1 LSB, and where a rounding can go wrong"""
    if fmt == "u8":
        return np.array([0, 1, 127, 128, 129, 254, 255], np.uint8)
    if fmt == "s16":
        return np.array([-32768, -32767, -1, 0, 1, 32766, 32767], "<i2")
    if fmt == "s24":
        return pack_s24([-(1 << 23), -(1 << 23) + 1, -1, 0, 1, (1 << 23) - 2, (1 << 23) - 1])
    if fmt == "s32":
        t = 1 << 24                                      # above 2^24 FP32 steps by 2: odd values are ties
        vals = [-(1 << 31), -(1 << 31) + 1, -1, 0, 1, (1 << 31) - 2, (1 << 31) - 1, (1 << 31) - 64, (1 << 31) - 65]
        for k in (t - 1, t, t + 1, t + 2, t + 3, t + 4, 2 * t + 1, 2 * t + 2, 2 * t + 3, 2 * t + 6):
            vals += [k, -k]
        return np.array(vals, "<i4")
    if fmt == "f32":                                     # bit patterns: signalling and quiet NaNs with payloads, subnormals
        return np.array([0x7FA00001, 0xFFA12345, 0x7F800001, 0x7FC00000, 0xFFFFFFFF, 0x7F800000, 0xFF800000, 0x00000001,
                         0x807FFFFF, 0x80000000, 0, 0x3F800000, 0x7F7FFFFF], "<u4").view("<f4")
    one = np.float64(1.)
    h = 2. ** -24                                        # half an FP32 step at 1
    fmax = np.float64(np.finfo(np.float32).max)
    vals = [0., -0., 1., -1., one + h, one + 3 * h, np.nextafter(one + h, 2.), np.nextafter(one + h, 0.),
            np.nextafter(one + 3 * h, 2.), np.nextafter(one + 3 * h, 0.), -(one + h), -(one + 3 * h),
            1e39, -1e39, 1e300, fmax, fmax + 2. ** 103, np.nextafter(fmax + 2. ** 103, 0.), -(fmax + 2. ** 103),
            1e-40, -1e-40, 2. ** -149, 2. ** -150, np.nextafter(2. ** -150, 1.), 1.5 * 2. ** -149, 2.5 * 2. ** -149,
            2. ** -126, np.nextafter(2. ** -126, 0.), np.nan, np.inf, -np.inf]
    return np.array(vals, "<f8")


def decoder_batch(fmt, channels):
    """raw bytes [pairs, IN_STRIDE * channels * sb] of seeded random samples with the specials at the start and near the
    end of every pair's valid part"""
    rng = np.random.default_rng(1000 + 10 * FORMATS.index(fmt) + channels)
    sb, count = SAMPLE_BYTES[fmt], len(LENGTHS) * IN_STRIDE * channels
    if fmt == "f64":
        x = (rng.standard_normal(count) * 10. ** rng.integers(-3, 3, count)).astype("<f8")
    elif fmt == "f32":
        x = rng.integers(0, 1 << 32, count, dtype=np.uint64).astype("<u4").view("<f4")
    else:
        x = rng.integers(0, 256, count * sb, dtype=np.uint8)
    raw = np.ascontiguousarray(x).view(np.uint8).reshape(len(LENGTHS), IN_STRIDE * channels * sb).copy()
    sp = np.ascontiguousarray(specials(fmt)).view(np.uint8).reshape(-1)
    for p, n in enumerate(LENGTHS):
        valid = n * channels * sb
        k = min(len(sp), valid) // sb * sb
        raw[p, :k] = sp[:k]
        if valid >= 2 * len(sp):
            raw[p, valid - len(sp):valid] = sp
    return raw


def sentinel_out(n_pairs, stride, channels):
    import torch
    return torch.from_numpy(np.full((n_pairs, stride, channels), SENTINEL, np.uint32).view(np.float32)).cuda()


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("fmt", FORMATS)
def test_decoder_equals_numpy_bit_for_bit(fmt, channels):
    import gstpeaq_amd
    import torch
    sb = SAMPLE_BYTES[fmt]
    raw = decoder_batch(fmt, channels)
    # S24 (U8, S16): the pair bases fall on every byte phase there is -- all four with one channel; a stereo pair is a
    # multiple of 6 (2, 4) bytes long, so only the even ones exist
    phases = {p * IN_STRIDE * channels * sb % 4 for p in range(len(LENGTHS))}
    if fmt == "s24":
        assert phases == ({0, 1, 2, 3} if channels == 1 else {0, 2})
        long_phases = {p * IN_STRIDE * channels * sb % 4 for p, n in enumerate(LENGTHS) if n >= 1023}
        assert long_phases == phases                     # ... each of them with a body of many vectors behind it
    assert IN_STRIDE != OUT_STRIDE
    d_raw = torch.from_numpy(raw).cuda()
    n = np.array(LENGTHS, np.uint32)
    out = sentinel_out(len(LENGTHS), OUT_STRIDE, channels)
    got = gstpeaq_amd.decode_pcm(ctx(), d_raw, fmt, channels, n=n, out=out)
    torch.cuda.synchronize()
    assert got is out
    got = got.cpu().numpy().view(np.uint32).reshape(len(LENGTHS), OUT_STRIDE * channels)
    for p, length in enumerate(LENGTHS):
        exp = numpy_decode(raw[p, :length * channels * sb].tobytes(), fmt).view(np.uint32)
        bad = np.flatnonzero(got[p, :length * channels] != exp)
        assert bad.size == 0, (fmt, channels, p, length, bad[:8], got[p, bad[:8]], exp[bad[:8]])
        assert (got[p, length * channels:] == SENTINEL).all(), (fmt, channels, p, length)      # past the length: untouched
    # n_uniform: every pair has in_stride samples; a destination the decoder makes itself (zeros, an even stride)
    full = gstpeaq_amd.decode_pcm(ctx(), d_raw, fmt, channels)
    torch.cuda.synchronize()
    assert tuple(full.shape) == (len(LENGTHS), IN_STRIDE + 1, channels)
    full = full.cpu().numpy().view(np.uint32)
    exp = numpy_decode(raw.tobytes(), fmt).view(np.uint32).reshape(len(LENGTHS), IN_STRIDE, channels)
    assert (full[:, :IN_STRIDE] == exp).all() and not full[:, IN_STRIDE:].any()


def test_decoder_specials_round_as_the_definition_says():
    """the yardstick itself, on the values the header names: ties to even, +-Inf beyond the range, payloads kept"""
    s32 = numpy_decode(np.array([(1 << 24) + 1, (1 << 24) + 3, -(1 << 24) - 1, (1 << 31) - 1, -(1 << 31)], "<i4").tobytes(), "s32")
    assert s32.tolist() == [2. ** -7, 2. ** -7 + 2. ** -29, -2. ** -7, 1., -1.]
    f64 = numpy_decode(np.array([1. + 2. ** -24, 1. + 3 * 2. ** -24, 1e39, -1e39, 1e-40], "<f8").tobytes(), "f64")
    assert f64[:4].tolist() == [1., 1. + 2. ** -22, np.inf, -np.inf] and 0. < f64[4] < 2. ** -126
    f32 = numpy_decode(np.array([0x7FA00001], "<u4").tobytes(), "f32")
    assert f32.view(np.uint32)[0] == 0x7FA00001


# ---- host-fed batch -----------------------------------------------------------------------------------------------
def quantise(x, fmt):
    """float [n, channels] -> the file's samples: int16 [n, channels] or S24 bytes [n, channels, 3]"""
    if fmt == "s16":
        return np.clip(np.round(x.astype(np.float64) * 32768.), -32768, 32767).astype("<i2")
    return pack_s24(np.clip(np.round(x.astype(np.float64) * 8388608.), -(1 << 23), (1 << 23) - 1))


def decoded(a, fmt, channels=2):
    return numpy_decode(np.ascontiguousarray(a).tobytes(), fmt).reshape(-1, channels)


@functools.lru_cache(maxsize=None)
def float_pairs():
    """seven seeded pairs of unequal lengths of 0.5 .. 1 s, one empty pair and one of 100 samples"""
    lengths = [(24000, 24000), (48000, 47000), (30001, 33333), (40960, 40960), (26623, 26624), (35000, 29000), (44100, 44100)]
    pairs = []
    for seed, (n_ref, n_test) in enumerate(lengths, start=41):
        r, t = synth_np.pair(seed, 2, max(n_ref, n_test))
        pairs.append((r[:n_ref], t[:n_test]))
    e = np.zeros((0, 2), np.float32)
    r, t = synth_np.pair(50, 2, 100)
    return pairs[:3] + [(e, e)] + pairs[3:5] + [(r, t)] + pairs[5:]


@functools.lru_cache(maxsize=None)
def file_pairs(fmt):
    return [(quantise(r, fmt), quantise(t, fmt)) for r, t in float_pairs()]


def shifted(test, d):
    """the test signal late by d samples (zeros in front) or, d < 0, early by -d (its first samples dropped)"""
    if d >= 0:
        return np.concatenate([np.zeros((d, test.shape[1]), np.float32), test])
    return test[-d:]


ALIGN_DELAYS = (0, 513, -1105)


@functools.lru_cache(maxsize=None)
def late_file_pairs(fmt):
    return [(quantise(r, fmt), quantise(shifted(t, d), fmt)) for (r, t), d in zip(float_pairs()[:3], ALIGN_DELAYS)]


def batch(pairs):
    """[(ref, test)] float32 of any lengths -> (ref tensor, test tensor, n_ref, n_test) with one stride"""
    import torch
    ch = pairs[0][0].shape[1]
    stride = max(max(len(r), len(t)) for r, t in pairs)
    stride = max(stride + (stride & 1), 2)
    a = np.zeros((2, len(pairs), stride, ch), np.float32)
    for p, (r, t) in enumerate(pairs):
        a[0, p, :len(r)], a[1, p, :len(t)] = r, t
    d = torch.from_numpy(a).cuda()
    return d[0], d[1], np.array([len(r) for r, _ in pairs], np.uint32), np.array([len(t) for _, t in pairs], np.uint32)


def reference_rows(pairs, fmt, advanced, **kw):
    """batch_run on the numpy-decoded floats: the 16 doubles of every pair"""
    import gstpeaq_amd
    import torch
    res = gstpeaq_amd.batch_run(ctx(), advanced, *batch([(decoded(r, fmt), decoded(t, fmt)) for r, t in pairs]), sync=False, **kw)
    torch.cuda.synchronize()
    return res.cpu().numpy()


@functools.lru_cache(maxsize=None)
def plain_reference(fmt, advanced):
    return reference_rows(file_pairs(fmt), fmt, advanced)


def host_rows(pairs, fmt, advanced, rate=48000, align=None, chunk_pairs=0):
    from gstpeaq_amd import capi
    return capi._run_host_rows(ctx(), advanced, pairs, fmt, 2, rate, align, chunk_pairs, 92.0)


def assert_same_rows(got, exp, what):
    assert got.shape == exp.shape == (len(exp), 16)
    for p in range(len(exp)):
        assert got[p].tobytes() == exp[p].tobytes(), (what, p, got[p], exp[p])


@pytest.mark.parametrize("chunk_pairs", [0, 1, 3])
@pytest.mark.parametrize("advanced", [0, 1], ids=["basic", "advanced"])
@pytest.mark.parametrize("fmt", ["s16", "s24"])
def test_run_host_equals_batch_run_on_the_decoded_floats(fmt, advanced, chunk_pairs):
    assert ctx().fir_mode() == "f64"                     # the default FIR mode
    got, _ = host_rows(file_pairs(fmt), fmt, advanced, chunk_pairs=chunk_pairs)
    assert_same_rows(got, plain_reference(fmt, advanced), (fmt, advanced, chunk_pairs))


@pytest.mark.parametrize("advanced", [0, 1], ids=["basic", "advanced"])
def test_run_host_at_44100_equals_batch_run_with_rate(advanced):
    pairs = file_pairs("s16")
    exp = reference_rows(pairs, "s16", advanced, rate=44100)
    for chunk_pairs in (0, 1, 3):
        got, _ = host_rows(pairs, "s16", advanced, rate=44100, chunk_pairs=chunk_pairs)
        assert_same_rows(got, exp, (advanced, chunk_pairs))


@pytest.mark.parametrize("advanced", [0, 1], ids=["basic", "advanced"])
@pytest.mark.parametrize("fmt", ["s16", "s24"])
def test_run_host_aligned_equals_estimate_then_batch_run_with_align(fmt, advanced):
    import gstpeaq_amd
    pairs = late_file_pairs(fmt)
    floats = [(decoded(r, fmt), decoded(t, fmt)) for r, t in pairs]
    est = gstpeaq_amd.estimate_delay(ctx(), *batch(floats)[:2], 4096, *batch(floats)[2:])
    assert [int(v) for v in est["lag"]] == list(ALIGN_DELAYS)
    exp = reference_rows(pairs, fmt, advanced, align=4096)
    for chunk_pairs in (0, 1, 2):
        got, rec = host_rows(pairs, fmt, advanced, align=4096, chunk_pairs=chunk_pairs)
        assert [rec[p].lag for p in range(len(pairs))] == [int(v) for v in est["lag"]]
        for k in ("peak", "runner_up", "norm"):
            assert np.array([getattr(rec[p], k) for p in range(len(pairs))]).tobytes() == est[k].tobytes(), (k, chunk_pairs)
        assert_same_rows(got, exp, (fmt, advanced, chunk_pairs))
    res, delays = gstpeaq_amd.run_host(ctx(), advanced, pairs, fmt, 2, align=4096)
    assert delays["lag"].tolist() == list(ALIGN_DELAYS) and delays["norm"].tobytes() == est["norm"].tobytes()
    assert np.array([r["odg"] for r in res]).tobytes() == exp[:, 12].tobytes()         # (bytes: a NaN grade too)


def test_a_pairs_result_does_not_depend_on_the_other_pairs_of_the_call():
    pairs = file_pairs("s16")
    for advanced in (0, 1):
        exp = plain_reference("s16", advanced)
        for keep in ([2], [6, 2], [8, 3, 0]):
            got, _ = host_rows([pairs[p] for p in keep], "s16", advanced)
            assert_same_rows(got, exp[keep], (advanced, keep))


@pytest.mark.parametrize("fmt", ["s16", "s24"])
def test_pageable_misaligned_source_buffers(fmt):
    """every source a view one byte (S24) or one sample (S16) into a buffer of its own"""
    views = []
    for pair in file_pairs(fmt):
        row = []
        for a in pair:
            flat = np.ascontiguousarray(a).reshape(-1)
            big = np.empty(flat.size + 1, flat.dtype)
            big[1:] = flat
            v = big[1:]
            assert v.size == 0 or v.ctypes.data == big.ctypes.data + big.itemsize
            row.append(v)
        views.append(tuple(row))
    assert any(r.ctypes.data % 4 for r, _ in views)
    got, _ = host_rows(views, fmt, 0, chunk_pairs=4)
    assert_same_rows(got, plain_reference(fmt, 0), fmt)


# ---- files: run_files and the CLI's --list ------------------------------------------------------------------------
def write_wav(path, samples, fmt, rate):
    """samples: int16 [n, 2], S24 bytes [n, 2, 3] or float32 [n, 2]"""
    tag, bits = dict(s16=(1, 16), s24=(1, 24), f32=(3, 32))[fmt]
    body = np.ascontiguousarray(samples).tobytes()
    block = bits // 8 * 2
    hdr = struct.pack("<HHIIHH", tag, 2, rate, rate * block, block, bits)
    chunks = b"fmt " + struct.pack("<I", len(hdr)) + hdr + b"data" + struct.pack("<I", len(body)) + body
    Path(path).write_bytes(b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks)


FIXTURES = (("s16", 48000), ("s24", 48000), ("f32", 48000), ("s16", 44100))


@pytest.fixture(scope="module")
def fixture_files(tmp_path_factory):
    """four pairs: S16, S24 and F32 at 48 kHz, S16 at 44.1 kHz -> [(ref path, test path, fmt, rate, (ref, test) arrays)]"""
    d = tmp_path_factory.mktemp("pcm")
    out = []
    for k, (fmt, rate) in enumerate(FIXTURES):
        r, t = float_pairs()[k if k < 3 else 4]
        arrays = (r, t) if fmt == "f32" else (quantise(r, fmt), quantise(t, fmt))
        paths = (d / f"ref{k}.wav", d / f"test{k}.wav")
        for path, a in zip(paths, arrays):
            write_wav(path, a, fmt, rate)
        out.append((paths[0], paths[1], fmt, rate, arrays))
    return out


def same_result(a, b):
    return all(np.array([a[k]]).tobytes() == np.array([b[k]]).tobytes() for k in ("di", "odg", "totalsnr")) and \
        a["frames"] == b["frames"] and a["fb_blocks"] == b["fb_blocks"] and a["movs"].tobytes() == b["movs"].tobytes()


def test_run_files_groups_by_format_and_returns_list_order(fixture_files, tmp_path):
    import gstpeaq_amd
    order = [2, 0, 3, 1, 0]                              # mixed formats, one pair twice
    files = [(fixture_files[k][0], fixture_files[k][1]) for k in order]
    got = gstpeaq_amd.run_files(ctx(), 0, files)
    assert len(got) == len(order)
    for i, k in enumerate(order):
        _, _, fmt, rate, arrays = fixture_files[k]
        exp = gstpeaq_amd.run_host(ctx(), 0, [arrays], fmt, 2, rate=rate)[0]
        assert same_result(got[i], exp), (i, k, got[i], exp)
    # S16 48 kHz pairs sit in one group: the same as one run_host over both
    both = gstpeaq_amd.run_host(ctx(), 0, [fixture_files[0][4], fixture_files[0][4]], "s16", 2)
    assert same_result(got[1], both[0]) and same_result(got[4], both[1])
    res, delays = gstpeaq_amd.run_files(ctx(), 0, files[:2], align=1024)
    assert len(res) == 2 and [d["lag"] for d in delays] == [0, 0]
    with pytest.raises(ValueError, match="test1.wav"):    # S16 against S24
        gstpeaq_amd.run_files(ctx(), 0, [(fixture_files[0][0], fixture_files[1][1])])
    with pytest.raises(ValueError, match="test3.wav"):    # 48 kHz against 44.1 kHz
        gstpeaq_amd.run_files(ctx(), 0, [(fixture_files[0][0], fixture_files[3][1])])
    mono = tmp_path / "mono.wav"
    body = np.zeros(100, "<i2").tobytes()
    hdr = struct.pack("<HHIIHH", 1, 1, 48000, 96000, 2, 16)
    chunks = b"fmt " + struct.pack("<I", 16) + hdr + b"data" + struct.pack("<I", len(body)) + body
    mono.write_bytes(b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks)
    with pytest.raises(ValueError, match="mono.wav"):
        gstpeaq_amd.run_files(ctx(), 0, [(fixture_files[0][0], mono)])


def run_cli(*args):
    return subprocess.run([str(gst_env.CLI), *map(str, args)], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def list_output(fixture_files, tmp_path_factory):
    assert gst_env.CLI.exists(), "gstpeaq_amd/cli/peaq is built by build()"
    path = tmp_path_factory.mktemp("list") / "pairs.txt"
    lines = ["# a corpus", ""] + [f"{r}\t{t}" for r, t, *_ in fixture_files]
    path.write_text("\n".join(lines) + "\n")
    out = run_cli(f"--list={path}")
    assert out.returncode == 0, out.stdout + out.stderr
    return path, out.stdout.splitlines()


@pytest.mark.parametrize("k", range(len(FIXTURES)), ids=[f"{f}-{r}" for f, r in FIXTURES])
def test_cli_list_line_carries_what_the_two_file_form_prints(fixture_files, list_output, k):
    ref, test, _, rate, _ = fixture_files[k]
    _, lines = list_output
    assert len(lines) == len(FIXTURES)
    one = run_cli(*(["--device-resample"] if rate != 48000 else []), ref, test)
    assert one.returncode == 0, one.stdout + one.stderr
    printed = one.stdout.strip().splitlines()
    assert printed[-2].startswith("Objective Difference Grade: ") and printed[-1].startswith("Distortion Index: ")
    assert lines[k] == f"{ref}\t{test}\t{printed[-2].split()[-1]}\t{printed[-1].split()[-1]}"


def test_cli_list_refuses_what_it_cannot_score(fixture_files, list_output, tmp_path):
    path, _ = list_output
    missing = tmp_path / "missing.txt"
    missing.write_text(path.read_text() + f"{fixture_files[0][0]}\t{tmp_path / 'nowhere.wav'}\n")
    out = run_cli(f"--list={missing}")
    assert out.returncode == 2 and out.stdout == "" and "nowhere.wav" in out.stderr, out.stdout + out.stderr
    mixed = tmp_path / "mixed.txt"
    mixed.write_text(f"{fixture_files[0][0]}\t{fixture_files[1][1]}\n")          # S16 against S24
    out = run_cli(f"--list={mixed}")
    assert out.returncode == 2 and out.stdout == "", out.stdout + out.stderr
    # positional files or --interval beside --list: a usage error
    assert run_cli(f"--list={path}", fixture_files[0][0], fixture_files[0][1]).returncode == 1
    assert run_cli(f"--list={path}", "--interval=1").returncode == 1

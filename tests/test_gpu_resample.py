"""The device rate converter (peaq_batch_resample, peaq_run_pair_rate; Python resample / rate=) on the MI355X.

Yardstick for samples: the CLI's converter (gstpeaq_amd/cli/peaq.c resample_to_48k, through PEAQ_AMD_CLI_DUMP), which
tests/test_cli_resampler.py pins to the real reference chain.  Both sides round the same FP64 sum to FP32 once (one
FP32 ulp: 2^-23 |y|); the sums differ by summation rounding and by the device contracting multiply and add, bounded by
2K 2^-53 sum|h| max|x| <= 514 x 1.1e-16 x 2.3 max|x| = 1.3e-13 max|x|, rounded up to 1e-12 max|x|.  Every sample is
compared, edges included.  End to end the yardstick is the real chain's recording (ref_e2e_resampled.json) at the
tolerance test_cli_resampler.py states for it, 5e-3."""
import ctypes as C
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import cases as case_defs
import synth_np
import test_cli_resampler as cli

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLD = json.loads((ROOT / "tests" / "golden" / "ref_e2e_resampled.json").read_text())
TOL = 5e-3
_CTX = []


def ctx():
    if not _CTX:
        import gstpeaq_amd
        _CTX.append(gstpeaq_amd.Context(0))
    return _CTX[0]


def ratio(rate):
    g = np.gcd(48000, rate)
    return 48000 // g, rate // g          # L, M


def taps(rate):
    """2K of the filter for `rate`"""
    half = 32.15 if rate < 48000 else 4. * np.ceil(64. * rate / 48000. / 8.)
    return 2 * (int(np.ceil(half)) + 1)


def convert(x, rate, n=None, **kw):
    """x: numpy [pairs, n, ch] -> (numpy [pairs, stride, ch], n_out)"""
    import torch
    import gstpeaq_amd
    y, n_out = gstpeaq_amd.resample(ctx(), torch.from_numpy(np.ascontiguousarray(x)).cuda(), rate, n, **kw)
    torch.cuda.synchronize()
    return y.cpu().numpy(), n_out


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def results_equal(a, b):
    return all(np.array_equal(np.array([a[k]]).view(np.uint64), np.array([b[k]]).view(np.uint64))
               for k in ("di", "odg", "totalsnr")) and a["frames"] == b["frames"] and \
        np.array_equal(a["movs"].view(np.uint64), b["movs"].view(np.uint64))


# ---- 1. samples against the CLI's converter -----------------------------------------------------------------
# 11025 Hz (L = 640) and 44112 Hz (1000 / 919) do not fit the tiled kernel's LDS: they run resample_any_kernel
@pytest.mark.skipif(not cli.CLI.exists(), reason="gstpeaq_amd/cli/peaq not built")
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("rate", [44100, 32000, 96000, 22050, 88200, 16000, 11025, 44112])
def test_samples_equal_the_cli_converters(tmp_path, rate, channels):
    import gstpeaq_amd
    L, M = ratio(rate)
    worst = 0.
    for k, rem in enumerate((0, 1, M - 1)):
        n = 2 * rate + 977                                   # a few seconds; lengths with n mod M = 0, 1, M - 1
        n += (rem - n) % M
        assert n % M == rem % M
        x, _ = synth_np.pair(500 + 10 * k + channels, channels, n)
        y_cli, _ = cli.cli_dump(tmp_path, dict(kind="raw", rate=rate, channels=channels, _x=x))
        y, n_out = convert(x[None], rate)
        assert n_out[0] == len(y_cli) == gstpeaq_amd.resampled_length(n, rate)
        y = y[0, :n_out[0]].astype(np.float64)
        bound = 2. ** -23 * np.abs(y_cli.astype(np.float64)) + 1e-12 * np.abs(x).max()
        err = np.abs(y - y_cli)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (rate, channels, n, int(np.argmax(err - bound)) // channels, float(err.max()))
    print(f"{rate} Hz x{channels}: worst error / bound {worst:.3f}")


# ---- 2. batch mechanics ------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,channels", [(44100, 2), (96000, 1), (11025, 2)])
def test_batch_mechanics(rate, channels):
    import torch
    import gstpeaq_amd
    n_pairs, stride = 64, 30000
    rng = np.random.default_rng(rate + channels)
    n_in = rng.integers(3, stride, n_pairs).astype(np.uint32)
    n_in[:5] = (0, 1, taps(rate) - 1, stride, 2)
    x = np.zeros((n_pairs, stride, channels), dtype=np.float32)
    for p in range(n_pairs):
        x[p] = synth_np.pair(900 + p, channels, stride)[p & 1]
    o_stride = gstpeaq_amd.resampled_length(stride, rate) + 38      # larger than needed (even)
    o_stride += o_stride & 1
    poison = np.float32(-1234.5)

    def run(stream=None):
        out = torch.full((n_pairs, o_stride, channels), float(poison), dtype=torch.float32, device="cuda")
        if stream is None:
            y, n_out = gstpeaq_amd.resample(ctx(), torch.from_numpy(x).cuda(), rate, n_in, out=out)
        else:
            d_x = torch.from_numpy(x).cuda()
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                y, n_out = gstpeaq_amd.resample(ctx(), d_x, rate, n_in, out=out, stream=stream)
        torch.cuda.synchronize()
        return y.cpu().numpy(), n_out

    y, n_out = run()
    for p in range(n_pairs):
        assert n_out[p] == gstpeaq_amd.resampled_length(int(n_in[p]), rate), p
        assert (y[p, n_out[p]:] == poison).all(), p                 # untouched past the converted length
        if n_in[p]:
            single, n1 = convert(x[p:p + 1, :n_in[p]], rate)
            assert n1[0] == n_out[p] and same_bits(single[0, :n1[0]], y[p, :n_out[p]]), p
    y2, n2 = run()
    assert same_bits(y, y2) and np.array_equal(n_out, n2)
    y3, n3 = run(torch.cuda.Stream())
    assert same_bits(y, y3) and np.array_equal(n_out, n3)
    # uniform lengths (no length arrays) are the same conversion
    yu, nu = convert(x, rate)
    p = 3
    assert nu[p] == n_out[p] and same_bits(yu[p, :nu[p]], y[p, :n_out[p]])


def test_calls_in_a_row_and_a_stream_that_is_not_current():
    """Per-pair lengths travel through four staging slots: six calls in a row with different lengths, nothing
    synchronised in between, each equal to the same call made alone.  And a stream handed over WITHOUT being torch's
    current one: the output the binding makes is zero-filled on that stream, so the fill cannot land on samples."""
    import torch
    import gstpeaq_amd
    rate, n_pairs, stride = 44100, 8, 20000
    x = torch.from_numpy(np.stack([synth_np.pair(300 + p, 2, stride)[0] for p in range(n_pairs)])).cuda()
    lens = [np.random.default_rng(k).integers(1, stride, n_pairs).astype(np.uint32) for k in range(6)]
    alone = []
    for n in lens:
        y, n_out = gstpeaq_amd.resample(ctx(), x, rate, n)
        torch.cuda.synchronize()
        alone.append((y.cpu().numpy(), n_out))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    row = [gstpeaq_amd.resample(ctx(), x, rate, n, stream=side) for n in lens]      # side is not the current stream
    torch.cuda.synchronize()
    for (y, n_out), (y1, n1) in zip(row, alone):
        assert np.array_equal(n_out, n1) and same_bits(y.cpu().numpy(), y1)
    ref, test = x[:4].contiguous(), x[4:].contiguous()
    a = gstpeaq_amd.batch_run(ctx(), 0, ref, test, lens[0][:4], lens[0][4:], rate=rate)
    res = gstpeaq_amd.batch_run(ctx(), 0, ref, test, lens[0][:4], lens[0][4:], rate=rate, stream=side, sync=False)
    torch.cuda.synchronize()
    b = [gstpeaq_amd.capi._result_dict(r, 0) for r in res.cpu().numpy()]
    assert all(results_equal(u, v) for u, v in zip(a, b))


# ---- 3. end to end against the real reference chain ----------------------------------------------------------
@pytest.mark.parametrize("rec", GOLD["records"], ids=lambda r: f"{r['case']['name']}-{'adv' if r['case']['advanced'] else 'basic'}")
def test_run_pair_at_its_rate_follows_the_reference_chain(rec):
    import gstpeaq_amd
    case = rec["case"]
    ref, test = case_defs.make_inputs(case)
    e = gstpeaq_amd.run_pair(ctx(), case["advanced"], ref, test, rate=case["rate"])
    print(f"{case['name']} adv={case['advanced']}: dODG {e['odg'] - float(rec['odg']):+.2e} dDI {e['di'] - float(rec['di']):+.2e}")
    assert e["frames"] == rec["frames"]
    assert abs(e["odg"] - float(rec["odg"])) <= TOL and abs(e["di"] - float(rec["di"])) <= TOL, \
        (case["name"], e["odg"], rec["odg"], e["di"], rec["di"])


def test_batch_run_at_a_rate_equals_run_pair_at_that_rate():
    import torch
    import gstpeaq_amd
    assert len(GOLD["records"]) == 8
    groups = {}
    for rec in GOLD["records"]:
        c = rec["case"]
        groups.setdefault((c["rate"], c["advanced"], c["channels"]), []).append(c)
    seen = 0
    for (rate, adv, ch), cs in sorted(groups.items()):
        pairs = [case_defs.make_inputs(c) for c in cs]
        stride = max(max(len(r), len(t)) for r, t in pairs)
        ref = np.zeros((len(pairs), stride, ch), dtype=np.float32)
        test = np.zeros_like(ref)
        for i, (r, t) in enumerate(pairs):
            ref[i, :len(r)], test[i, :len(t)] = r, t
        got = gstpeaq_amd.batch_run(ctx(), adv, torch.from_numpy(ref).cuda(), torch.from_numpy(test).cuda(),
                                    [len(r) for r, _ in pairs], [len(t) for _, t in pairs], rate=rate)
        for (r, t), g in zip(pairs, got):
            assert results_equal(g, gstpeaq_amd.run_pair(ctx(), adv, r, t, rate=rate)), (rate, adv)
            seen += 1
    assert seen == 8


# ---- 4. composition with trajectories ----------------------------------------------------------------------
@pytest.mark.parametrize("advanced", [0, 1])
def test_trajectory_at_44100(advanced):
    import torch
    import gstpeaq_amd
    n_pairs, n, interval = 3, 3 * 44100 + 11, 48000
    x = np.stack([np.stack(synth_np.pair(700 + p, 2, n)) for p in range(n_pairs)])      # [pair][ref/test][n][2]
    ref, test = torch.from_numpy(x[:, 0].copy()).cuda(), torch.from_numpy(x[:, 1].copy()).cuda()
    n_in = [n, n - 5000, n - 1]
    n_points = 4
    pts, res = gstpeaq_amd.batch_trajectory(ctx(), advanced, ref, test, interval, n_points, n_in, n_in, rate=44100)
    plain = gstpeaq_amd.batch_run(ctx(), advanced, ref, test, n_in, n_in, rate=44100)
    r48, n_r = gstpeaq_amd.resample(ctx(), ref, 44100, n_in)
    t48, n_t = gstpeaq_amd.resample(ctx(), test, 44100, n_in)
    pts48, res48 = gstpeaq_amd.batch_trajectory(ctx(), advanced, r48, t48, interval, n_points, n_r, n_t)
    for p in range(n_pairs):
        assert results_equal(res[p], plain[p]) and results_equal(res[p], res48[p]), p
        for k in range(n_points):
            a, b = pts[p][k], pts48[p][k]
            assert a["frames"] == b["frames"] and np.array_equal(a["movs"], b["movs"], equal_nan=True), (p, k)
            assert np.array_equal([a["di"], a["odg"]], [b["di"], b["odg"]], equal_nan=True), (p, k)
    one_pts, one_res = gstpeaq_amd.run_pair_trajectory(ctx(), advanced, x[1, 0, :n_in[1]], x[1, 1, :n_in[1]], interval,
                                                       n_points, rate=44100)
    assert results_equal(one_res, res[1])
    assert all(np.array_equal(a["movs"], b["movs"], equal_nan=True) for a, b in zip(one_pts, pts[1]))


# ---- 5. the default is untouched ---------------------------------------------------------------------------
@pytest.mark.parametrize("advanced", [0, 1])
def test_rate_48000_is_the_plain_call(advanced):
    import gstpeaq_amd
    ref, test = gstpeaq_amd.synth_fill(ctx(), 40, 16, 2, 48000)
    a = gstpeaq_amd.batch_run(ctx(), advanced, ref, test)
    b = gstpeaq_amd.batch_run(ctx(), advanced, ref, test, rate=48000)
    assert all(results_equal(x, y) for x, y in zip(a, b))
    r, t = synth_np.pair(40, 2, 48000)
    assert results_equal(gstpeaq_amd.run_pair(ctx(), advanced, r, t), gstpeaq_amd.run_pair(ctx(), advanced, r, t, rate=48000))


# ---- 6. CLI ------------------------------------------------------------------------------------------------
def run_cli(*args):
    return subprocess.run([str(cli.CLI), *map(str, args)], capture_output=True, text=True, timeout=300)


def printed(out):
    return [float(v) for v in re.findall(r"(?:Grade|Index): (-?[0-9.]+)", out.stdout)]


@pytest.mark.skipif(not cli.CLI.exists(), reason="gstpeaq_amd/cli/peaq not built")
def test_cli_device_resample(tmp_path):
    """ODG / DI lines with and without --device-resample within 1e-6 (they are printed with three decimals: equal
    unless a value sits on a rounding edge).  Measured on an MI355X: identical lines in both versions."""
    ref, test = synth_np.pair(61, 2, 3 * 44100)
    cli.write_wav_f32(tmp_path / "r.wav", ref, 44100)
    cli.write_wav_f32(tmp_path / "t.wav", test, 44100)
    for version in ("--basic", "--advanced"):
        host = run_cli(version, tmp_path / "r.wav", tmp_path / "t.wav")
        dev = run_cli(version, "--device-resample", tmp_path / "r.wav", tmp_path / "t.wav")
        assert host.returncode == 0 and dev.returncode == 0, host.stdout + host.stderr + dev.stdout + dev.stderr
        assert dev.stderr == ""
        a, b = printed(host), printed(dev)
        print(version, a, b)
        assert len(a) == 2 and len(b) == 2 and max(abs(u - v) for u, v in zip(a, b)) <= 1e-6, (a, b)
    # fall-backs: mixed rates, and a rate the device does not take
    cli.write_wav_f32(tmp_path / "t32.wav", test[: 3 * 32000], 32000)
    cli.write_wav_f32(tmp_path / "r01.wav", ref, 44101)
    cli.write_wav_f32(tmp_path / "t01.wav", test, 44101)
    for files in ((tmp_path / "r.wav", tmp_path / "t32.wav"), (tmp_path / "r01.wav", tmp_path / "t01.wav")):
        host = run_cli(*files)
        dev = run_cli("--device-resample", *files)
        assert host.returncode == 0 and dev.returncode == 0, dev.stdout + dev.stderr
        assert "converting on the host" in dev.stderr and len(dev.stderr.strip().splitlines()) == 1
        assert printed(host) == printed(dev) and len(printed(dev)) == 2


# ---- 7. errors ---------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable():
    import torch
    import gstpeaq_amd
    c = ctx()
    L = c.L
    x = torch.zeros((2, 1000, 2), dtype=torch.float32, device="cuda")
    out = torch.zeros((2, 2000, 2), dtype=torch.float32, device="cuda")
    px, po = C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr())

    def call(channels=2, rate=44100, d_in=px, in_stride=1000, n_uniform=1000, d_out=po, out_stride=2000):
        return L.peaq_batch_resample(c.h, channels, rate, 2, d_in, in_stride, None, n_uniform, d_out, out_stride, None, None)

    for kw, word in ((dict(rate=48000), b"48000"), (dict(rate=44101), b"44101"), (dict(channels=3), b"channels"),
                     (dict(out_stride=1087), b"out_stride"), (dict(d_in=None), b"NULL"), (dict(d_out=None), b"NULL"),
                     (dict(n_uniform=1001), b"in_stride")):
        assert call(**kw) == -1, kw
        assert word in L.peaq_last_error(), (kw, L.peaq_last_error())
    assert gstpeaq_amd.resampled_length(1000, 44100) == 1088
    assert call(out_stride=1088) == 0
    with pytest.raises(gstpeaq_amd.PeaqError):
        gstpeaq_amd.resample(c, x, 44101)
    with pytest.raises(gstpeaq_amd.PeaqError):
        gstpeaq_amd.run_pair(c, 0, np.zeros((100, 2), np.float32), np.zeros((100, 2), np.float32), rate=7999)
    r, t = synth_np.pair(5, 2, 44100)
    e = gstpeaq_amd.run_pair(c, 0, r, t, rate=44100)
    assert e["frames"] == gstpeaq_amd.load_library().peaq_frame_count(48000, 48000, 0) and np.isfinite(e["odg"])

"""The FFT-model back end fetches a frame's record in one round trip: the record's seven scalars of both
channels come in ONE gather -- lanes 0 .. 6 channel 0's, lanes 8 .. 14 channel 1's -- and are handed out by lane reads;
the two totalsnr energies run in registers through the frame loop; channel 0's wave touches the next frame's record(s)
while a next frame of the launch exists.  What could go wrong with that, on the shipped instantiations:
  * a wrong lane or offset of the gather: every scalar of the records below differs between the channels and from frame
    to frame, so a scalar taken from the other channel, from a neighbouring slot or from another frame changes the
    result (against the oracle's records back end, tolerances of tests/test_gpu_backend_gates.py);
  * a mono pair reading "channel 1" lanes: the slot behind a mono record is the NEXT frame's record, whose flags and
    energies differ from this frame's;
  * the energies in registers across launches and at a reading point: launch cuts bit for bit, a ragged batch against
    each pair alone bit for bit, a trajectory reading against the session's bit for bit;
  * the touch at the end of a launch: a launch's last frame has nothing to warm and its first is never warmed -- cut into
    launches of 1, 2 and 7 frames the result is the uncut one bit for bit.  (A harmless read beyond the launch's last
    record is invisible to any test: the guard `frame + 1 < f_end` stands where the touch's address is chosen, in
    gstpeaq_amd/csrc/peaq_backend_fft.inc.)
Needs an MI355X (`-m gpu`)."""
import functools

import numpy as np
import pytest

import backend_scenarios as scn
import oracle_lib as orc

pytestmark = pytest.mark.gpu

N = 30                              # crosses frame 24 and the loudness gate's lag of 3 frames
KEYS = ("movs", "di", "odg", "totalsnr", "frames", "fb_blocks")


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (there is no CPU fallback in the product)")
    import gpu_common
    return gpu_common.ctx()


@functools.lru_cache(maxsize=None)
def stereo_records():
    """30 neutral stereo frames in which every scalar of the record differs between the channels and between frames"""
    rec = scn.neutral(N, 2)
    f = np.arange(N)
    # bit 0 of the reference's flag word: frames 0, 3, 6 .. channel 0 alone, 1, 4, 7 .. channel 1 alone, 2, 5, 8 .. both --
    # but none on 10 .. 12 and 27 (the accumulators go tentative and come back, movaccum.c:317-362)
    above = np.stack([f % 3 != 1, f % 3 != 0], axis=1)
    above[10:13] = above[27] = False
    # the energy bits: on frames 1, 5, 9 .. only in channel 1's TEST word (EHS is admitted), on 3, 7, 11 .. nowhere
    # (it is not); on the even frames channel 0's reference and channel 1's test carry it
    e_ref = np.stack([f % 2 == 0, np.zeros(N, dtype=bool)], axis=1)
    e_test = np.stack([np.zeros(N, dtype=bool), (f % 2 == 0) | (f % 4 == 1)], axis=1)
    rec[:, :, scn.R_FL_REF] = above + 2. * e_ref
    rec[:, :, scn.R_FL_TEST] = 2. * e_test
    # bw_ref on either side of 346 per channel: channel 0 rises through it behind frame 9, channel 1 falls through it
    # behind frame 13
    rec[:, 0, scn.R_BW_REF], rec[:, 1, scn.R_BW_REF] = 300. + 5. * f, 400. - 4. * f
    rec[:, 0, scn.R_BW_TEST], rec[:, 1, scn.R_BW_TEST] = 200. + f, 250. + 2. * f
    rec[:, 0, scn.R_EHS], rec[:, 1, scn.R_EHS] = 0.01 * (1. + f), 0.02 * (31. - f)
    rec[:, 0, scn.R_SIG_E], rec[:, 1, scn.R_SIG_E] = 1. + 0.1 * f, 2.5 + 0.07 * f
    rec[:, 0, scn.R_NOISE_E], rec[:, 1, scn.R_NOISE_E] = 0.01 * (1. + f), 0.03 * (40. - f)
    for k in (scn.R_BW_REF, scn.R_BW_TEST, scn.R_EHS, scn.R_SIG_E, scn.R_NOISE_E):
        assert (rec[:, 0, k] != rec[:, 1, k]).all(), k                   # between the channels
        assert (np.diff(rec[:, :, k], axis=0) != 0.).all(), k            # from frame to frame
    for k in (scn.R_FL_REF, scn.R_FL_TEST):                              # (two bits: on most frames)
        assert (rec[:, 0, k] != rec[:, 1, k]).sum() >= N // 2, k
    assert ((rec[:, 0, scn.R_BW_REF] > 346.) != (rec[:, 1, scn.R_BW_REF] > 346.)).any()
    rec.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=None)
def oracle_result(channels):
    return orc.backend_records(stereo_records()[:, :channels])


@functools.lru_cache(maxsize=None)
def plain_uncut(channels):
    import gpu_common
    import gstpeaq_amd.capi as capi
    return capi.debug_backend_plain(gpu_common.ctx(), stereo_records()[:, :channels])


def same_bits(a, b):
    return all(np.asarray(a[k], dtype=np.float64).tobytes() == np.asarray(b[k], dtype=np.float64).tobytes() for k in KEYS)


def compare_with_oracle(got, exp):
    """tests/test_gpu_backend_gates.py's bounds: MOVs rtol 1e-7 / atol 1e-9, DI and ODG 1e-6, the quotients of small
    integer sums (RelDistFrames, both bandwidths) rtol 1e-14, totalsnr 1e-12"""
    g, e = got["movs"][:11], exp["movs"][:11]
    assert got["frames"] == exp["frames"] == N
    assert np.array_equal(np.isnan(g), np.isnan(e)), (g, e)
    ok = ~np.isnan(e)
    print("largest relative error of a MOV", np.max(np.abs(g[ok] - e[ok]) / np.maximum(np.abs(e[ok]), 1e-300)),
          "totalsnr", abs(got["totalsnr"] - exp["totalsnr"]))
    np.testing.assert_allclose(g[ok], e[ok], rtol=1e-7, atol=1e-9)
    for k in ("di", "odg"):
        assert abs(got[k] - exp[k]) < 1e-6, (k, got[k], exp[k])
    for i in (scn.RELDIST, scn.BW_REF, scn.BW_TEST):
        assert ok[i]
        np.testing.assert_allclose(g[i], e[i], rtol=1e-14, atol=0.)
    assert abs(got["totalsnr"] - exp["totalsnr"]) <= 1e-12, (got["totalsnr"], exp["totalsnr"])


def test_the_scenario_decides_what_it_says():
    """(in the oracle) both bandwidths average over frames of either channel's own; EHS is admitted on the frames with an
    energy bit anywhere and on no other; the energies are both channels' sums"""
    rec, o = stereo_records(), oracle_result(2)
    exp = 10. * np.log10(rec[:, :, scn.R_SIG_E].sum() / rec[:, :, scn.R_NOISE_E].sum())
    assert scn.close(o["totalsnr"], exp, 1e-13), (o["totalsnr"], exp)
    assert not np.isnan(o["movs"][:11]).any()
    mono = oracle_result(1)
    assert all(abs(o["movs"][i] - mono["movs"][i]) > 1e-3 * abs(o["movs"][i]) for i in (scn.BW_REF, scn.BW_TEST, scn.EHS))
    assert abs(o["totalsnr"] - mono["totalsnr"]) > 1e-3


@pytest.mark.parametrize("channels", [2, 1], ids=["stereo", "mono"])
def test_every_scalar_of_the_record_reaches_its_place(ctx, channels):
    import gstpeaq_amd.capi as capi
    rec = stereo_records()[:, :channels]
    plain = plain_uncut(channels)
    compare_with_oracle(plain, oracle_result(channels))
    _, res = capi.debug_backend(ctx, rec)             # the debug instantiation, one launch
    assert same_bits(plain, res), (plain, res)


@pytest.mark.parametrize("channels", [2, 1], ids=["stereo", "mono"])
@pytest.mark.parametrize("frames_per_launch", [1, 2, 7])
def test_launch_cuts_change_no_bit(ctx, channels, frames_per_launch):
    import gstpeaq_amd.capi as capi
    cut = capi.debug_backend_plain(ctx, stereo_records()[:, :channels], frames_per_launch)
    assert same_bits(cut, plain_uncut(channels)), (frames_per_launch, cut, plain_uncut(channels))


def signals(frames, seed):
    """a synthetic stereo pair whose flushed run has `frames` frames"""
    import gstpeaq_amd.capi as capi
    import synth_np
    n = 1024 * frames if frames > 1 else 1024
    assert capi.frame_count(n, n) == frames, (n, frames)
    return synth_np.pair(seed, 2, n)


def test_ragged_batch_equals_each_pair_alone(ctx):
    """pairs of 1, 2, 25 and 30 frames in one batch: the last frame of each pair is the last of ITS launch"""
    import torch
    import gstpeaq_amd
    pairs = [signals(k, 40 + i) for i, k in enumerate((1, 2, 25, 30))]
    stride = max(len(r) for r, _ in pairs)
    ref = np.zeros((len(pairs), stride, 2), dtype=np.float32)
    test = np.zeros_like(ref)
    for i, (r, t) in enumerate(pairs):
        ref[i, :len(r)], test[i, :len(t)] = r, t
    n = np.array([len(r) for r, _ in pairs], dtype=np.uint32)
    got = gstpeaq_amd.batch_run(ctx, 0, torch.from_numpy(ref).cuda(), torch.from_numpy(test).cuda(), n, n)
    for i, (r, t) in enumerate(pairs):
        alone = gstpeaq_amd.run_pair(ctx, 0, r, t)
        assert got[i]["frames"] == alone["frames"] == (1, 2, 25, 30)[i]
        assert same_bits(got[i], alone), (i, got[i], alone)


def test_a_reading_point_takes_the_energies_from_the_registers(ctx):
    """one reading after frame 26 of a 30-frame stereo pair (points instantiation): the session's reading after the
    same samples bit for bit (the plain instantiation, whose sums went through memory between its launches), and
    totalsnr from the front-end records' energies summed as the kernel sums them"""
    import torch
    import gstpeaq_amd
    import gstpeaq_amd.capi as capi
    r, t = signals(30, 47)
    upto = 2048 + 26 * 1024                           # frame 26 is complete
    d_ref, d_test = torch.from_numpy(r).cuda(), torch.from_numpy(t).cuda()
    points, _ = gstpeaq_amd.batch_trajectory(ctx, 0, d_ref[None], d_test[None], upto, 1)
    got = points[0][0]
    assert got["frames"] == 27
    s = gstpeaq_amd.Session(ctx, 0, 2)
    s.push_ref(r[:upto])
    s.push_test(t[:upto])
    exp = s.results()
    s.close()
    assert exp["frames"] == 27 and same_bits(got, exp), (got, exp)
    rec = capi.debug_frontend(ctx, 109, d_ref, d_test, 27)
    e_sig = e_noise = 0.
    for f in range(27):
        e_sig += rec[f, 0, scn.R_SIG_E] + rec[f, 1, scn.R_SIG_E]
        e_noise += rec[f, 0, scn.R_NOISE_E] + rec[f, 1, scn.R_NOISE_E]
    assert abs(got["totalsnr"] - 10. * np.log10(e_sig / e_noise)) <= 1e-12, (got["totalsnr"], e_sig, e_noise)

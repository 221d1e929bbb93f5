"""-m gpu: the meter through the `peaq` element (gst/gstpeaq_amd.c): `meter-window` / `meter-hop` turn it
on, every delivered reading is an element message `peaq-meter` on the bus -- from the chain function while the stream
runs, and for the last ones before the EOS message --, under PEAQ_AMD_BROKER the geometry is the process's
(PEAQ_AMD_BROKER_METER), and the text the element prints at the end of the stream is what it prints without the meter.

The streams are audiotestsrc's saw and triangle (128 buffers of 1024 samples, as the reference's own runtest pipelines),
which tests/synth_np.py restates: the installed GStreamer has no WAV parser to read a file pair with."""
import re
import subprocess

import numpy as np
import pytest

import gpu_common as gpu
import gst_env
import synth_np

pytestmark = pytest.mark.gpu

N = 128 * 1024
PIPELINE = ["audiotestsrc", "name=src0", "num-buffers=128", "wave=saw", "freq=440",
            "audiotestsrc", "name=src1", "num-buffers=128", "wave=triangle", "freq=440"]


@pytest.fixture(scope="module", autouse=True)
def _need_gst():
    if not gst_env.have_gst():
        pytest.fail("GStreamer tools / built plugin missing on the GPU box")


def launch(props, **environ):
    cmd = ["gst-launch-1.0", "-m", f"--gst-plugin-load={gst_env.PLUGIN}", *PIPELINE, "peaq", "name=peaq", *props,
           "src0.src!peaq.ref", "src1.src!peaq.test"]
    out = subprocess.run(cmd, capture_output=True, text=True, env=dict(gst_env.env(), **environ), timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


def messages(stdout):
    """the peaq-meter messages in the order they were posted, and the position of the EOS message among the lines"""
    rows, eos_at, last_at = [], None, None
    for i, line in enumerate(stdout.splitlines()):
        if "peaq-meter" in line:
            f = {k: v for k, v in re.findall(r"(\w+)=\(\w+\)([^,;<]+)", line)}
            rows.append(dict(index=int(f["index"]), start=int(f["start"]), duration=int(f["duration"]), odg=float(f["odg"]),
                             di=float(f["di"]), totalsnr=float(f["totalsnr"])))
            assert "movs=" in line
            last_at = i
        elif eos_at is None and re.search(r"\(eos\)|end-of-stream|EOS", line) and "message" in line.lower():
            eos_at = i
    return rows, eos_at, last_at


def end_text(stdout):
    """what the element itself prints at the end of the stream: the MOV table and the grade"""
    return [l for l in stdout.splitlines() if re.match(r"\s*[\w ]+B: |Objective Difference Grade:", l)]


@pytest.fixture(scope="module")
def expected():
    """the readings of a Python session fed the same two streams in the element's buffers"""
    import gstpeaq_amd
    ref, test = synth_np.audiotestsrc("saw", N), synth_np.audiotestsrc("triangle", N)
    window, hop = gstpeaq_amd.meter_frames(0.5), gstpeaq_amd.meter_frames(0.25)
    s = gstpeaq_amd.Session(gpu.ctx(), False, 1)
    s.set_meter(window, hop, 64)
    for pos in range(0, N, 1024):
        s.push(0, ref[pos:pos + 1024])
        s.push(1, test[pos:pos + 1024])
    s.flush()
    rows, dropped = s.meter_read()
    s.close()
    assert dropped == 0 and len(rows) == len(gstpeaq_amd.meter_windows(N, N, window, hop)) > 5
    return rows


def check(rows, expected):
    assert [r["index"] for r in rows] == list(range(len(expected)))       # in index order, meter_windows' count
    for r, e in zip(rows, expected):
        assert r["start"] == e["first_frame"] * 1024 * 10**9 // 48000
        assert r["duration"] == (e["n_frames"] + 1) * 1024 * 10**9 // 48000
        for k in ("odg", "di", "totalsnr"):
            # (the first window lies in the gated start of the stream: NaN, as the reference's empty accumulators read)
            assert (np.isnan(r[k]) and np.isnan(e[k])) or abs(r[k] - e[k]) <= 1e-9, (r["index"], k, r[k], e[k])


def test_the_element_posts_every_reading_and_its_end_text_is_unchanged(expected):
    plain = launch([])
    out = launch(["meter-window=0.5", "meter-hop=0.25"])
    rows, eos_at, last_at = messages(out)
    check(rows, expected)
    assert eos_at is None or last_at < eos_at                # the last readings come before the EOS message
    assert not messages(plain)[0]
    assert end_text(out) == end_text(plain) and len(end_text(plain)) == 12
    assert end_text(plain)[-1] == "Objective Difference Grade: -2.007"


def test_under_the_broker_the_geometry_is_the_processes(expected):
    out = launch([], PEAQ_AMD_BROKER="4", PEAQ_AMD_BROKER_METER="0.5:0.25")
    rows, eos_at, last_at = messages(out)
    check(rows, expected)
    assert eos_at is None or last_at < eos_at
    assert end_text(out)[-1] == "Objective Difference Grade: -2.007"
    assert not messages(launch([], PEAQ_AMD_BROKER="4"))[0]  # no meter asked for: no message

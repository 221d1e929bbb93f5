"""-m gpu: live alignment through the `peaq` element (gst/gstpeaq_amd.c): `align-max-lag` makes the
element hold its stream, find the delay between its pads and score the aligned pair -- an element message `peaq-delay`
once, the `delay` property, and the grade of the aligned pair, not -3.5 --; `delay-watch` posts an element message
`peaq-delay-watch` per watch window, with consecutive indices; under PEAQ_AMD_BROKER the configuration is the process's
(PEAQ_AMD_BROKER_ALIGN).

The streams are the mono case of tests/test_gpu_live_align.py that fails without the feature, the test signal 37 samples
late, read from raw F32 files in buffers of 1024 samples (filesrc ! queue ! rawaudioparse)."""
import re
import subprocess

import pytest

import gpu_common as gpu
import gst_env
from test_gpu_live_align import MAX_LAG, PROBE, delayed, inputs

pytestmark = pytest.mark.gpu

L = 37


@pytest.fixture(scope="module", autouse=True)
def _need_gst():
    if not gst_env.have_gst():
        pytest.fail("GStreamer tools / built plugin missing on the GPU box")


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("live_align")
    ref, test = delayed(*inputs("late_mono"), L)
    ref.tofile(tmp / "ref.f32")
    test.tofile(tmp / "test.f32")
    return tmp / "ref.f32", tmp / "test.f32", ref, test


def launch(pair, props, **environ):
    def src(path):
        # (the queue keeps filesrc in push mode: buffers of 1024 samples, not the parser's pulls of 16384)
        return ["filesrc", f"location={path}", "blocksize=4096", "!", "queue", "!", "rawaudioparse", "format=pcm", "pcm-format=f32le",
                "sample-rate=48000", "num-channels=1", "!"]
    cmd = ["gst-launch-1.0", "-m", "-v", f"--gst-plugin-load={gst_env.PLUGIN}", "peaq", "name=peaq", "advanced=true", *props,
           *src(pair[0]), "peaq.ref", *src(pair[1]), "peaq.test"]
    out = subprocess.run(cmd, capture_output=True, text=True, env=dict(gst_env.env(), **environ), timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


def messages(stdout, name):
    """the element messages `name` in the order they were posted, fields as text"""
    return [{k: v.strip() for k, v in re.findall(r"([\w-]+)=\(\w+\)([^,;<]+)", line)}
            for line in stdout.splitlines() if re.search(name + r"\b(?!-)", line) and "message" in line.lower()]


def grade(stdout):
    (line,) = [l for l in stdout.splitlines() if l.startswith("Objective Difference Grade:")]
    return line


@pytest.fixture(scope="module")
def aligned(pair):
    """the session with the same alignment, fed the same buffers"""
    import gstpeaq_amd
    _, _, ref, test = pair
    s = gstpeaq_amd.Session(gpu.ctx(), True, 1)
    s.set_align(MAX_LAG, probe=PROBE)
    for pos in range(0, len(test), 1024):
        s.push(0, ref[pos:pos + 1024])
        s.push(1, test[pos:pos + 1024])
    s.flush()
    res, rec = s.results(), s.align_read()
    s.close()
    assert rec["lag"] == L
    return res, rec


def check_delay(out, aligned):
    res, rec = aligned
    (m,) = messages(out, "peaq-delay")
    assert int(m["lag"]) == L and (int(m["skip-ref"]), int(m["skip-test"])) == (0, L)
    for k, f in (("peak", "peak"), ("runner_up", "runner-up"), ("norm", "norm")):
        assert abs(float(m[f]) - rec[k]) <= 1e-9 * rec["norm"], (k, m[f], rec[k])
    assert re.search(r"GstPeaq:peaq: delay = 37\b", out) and re.search(r"GstPeaq:peaq: delay-acquired = true", out)
    assert grade(out) == "Objective Difference Grade: %.3f" % res["odg"] and res["odg"] > 0.0


def test_the_element_finds_the_delay_and_grades_the_aligned_pair(pair, aligned):
    plain = launch(pair, [])
    assert not messages(plain, "peaq-delay") and float(grade(plain).split(":")[1]) < -3.0
    out = launch(pair, [f"align-max-lag={MAX_LAG}", f"align-probe={PROBE}"])
    check_delay(out, aligned)
    assert not messages(out, "peaq-delay-watch")


def test_the_element_posts_a_message_per_watch_window(pair):
    import gstpeaq_amd
    frames = gstpeaq_amd.meter_frames(0.1)
    out = launch(pair, [f"align-max-lag={MAX_LAG}", f"align-probe={PROBE}", "delay-watch=0.1"])
    rows = messages(out, "peaq-delay-watch")
    whole = (31700 - 2048) // 1024 + 1
    assert [int(r["index"]) for r in rows] == list(range(whole // frames)) and len(rows) >= 5
    for r in rows:
        assert (int(r["first-frame"]), int(r["frames"])) == (int(r["index"]) * frames, frames)
        assert int(r["offset"]) == 0 and float(r["peak"]) > 0.5 * float(r["norm"]) > 0.0
    assert len(messages(out, "peaq-delay")) == 1


def test_under_the_broker_the_alignment_is_the_processes(pair, aligned):
    out = launch(pair, [], PEAQ_AMD_BROKER="4", PEAQ_AMD_BROKER_ALIGN=f"{MAX_LAG}:{PROBE}:0.1")
    check_delay(out, aligned)
    rows = messages(out, "peaq-delay-watch")
    assert rows and [int(r["index"]) for r in rows] == sorted({int(r["index"]) for r in rows})
    assert int(rows[-1]["index"]) == 4 and all(int(r["offset"]) == 0 for r in rows)
    assert not messages(launch(pair, [], PEAQ_AMD_BROKER="4"), "peaq-delay")   # no alignment asked for: no message

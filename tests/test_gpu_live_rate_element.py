"""-m gpu: live rate conversion through the `peaq` element (gst/gstpeaq_amd.c): the sink pads take the
rates the device converter takes, so a 44.1 kHz pair needs no `audioresample` in front of the element and reads the
rated session's grade; under PEAQ_AMD_BROKER the rates are the process's (PEAQ_AMD_BROKER_RATES), a pad whose caps
say another rate is refused with a message that names both, and a branch that starts later than the other loses nothing.

The streams are the case of tests/test_gpu_live_rate.py that shows the point (BOX, stereo, basic version), read from raw
F32 files in buffers of 1024 samples (filesrc ! queue ! rawaudioparse sample-rate=44100)."""
import subprocess

import pytest

import gpu_common as gpu
import gst_env
from test_gpu_live_rate import inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gst():
    if not gst_env.have_gst():
        pytest.fail("GStreamer tools / built plugin missing on the GPU box")


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("live_rate")
    ref, test = inputs("box")
    ref.tofile(tmp / "ref.f32")
    test.tofile(tmp / "test.f32")
    return tmp / "ref.f32", tmp / "test.f32", ref, test


def launch(pair, rates=(44100, 44100), check=True, **environ):
    def src(path, rate):
        # (the queue keeps filesrc in push mode: buffers of 1024 samples, not the parser's pulls of 16384)
        return ["filesrc", f"location={path}", "blocksize=8192", "!", "queue", "!", "rawaudioparse", "format=pcm",
                "pcm-format=f32le", f"sample-rate={rate}", "num-channels=2", "!"]
    cmd = ["gst-launch-1.0", "-m", f"--gst-plugin-load={gst_env.PLUGIN}", "peaq", "name=peaq",
           *src(pair[0], rates[0]), "peaq.ref", *src(pair[1], rates[1]), "peaq.test"]
    out = subprocess.run(cmd, capture_output=True, text=True, env=dict(gst_env.env(), **environ), timeout=300)
    if check:
        assert out.returncode == 0, out.stderr[-2000:]
    return out


def grade(stdout):
    (line,) = [l for l in stdout.splitlines() if l.startswith("Objective Difference Grade:")]
    return line


@pytest.fixture(scope="module")
def rated(pair):
    """the rated session fed the same buffers"""
    import gstpeaq_amd
    _, _, ref, test = pair
    s = gstpeaq_amd.Session(gpu.ctx(), False, 2, rates=(44100, 44100))
    for pos in range(0, len(ref), 1024):
        s.push(0, ref[pos:pos + 1024])
        s.push(1, test[pos:pos + 1024])
    s.flush()
    res = s.results()
    s.close()
    assert -1.3 < res["odg"] < -0.8                                      # (the converted pair's grade, not -1.92)
    return res


def test_a_44100_pair_without_audioresample_reads_the_rated_sessions_grade(pair, rated):
    assert grade(launch(pair).stdout) == "Objective Difference Grade: %.3f" % rated["odg"]


def test_under_the_broker_the_rates_are_the_processes(pair, rated):
    out = launch(pair, PEAQ_AMD_BROKER="4", PEAQ_AMD_BROKER_RATES="44100")
    assert grade(out.stdout) == "Objective Difference Grade: %.3f" % rated["odg"]


def test_caps_that_differ_from_the_brokers_rates_are_refused(pair):
    out = launch(pair, check=False, PEAQ_AMD_BROKER="4")                 # the broker takes 48000 Hz
    text = out.stdout + out.stderr
    assert out.returncode != 0 and "44100 Hz" in text and "48000 Hz" in text, text[-2000:]
    out = launch(pair, check=False, PEAQ_AMD_BROKER="4", PEAQ_AMD_BROKER_RATES="44100:32000")
    text = out.stdout + out.stderr
    assert out.returncode != 0 and "test pad's caps say 44100 Hz" in text and "32000 Hz" in text, text[-2000:]


def test_a_branch_that_starts_later_loses_nothing(pair, rated):
    """The test branch reads its samples from the launcher's standard input, which stays empty until the reference
    branch has pushed buffers into the element: the test pad's caps then arrive in mid-stream of the other pad, and the
    grade is still the rated session's -- what the reference pad pushed before was kept, not scored against a session
    that assumed 48 kHz on the other pad."""
    import threading
    ref_path, _, _, test = pair
    parse = ["rawaudioparse", "format=pcm", "pcm-format=f32le", "sample-rate=44100", "num-channels=2", "!"]
    cmd = ["gst-launch-1.0", "-v", f"--gst-plugin-load={gst_env.PLUGIN}", "peaq", "name=peaq",
           "filesrc", f"location={ref_path}", "blocksize=8192", "!", "queue", "!", *parse,
           "identity", "name=early", "silent=false", "!", "peaq.ref",
           "fdsrc", "fd=0", "blocksize=8192", "!", "queue", "!", *parse, "peaq.test"]
    p = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=gst_env.env())
    lines, pushed = [], threading.Event()

    def drain():
        chains = 0
        for raw in p.stdout:
            line = raw.decode(errors="replace")
            lines.append(line)
            chains += "early" in line and "chain" in line
            if chains >= 3:
                pushed.set()
        pushed.set()

    t = threading.Thread(target=drain)
    t.start()
    assert pushed.wait(timeout=120)                                     # the reference pad has taken buffers
    assert not any("peaq.GstPad:test: caps" in l for l in lines)        # ... and the test pad has no caps yet
    p.stdin.write(test.tobytes())
    p.stdin.close()
    assert p.wait(timeout=120) == 0, p.stderr.read()[-2000:]
    t.join()
    assert grade("".join(lines)) == "Objective Difference Grade: %.3f" % rated["odg"]

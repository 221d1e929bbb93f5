"""The CLI's --align-steps.  Without a GPU: the option is refused, before anything is initialised, with --list,
--interval, --trace, --align-track, --align-drift and --align-subsample, in the wording of the other alignment options'
refusals; a window out of range is refused with its value; the help text names it.  On the GPU: one run on a pair with
a 300-sample step prints the step's position and size, and the grades peaq_run_pair_steps gives."""
import subprocess

import numpy as np
import pytest

import gst_env


def cli(*args):
    if not gst_env.CLI.exists():
        pytest.skip("the CLI is not built")
    return subprocess.run([str(gst_env.CLI), *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args, words", [
    (("--align-steps", "--list=none.txt"), "--align-steps is not taken with --list"),
    (("--align-steps", "--interval=1", "a.wav", "b.wav"), "--align-steps belongs to the plain one-call mode (not with --interval or --trace)"),
    (("--align-steps=8192", "--trace=t.csv", "a.wav", "b.wav"), "--align-steps belongs to the plain one-call mode"),
    (("--align-steps", "--align-track", "a.wav", "b.wav"), "--align-steps and --align-track exclude each other"),
    (("--align-drift=8192", "--align-steps", "a.wav", "b.wav"), "--align-steps and --align-drift exclude each other"),
    (("--align-subsample", "--align-steps=5001", "a.wav", "b.wav"), "--align-steps and --align-subsample exclude each other"),
    (("--align-steps=4095", "a.wav", "b.wav"), "invalid steps window 4095 (4096 .. 1048576 samples)"),
    (("--align-steps=1048577", "a.wav", "b.wav"), "invalid steps window 1048577"),
    (("--align-steps=", "a.wav", "b.wav"), "invalid steps window"),
])
def test_align_steps_is_refused(args, words):
    run = cli(*args)
    assert run.returncode == 1 and run.stderr.startswith("Failed to initialize: ") and words in run.stderr, run.stderr


def test_help_names_the_option():
    run = cli("--help")
    assert run.returncode == 0 and "--align-steps[=WINDOW]" in run.stdout + run.stderr


@pytest.mark.gpu
def test_the_cli_prints_the_step(tmp_path):
    import gpu_common
    import gstpeaq_amd
    from test_gpu_steps import W, stepped_pair
    from test_gpu_subsample import write_wav
    ref, test, c0 = stepped_pair()
    one = gstpeaq_amd.run_pair(gpu_common.ctx("default"), 0, ref, test, align=4096, steps=W)
    write_wav(tmp_path / "r.wav", ref)                  # (32-bit float files hand the CLI the samples as they are)
    write_wav(tmp_path / "t.wav", test)
    run = cli("--align-steps=%d" % W, str(tmp_path / "r.wav"), str(tmp_path / "t.wav"))
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().splitlines()
    tr, st = one["track"], one["steps"][0]
    assert lines[0] == "Delay: %d samples, track %+.4f .. %+.4f (%d of %d windows), 1 of 1 steps accepted" % (
        one["delay"]["lag"], tr["d_min"], tr["d_max"], tr["n_valid"], tr["n_windows"]), run.stdout
    assert lines[1] == "Step: at %d by %+d samples (gains %.3f and %.3f)" % (
        st["c"], 300, st["gain_left"] / st["norm"], st["gain_right"] / st["norm"]), run.stdout
    assert abs(int(st["c"]) - c0) <= 3 and np.int64(st["LB"]) - np.int64(st["LA"]) == 300
    assert lines[2] == "Objective Difference Grade: %.3f" % one["odg"], run.stdout
    assert lines[3] == "Distortion Index: %.3f" % one["di"], run.stdout

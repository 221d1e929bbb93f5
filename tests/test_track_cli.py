"""The CLI's --align-track without a GPU: the option is refused, before anything is initialised, with --list,
--interval, --trace, --align-drift and --align-subsample, in the wording of the other alignment options' refusals; a
window out of range is refused with its value; the help text names it."""
import subprocess

import pytest

import gst_env


def cli(*args):
    if not gst_env.CLI.exists():
        pytest.skip("the CLI is not built")
    return subprocess.run([str(gst_env.CLI), *args], capture_output=True, text=True)


@pytest.mark.parametrize("args, words", [
    (("--align-track", "--list=none.txt"), "--align-track is not taken with --list"),
    (("--align-track", "--interval=1", "a.wav", "b.wav"), "--align-track belongs to the plain one-call mode (not with --interval or --trace)"),
    (("--align-track=8192", "--trace=t.csv", "a.wav", "b.wav"), "--align-track belongs to the plain one-call mode"),
    (("--align-track", "--align-drift", "a.wav", "b.wav"), "--align-track and --align-drift exclude each other"),
    (("--align-subsample", "--align-track=5001", "a.wav", "b.wav"), "--align-track and --align-subsample exclude each other"),
    (("--align-track=4095", "a.wav", "b.wav"), "invalid track window 4095 (4096 .. 1048576 samples)"),
    (("--align-track=1048577", "a.wav", "b.wav"), "invalid track window 1048577"),
    (("--align-track=", "a.wav", "b.wav"), "invalid track window"),
])
def test_align_track_is_refused(args, words):
    run = cli(*args)
    assert run.returncode == 1 and run.stderr.startswith("Failed to initialize: ") and words in run.stderr, run.stderr


def test_help_names_the_option():
    run = cli("--help")
    assert run.returncode == 0 and "--align-track[=WINDOW]" in run.stdout + run.stderr

"""The schedule of the front end's two-stream upward spreading (gstpeaq_amd/csrc/peaq_spread_sched.h) without a GPU:
tools/spread_sched_check.cpp runs the kernel's loop on a 64-element array -- lane moves as array shifts, the half-wave
swap as a copy, the activation step as a condition -- against the O(B^2) double loop of Kabal (27), for 109 and 55
bands, with energies in [1e-3, 1e12] and slopes a in [0.3, 0.999].  Compiling the program also evaluates the header's
static_asserts: every (source lane, distance) pair with a target is covered exactly once.

The bound: all terms are positive, so the error of a band is at most that of its worst term: a start term from ~ 12
multiplications, at most 38 walking multiplications, one multiply-add and a sum of at most 108 terms -- below 200
roundings of 1.1e-16 on either side, 5e-14 in all.  Held to 1e-12."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
STEPS = {109: 39, 55: 14}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path_factory.mktemp("spread") / "spread_sched_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-o", str(exe), str(ROOT / "tools" / "spread_sched_check.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(cmd + san, capture_output=True).returncode:      # (a compiler without the sanitizers' runtimes)
        subprocess.run(cmd, check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    print(out)
    rows = {}
    for line in out.splitlines():
        f = line.split()
        rows[(int(f[0]), f[1])] = dict(steps=int(f[3]), err=float(f[5]), zeros=int(f[7]))
    return rows


@pytest.mark.parametrize("bands", [109, 55])
@pytest.mark.parametrize("case", ["random", "silent", "top_only", "slopes"])
def test_schedule_matches_the_double_loop(lines, bands, case):
    row = lines[(bands, case)]
    assert row["steps"] == STEPS[bands], row
    assert row["err"] <= 1e-12, row
    assert row["zeros"] == 1, row              # bands no source reaches are exact zeros

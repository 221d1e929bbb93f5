"""The schedule of the front end's band sums (gstpeaq_amd/csrc/peaq_group_sched.h) without a GPU:
tools/group_sched_check.cpp, linked against peaq_tables.cpp, sums every band of the real 109- and 55-band tables by
read slots -- a fixed number of pairs per band, zero words beyond the band's end, the odd bin last -- against the plain
loop of fftearmodel.c:604-620.  The sums must be the plain loop's BIT FOR BIT (adding +0 is exact and the order of the
additions is the loop's), the floor of 1e-12 included: on powers over 24 decades, on powers of one size, on an all-zero
spectrum and with a single non-zero bin walked over every position from lo[0] to hi[NB - 1] -- a bin that is lost, read
twice or given the wrong edge weight changes a sum.  The program also reports the largest number of whole pairs in
each half of the tables beside the slot count, and what the run-time check says about a table made one pair too long.

It is built with the address and undefined-behaviour sanitizers where the compiler has their runtimes (the spectrum is
allocated with exactly the kernel's length and exactly the zero words the schedule asks for, so a read beyond either
is reported), and without them otherwise."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SLOTS = {109: dict(narrow=1, wide=12), 55: dict(narrow=3, wide=25)}      # the issue's counts; the header's must be these
CASES = ["random", "level", "zeros", "walk"]


def host_compiler():
    """peaq_tables.cpp uses _Float16: clang, the one the project's own tools are built with first"""
    for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("amdclang++")):
        if c and Path(c).exists():
            return c
    return None


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    cxx = host_compiler()
    assert cxx, "a host clang++ is needed"
    exe = tmp_path_factory.mktemp("group") / "group_sched_check"
    csrc = ROOT / "gstpeaq_amd" / "csrc"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", f"-I{csrc}", f"-I{ROOT / 'include'}", "-o", str(exe),
           str(ROOT / "tools" / "group_sched_check.cpp"), str(csrc / "peaq_tables.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(cmd + san, capture_output=True).returncode:      # (a compiler without the sanitizers' runtimes)
        subprocess.run(cmd, check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    print(out)
    table = {}
    for line in out.splitlines():
        f = line.split()
        table[(int(f[0]), f[1])] = {f[i]: int(f[i + 1]) for i in range(2, len(f) - 1) if f[i + 1].lstrip("-").isdigit()}
    return table


@pytest.mark.parametrize("bands", [109, 55])
@pytest.mark.parametrize("case", CASES)
def test_slot_schedule_is_the_plain_loop_bit_for_bit(rows, bands, case):
    row = rows[(bands, case)]
    assert row["sums"] >= bands + 1, row           # every band, the middle one with both slot counts
    assert row["mismatches"] == 0, row


@pytest.mark.parametrize("bands", [109, 55])
def test_slot_counts_are_those_of_the_tables(rows, bands):
    """The slots are neither too few (a band would lose bins) nor more than the widest band of the half needs (every
    slot costs each lane a compare, a select, an LDS read and two additions)."""
    row = rows[(bands, "slots")]
    assert row["narrow_slots"] == SLOTS[bands]["narrow"] and row["wide_slots"] == SLOTS[bands]["wide"], row
    assert row["narrow_max"] == row["narrow_slots"] and row["wide_max"] == row["wide_slots"], row
    assert row["misfit"] == -1, row
    bad = rows[(bands, "misfit_detected")]
    assert bad["narrow"] == 0 and bad["wide"] == bands - 1, bad   # one pair too many in either half is told, with its band

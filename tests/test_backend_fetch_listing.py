"""What the FFT-model back end's frame loop asks of memory, read from the compiler's listing (hipcc cross-compiles for
gfx950 without a GPU).  DESIGN.md 3.2: a frame's record is fetched in ONE round trip -- the three band vectors and one
gather of the record's scalars, requested back to back at the top of the frame and waited for once -- and behind them
channel 0's wave touches the next frame's record(s), one dword per 128-byte line, so that they are in L2 when their
frame comes.  The form that ships is the TOUCH (at most five loads in the loop), not a register prefetch of the next
frame's band vectors (which would make it seven).  The frames of a pair run in order, so every further trip to memory
inside the loop is latency on the pair's critical path, during which the wave keeps a slot of its SIMD from the front
end that runs beside it."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "gstpeaq_amd" / "csrc"

PLAIN_109 = "_ZN4peaq14backend_kernelILi109ELb0ELb0EEEvNS_11BackendArgsE"
PLAIN_55 = "_ZN4peaq14backend_kernelILi55ELb1ELb0EEEvNS_11BackendArgsE"


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("be") / "peaq_backend.s"
    subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", f"-I{CSRC}", f"-I{ROOT / 'include'}", "-S",
                    "--cuda-device-only", "-o", str(out), str(CSRC / "peaq_backend.hip")], check=True, capture_output=True)
    return out.read_text().splitlines()


def frame_loop(listing, kernel):
    """The instructions of the kernel's frame loop in listing order: the blocks the compiler marks as the header of, or
    as lying in, one loop of depth 1 (loops nested in it included).  The kernel's other loops copy tables and are a few
    instructions long; the frame loop is the largest by far."""
    start = next(i for i, line in enumerate(listing) if line.startswith(kernel + ":"))
    end = next(i for i in range(start, len(listing)) if listing[i].startswith(".Lfunc_end"))
    loops, current = {}, None
    for line in listing[start + 1:end]:
        label = re.match(r"\s*(?:\.L(BB\d+_\d+):|; %bb\.\d+:)(.*)", line)
        if label:
            name, comment = label.groups()
            current = None
            if "Loop Header: Depth=1" in comment:
                current = name
            else:
                m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=1\b", comment) or \
                    re.search(r"Parent Loop (BB\d+_\d+) Depth=1\b", comment)
                if m:
                    current = m.group(1)
            continue
        code = line.split(";")[0].strip()
        if current and code and not code.startswith("."):
            loops.setdefault(current, []).append(code)
    assert loops, "no loop found in " + kernel
    body = max(loops.values(), key=len)
    assert len(body) > 200, len(body)      # (about 1100 instructions a frame with 109 bands, about 270 with 55)
    return body


def loads_of(code):
    return [(i, c) for i, c in enumerate(code) if c.startswith("global_load") or c.startswith("buffer_load") or
            c.startswith("flat_load") or c.startswith("scratch_load")]


@pytest.mark.parametrize("kernel", [PLAIN_109, PLAIN_55], ids=["109 bands", "55 bands"])
def test_a_frame_fetches_its_record_in_one_round_trip(listing, kernel):
    body = frame_loop(listing, kernel)
    barriers = [i for i, c in enumerate(body) if c.startswith("s_barrier")]
    # the basic version's frame has two barriers; the 55-band path's has none, and its whole frame stands "in front"
    assert (len(barriers) == 0) == (kernel == PLAIN_55), barriers
    first_barrier = barriers[0] if barriers else len(body)
    loads = loads_of(body)
    front = [(i, c) for i, c in loads if i < first_barrier]
    print(kernel, "loads of the frame loop:", loads, "first barrier at", first_barrier, "of", len(body))
    # (a) nothing is fetched behind the frame's first barrier (six loads stood there before the gather)
    assert [c for i, c in loads if i > first_barrier] == []
    # (b) three band vectors (two on the 55-band path, which never reads the test signal's), the gather, the touch
    assert len(front) <= 5, front
    vectors = [(i, c) for i, c in front if c.startswith("global_load_dwordx4")]
    gather = [(i, c) for i, c in front if c.startswith("global_load_dwordx2")]
    touch = [(i, c) for i, c in front if c.startswith("global_load_dword ")]
    assert len(vectors) == (2 if kernel == PLAIN_55 else 3) and len(gather) == 1 and len(touch) == 1, front
    # (c) the frame's own loads are requested back to back: no wait for memory between the first and the last of them
    own = sorted(i for i, c in vectors + gather)
    waits = [i for i, c in enumerate(body) if c.startswith("s_waitcnt") and "vmcnt" in c]
    assert [i for i in waits if own[0] < i < own[-1]] == [], (own, waits)
    # ... and the touch is issued behind them (the wait for the frame's own loads counts in issue order), with no wait
    # between: the frame's first wait leaves exactly the touch outstanding, or nothing where the wave has no touch
    assert touch[0][0] > own[-1], (touch, own)
    assert [i for i in waits if own[0] < i < touch[0][0]] == [], (own, touch, waits)
    # the plain kernels keep nothing in scratch (tests/test_kernel_budgets.py holds the register budget)
    assert not any(c.startswith("scratch_") for c in body)

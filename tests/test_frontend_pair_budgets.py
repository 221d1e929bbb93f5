"""What the one-wave front end (frontend_pair_kernel<109>, reference and test of a frame in one wave) must hold to run
two waves per SIMD and eight workgroups per CU, read from the compiler's own metadata and listing (hipcc cross-compiles
for gfx950 without a GPU):
  * registers: at most 256 per lane, nothing spilled, no scratch;
  * LDS: at most 20 KiB per workgroup, as the launch asks for it (the kernel's LDS is dynamic: the size is the
    constant the launch multiplies out, read from the source and held there by a static_assert as well);
  * one wave of it and one of the basic back end fit a SIMD's 512 registers together;
  * no workgroup barrier: a one-wave workgroup has nobody to wait for;
  * the two-wave kernels are still there under their own names, one each (the tests on them look them up by these)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "gstpeaq_amd" / "csrc"
PAIR = "frontend_pair_kernelILi109E"
FIELDS = "vgpr_count|vgpr_spill_count|sgpr_spill_count|agpr_count|private_segment_fixed_size|group_segment_fixed_size"


def listing(source, tmp):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("no hipcc")
    out = tmp / (source + ".s")
    subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", f"-I{CSRC}", f"-I{ROOT / 'include'}", "-S",
                    "--cuda-device-only", "-o", str(out), str(CSRC / source)], check=True, capture_output=True)
    return out.read_text()


def metadata(text):
    """kernel name -> its numbers; an entry of amdhsa.kernels starts at a "  - " line, keys in alphabetical order (the
    accumulation registers come before the name)"""
    meta = {}
    for entry in re.split(r"(?m)^  - (?=\.)", text[text.index("amdhsa.kernels:"):])[1:]:
        name = re.search(r"(?m)^\s*\.name:\s+(\S+)", entry)
        if name:
            meta[name.group(1)] = {k: int(v) for k, v in re.findall(rf"(?m)^\s*\.({FIELDS}):\s+(\d+)", entry)}
    return meta


def find(meta, fragment):
    (k, v), = [(k, v) for k, v in meta.items() if fragment in k]
    return k, v


@pytest.fixture(scope="module")
def fe(tmp_path_factory):
    text = listing("peaq_frontend.hip", tmp_path_factory.mktemp("fe"))
    return text, metadata(text)


def test_registers_two_waves_per_simd_nothing_spilled(fe):
    _, v = find(fe[1], PAIR)
    assert v["vgpr_count"] + v.get("agpr_count", 0) <= 256, v
    assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, v


def test_lds_eight_workgroups_per_cu():
    src = (CSRC / "peaq_frontend.hip").read_text()
    consts = dict(kPwLen=776, kLogTabEntries=129)
    for name, expr in re.findall(r"constexpr int (kPairOff\w+|kPairLdsDoubles|kLogTabDoubles) = ([^;]+);", src):
        consts[name] = eval(expr, {}, consts)        # plain sums of the constants before them
    assert f"constexpr int kPwLen = {consts['kPwLen']};" in src
    assert f"constexpr int kLogTabEntries = {consts['kLogTabEntries']};" in (CSRC / "peaq_device.h").read_text()
    assert "dim3(64), kPairLdsDoubles * sizeof(double), stream" in src      # what the launch asks for
    assert "static_assert(kPairLdsDoubles * sizeof(double) <= 20480" in src
    assert consts["kPairLdsDoubles"] * 8 <= 20480 and 8 * consts["kPairLdsDoubles"] * 8 <= 160 * 1024, consts


def test_fits_a_simd_beside_the_basic_back_end(fe, tmp_path):
    _, v = find(fe[1], PAIR)
    _, be = find(metadata(listing("peaq_backend.hip", tmp_path)), "backend_kernelILi109ELb0ELb0E")
    assert v["vgpr_count"] + v.get("agpr_count", 0) + be["vgpr_count"] + be.get("agpr_count", 0) <= 512, (v, be)


def test_no_workgroup_barrier(fe):
    text, meta = fe
    name, _ = find(meta, PAIR)
    start = text.index(f"\n{name}:")
    body = text[start:text.index(".Lfunc_end", start)]
    assert body.count("\n") > 3000, "the kernel's listing"
    assert "s_barrier" not in body


def test_two_wave_kernels_keep_their_names(fe):
    for fragment in ("frontend_kernelILi109E", "frontend_kernelILi55E"):
        find(fe[1], fragment)                        # exactly one match each

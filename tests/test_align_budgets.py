"""Budgets of the aligner's kernels, the ceilings DESIGN.md 11 states, read from the compiler's kernel metadata (hipcc
cross-compiles for gfx950 without a GPU):
  * every kernel of peaq_align.hip: nothing in scratch, no spilled VGPRs or SGPRs, LDS within a CU's 160 KB (all of it
    static: the host adds no dynamic LDS);
  * align_spectra_kernel and align_inverse_kernel (one 1024-point transform per wave): at most 128 VGPRs, FOUR waves
    per SIMD, and 34 KB of LDS per workgroup of four waves, so that four workgroups share a CU;
  * align_accumulate_kernel (16 products and a ring of 16 spectra per thread): at most 168 VGPRs, THREE waves per SIMD;
  * align_pick_kernel and align_cut_kernel: at most 64 VGPRs, eight waves per SIMD."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "gstpeaq_amd" / "csrc"
KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size", "max_flat_workgroup_size")
LDS_PER_CU = 160 * 1024
DYNAMIC_LDS = 0                  # what peaq_align.hip's launches ask for beside the static figure


def kernel_metadata(source, tmp_path):
    """{kernel name: {key: value}} from the amdhsa.kernels list of the device assembly; an entry runs from one list
    item ("  - .key:") to the next, whatever the order of the keys inside it"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("no hipcc")
    out = tmp_path / (source + ".s")
    subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", f"-I{CSRC}", f"-I{ROOT / 'include'}", "-S",
                    "--cuda-device-only", "-o", str(out), str(CSRC / source)], check=True, capture_output=True)
    text = out.read_text()
    text = text[text.index("amdhsa.kernels:"):]
    meta = {}
    for item in re.split(r"\n  - (?=\.)", text)[1:]:
        item = item.split("\namdhsa.", 1)[0]
        name = re.search(r"^\s*\.name:\s+(\S+)", item, flags=re.M)
        if not name:
            continue
        vals = {k: int(v) for k, v in re.findall(r"^\s*\.(\w+):\s+(\d+)\s*$", item, flags=re.M) if k in KEYS}
        meta[name.group(1)] = vals
    return meta


def find(meta, fragment):
    (k, v), = [(k, v) for k, v in meta.items() if fragment in k]
    return v


# VGPR ceiling per kernel = 512 / waves per SIMD, rounded down to the allocation granule of 8
CEILINGS = {"align_spectra_kernel": 128, "align_inverse_kernel": 128, "align_accumulate_kernel": 168,
            "align_pick_kernel": 64, "align_cut_kernel": 64}


def test_aligner_kernels_have_no_scratch_and_fit_their_registers_and_lds(tmp_path):
    meta = kernel_metadata("peaq_align.hip", tmp_path)
    assert len(meta) == len(CEILINGS), sorted(meta)
    for name, ceiling in CEILINGS.items():
        v = find(meta, name)
        assert v["private_segment_fixed_size"] == 0, (name, v)
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["group_segment_fixed_size"] + DYNAMIC_LDS <= LDS_PER_CU, (name, v)
        assert v["vgpr_count"] + v.get("agpr_count", 0) <= ceiling, (name, v)
        assert v["max_flat_workgroup_size"] == 256, (name, v)
    # one transform per wave: four waves' exchange buffers, four workgroups (16 waves) per CU
    for name in ("align_spectra_kernel", "align_inverse_kernel"):
        assert 4 * find(meta, name)["group_segment_fixed_size"] <= LDS_PER_CU, name
    assert find(meta, "align_accumulate_kernel")["group_segment_fixed_size"] == 0

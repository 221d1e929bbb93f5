"""Budgets of the PCM decoder's kernels, the ceilings DESIGN.md 12 states, read from the compiler's kernel metadata
(hipcc cross-compiles for gfx950 without a GPU).  Every kernel of peaq_pcm.hip -- one pcm_decode_kernel per sample
format -- : nothing in scratch, no spilled VGPRs or SGPRs, at most 64 VGPRs (eight waves per SIMD), no LDS (static; the
host adds no dynamic LDS), workgroups of 256."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "gstpeaq_amd" / "csrc"
KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size", "max_flat_workgroup_size")
FORMATS = 6                      # PEAQ_PCM_U8 .. PEAQ_PCM_F64: pcm_decode_kernel<0> .. <5>
VGPR_CEILING = 64


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


def test_decoder_kernels_have_no_scratch_no_lds_and_at_most_64_vgprs(tmp_path):
    meta = kernel_metadata("peaq_pcm.hip", tmp_path)
    assert len(meta) == FORMATS, sorted(meta)
    for fmt in range(FORMATS):
        (name, v), = [(k, v) for k, v in meta.items() if f"pcm_decode_kernelILi{fmt}E" in k]
        assert v["private_segment_fixed_size"] == 0, (name, v)
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["vgpr_count"] + v.get("agpr_count", 0) <= VGPR_CEILING, (name, v)
        assert v["group_segment_fixed_size"] == 0, (name, v)
        assert v["max_flat_workgroup_size"] == 256, (name, v)

"""Budgets of the rate converter's kernels, the ceilings DESIGN.md 10 states, read from the compiler's kernel metadata
(hipcc cross-compiles for gfx950 without a GPU) and from the host's own plan of each rate (peaq_resample_plan_info):
  * resample_tile_kernel: nothing in scratch, no spilled SGPRs, at most 64 VGPRs -- eight waves per SIMD as far as
    registers go, so that LDS alone decides how many workgroups a CU holds (32 today);
  * its two LDS tiles are dynamic, sized per rate on the host: at 44.1 kHz at most 80 KB, i.e. TWO workgroups
    (16 waves) per CU -- one float more per row past that would halve the occupancy without any other sign --, and at
    every other rate the tiled kernel takes at most the CU's 160 KB;
  * which of the common rates the tiled kernel takes: all but 11.025 kHz (L = 640)."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "gstpeaq_amd" / "csrc"
KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size", "max_flat_workgroup_size")


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


def test_rate_converter_kernels_have_no_scratch_and_fit_their_registers(tmp_path):
    meta = kernel_metadata("peaq_resample.hip", tmp_path)
    assert len(meta) == 2, sorted(meta)
    tile, any_ = find(meta, "resample_tile_kernel"), find(meta, "resample_any_kernel")
    for v in (tile, any_):
        assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, v
        assert v["sgpr_spill_count"] == 0, v
        assert v["group_segment_fixed_size"] == 0, v          # no static LDS: the tiles are dynamic (next test)
        assert v["vgpr_count"] + v.get("agpr_count", 0) <= 64, v
    assert tile["max_flat_workgroup_size"] == 512, tile        # what the LDS figures below are per


TILED = (8000, 16000, 22050, 24000, 32000, 44100, 88200, 96000, 176400, 192000)


def test_lds_tiles_of_every_tiled_rate():
    import gstpeaq_amd
    if not gstpeaq_amd.library_path().exists():
        gstpeaq_amd.build_library()
    for rate in TILED:
        pl = gstpeaq_amd.resample_plan(rate)
        assert pl["tiled"] == 1, (rate, pl)
        assert 0 < pl["lds_bytes"] <= 160 * 1024, (rate, pl)
        assert pl["period_out"] % 4 == 0 and pl["period_out"] >= 32 and pl["period_out"] % pl["L"] == 0, (rate, pl)
        assert pl["period_in"] * pl["L"] == pl["period_out"] * pl["M"], (rate, pl)
    assert gstpeaq_amd.resample_plan(44100)["lds_bytes"] <= 80 * 1024       # two workgroups per CU
    pl = gstpeaq_amd.resample_plan(44100)
    assert (pl["L"], pl["M"], pl["taps"], pl["zero_taps"]) == (160, 147, 68, 4), pl
    assert gstpeaq_amd.resample_plan(96000)["taps"] == 130
    for rate in (11025, 44112, 384000):                                        # resample_any_kernel's
        pl = gstpeaq_amd.resample_plan(rate)
        assert pl["tiled"] == 0 and pl["lds_bytes"] == 0, (rate, pl)
    # the factor in the bound of tests/test_gpu_resample.py: 2K 2^-53 sum|h| <= 1e-12 for every rate above
    for rate in TILED + (11025, 44112, 384000):
        pl = gstpeaq_amd.resample_plan(rate)
        assert (pl["taps"] + pl["zero_taps"]) * 2. ** -53 * pl["max_sum_abs_taps"] <= 1e-12, (rate, pl)

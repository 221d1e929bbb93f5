"""Budgets of the track stage's one kernel, the ceilings DESIGN.md 18 states, read from the compiler's kernel metadata
(hipcc cross-compiles for gfx950 without a GPU), the way tests/test_drift_budgets.py reads the drift stage's.
track_cut_kernel of peaq_track.hip: nothing in scratch, no spilled VGPRs or SGPRs, at most 128 VGPRs (four waves per
SIMD), workgroups of 256, no dynamic LDS (read from the source), and 8864 bytes of static LDS per workgroup -- 1024 + 64
+ 20 staged samples of two channels -- of which eighteen fit a CU's 160 KiB, so LDS never keeps the workgroups per CU
below the four the registers allow (the ceiling asked for is at least two)."""
import re
from pathlib import Path

from test_pcm_budgets import kernel_metadata

ROOT = Path(__file__).resolve().parent.parent
VGPR_CEILING = 128
LDS_PER_CU = 160 * 1024
LDS = {"track_cut_kernel": 2 * (1024 + 64 + 20) * 4}


def test_track_kernel_holds_its_budgets(tmp_path):
    meta = kernel_metadata("peaq_track.hip", tmp_path)
    assert len(meta) == len(LDS), sorted(meta)
    for kernel, lds in LDS.items():
        (name,) = [k for k in meta if kernel in k]
        v = meta[name]
        assert v["private_segment_fixed_size"] == 0, (name, v)
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["max_flat_workgroup_size"] == 256, (name, v)
        assert v["vgpr_count"] + v.get("agpr_count", 0) <= VGPR_CEILING, (name, v)
        assert v["group_segment_fixed_size"] == lds, (name, v)
        assert LDS_PER_CU // v["group_segment_fixed_size"] >= 2, (name, v)


def test_launch_passes_no_dynamic_lds():
    text = (ROOT / "gstpeaq_amd" / "csrc" / "peaq_track.hip").read_text()
    launches = re.findall(r"hipLaunchKernelGGL\((\w+), dim3\([^;]*?\), dim3\((\d+)\), (\w+), stream", text)
    assert launches == [("track_cut_kernel", "256", "0")], launches

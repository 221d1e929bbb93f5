"""Budgets of the steps stage's three kernels, the ceilings DESIGN.md 19 states, read from the compiler's kernel metadata
(hipcc cross-compiles for gfx950 without a GPU), the way tests/test_track_budgets.py reads the track stage's.
Every kernel of peaq_steps.hip: nothing in scratch, no spilled VGPRs or SGPRs, at most 128 VGPRs (four waves per SIMD),
workgroups of 256, no dynamic LDS (read from the source), and the static LDS below: pieces_cut_kernel stages 1024 + 64 +
20 samples of two channels, track_cut_kernel's 8864 bytes; steps_chunk_kernel holds two arrays of 256 doubles, one of
256 words and its small sums; steps_pick_kernel a candidate's 1025 running sums and its tree (and 8 bytes of
alignment).  The ceilings are what the
build shows, rounded up to the next multiple of 8 registers."""
import re
from pathlib import Path

from test_pcm_budgets import kernel_metadata

ROOT = Path(__file__).resolve().parent.parent
LDS_PER_CU = 160 * 1024
# kernel: (VGPR ceiling, SGPR ceiling, static LDS in bytes)
BUDGETS = {"steps_chunk_kernel": (128, 88, 256 * 8 + 4 * 8 + 4 * 3 * 8 + 256 * 8 + 256 * 4),
           "steps_pick_kernel": (24, 40, 1025 * 8 + 3 * 8 + 256 * 8 + 256 * 4 + 8),
           "pieces_cut_kernel": (120, 80, 2 * (1024 + 64 + 20) * 4)}


def test_steps_kernels_hold_their_budgets(tmp_path):
    meta = kernel_metadata("peaq_steps.hip", tmp_path)
    assert len(meta) == len(BUDGETS), sorted(meta)
    for kernel, (vgprs, sgprs, lds) in BUDGETS.items():
        (name,) = [k for k in meta if kernel in k]
        v = meta[name]
        assert v["private_segment_fixed_size"] == 0, (name, v)
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["max_flat_workgroup_size"] == 256, (name, v)
        assert v["vgpr_count"] + v.get("agpr_count", 0) <= vgprs <= 128, (name, v)
        assert v["sgpr_count"] <= sgprs, (name, v)
        assert v["group_segment_fixed_size"] == lds, (name, v)
        assert LDS_PER_CU // v["group_segment_fixed_size"] >= 8, (name, v)


def test_launches_pass_no_dynamic_lds():
    text = (ROOT / "gstpeaq_amd" / "csrc" / "peaq_steps.hip").read_text()
    launches = re.findall(r"hipLaunchKernelGGL\((\w+), dim3\([^;]*?\), dim3\((\d+)\), (\w+), stream", text)
    assert launches == [("steps_chunk_kernel", "256", "0"), ("steps_pick_kernel", "256", "0"), ("pieces_cut_kernel", "256", "0")], launches

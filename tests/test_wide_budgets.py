"""Budgets of the wide delay search's kernels, the design conditions DESIGN.md 27 states, read from the compiler's kernel
metadata (hipcc cross-compiles for gfx950 without a GPU), the way tests/test_align_budgets.py reads the aligner's.
Every kernel of peaq_wide.hip -- the decimator in both modes and the envelope's centring kernel: nothing in scratch, no
spilled VGPRs or SGPRs, at most 128 VGPRs (four waves per SIMD), workgroups of 256, no dynamic LDS (read from the
source), static LDS of at most 40 KB per workgroup (four workgroups per CU).  These are the align stage's ceilings and
the stage's design conditions, not measurements."""
import re
from pathlib import Path

from test_pcm_budgets import kernel_metadata

ROOT = Path(__file__).resolve().parent.parent
LDS_PER_CU = 160 * 1024
LDS_CEILING = 40 * 1024
KERNELS = ("wide_decimate_kernelILi0E", "wide_decimate_kernelILi1E", "wide_center_kernel")


def test_wide_kernels_hold_their_budgets(tmp_path):
    meta = kernel_metadata("peaq_wide.hip", tmp_path)
    assert len(meta) == len(KERNELS), sorted(meta)
    for kernel in KERNELS:
        (name,) = [k for k in meta if kernel in k]
        v = meta[name]
        assert v["private_segment_fixed_size"] == 0, (name, v)
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["max_flat_workgroup_size"] == 256, (name, v)
        assert v["vgpr_count"] + v.get("agpr_count", 0) <= 128, (name, v)
        assert v["group_segment_fixed_size"] <= LDS_CEILING, (name, v)
        assert LDS_PER_CU // max(v["group_segment_fixed_size"], 1) >= 4, (name, v)


def test_the_tile_is_the_largest_factor_s_and_the_launches_pass_no_dynamic_lds(tmp_path):
    meta = kernel_metadata("peaq_wide.hip", tmp_path)
    for mode in (0, 1):                                 # 64 rows of 62 + 17 doubles
        (name,) = [k for k in meta if f"wide_decimate_kernelILi{mode}E" in k]
        assert meta[name]["group_segment_fixed_size"] == 64 * (62 + 17) * 8, (name, meta[name])
    text = (ROOT / "gstpeaq_amd" / "csrc" / "peaq_wide.hip").read_text()
    launches = re.findall(r"hipLaunchKernelGGL\(([\w<>]+), dim3\([^;]*?\), dim3\((\d+)\), (\w+), stream", text)
    assert launches == [("wide_decimate_kernel<PEAQ_WIDE_ENVELOPE>", "256", "0"), ("wide_center_kernel", "256", "0"),
                        ("wide_decimate_kernel<PEAQ_WIDE_WAVEFORM>", "256", "0")], launches

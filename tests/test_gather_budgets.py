"""Budgets of the gather kernel, the ceilings DESIGN.md 14 states, read from the compiler's kernel metadata (hipcc
cross-compiles for gfx950 without a GPU), the way tests/test_pcm_budgets.py reads the decoder's.  Every kernel of
peaq_gather.hip: nothing in scratch, no spilled VGPRs or SGPRs, at most 64 VGPRs (eight waves per SIMD), no LDS (static;
the host adds no dynamic LDS), workgroups of 256."""
from test_pcm_budgets import VGPR_CEILING, kernel_metadata


def test_gather_kernels_have_no_scratch_no_lds_and_at_most_64_vgprs(tmp_path):
    meta = kernel_metadata("peaq_gather.hip", tmp_path)
    assert len(meta) == 1 and "gather_kernel" in next(iter(meta)), sorted(meta)
    for name, v in meta.items():
        assert v["private_segment_fixed_size"] == 0, (name, v)
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["vgpr_count"] + v.get("agpr_count", 0) <= VGPR_CEILING, (name, v)
        assert v["group_segment_fixed_size"] == 0, (name, v)
        assert v["max_flat_workgroup_size"] == 256, (name, v)

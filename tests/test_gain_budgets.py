"""Budgets of the gain stage's kernels, the ceilings DESIGN.md 15 states, read from the compiler's kernel metadata
(hipcc cross-compiles for gfx950 without a GPU), the way tests/test_gather_budgets.py reads the gather kernel's.  Every
kernel of peaq_gain.hip: nothing in scratch, no spilled VGPRs or SGPRs, workgroups of 256, no dynamic LDS (the host
passes 0; tests/test_gain_host.py::test_launches_pass_no_dynamic_lds reads that from the source).  gain_cut_kernel: at
most 64 VGPRs (eight waves per SIMD) and no LDS.  The two measure kernels: at most 128 VGPRs and no static LDS but
the workgroup reduction's 4 waves x 6 sums x 8 bytes."""
from test_pcm_budgets import VGPR_CEILING, kernel_metadata

MEASURE_VGPR_CEILING = 128
REDUCTION_LDS = 4 * 6 * 8


def test_gain_kernels_hold_their_budgets(tmp_path):
    meta = kernel_metadata("peaq_gain.hip", tmp_path)
    assert len(meta) == 3, sorted(meta)
    (cut,) = [k for k in meta if "gain_cut_kernel" in k]
    measure = [k for k in meta if "gain_measure_kernel" in k or "gain_finish_kernel" in k]
    assert len(measure) == 2, sorted(meta)
    for name, v in meta.items():
        assert v["private_segment_fixed_size"] == 0, (name, v)
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["max_flat_workgroup_size"] == 256, (name, v)
    v = meta[cut]
    assert v["vgpr_count"] + v.get("agpr_count", 0) <= VGPR_CEILING, (cut, v)
    assert v["group_segment_fixed_size"] == 0, (cut, v)
    for name in measure:
        v = meta[name]
        assert v["vgpr_count"] + v.get("agpr_count", 0) <= MEASURE_VGPR_CEILING, (name, v)
        assert v["group_segment_fixed_size"] == REDUCTION_LDS, (name, v)

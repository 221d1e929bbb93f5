"""Budgets of the sub-sample stage's kernels, the ceilings DESIGN.md 16 states, read from the compiler's kernel metadata
(hipcc cross-compiles for gfx950 without a GPU), the way tests/test_gain_budgets.py reads the gain stage's.  Every kernel
of peaq_frac.hip: nothing in scratch, no spilled VGPRs or SGPRs, at most 128 VGPRs (four waves per SIMD), workgroups
of 256, no dynamic LDS (tests/test_subsample_host.py::test_launches_pass_no_dynamic_lds reads that from the source), and
the static LDS per workgroup that DESIGN.md 16 states:
  frac_corr_kernel  36160 bytes: the chunk's window of 4096 + 32 doubles, one of padding per 16 and two more, and the
                    four waves' 33 sums
  frac_sum_kernel   352 bytes: the four waves' 11 sums of a pass
  frac_pick_kernel  48 bytes: the four waves' maxima and keys
  frac_cut_kernel   8832 bytes: two rows of 1024 + 64 + 16 floats"""
from test_pcm_budgets import kernel_metadata

VGPR_CEILING = 128
LDS = {"frac_corr_kernel": (4096 + 32 + (4096 + 32) // 16 + 2) * 8 + 4 * 33 * 8,
       "frac_sum_kernel": 4 * 11 * 8,
       "frac_pick_kernel": 4 * 8 + 4 * 4,
       "frac_cut_kernel": 2 * (1024 + 64 + 16) * 4}


def test_subsample_kernels_hold_their_budgets(tmp_path):
    meta = kernel_metadata("peaq_frac.hip", tmp_path)
    assert len(meta) == len(LDS), sorted(meta)
    for kernel, lds in LDS.items():
        (name,) = [k for k in meta if kernel in k]
        v = meta[name]
        assert v["private_segment_fixed_size"] == 0, (name, v)
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (name, v)
        assert v["max_flat_workgroup_size"] == 256, (name, v)
        assert v["vgpr_count"] + v.get("agpr_count", 0) <= VGPR_CEILING, (name, v)
        assert v["group_segment_fixed_size"] == lds, (name, v)

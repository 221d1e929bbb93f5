"""Budgets of the summary instantiations of the FFT back end (backend_summary_kernel), read from the
compiler's own kernel metadata as tests/test_pattern_bands_budgets.py does: both exist, keep nothing in scratch and spill
no vector register, run at the waves per SIMD of the plain instantiations they stand in for -- whose counts come from the
same build, not from a constant -- and three workgroups' LDS (the running rows live there) fit a CU's 160 KB.

The metadata is read per list item (tests/test_align_budgets.py's reader): the LDS size stands before the kernel's name
in an item, and a reader that goes line by line would book it to the kernel before."""
import pytest

from test_align_budgets import kernel_metadata
from test_kernel_budgets import find
from test_trace_budgets import waves_per_simd

# (summary kernel, its plain counterpart), as parts of the mangled names
PAIRS = [("backend_summary_kernelILi109ELb0E", "backend_kernelILi109ELb0ELb0E"),
         ("backend_summary_kernelILi55ELb1E", "backend_kernelILi55ELb1ELb0E")]
# the name fragments by which the other budget tests find their kernels, each of which has to go on matching one kernel
OTHERS = ["backend_kernelILi", "backend_bands_kernel", "backend_pattern_bands_kernel", "backend_trace_kernel"]
ROWS_LDS = {"backend_summary_kernelILi109ELb0E": 2 * 8 * 110 * 8, "backend_summary_kernelILi55ELb1E": 2 * 4 * 56 * 8}


@pytest.fixture(scope="module")
def be_meta(tmp_path_factory):
    return kernel_metadata("peaq_backend.hip", tmp_path_factory.mktemp("be_band_summary"))


@pytest.mark.parametrize("summary,plain", PAIRS)
def test_summary_kernels_exist_without_scratch_at_the_plain_kernels_occupancy(be_meta, summary, plain):
    b, p = find(be_meta, summary), find(be_meta, plain)
    assert b["private_segment_fixed_size"] == 0, b
    assert b["vgpr_spill_count"] == 0, b
    # Scalar "spills" never reach memory here (no scratch, asserted above): they sit in lanes of vector registers, which
    # are part of vgpr_count, which the occupancy check below holds.  The two row arrays' addresses and the rows' state
    # are the scalars this kernel keeps beyond its counterpart's: the allowance of tests/test_bands_budgets.py.
    assert b["sgpr_spill_count"] <= p["sgpr_spill_count"] + 64, (b, p)
    assert waves_per_simd(b) == waves_per_simd(p), (b, p)
    # three workgroups per CU, and the rows are in there: two channels' rows on top of the plain kernel's tables
    assert 3 * b["group_segment_fixed_size"] <= 160 * 1024, b
    assert b["group_segment_fixed_size"] >= p["group_segment_fixed_size"] + ROWS_LDS[summary], (b, p)


def test_the_new_kernels_names_match_none_of_the_other_budget_tests_fragments(be_meta):
    names = [k for k in be_meta if "backend_summary_kernel" in k]
    assert len(names) == 2, names
    for name in names:
        assert not any(frag in name for frag in OTHERS), name

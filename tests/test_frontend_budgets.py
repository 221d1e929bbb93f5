"""The register budget the front end's early table requests are built against: a wave may hold
at most 168 vector registers -- three waves per SIMD with the allocation granule of 8 -- with nothing spilled and no
scratch, in both instantiations.  Values requested ahead of the LDS exchanges they are used behind stay live across
them; a request that does not fit is dropped, not the budget.  Read from the compiler's own kernel metadata, as in
tests/test_kernel_budgets.py (hipcc cross-compiles for gfx950 without a GPU)."""
import pytest

from test_kernel_budgets import find, kernel_metadata


@pytest.fixture(scope="module")
def fe_meta(tmp_path_factory):
    return kernel_metadata("peaq_frontend.hip", tmp_path_factory.mktemp("fe"))


@pytest.mark.parametrize("kernel", ["frontend_kernelILi109E", "frontend_kernelILi55E"])
def test_front_end_holds_168_registers_without_spills_or_scratch(fe_meta, kernel):
    v = find(fe_meta, kernel)
    assert v["vgpr_count"] <= 168, v
    assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, v
    assert v["private_segment_fixed_size"] == 0, v

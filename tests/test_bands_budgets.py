"""Register budgets of the bands instantiations of the FFT back end (backend_bands_kernel), read from the
compiler's own kernel metadata as tests/test_trace_budgets.py does: both exist, keep nothing in scratch and spill
nothing, and run at the waves per SIMD of the plain instantiations they stand in for -- whose counts come from the same
build, not from a constant."""
import pytest

from test_kernel_budgets import find, kernel_metadata
from test_trace_budgets import waves_per_simd

# (bands kernel, its plain counterpart), as parts of the mangled names
PAIRS = [("backend_bands_kernelILi109ELb0E", "backend_kernelILi109ELb0ELb0E"),
         ("backend_bands_kernelILi55ELb1E", "backend_kernelILi55ELb1ELb0E")]


@pytest.fixture(scope="module")
def be_meta(tmp_path_factory):
    return kernel_metadata("peaq_backend.hip", tmp_path_factory.mktemp("be_bands"))


@pytest.mark.parametrize("bands,plain", PAIRS)
def test_bands_kernels_exist_without_scratch_at_the_plain_kernels_occupancy(be_meta, bands, plain):
    b, p = find(be_meta, bands), find(be_meta, plain)
    assert b["private_segment_fixed_size"] == 0, b
    assert b["vgpr_spill_count"] == 0, b
    # Scalar "spills" never reach memory here (no scratch, asserted above): the compiler parks them in lanes of vector
    # registers, 64 to a register, and those registers are part of vgpr_count, which the occupancy check below holds.
    # The bands kernels keep a few more scalars than their counterparts (the row array's address, its stride, the
    # plane mask): at most one vector register's worth of lanes more, the allowance of tests/test_trace_budgets.py.
    assert b["sgpr_spill_count"] <= p["sgpr_spill_count"] + 64, (b, p)
    assert waves_per_simd(b) == waves_per_simd(p), (b, p)

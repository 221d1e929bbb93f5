"""Register budget of the pattern-bands instantiation of the FFT back end (backend_pattern_bands_kernel),
read from the compiler's own kernel metadata as tests/test_bands_budgets.py does: it exists, keeps nothing in scratch
and spills no vector register, and runs at the waves per SIMD of the plain basic instantiation -- whose count comes
from the same build, not from a constant."""
import pytest

from test_kernel_budgets import find, kernel_metadata
from test_trace_budgets import waves_per_simd

PATTERN, PLAIN = "backend_pattern_bands_kernelILi109ELb0E", "backend_kernelILi109ELb0ELb0E"


@pytest.fixture(scope="module")
def be_meta(tmp_path_factory):
    return kernel_metadata("peaq_backend.hip", tmp_path_factory.mktemp("be_pattern_bands"))


def test_pattern_bands_kernel_exists_without_scratch_at_the_plain_kernels_occupancy(be_meta):
    b, p = find(be_meta, PATTERN), find(be_meta, PLAIN)
    assert b["private_segment_fixed_size"] == 0, b
    assert b["vgpr_spill_count"] == 0, b
    # Scalar "spills" never reach memory here (no scratch, asserted above): they sit in lanes of vector registers, which
    # are part of vgpr_count, which the occupancy check below holds.  The row array's address, its stride and the plane
    # mask are the scalars this kernel keeps beyond its counterpart's: the allowance of tests/test_bands_budgets.py.
    assert b["sgpr_spill_count"] <= p["sgpr_spill_count"] + 64, (b, p)
    assert waves_per_simd(b) == waves_per_simd(p), (b, p)

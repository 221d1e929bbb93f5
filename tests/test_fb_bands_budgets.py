"""Register budget of the bands instantiation of the filter-bank back end (fb_backend_bands_kernel), read
from the compiler's own kernel metadata as tests/test_trace_budgets.py does for the trace instantiation and held to the
same budget: it exists, keeps nothing in scratch and spills no vector register, parks at most one vector register's
worth of scalars more than the plain instantiation of the same build, and runs at that kernel's waves per SIMD."""
import pytest

from test_kernel_budgets import find, kernel_metadata
from test_trace_budgets import waves_per_simd

BANDS, PLAIN = "fb_backend_bands_kernel", "fb_backend_kernelILb0E"


@pytest.fixture(scope="module")
def be_meta(tmp_path_factory):
    return kernel_metadata("peaq_backend.hip", tmp_path_factory.mktemp("be_fb_bands"))


def test_fb_bands_kernel_exists_without_scratch_at_the_plain_kernel_s_occupancy(be_meta):
    t, p = find(be_meta, BANDS), find(be_meta, PLAIN)
    assert t["private_segment_fixed_size"] == 0, t
    assert t["vgpr_spill_count"] == 0, t
    # (scalar "spills" are lanes of vector registers here, never memory: see tests/test_trace_budgets.py)
    assert t["sgpr_spill_count"] <= p["sgpr_spill_count"] + 64, (t, p)
    assert waves_per_simd(t) == waves_per_simd(p), (t, p)

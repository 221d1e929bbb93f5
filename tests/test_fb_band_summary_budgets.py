"""Register budget of the summary instantiation of the filter-bank back end (fb_band_summary_kernel), read
from the compiler's own kernel metadata as tests/test_fb_bands_budgets.py does for the bands instantiation and held
against the plain instantiation of the same build: it exists under a name that no other budget test's fragment matches,
keeps no more in scratch and spills no more vector registers than the plain kernel, parks at most one vector register's
worth of scalars more, and runs at that kernel's waves per SIMD."""
import pytest

from test_kernel_budgets import find, kernel_metadata
from test_trace_budgets import waves_per_simd

SUMMARY, PLAIN = "fb_band_summary_kernel", "fb_backend_kernelILb0E"
# the fragments by which the other budget tests find their kernels: exactly one match each (two for the FFT summary)
OTHERS = ("backend_summary_kernel", "fb_backend_bands_kernel", PLAIN, "backend_trace_kernel", "backend_bands_kernel",
          "backend_pattern_bands_kernel")


@pytest.fixture(scope="module")
def be_meta(tmp_path_factory):
    return kernel_metadata("peaq_backend.hip", tmp_path_factory.mktemp("be_fb_band_summary"))


def test_exactly_one_kernel_has_the_name_and_no_other_test_s_fragment_matches_it(be_meta):
    names = [k for k in be_meta if SUMMARY in k]
    assert len(names) == 1, names
    for frag in OTHERS:
        assert frag not in names[0], (frag, names[0])
    # (the FFT summary's two instantiations are still the only ones of their fragment)
    assert len([k for k in be_meta if "backend_summary_kernel" in k]) == 2


def test_fb_band_summary_kernel_stays_within_the_plain_kernel_s_budget(be_meta):
    t, p = find(be_meta, SUMMARY), find(be_meta, PLAIN)
    print("summary", {k: t.get(k) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                        "private_segment_fixed_size", "group_segment_fixed_size")})
    print("plain  ", {k: p.get(k) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                                        "private_segment_fixed_size", "group_segment_fixed_size")})
    assert t["vgpr_spill_count"] <= p["vgpr_spill_count"], (t, p)
    assert t["private_segment_fixed_size"] <= p["private_segment_fixed_size"], (t, p)
    # (scalar "spills" are lanes of vector registers here, never memory: see tests/test_trace_budgets.py)
    assert t["sgpr_spill_count"] <= p["sgpr_spill_count"] + 64, (t, p)
    assert waves_per_simd(t) == waves_per_simd(p), (t, p)

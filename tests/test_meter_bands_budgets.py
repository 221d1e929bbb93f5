"""What the band meter's kernels are built on, read from the compiler's own kernel metadata as
tests/test_meter_budgets.py reads it: meter_bands_kernel keeps a lane's sixteen doubles of rows in registers for the
whole walk -- no scratch, nothing spilled, no LDS --, the live-band instantiations of the FFT back end cost no scratch
and no spilled vector register beyond the bands instantiations of the same template arguments, and the new names are
not taken for other kernels by the fragments the older budget tests search for."""
import re

import pytest

from test_kernel_budgets import find, kernel_metadata

KERNELS = ("meter_bands_kernelILi109E", "meter_bands_kernelILi55E")
# (live-band instantiation, the bands instantiation of the same template arguments): fragments of the mangled names
LIVEBAND = (("backend_liveband_kernelILi109ELb0E", "backend_bands_kernelILi109ELb0E"),
            ("backend_liveband_kernelILi55ELb1E", "backend_bands_kernelILi55ELb1E"))
# what the existing budget tests find back-end kernels by, expecting a fixed number of matches
FRAGMENTS = ("live_kernel", "backend_kernelI", "backend_bands_kernel", "backend_trace_kernel", "backend_summary_kernel",
             "backend_pattern_bands_kernel")


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    """(the metadata of every kernel of peaq_meter_bands.hip by name, the assembly text they were read from)"""
    tmp = tmp_path_factory.mktemp("meter_bands")
    return kernel_metadata("peaq_meter_bands.hip", tmp), (tmp / "peaq_meter_bands.hip.s").read_text()


@pytest.fixture(scope="module")
def backend_meta(tmp_path_factory):
    return kernel_metadata("peaq_backend.hip", tmp_path_factory.mktemp("meter_bands_backend"))


def test_the_file_has_the_two_instantiations_and_nothing_else(assembly):
    kernels = [k for k in assembly[0] if k.startswith("_Z")]    # (the metadata names the kernels' arguments too)
    assert len(kernels) == 2, kernels
    for name in KERNELS:
        find(assembly[0], name)


@pytest.mark.parametrize("name", KERNELS)
def test_the_band_kernel_has_no_scratch_and_spills_nothing(assembly, name):
    k = find(assembly[0], name)
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k


@pytest.mark.parametrize("name", KERNELS)
def test_the_band_kernel_uses_no_lds(assembly, name):
    """(read from the kernel's own descriptor: in the metadata the LDS size comes before the name it belongs to)"""
    meta, text = assembly
    (full,) = [k for k in meta if name in k]
    block = text[text.index(".amdhsa_kernel " + full):]
    block = block[:block.index(".end_amdhsa_kernel")]
    assert re.search(r"\.amdhsa_group_segment_fixed_size\s+0\s", block), block


@pytest.mark.parametrize("liveband,bands", LIVEBAND)
def test_a_live_band_back_end_has_no_more_scratch_than_the_bands_one(backend_meta, liveband, bands):
    lb, bd = find(backend_meta, liveband), find(backend_meta, bands)
    assert lb["private_segment_fixed_size"] <= bd["private_segment_fixed_size"], (lb, bd)
    assert lb["vgpr_spill_count"] <= bd["vgpr_spill_count"], (lb, bd)


def test_the_new_kernels_are_not_taken_for_other_kernels(assembly, backend_meta):
    new = [k for k in assembly[0] if k.startswith("_Z")] + [k for k in backend_meta if "backend_liveband_kernel" in k]
    assert len(new) == 4, new
    for fragment in FRAGMENTS:
        assert not [k for k in new if fragment in k], (fragment, new)


def test_the_back_end_still_has_three_live_kernels(backend_meta):
    assert len([k for k in backend_meta if "live_kernel" in k]) == 3, sorted(backend_meta)

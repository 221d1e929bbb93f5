"""What the three kernels of peaq_meter.hip and the live instantiations of the back ends are built on,
read from the compiler's own kernel metadata as tests/test_replay_budgets.py reads it: the accumulator's twelve fields and
the unit in flight live in registers for the whole walk -- no scratch, nothing spilled --, the kernels use no LDS, and
leaving the records launch-relative costs the back ends no scratch beyond what the trace instantiations have."""
import re

import pytest

from test_kernel_budgets import find, kernel_metadata

KERNELS = ("meter_basic_kernel", "meter_adv_fft_kernel", "meter_adv_fb_kernel")
# (live instantiation, the trace instantiation it is modelled on): fragments of the mangled names
LIVE = (("backend_live_kernelILi109ELb0E", "backend_trace_kernelILi109ELb0E"),
        ("backend_live_kernelILi55ELb1E", "backend_trace_kernelILi55ELb1E"),
        ("fb_backend_live_kernel", "fb_backend_trace_kernel"))
# what tests/test_kernel_budgets.py and tests/test_replay_budgets.py find kernels by, expecting one match
FRAGMENTS = ("finalize_kernel", "state_init_kernel", "backend_kernelI", "fb_backend_kernelILb0E", "fb_backend_kernelI",
             "window_replay_kernel", "span_replay_fft_kernel", "span_replay_fb_kernel")


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    """(the metadata of every kernel of peaq_meter.hip by name, the assembly text they were read from)"""
    tmp = tmp_path_factory.mktemp("meter")
    return kernel_metadata("peaq_meter.hip", tmp), (tmp / "peaq_meter.hip.s").read_text()


@pytest.fixture(scope="module")
def backend_meta(tmp_path_factory):
    return kernel_metadata("peaq_backend.hip", tmp_path_factory.mktemp("meter_backend"))


def test_the_file_has_the_three_meter_kernels_and_nothing_else(assembly):
    kernels = [k for k in assembly[0] if k.startswith("_Z")]    # (the metadata names the kernels' arguments too)
    assert len(kernels) == 3, kernels
    for name in KERNELS:
        find(assembly[0], name)


@pytest.mark.parametrize("name", KERNELS)
def test_the_meter_has_no_scratch(assembly, name):
    k = find(assembly[0], name)
    assert k["private_segment_fixed_size"] == 0, k


@pytest.mark.parametrize("name", KERNELS)
def test_the_meter_spills_no_registers(assembly, name):
    k = find(assembly[0], name)
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k


@pytest.mark.parametrize("name", KERNELS)
def test_the_meter_uses_no_lds(assembly, name):
    """(read from the kernel's own descriptor: in the metadata the LDS size comes before the name it belongs to)"""
    meta, text = assembly
    (full,) = [k for k in meta if name in k]
    block = text[text.index(".amdhsa_kernel " + full):]
    block = block[:block.index(".end_amdhsa_kernel")]
    assert re.search(r"\.amdhsa_group_segment_fixed_size\s+0\s", block), block


@pytest.mark.parametrize("live,trace", LIVE)
def test_a_live_back_end_has_no_more_scratch_than_the_trace_one(backend_meta, live, trace):
    lv, tr = find(backend_meta, live), find(backend_meta, trace)
    assert lv["private_segment_fixed_size"] <= tr["private_segment_fixed_size"], (lv, tr)
    assert lv["vgpr_spill_count"] <= tr["vgpr_spill_count"], (lv, tr)


def test_the_new_kernels_are_not_taken_for_other_kernels(assembly, backend_meta):
    """the budget tests find kernels by a fragment of their name and expect one match"""
    new = [k for k in assembly[0] if k.startswith("_Z")] + [k for k in backend_meta if "live_kernel" in k]
    assert len(new) == 6, new
    for fragment in FRAGMENTS:
        assert not [k for k in new if fragment in k], (fragment, new)

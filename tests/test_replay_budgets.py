"""What window_replay_kernel, span_replay_fft_kernel and span_replay_fb_kernel (peaq_replay.hip) are
built on, read from the compiler's own kernel metadata as tests/test_kernel_budgets.py reads it: the accumulator's twelve
fields and the unit in flight live in registers for the whole walk -- no scratch, nothing spilled -- and the kernels use
no LDS."""
import re

import pytest

from test_kernel_budgets import find, kernel_metadata

KERNELS = ("window_replay_kernel", "span_replay_fft_kernel", "span_replay_fb_kernel")


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    """(the metadata of every kernel of peaq_replay.hip by name, the assembly text they were read from)"""
    tmp = tmp_path_factory.mktemp("replay")
    return kernel_metadata("peaq_replay.hip", tmp), (tmp / "peaq_replay.hip.s").read_text()


def test_the_file_has_the_three_replays_and_nothing_else(assembly):
    kernels = [k for k in assembly[0] if k.startswith("_Z")]    # (the metadata names the kernels' arguments too)
    assert len(kernels) == 3, kernels
    for name in KERNELS:
        find(assembly[0], name)


@pytest.mark.parametrize("name", KERNELS)
def test_the_replay_has_no_scratch(assembly, name):
    k = find(assembly[0], name)
    assert k["private_segment_fixed_size"] == 0, k


@pytest.mark.parametrize("name", KERNELS)
def test_the_replay_spills_no_registers(assembly, name):
    k = find(assembly[0], name)
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k


@pytest.mark.parametrize("name", KERNELS)
def test_the_replay_uses_no_lds(assembly, name):
    """(read from the kernel's own descriptor: in the metadata the LDS size comes before the name it belongs to)"""
    meta, text = assembly
    (full,) = [k for k in meta if name in k]
    block = text[text.index(".amdhsa_kernel " + full):]
    block = block[:block.index(".end_amdhsa_kernel")]
    assert re.search(r"\.amdhsa_group_segment_fixed_size\s+0\s", block), block


def test_the_replays_are_not_taken_for_other_kernels(assembly):
    """tests/test_kernel_budgets.py finds kernels by a fragment of their name and expects one match"""
    for fragment in ("finalize_kernel", "state_init_kernel", "backend_kernelI", "fb_backend_kernelI"):
        assert not [k for k in assembly[0] if fragment in k], (fragment, list(assembly[0]))

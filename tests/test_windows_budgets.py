"""What window_replay_kernel (peaq_windows.hip) is built on, read from the compiler's own kernel metadata
as tests/test_kernel_budgets.py reads it: the accumulator's twelve fields and the frame in flight live in registers for
the whole walk -- no scratch, nothing spilled -- and the kernel uses no LDS."""
import re

import pytest

from test_kernel_budgets import find, kernel_metadata


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    """(the metadata of every kernel of peaq_windows.hip by name, the assembly text they were read from)"""
    tmp = tmp_path_factory.mktemp("windows")
    return kernel_metadata("peaq_windows.hip", tmp), (tmp / "peaq_windows.hip.s").read_text()


@pytest.fixture(scope="module")
def replay(assembly):
    return find(assembly[0], "window_replay_kernel")


def test_the_replay_has_no_scratch(replay):
    assert replay["private_segment_fixed_size"] == 0, replay


def test_the_replay_spills_no_registers(replay):
    assert replay["vgpr_spill_count"] == 0 and replay["sgpr_spill_count"] == 0, replay


def test_the_replay_uses_no_lds(assembly):
    """(read from the kernel's own descriptor: in the metadata the LDS size comes before the name it belongs to)"""
    meta, text = assembly
    (name,) = [k for k in meta if "window_replay_kernel" in k]
    block = text[text.index(".amdhsa_kernel " + name):]
    block = block[:block.index(".end_amdhsa_kernel")]
    assert re.search(r"\.amdhsa_group_segment_fixed_size\s+0\s", block), block


def test_the_new_kernel_is_not_taken_for_an_existing_one(assembly):
    """tests/test_kernel_budgets.py finds kernels by a fragment of their name and expects one match"""
    for fragment in ("finalize_kernel", "state_init_kernel", "backend_kernelI", "fb_backend_kernelI"):
        assert not [k for k in assembly[0] if fragment in k], (fragment, list(assembly[0]))

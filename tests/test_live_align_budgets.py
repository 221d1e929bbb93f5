"""What the two kernels of peaq_watch.hip are built on, read from the compiler's own kernel metadata as
tests/test_meter_budgets.py reads it: nothing in scratch, nothing spilled, the frames kernel's LDS small enough for two
workgroups on a CU, and names that the other budget tests do not take for one of their kernels."""
import re

import pytest

import test_meter_budgets
import test_replay_budgets
from test_kernel_budgets import find, kernel_metadata

KERNELS = ("delay_watch_frames_kernel", "delay_watch_fold_kernel")


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    """(the metadata of every kernel of peaq_watch.hip by name, the assembly text they were read from)"""
    tmp = tmp_path_factory.mktemp("watch")
    return kernel_metadata("peaq_watch.hip", tmp), (tmp / "peaq_watch.hip.s").read_text()


@pytest.fixture(scope="module")
def meta(assembly):
    return assembly[0]


def lds_bytes(assembly, name):
    """(read from the kernel's own descriptor: in the metadata the LDS size comes before the name it belongs to)"""
    meta, text = assembly
    (full,) = [k for k in meta if name in k]
    block = text[text.index(".amdhsa_kernel " + full):]
    block = block[:block.index(".end_amdhsa_kernel")]
    return int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)\s", block).group(1))


def kernels_of(meta):
    return [k for k in meta if k.startswith("_Z")]          # (the metadata names the kernels' arguments too)


def test_the_file_has_the_two_watch_kernels_and_nothing_else(meta):
    assert len(kernels_of(meta)) == 2, kernels_of(meta)
    for name in KERNELS:
        find(meta, name)


@pytest.mark.parametrize("name", KERNELS)
def test_the_watch_has_no_scratch_and_spills_no_registers(meta, name):
    k = find(meta, name)
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k


def test_two_workgroups_of_the_frames_kernel_fit_a_cu(assembly):
    lds = lds_bytes(assembly, "delay_watch_frames_kernel")
    assert lds <= 80 * 1024, lds                            # 160 KB of LDS per CU
    # four waves, each its own r over [512, 1536) and t over [481, 1567) as doubles: 4 (1024 + 1086) 8 bytes at least
    assert lds >= 4 * (1024 + 1086) * 8, lds
    assert lds_bytes(assembly, "delay_watch_fold_kernel") == 0


def test_the_new_kernels_are_not_taken_for_other_kernels(meta):
    """the budget tests find kernels by a fragment of their name and expect one match"""
    fragments = set(test_meter_budgets.FRAGMENTS) | set(test_meter_budgets.KERNELS)
    fragments |= {f for pair in test_meter_budgets.LIVE for f in pair}
    fragments |= {v for v in vars(test_replay_budgets).values() if isinstance(v, str) and v.endswith("_kernel")}
    assert len(fragments) >= len(test_meter_budgets.FRAGMENTS) + 3
    for fragment in fragments:
        assert not [k for k in kernels_of(meta) if fragment in k], (fragment, kernels_of(meta))

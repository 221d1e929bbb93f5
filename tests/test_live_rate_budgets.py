"""What the range converter of live streams (peaq_live_rate.hip) is built on, read from the compiler's own
kernel metadata as tests/test_live_align_budgets.py reads it: one kernel, nothing in scratch, nothing spilled, LDS small
enough for two workgroups on a CU (it is far smaller: the staged span of 256 outputs), and a name that the other budget
tests do not take for one of their kernels."""
import pytest

import test_meter_budgets
import test_replay_budgets
from test_kernel_budgets import find, kernel_metadata
from test_live_align_budgets import kernels_of, lds_bytes
import test_live_align_budgets

KERNEL = "resample_range_kernel"


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    """(the metadata of every kernel of peaq_live_rate.hip by name, the assembly text they were read from)"""
    tmp = tmp_path_factory.mktemp("live_rate")
    return kernel_metadata("peaq_live_rate.hip", tmp), (tmp / "peaq_live_rate.hip.s").read_text()


@pytest.fixture(scope="module")
def meta(assembly):
    return assembly[0]


def test_the_file_has_its_one_kernel(meta):
    assert len(kernels_of(meta)) == 1, kernels_of(meta)
    find(meta, KERNEL)


def test_no_scratch_and_no_spills(meta):
    k = find(meta, KERNEL)
    assert k["private_segment_fixed_size"] == 0, k
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k


def test_two_workgroups_fit_a_cu(assembly):
    lds = lds_bytes(assembly, KERNEL)
    assert lds <= 80 * 1024, lds                            # 160 KB of LDS per CU
    # the raw span of 256 outputs at the steepest ratio, 8 inputs an output, and the longest filter, 514 taps, stereo
    assert lds >= (256 * 8 + 514) * 2 * 4, lds


def test_the_kernel_is_not_taken_for_another_budget_tests_kernel(meta):
    """the budget tests find kernels by a fragment of their name and expect one match"""
    fragments = set(test_meter_budgets.FRAGMENTS) | set(test_meter_budgets.KERNELS) | set(test_live_align_budgets.KERNELS)
    fragments |= {f for pair in test_meter_budgets.LIVE for f in pair}
    fragments |= {v for v in vars(test_replay_budgets).values() if isinstance(v, str) and v.endswith("_kernel")}
    fragments |= {"resample_tile_kernel", "resample_any_kernel"}
    for fragment in fragments:
        assert not [k for k in kernels_of(meta) if fragment in k], (fragment, kernels_of(meta))

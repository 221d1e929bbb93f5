"""Register budgets of the trace instantiations of the two back ends (backend_trace_kernel, fb_backend_trace_kernel;
DESIGN.md 13), read from the compiler's own kernel metadata as tests/test_kernel_budgets.py does: they exist, keep
nothing in scratch and spill nothing, and run at the waves per SIMD of the plain instantiations they stand in for --
whose counts come from the same build, not from a constant."""
import pytest

from test_kernel_budgets import find, kernel_metadata

# (trace kernel, its plain counterpart), as parts of the mangled names
PAIRS = [("backend_trace_kernelILi109ELb0E", "backend_kernelILi109ELb0ELb0E"),
         ("backend_trace_kernelILi55ELb1E", "backend_kernelILi55ELb1ELb0E"),
         ("fb_backend_trace_kernel", "fb_backend_kernelILb0E")]


@pytest.fixture(scope="module")
def be_meta(tmp_path_factory):
    return kernel_metadata("peaq_backend.hip", tmp_path_factory.mktemp("be_trace"))


def waves_per_simd(v):
    """a SIMD has 512 registers per lane; a wave's share is its vector and accumulation registers in blocks of 8"""
    regs = v["vgpr_count"] + v.get("agpr_count", 0)
    return min(8, 512 // (-(-regs // 8) * 8))


@pytest.mark.parametrize("trace,plain", PAIRS)
def test_trace_kernels_exist_without_scratch_at_the_plain_kernels_occupancy(be_meta, trace, plain):
    t, p = find(be_meta, trace), find(be_meta, plain)
    assert t["private_segment_fixed_size"] == 0, t
    assert t["vgpr_spill_count"] == 0, t
    # Scalar "spills" never reach memory here (no scratch, asserted above): the compiler parks them in lanes of vector
    # registers, 64 to a register, and those registers are part of vgpr_count, which the occupancy check below holds.
    # The trace kernels keep a few more scalars than their counterparts (the record's address, the pair's full-frame
    # count): at most one vector register's worth of lanes more.
    assert t["sgpr_spill_count"] <= p["sgpr_spill_count"] + 64, (t, p)
    assert waves_per_simd(t) == waves_per_simd(p), (t, p)

"""CPU-side checks of the trajectory entry points (peaq_batch_run_trajectory, include/peaq_amd.h): declared and
exported, arguments refused with a message before any device work, the workspace they report, and the register budgets
of the back ends' points instantiations read from the compiler's kernel metadata (tests/test_kernel_budgets.py)."""
import ctypes as C
import re
from pathlib import Path

import pytest

from test_kernel_budgets import find, kernel_metadata

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("peaq_batch_run_trajectory", "peaq_batch_trajectory_workspace_bytes", "peaq_run_pair_trajectory")


@pytest.fixture(scope="module")
def lib():
    import gstpeaq_amd
    if not gstpeaq_amd.library_path().exists():
        gstpeaq_amd.build_library()
    return gstpeaq_amd.load_library()


def test_header_declares_and_library_exports_the_entries(lib):
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "peaq_amd.h").read_text(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), name


def trajectory(lib, ctx=None, interval=1024, n_points=4, d_points=C.c_void_p(16), n_pairs=1):
    return lib.peaq_batch_run_trajectory(ctx, 0, 2, 92.0, n_pairs, C.c_void_p(16), C.c_void_p(16), 4096, None, None,
                                         4096, interval, n_points, d_points, None, None)


def test_batch_trajectory_refuses_bad_arguments(lib):
    lib.peaq_last_error.restype = C.c_char_p
    for kw, word in ((dict(), b"ctx is NULL"), (dict(interval=0), b"interval"), (dict(n_points=0), b"n_points"),
                     (dict(n_points=-3), b"n_points"), (dict(d_points=None), b"d_points")):
        assert trajectory(lib, **kw) == -1, kw                               # PEAQ_ERR_ARG
        msg = lib.peaq_last_error()
        assert msg.startswith(b"peaq_batch_run_trajectory") and word in msg, (kw, msg)
    lib.peaq_run_pair_trajectory.restype = C.c_int
    assert lib.peaq_run_pair_trajectory(None, 0, 1, 92.0, None, 0, None, 0, 0, 4, None, None) == -1
    assert b"interval" in lib.peaq_last_error()
    out = (C.c_double * 16)()
    assert lib.peaq_run_pair_trajectory(None, 0, 1, 92.0, None, 0, None, 0, 48000, 4, out, out) == -1
    assert b"NULL" in lib.peaq_last_error()


def test_trajectory_workspace_adds_the_snapshots(lib):
    for adv, ch, pairs, n in ((0, 2, 4096, 480000), (1, 2, 64, 480000), (0, 1, 1, 1000)):
        base = lib.peaq_batch_workspace_bytes(adv, ch, pairs, n)
        w1 = lib.peaq_batch_trajectory_workspace_bytes(adv, ch, pairs, n, 1)
        w10 = lib.peaq_batch_trajectory_workspace_bytes(adv, ch, pairs, n, 10)
        assert base < w1 < w10, (adv, ch, pairs, n, base, w1, w10)
        per_point = (w10 - w1) / 9 / pairs
        assert 2000 <= per_point <= 2400, per_point                           # about 2.2 KB per pair and point


@pytest.fixture(scope="module")
def be_meta(tmp_path_factory):
    return kernel_metadata("peaq_backend.hip", tmp_path_factory.mktemp("be"))


def test_points_instantiations_keep_the_register_budgets(be_meta):
    """The basic points back end runs beside the next chunk's front end like backend_kernel<109,false,false>: three
    waves per SIMD, <= 170 registers, nothing spilled.  The filter-bank points back end may not spill more, or use more
    scratch, than fb_backend_kernel<false> in the same compile."""
    v = find(be_meta, "backend_points_kernelILi109ELb0E")
    assert v["vgpr_count"] <= 170 and v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, v
    v = find(be_meta, "backend_points_kernelILi55ELb1E")
    assert v["vgpr_count"] <= 170 and v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, v
    pts, plain = find(be_meta, "fb_backend_points_kernel"), find(be_meta, "fb_backend_kernelILb0E")
    assert pts["vgpr_count"] <= 128, pts
    assert pts["vgpr_spill_count"] <= plain["vgpr_spill_count"], (pts, plain)
    assert pts["private_segment_fixed_size"] <= plain["private_segment_fixed_size"], (pts, plain)

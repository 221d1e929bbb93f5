"""CPU-side tests of the band meter (peaq_session_set_meter_bands, include/peaq_amd.h "meter: band rows"):
the names are declared, exported and bound, the row count, the workspace arithmetic against the formula of the header,
the narrower limits of the geometry, and the refusals that need no device.  No GPU.  (A session exists only on a
device: what one refuses, and the rows themselves, are in tests/test_gpu_meter_bands.py.)"""
import ctypes as C
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("peaq_meter_band_rows", "peaq_meter_bands_workspace", "peaq_session_set_meter_bands",
           "peaq_session_meter_read_bands", "peaq_broker_set_meter_bands", "peaq_broker_meter_read_bands")


@pytest.fixture(scope="module")
def lib():
    import gstpeaq_amd
    if not gstpeaq_amd.library_path().exists():
        gstpeaq_amd.build_library()
    L = gstpeaq_amd.load_library()
    L.peaq_last_error.restype = C.c_char_p
    return L


def workspace(lib, W, H, D, advanced, channels):
    import gstpeaq_amd
    cfg = gstpeaq_amd.MeterConfig(W, H, D)
    n = C.c_size_t(12345)
    rc = lib.peaq_meter_bands_workspace(C.byref(cfg), advanced, channels, C.byref(n))
    return rc, n.value


def test_every_new_declared_name_is_exported_and_bound(lib):
    import gstpeaq_amd
    header = (ROOT / "include" / "peaq_amd.h").read_text()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    declared = set(re.findall(r"\b(peaq_[a-z_0-9]*meter_(?:band|read_band)[a-z_0-9]*)\s*\(", code))
    assert declared == set(ENTRIES), declared
    for name in ENTRIES:
        assert hasattr(lib, name), name
    for name in ("METER_BAND_ROWS", "METER_BANDS_MAX_OPEN", "METER_BANDS_MAX_DEPTH", "meter_bands_workspace"):
        assert hasattr(gstpeaq_amd, name) and name in gstpeaq_amd.__all__, name
    for cls in (gstpeaq_amd.Session, gstpeaq_amd.Broker):
        assert hasattr(cls, "set_meter_bands")
        for method in ("set_meter", "meter_read"):
            assert "bands" in getattr(cls, method).__code__.co_varnames, (cls, method)
    assert (gstpeaq_amd.METER_BANDS_MAX_OPEN, gstpeaq_amd.METER_BANDS_MAX_DEPTH) == (16, 256)


def test_there_are_four_rows_the_first_four_of_the_band_summary(lib):
    import gstpeaq_amd
    assert lib.peaq_meter_band_rows() == 4 == gstpeaq_amd.METER_BAND_ROWS
    assert gstpeaq_amd.BAND_SUMMARY_ROWS[:4] == ("nmr_sum", "nmr_max", "nmr_disturbed", "exc_ref_sum")
    header = (ROOT / "include" / "peaq_amd.h").read_text()
    for k, name in enumerate(("NMR_SUM", "NMR_MAX", "NMR_DISTURBED", "EXC_REF_SUM")):
        assert re.search(r"#define PEAQ_BAND_SUMMARY_%s\s+%d\b" % (name, k), header), name


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("advanced", [0, 1])
def test_the_workspace_is_the_formula_of_the_header(lib, advanced, channels):
    """*bytes = 8 channels (K (8 row + 2) + 4 (D + 2) row + 2 * 64 row)"""
    header = (ROOT / "include" / "peaq_amd.h").read_text()
    assert "*bytes = 8 channels (K (8 row + 2) + 4 (D + 2) row + 2 * 64 row)" in header
    row = lib.peaq_band_row(advanced)
    assert row == (56 if advanced else 110)
    for W, H, D in ((16, 4, 256), (4, 2, 1), (1, 1, 64), (16, 1, 7), (5, 9, 2), (200, 200, 256), (31, 2, 100)):
        K = -(-W // H)
        rc, got = workspace(lib, W, H, D, advanced, channels)
        assert rc == 0, lib.peaq_last_error()
        assert got == 8 * channels * (K * (8 * row + 2) + 4 * (D + 2) * row + 2 * 64 * row), (W, H, D)
    import gstpeaq_amd
    assert gstpeaq_amd.meter_bands_workspace(16, 4, 256, advanced=bool(advanced), channels=channels) == \
        workspace(lib, 16, 4, 256, advanced, channels)[1]


def test_the_geometry_is_held_to_sixteen_open_windows_and_a_depth_of_256(lib):
    assert workspace(lib, 16, 1, 256, 0, 2)[0] == 0        # K = 16, depth 256: the limits themselves
    assert workspace(lib, 32, 2, 256, 1, 1)[0] == 0
    rc, n = workspace(lib, 17, 1, 64, 0, 2)                # K = 17
    assert rc == -1 and n == 0
    msg = lib.peaq_last_error()
    assert b"peaq_meter_bands_workspace" in msg and b"17 windows open at once" in msg and b"16" in msg, msg
    rc, n = workspace(lib, 33, 2, 64, 0, 2)                # K = ceil (33 / 2) = 17
    assert rc == -1 and b"17 windows open at once" in lib.peaq_last_error()
    rc, n = workspace(lib, 16, 4, 257, 0, 2)
    assert rc == -1 and n == 0
    msg = lib.peaq_last_error()
    assert b"peaq_meter_bands_workspace" in msg and b"depth 257" in msg and b"256" in msg, msg
    # what the meter itself refuses is refused here as well
    assert workspace(lib, 0, 1, 64, 0, 2)[0] == -1 and b"must both be at least 1" in lib.peaq_last_error()
    assert workspace(lib, 16, 4, 0, 0, 2)[0] == -1 and b"depth 0" in lib.peaq_last_error()
    assert workspace(lib, 16, 4, 64, 0, 3)[0] == -1 and b"channels must be 1 or 2" in lib.peaq_last_error()


def test_null_arguments_are_refused_by_name(lib):
    import gstpeaq_amd
    cfg = gstpeaq_amd.MeterConfig(16, 4, 64)
    n = C.c_size_t(0)
    k = C.c_int(0)
    lib.peaq_meter_bands_workspace.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    try:
        assert lib.peaq_meter_bands_workspace(None, 0, 2, C.byref(n)) == -1
        assert b"peaq_meter_bands_workspace: NULL argument" in lib.peaq_last_error()
        assert lib.peaq_meter_bands_workspace(C.byref(cfg), 0, 2, None) == -1
        assert b"peaq_meter_bands_workspace: NULL argument" in lib.peaq_last_error()
    finally:
        lib.peaq_meter_bands_workspace.argtypes = [C.POINTER(gstpeaq_amd.MeterConfig), C.c_int, C.c_int,
                                                   C.POINTER(C.c_size_t)]
    assert lib.peaq_session_set_meter_bands(None, 1) == -1
    assert b"peaq_session_set_meter_bands: session is NULL" in lib.peaq_last_error()
    assert lib.peaq_broker_set_meter_bands(None, 1) == -1
    assert b"peaq_broker_set_meter_bands: broker is NULL" in lib.peaq_last_error()
    assert lib.peaq_session_meter_read_bands(None, None, None, 0, C.byref(k), None) == -1
    assert b"peaq_session_meter_read_bands: NULL argument" in lib.peaq_last_error()
    assert lib.peaq_broker_meter_read_bands(None, 0, None, None, 0, C.byref(k), None) == -1
    assert b"peaq_broker_meter_read_bands: NULL argument" in lib.peaq_last_error()

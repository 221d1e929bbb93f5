"""ctypes binding of libpeaq_amd.so (include/peaq_amd.h)."""
import collections
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

PKG = Path(__file__).resolve().parent
ROOT = PKG.parent

# gstpeaq.c:95-108 / :86-93
MOV_NAMES_BASIC = ["BandwidthRefB", "BandwidthTestB", "TotalNMRB", "WinModDiff1B", "ADBB", "EHSB",
                   "AvgModDiff1B", "AvgModDiff2B", "RmsNoiseLoudB", "MFPDB", "RelDistFramesB"]
MOV_NAMES_ADVANCED = ["RmsModDiffA", "RmsNoiseLoudAsymA", "SegmentalNMRB", "EHSB", "AvgLinDistA"]

RESULT_DOUBLES = 16
RECORD_DOUBLES = 576


class Settings(C.Structure):
    """mirrors peaq_settings (include/peaq_amd.h): the reference's settings.h switches"""
    _fields_ = [("swap_mod_patts_for_noise_loudness_movs", C.c_int), ("center_ehs_correlation_window", C.c_int),
                ("ehs_subtract_dc_before_window", C.c_int), ("use_floor_for_steps_above_threshold", C.c_int),
                ("clamp_movs", C.c_int), ("swap_slope_filter_coefficients", C.c_int)]


class PeaqError(RuntimeError):
    pass


class ResamplePlan(C.Structure):
    """mirrors peaq_resample_plan (include/peaq_amd.h)"""
    _fields_ = [("L", C.c_uint32), ("M", C.c_uint32), ("taps", C.c_uint32), ("tiled", C.c_int),
                ("period_out", C.c_uint32), ("period_in", C.c_uint32), ("zero_taps", C.c_uint32),
                ("lds_bytes", C.c_uint32), ("table_bytes", C.c_uint64), ("max_sum_abs_taps", C.c_double)]


class RateSegment(C.Structure):
    """mirrors peaq_rate_segment (include/peaq_amd.h)"""
    _fields_ = [("out_first", C.c_uint64), ("in_base", C.c_uint64), ("in_total", C.c_uint64),
                ("out_count", C.c_uint32), ("in_have", C.c_uint32)]


class Delay(C.Structure):
    """mirrors peaq_delay (include/peaq_amd.h)"""
    _fields_ = [("lag", C.c_int32), ("reserved", C.c_int32), ("peak", C.c_double), ("runner_up", C.c_double),
                ("norm", C.c_double)]


class Gain(C.Structure):
    """mirrors peaq_gain (include/peaq_amd.h)"""
    _fields_ = [("gain", C.c_double * 2), ("srr", C.c_double * 2), ("stt", C.c_double * 2), ("srt", C.c_double * 2),
                ("flags", C.c_uint32 * 2), ("n", C.c_uint32), ("reserved", C.c_uint32)]


# PEAQ_GAIN_* (include/peaq_amd.h) and the record as a numpy structured dtype
GAIN_MODES = {None: 0, "off": 0, "lsq": 1, "rms": 2, "polarity": 3}
GAIN_PER_CHANNEL = 0x10
GAIN_F_SILENT, GAIN_F_NONFINITE, GAIN_F_ZERO, GAIN_F_RANGE = 1, 2, 4, 8
GAIN_DTYPE = np.dtype([("gain", "<f8", (2,)), ("srr", "<f8", (2,)), ("stt", "<f8", (2,)), ("srt", "<f8", (2,)),
                       ("flags", "<u4", (2,)), ("n", "<u4"), ("reserved", "<u4")])


class SubDelay(C.Structure):
    """mirrors peaq_subdelay (include/peaq_amd.h)"""
    _fields_ = [("lag", C.c_int32), ("q", C.c_int32), ("frac", C.c_double), ("peak", C.c_double), ("c0", C.c_double),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


# PEAQ_SUB_* (include/peaq_amd.h) and the record as a numpy structured dtype
SUB_STEPS, SUB_LAGS, SUB_HALF = 256, 16, 32
SUB_F_NONE, SUB_F_EDGE = 1, 2
SUBDELAY_DTYPE = np.dtype([("lag", "<i4"), ("q", "<i4"), ("frac", "<f8"), ("peak", "<f8"), ("c0", "<f8"), ("flags", "<u4"),
                           ("reserved", "<u4")])


class Drift(C.Structure):
    """mirrors peaq_drift (include/peaq_amd.h)"""
    _fields_ = [("lag0", C.c_int32), ("flags", C.c_uint32), ("a", C.c_double), ("e", C.c_double), ("ppm", C.c_double),
                ("resid_rms", C.c_double), ("n_windows", C.c_uint32), ("n_valid", C.c_uint32)]


# PEAQ_DRIFT_* (include/peaq_amd.h), the record as a numpy structured dtype, and this binding's defaults
DRIFT_F_NONE, DRIFT_F_RANGE = 1, 2
DRIFT_MIN_WINDOW, DRIFT_MAX_WINDOW, DRIFT_MAX_WINDOWS, DRIFT_MAX_E = 4096, 1 << 20, 4096, 1e-3
DRIFT_WINDOW, DRIFT_MIN_CORR = 32768, 0.5
DRIFT_DTYPE = np.dtype([("lag0", "<i4"), ("flags", "<u4"), ("a", "<f8"), ("e", "<f8"), ("ppm", "<f8"), ("resid_rms", "<f8"),
                        ("n_windows", "<u4"), ("n_valid", "<u4")])
DELAY_DTYPE = np.dtype([("lag", "<i4"), ("reserved", "<i4"), ("peak", "<f8"), ("runner_up", "<f8"), ("norm", "<f8")])


class WideDelay(C.Structure):
    """mirrors peaq_wide_delay (include/peaq_amd.h)"""
    _fields_ = [("lag", C.c_int32), ("coarse_lag", C.c_int32), ("factor", C.c_uint32), ("flags", C.c_uint32),
                ("fine", Delay), ("coarse", Delay)]


# PEAQ_WIDE_* (include/peaq_amd.h) and the record as a numpy structured dtype
WIDE_WAVEFORM, WIDE_ENVELOPE = 0, 1
WIDE_MODES = {"waveform": WIDE_WAVEFORM, "envelope": WIDE_ENVELOPE}
WIDE_CHUNK = 248
WIDE_MAX_OFFSET = 1 << 20
WIDE_F_NONE, WIDE_F_RANGE, WIDE_F_EDGE = 1, 2, 4
WIDE_DELAY_DTYPE = np.dtype([("lag", "<i4"), ("coarse_lag", "<i4"), ("factor", "<u4"), ("flags", "<u4"),
                             ("fine", DELAY_DTYPE), ("coarse", DELAY_DTYPE)])


class Track(C.Structure):
    """mirrors peaq_track (include/peaq_amd.h)"""
    _fields_ = [("lag0", C.c_int32), ("flags", C.c_uint32), ("n_windows", C.c_uint32), ("n_valid", C.c_uint32),
                ("n_filled", C.c_uint32), ("n_segments", C.c_uint32), ("d_min", C.c_double), ("d_max", C.c_double),
                ("max_abs_e", C.c_double)]


# PEAQ_TRACK_* (include/peaq_amd.h), the record as a numpy structured dtype, and this binding's default window
TRACK_F_NONE, TRACK_F_RANGE = 1, 2
TRACK_MAX_E, TRACK_MAX_STEP, TRACK_MAX_SEGMENTS_PER_CALL = 1 / 64, 1 / 256, 1 << 20
TRACK_WINDOW = 16384
WINDOWS_MAX = 4096                                # peaq_batch_run_windows: windows per call (PEAQ_WINDOWS_MAX)
TRACK_DTYPE = np.dtype([("lag0", "<i4"), ("flags", "<u4"), ("n_windows", "<u4"), ("n_valid", "<u4"), ("n_filled", "<u4"),
                        ("n_segments", "<u4"), ("d_min", "<f8"), ("d_max", "<f8"), ("max_abs_e", "<f8")])


class StepCandidate(C.Structure):
    """mirrors peaq_step_candidate (include/peaq_amd.h)"""
    _fields_ = [("pair", C.c_uint32), ("lo", C.c_uint32), ("hi", C.c_uint32), ("LA", C.c_int32), ("LB", C.c_int32)]


class Step(C.Structure):
    """mirrors peaq_step (include/peaq_amd.h)"""
    _fields_ = [("pair", C.c_uint32), ("c", C.c_uint32), ("LA", C.c_int32), ("LB", C.c_int32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32), ("gain_left", C.c_double), ("gain_right", C.c_double), ("norm", C.c_double)]


class Pieces(C.Structure):
    """mirrors peaq_pieces (include/peaq_amd.h)"""
    _fields_ = [("flags", C.c_uint32), ("n_candidates", C.c_uint32), ("n_accepted", C.c_uint32), ("n_pieces", C.c_uint32),
                ("max_abs_e", C.c_double)]


# PEAQ_STEP_* and PEAQ_PIECES_* (include/peaq_amd.h), the records as numpy structured dtypes
STEP_F_NONE, STEP_F_SPAN, STEP_F_WEAK = 1, 2, 4
STEP_MAX_SPAN, STEP_MAX_L = 1 << 22, (1 << 20) + 16384
STEP_MIN_STEP, STEP_RATIO, STEP_MIN_GAIN = 0.75, 3.0, 0.0021
PIECES_F_RANGE, PIECES_MAX_PER_PAIR, PIECES_MAX_PER_CALL = 2, 8192, 1 << 20
STEP_CANDIDATE_DTYPE = np.dtype([("pair", "<u4"), ("lo", "<u4"), ("hi", "<u4"), ("LA", "<i4"), ("LB", "<i4")])
STEP_DTYPE = np.dtype([("pair", "<u4"), ("c", "<u4"), ("LA", "<i4"), ("LB", "<i4"), ("flags", "<u4"), ("reserved", "<u4"),
                       ("gain_left", "<f8"), ("gain_right", "<f8"), ("norm", "<f8")])
PIECES_DTYPE = np.dtype([("flags", "<u4"), ("n_candidates", "<u4"), ("n_accepted", "<u4"), ("n_pieces", "<u4"),
                         ("max_abs_e", "<f8")])


class FrameTrace(C.Structure):
    """mirrors peaq_frame_trace (include/peaq_amd.h)"""
    _fields_ = [("ch", (C.c_double * 6) * 2), ("p_detect", C.c_double), ("steps", C.c_double), ("flags", C.c_uint32),
                ("frame", C.c_uint32), ("reserved", C.c_double)]


class BlockTrace(C.Structure):
    """mirrors peaq_block_trace (include/peaq_amd.h)"""
    _fields_ = [("ch", (C.c_double * 5) * 2), ("flags", C.c_uint32), ("block", C.c_uint32), ("reserved", C.c_double)]


# PEAQ_TRACE_* (include/peaq_amd.h) and the records as numpy structured dtypes; the names of the values in `ch`
TRACE_ABOVE, TRACE_MOD_OPEN, TRACE_LOUD_OPEN, TRACE_FLUSH = 1, 2, 4, 8
FRAME_TRACE_DTYPE = np.dtype([("ch", "<f8", (2, 6)), ("p_detect", "<f8"), ("steps", "<f8"), ("flags", "<u4"),
                              ("frame", "<u4"), ("reserved", "<f8")])
BLOCK_TRACE_DTYPE = np.dtype([("ch", "<f8", (2, 5)), ("flags", "<u4"), ("block", "<u4"), ("reserved", "<f8")])
FRAME_TRACE_VALUES = ["moddiff1", "moddiff2", "tempwt", "noiseloud", "nmr_mean", "nmr_max"]
FRAME_TRACE_VALUES_ADVANCED = ["segnmr_db", "nmr_mean"]
BLOCK_TRACE_VALUES = ["rmsmoddiff", "tempwt", "noiseloud", "missing", "lindist"]

# PEAQ_BAND_* (include/peaq_amd.h) by name, in the order of their bits -- which is the order of the plane slots
BAND_PLANES = {"nmr": 1, "exc_ref": 2, "exc_test": 4, "detect": 8, "steps": 16}
# PEAQ_FB_BAND_* (include/peaq_amd.h) by name, in the order of their bits -- which is the order of the plane slots
FB_BAND_PLANES = {"moddiff": 0x1, "modwt": 0x2, "noiseloud": 0x4, "missing": 0x8, "lindist": 0x10, "unsm_ref": 0x20,
                  "unsm_test": 0x40, "exc_ref": 0x80, "exc_test": 0x100, "adapt_ref": 0x200, "adapt_test": 0x400,
                  "mod_ref": 0x800, "mod_test": 0x1000}
# PEAQ_PAT_BAND_* (include/peaq_amd.h) by name, in the order of their bits -- which is the order of the plane slots
PATTERN_BAND_PLANES = {"moddiff1": 0x1, "moddiff2": 0x2, "modwt": 0x4, "noiseloud": 0x8, "unsm_ref": 0x10,
                       "unsm_test": 0x20, "exc_ref": 0x40, "exc_test": 0x80, "adapt_ref": 0x100, "adapt_test": 0x200,
                       "mod_ref": 0x400, "mod_test": 0x800, "avgloud_ref": 0x1000}
# PEAQ_BAND_SUMMARY_* (include/peaq_amd.h) by name, in row order; the advanced version has the first four
BAND_SUMMARY_ROWS = ("nmr_sum", "nmr_max", "nmr_disturbed", "exc_ref_sum", "exc_test_sum", "moddiff1_wsum",
                     "moddiff2_wsum", "noiseloud_sum")
# PEAQ_FB_BAND_SUMMARY_* (include/peaq_amd.h) by name, in row order (advanced version, filter-bank path)
FB_BAND_SUMMARY_ROWS = ("exc_ref_sum", "exc_test_sum", "moddiff_wsum", "moddiff_sq", "noiseloud_sq", "missing_sq",
                        "lindist_sum")


class HostPair(C.Structure):
    """mirrors peaq_host_pair (include/peaq_amd.h)"""
    _fields_ = [("ref", C.c_void_p), ("test", C.c_void_p), ("n_ref", C.c_uint64), ("n_test", C.c_uint64)]


class HostSignal(C.Structure):
    """mirrors peaq_host_signal (include/peaq_amd.h)"""
    _fields_ = [("data", C.c_void_p), ("n", C.c_uint64)]


class HostTest(C.Structure):
    """mirrors peaq_host_test (include/peaq_amd.h)"""
    _fields_ = [("data", C.c_void_p), ("n", C.c_uint64), ("ref", C.c_uint32), ("reserved", C.c_uint32)]


class Feed(C.Structure):
    """mirrors peaq_feed (include/peaq_amd.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("format", C.c_int), ("channels", C.c_int), ("rate", C.c_uint32),
                ("align_max_lag", C.c_uint32), ("chunk_pairs", C.c_uint32)]


# PEAQ_PCM_* (include/peaq_amd.h) by name, and the numpy dtype a file's samples are held in (S24: its bytes)
PCM_FORMATS = {"u8": 0, "s16": 1, "s24": 2, "s32": 3, "f32": 4, "f64": 5}
PCM_DTYPES = {0: np.dtype(np.uint8), 1: np.dtype("<i2"), 2: np.dtype(np.uint8), 3: np.dtype("<i4"), 4: np.dtype("<f4"),
              5: np.dtype("<f8")}


class _Calibration(C.Structure):
    _fields_ = [("elapsed_ms", C.c_double), ("shader_clock_mhz", C.c_double), ("fp64_tflops", C.c_double),
                ("cycles_per_fma", C.c_double), ("max_clock_mhz", C.c_double), ("compute_units", C.c_int),
                ("ramp_clock_mhz", C.c_double), ("ramp_cycles_per_fma", C.c_double), ("event_fp64_tflops", C.c_double),
                ("simds_used", C.c_int), ("max_waves_on_a_simd", C.c_int), ("dispatch_spread_ms", C.c_double)]


class _Timing(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("frontend_ms", C.c_float), ("frontend_launches", C.c_int),
                ("backend_ms", C.c_float), ("backend_launches", C.c_int),
                ("fb_ms", C.c_float), ("fb_launches", C.c_int)]


_LIB = None


class MeterConfig(C.Structure):
    """peaq_meter_config: the meter's geometry in FFT frames"""
    _fields_ = [("window_frames", C.c_uint32), ("hop_frames", C.c_uint32), ("depth", C.c_uint32)]


class MeterReading(C.Structure):
    """peaq_meter_reading"""
    _fields_ = [("index", C.c_uint64), ("start", C.c_uint64), ("length", C.c_uint64), ("first_frame", C.c_uint32),
                ("n_frames", C.c_uint32), ("first_block", C.c_uint32), ("n_blocks", C.c_uint32),
                ("r", C.c_double * RESULT_DOUBLES)]


METER_MAX_OPEN, METER_MAX_DEPTH = 64, 4096
# the band meter (include/peaq_amd.h, "meter: band rows"): rows per channel and reading -- the first four of
# BAND_SUMMARY_ROWS --, and the narrower limits of the geometry with bands on
METER_BAND_ROWS, METER_BANDS_MAX_OPEN, METER_BANDS_MAX_DEPTH = 4, 16, 256


class LiveAlignConfig(C.Structure):
    """peaq_live_align_config: acquisition (max_lag, probe in samples) and watch (watch_frames in FFT frames)"""
    _fields_ = [("max_lag", C.c_uint32), ("probe", C.c_uint32), ("watch_frames", C.c_uint32), ("reserved", C.c_uint32)]


class LiveDelay(C.Structure):
    """peaq_live_delay"""
    _fields_ = [("acquired", C.c_int32), ("probe_ref", C.c_uint32), ("probe_test", C.c_uint32), ("skip_ref", C.c_uint32),
                ("skip_test", C.c_uint32), ("reserved", C.c_uint32), ("d", Delay)]


WATCH_LAGS = 31


class DelayWatch(C.Structure):
    """peaq_delay_watch"""
    _fields_ = [("index", C.c_uint64), ("first_frame", C.c_uint32), ("n_frames", C.c_uint32), ("offset", C.c_int32),
                ("reserved", C.c_int32), ("peak", C.c_double), ("runner_up", C.c_double), ("norm", C.c_double),
                ("e_ref", C.c_double), ("e_test", C.c_double), ("c", C.c_double * (2 * WATCH_LAGS + 1))]


class _BrokerStats(C.Structure):
    _fields_ = [("ticks", C.c_uint64), ("launches", C.c_uint64), ("frames", C.c_uint64),
                ("max_active", C.c_uint32), ("worker_failed", C.c_uint32),
                ("tick_host_us_max", C.c_double), ("tick_host_us_p99", C.c_double), ("tick_host_us_mean", C.c_double),
                ("tick_device_us_max", C.c_double), ("tick_device_us_p99", C.c_double), ("tick_device_us_mean", C.c_double),
                ("latency_us_max", C.c_double), ("latency_us_p99", C.c_double), ("latency_us_mean", C.c_double),
                ("latency_samples", C.c_uint64)]


def library_path():
    # PEAQ_AMD_LIB: development knob for A/B runs of kernel variants (tools/variants.sh); the
    # product is the in-tree libpeaq_amd.so
    return Path(os.environ["PEAQ_AMD_LIB"]) if os.environ.get("PEAQ_AMD_LIB") else PKG / "libpeaq_amd.so"


def build_library(verbose=False):
    """Compile the HIP sources for gfx950 (hipcc cross-compiles without a GPU)."""
    env = dict(os.environ)
    env.setdefault("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run(["make", "-C", str(PKG / "csrc"), "-j", "8"], env=env, capture_output=True, text=True)
    if verbose or r.returncode:
        print(r.stdout[-4000:], r.stderr[-4000:])
    if r.returncode:
        raise PeaqError("building libpeaq_amd.so failed")
    return library_path()


def load_library():
    """Load libpeaq_amd.so; never falls back to anything else."""
    global _LIB
    if _LIB is not None:
        return _LIB
    so = library_path()
    if not so.exists():
        raise PeaqError(f"{so} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(the HIP extension is required, there is no CPU path)")
    # PyTorch ships its own HIP runtime (torch/lib/libamdhip64.so); whichever copy is mapped first
    # serves the whole process, and torch finds no GPU when it is not its own.  This binding uses
    # torch for device memory and streams anyway, so let it load its runtime first.
    import torch  # noqa: F401
    L = C.CDLL(str(so))
    vp, dp, fp, u32p = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    L.peaq_last_error.restype = C.c_char_p
    L.peaq_version.restype = C.c_char_p
    L.peaq_frame_count.restype = C.c_uint32
    L.peaq_frame_count.argtypes = [C.c_uint64, C.c_uint64, C.c_int]
    L.peaq_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.peaq_ctx_destroy.argtypes = [vp]
    L.peaq_ctx_device.argtypes = [vp]
    L.peaq_settings_default.restype = None
    L.peaq_settings_default.argtypes = [C.POINTER(Settings)]
    L.peaq_ctx_set_settings.argtypes = [vp, C.POINTER(Settings)]
    L.peaq_ctx_get_settings.argtypes = [vp, C.POINTER(Settings)]
    L.peaq_ctx_set_fir_fp64.argtypes = [vp, C.c_int]
    L.peaq_ctx_get_fir_fp64.argtypes = [vp]
    L.peaq_ctx_set_fir_mode.argtypes = [vp, C.c_int]
    L.peaq_ctx_get_fir_mode.argtypes = [vp]
    L.peaq_session_create.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.POINTER(vp)]
    L.peaq_session_destroy.argtypes = [vp]
    L.peaq_session_push.argtypes = [vp, C.c_int, fp, C.c_size_t]
    L.peaq_session_flush.argtypes = [vp]
    L.peaq_session_results.argtypes = [vp, dp]
    L.peaq_session_reset.argtypes = [vp]
    L.peaq_session_set_level.argtypes = [vp, C.c_double]
    L.peaq_debug_backend.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp]
    L.peaq_debug_backend_plain.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp, C.c_int, C.c_int, dp, C.c_int, dp]
    if hasattr(L, "peaq_debug_backend_advanced"):
        L.peaq_debug_backend_advanced.argtypes = [vp, C.c_int, C.c_int, dp, C.c_int, dp, dp, dp, dp]
    L.peaq_batch_run.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_int, vp, vp, C.c_size_t,
                                 u32p, u32p, C.c_uint32, vp, vp]
    L.peaq_run_pair.argtypes = [vp, C.c_int, C.c_int, C.c_double, fp, C.c_size_t, fp, C.c_size_t, dp]
    L.peaq_batch_workspace_bytes.restype = C.c_size_t
    L.peaq_batch_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32]
    if hasattr(L, "peaq_batch_run_trajectory"):      # (A/B runs load older variant libraries through PEAQ_AMD_LIB)
        L.peaq_batch_run_trajectory.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_int, vp, vp, C.c_size_t,
                                                u32p, u32p, C.c_uint32, C.c_uint32, C.c_int, vp, vp, vp]
        L.peaq_batch_trajectory_workspace_bytes.restype = C.c_size_t
        L.peaq_batch_trajectory_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int]
        L.peaq_run_pair_trajectory.argtypes = [vp, C.c_int, C.c_int, C.c_double, fp, C.c_size_t, fp, C.c_size_t,
                                               C.c_uint32, C.c_int, dp, dp]
    if hasattr(L, "peaq_batch_run_trace"):           # (A/B runs load older variant libraries through PEAQ_AMD_LIB)
        L.peaq_batch_run_trace.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_int, vp, vp, C.c_size_t, u32p, u32p,
                                           C.c_uint32, vp, C.c_size_t, vp, C.c_size_t, vp, vp]
        L.peaq_trace_sizes.restype = C.c_size_t
        L.peaq_trace_sizes.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.peaq_run_pair_trace.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_uint32, C.c_uint32, fp, C.c_size_t, fp,
                                          C.c_size_t, vp, C.c_size_t, u32p, vp, C.c_size_t, u32p, C.POINTER(Delay), dp]
    if hasattr(L, "peaq_batch_run_bands"):           # (A/B runs load older variant libraries through PEAQ_AMD_LIB)
        L.peaq_band_count.argtypes = [C.c_int]
        L.peaq_band_row.argtypes = [C.c_int]
        L.peaq_band_tables.argtypes = [C.c_int, dp, dp]
        L.peaq_batch_run_bands.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_int, vp, vp, C.c_size_t, u32p, u32p,
                                           C.c_uint32, C.c_uint32, vp, C.c_size_t, vp, vp]
        L.peaq_run_pair_bands.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_uint32, C.c_uint32, fp, C.c_size_t, fp,
                                          C.c_size_t, C.c_uint32, vp, C.c_size_t, u32p, C.POINTER(Delay), dp]
    if hasattr(L, "peaq_batch_run_fb_bands"):        # (A/B runs load older variant libraries through PEAQ_AMD_LIB)
        L.peaq_fb_band_count.argtypes = []
        L.peaq_fb_band_tables.argtypes = [dp, dp]
        L.peaq_batch_run_fb_bands.argtypes = [vp, C.c_int, C.c_double, C.c_int, vp, vp, C.c_size_t, u32p, u32p,
                                              C.c_uint32, C.c_uint32, vp, C.c_size_t, vp, vp]
        L.peaq_run_pair_fb_bands.argtypes = [vp, C.c_int, C.c_double, C.c_uint32, C.c_uint32, fp, C.c_size_t, fp,
                                             C.c_size_t, C.c_uint32, vp, C.c_size_t, u32p, C.POINTER(Delay), dp]
    if hasattr(L, "peaq_batch_run_pattern_bands"):   # (A/B runs load older variant libraries through PEAQ_AMD_LIB)
        L.peaq_pattern_band_tables.argtypes = [dp, dp]
        L.peaq_batch_run_pattern_bands.argtypes = [vp, C.c_int, C.c_double, C.c_int, vp, vp, C.c_size_t, u32p, u32p,
                                                   C.c_uint32, C.c_uint32, vp, C.c_size_t, vp, vp]
        L.peaq_run_pair_pattern_bands.argtypes = [vp, C.c_int, C.c_double, C.c_uint32, C.c_uint32, fp, C.c_size_t, fp,
                                                  C.c_size_t, C.c_uint32, vp, C.c_size_t, u32p, C.POINTER(Delay), dp]
    if hasattr(L, "peaq_batch_run_band_summary"):    # (A/B runs load older variant libraries through PEAQ_AMD_LIB)
        L.peaq_band_summary_rows.argtypes = [C.c_int]
        L.peaq_batch_run_band_summary.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_int, vp, vp, C.c_size_t, u32p,
                                                  u32p, C.c_uint32, vp, vp, vp]
        L.peaq_run_pair_band_summary.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_uint32, C.c_uint32, fp, C.c_size_t,
                                                 fp, C.c_size_t, vp, C.POINTER(Delay), dp]
    if hasattr(L, "peaq_batch_run_windows"):           # (A/B runs load older variant libraries through PEAQ_AMD_LIB)
        L.peaq_window_frames.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u32p, u32p]
        L.peaq_batch_run_windows.argtypes = [vp, C.c_int, C.c_double, C.c_int, vp, vp, C.c_size_t, u32p, u32p, C.c_uint32,
                                             vp, C.c_int, vp, vp, vp]
        L.peaq_batch_windows_workspace_bytes.restype = C.c_size_t
        L.peaq_batch_windows_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_int]
        L.peaq_run_pair_windows.argtypes = [vp, C.c_int, C.c_double, C.c_uint32, C.c_uint32, fp, C.c_size_t, fp, C.c_size_t,
                                            vp, C.c_int, vp, C.POINTER(Delay), dp]
    if hasattr(L, "peaq_batch_run_adv_spans"):         # (A/B runs load older variant libraries through PEAQ_AMD_LIB)
        L.peaq_span_blocks.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u32p, u32p]
        L.peaq_batch_run_adv_spans.argtypes = [vp, C.c_int, C.c_double, C.c_int, vp, vp, C.c_size_t, u32p, u32p,
                                               C.c_uint32, vp, C.c_int, vp, vp, vp]
        L.peaq_batch_adv_spans_workspace_bytes.restype = C.c_size_t
        L.peaq_batch_adv_spans_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_int]
        L.peaq_run_pair_adv_spans.argtypes = [vp, C.c_int, C.c_double, C.c_uint32, C.c_uint32, fp, C.c_size_t, fp,
                                              C.c_size_t, vp, C.c_int, vp, C.POINTER(Delay), dp]
    if hasattr(L, "peaq_session_set_meter"):           # (A/B runs load older variant libraries through PEAQ_AMD_LIB)
        L.peaq_meter_reading_size.restype = C.c_size_t
        L.peaq_meter_reading_size.argtypes = []
        L.peaq_meter_frames.argtypes = [C.c_double, u32p]
        L.peaq_meter_readings.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(MeterConfig), C.POINTER(MeterReading), C.c_int,
                                         C.POINTER(C.c_int)]
        L.peaq_session_set_meter.argtypes = [vp, C.POINTER(MeterConfig)]
        L.peaq_session_meter_read.argtypes = [vp, C.POINTER(MeterReading), C.c_int, C.POINTER(C.c_int),
                                              C.POINTER(C.c_uint64)]
        L.peaq_broker_set_meter.argtypes = [vp, C.POINTER(MeterConfig)]
        L.peaq_broker_meter_read.argtypes = [vp, C.c_int, C.POINTER(MeterReading), C.c_int, C.POINTER(C.c_int),
                                             C.POINTER(C.c_uint64)]
        if L.peaq_meter_reading_size() != C.sizeof(MeterReading):
            raise PeaqError(f"peaq_meter_reading is {L.peaq_meter_reading_size()} bytes in the library, "
                            f"{C.sizeof(MeterReading)} in this binding")
    if hasattr(L, "peaq_session_set_meter_bands"):     # (A/B runs load older variant libraries through PEAQ_AMD_LIB)
        L.peaq_meter_band_rows.argtypes = []
        L.peaq_meter_bands_workspace.argtypes = [C.POINTER(MeterConfig), C.c_int, C.c_int, C.POINTER(C.c_size_t)]
        L.peaq_session_set_meter_bands.argtypes = [vp, C.c_int]
        L.peaq_session_meter_read_bands.argtypes = [vp, C.POINTER(MeterReading), dp, C.c_int, C.POINTER(C.c_int),
                                                    C.POINTER(C.c_uint64)]
        L.peaq_broker_set_meter_bands.argtypes = [vp, C.c_int]
        L.peaq_broker_meter_read_bands.argtypes = [vp, C.c_int, C.POINTER(MeterReading), dp, C.c_int, C.POINTER(C.c_int),
                                                   C.POINTER(C.c_uint64)]
    if hasattr(L, "peaq_session_set_align"):           # (A/B runs load older variant libraries through PEAQ_AMD_LIB)
        i32p = C.POINTER(C.c_int32)
        L.peaq_live_delay_size.restype = C.c_size_t
        L.peaq_live_delay_size.argtypes = []
        L.peaq_delay_watch_size.restype = C.c_size_t
        L.peaq_delay_watch_size.argtypes = []
        L.peaq_live_align_plan.argtypes = [C.POINTER(LiveAlignConfig), C.c_uint64, C.c_uint64, C.c_int32, u32p, u32p, u32p,
                                           u32p]
        L.peaq_delay_watch_pick.argtypes = [dp, C.c_double, C.c_double, i32p, dp, dp, dp]
        L.peaq_session_set_align.argtypes = [vp, C.POINTER(LiveAlignConfig)]
        L.peaq_session_align_read.argtypes = [vp, C.POINTER(LiveDelay)]
        L.peaq_session_watch_read.argtypes = [vp, C.POINTER(DelayWatch)]
        L.peaq_broker_set_align.argtypes = [vp, C.POINTER(LiveAlignConfig)]
        L.peaq_broker_align_read.argtypes = [vp, C.c_int, C.POINTER(LiveDelay)]
        L.peaq_broker_watch_read.argtypes = [vp, C.c_int, C.POINTER(DelayWatch)]
        for what, size, mirror in (("peaq_live_delay", L.peaq_live_delay_size(), LiveDelay),
                                   ("peaq_delay_watch", L.peaq_delay_watch_size(), DelayWatch)):
            if size != C.sizeof(mirror):
                raise PeaqError(f"{what} is {size} bytes in the library, {C.sizeof(mirror)} in this binding")
    if hasattr(L, "peaq_batch_run_fb_band_summary"):   # (A/B runs load older variant libraries through PEAQ_AMD_LIB)
        L.peaq_fb_band_summary_rows.argtypes = []
        L.peaq_fb_band_summary_row.argtypes = []
        L.peaq_batch_run_fb_band_summary.argtypes = [vp, C.c_int, C.c_double, C.c_int, vp, vp, C.c_size_t, u32p, u32p,
                                                     C.c_uint32, vp, vp, vp]
        L.peaq_run_pair_fb_band_summary.argtypes = [vp, C.c_int, C.c_double, C.c_uint32, C.c_uint32, fp, C.c_size_t, fp,
                                                    C.c_size_t, vp, C.POINTER(Delay), dp]
    if hasattr(L, "peaq_batch_resample"):            # (A/B runs load older variant libraries through PEAQ_AMD_LIB)
        L.peaq_resample_supported.argtypes = [C.c_uint32]
        L.peaq_resampled_length.restype = C.c_uint32
        L.peaq_resampled_length.argtypes = [C.c_uint64, C.c_uint32]
        L.peaq_batch_resample.argtypes = [vp, C.c_int, C.c_uint32, C.c_int, vp, C.c_size_t, u32p, C.c_uint32,
                                          vp, C.c_size_t, u32p, vp]
        L.peaq_run_pair_rate.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_uint32, fp, C.c_size_t, fp, C.c_size_t, dp]
        L.peaq_resample_plan_info.argtypes = [C.c_uint32, C.POINTER(ResamplePlan)]
    if hasattr(L, "peaq_batch_resample_range"):      # (A/B runs load older variant libraries through PEAQ_AMD_LIB)
        L.peaq_rate_segment_size.restype = C.c_size_t
        L.peaq_rate_segment_size.argtypes = []
        L.peaq_live_rate_ready.argtypes = [C.c_uint32, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
        L.peaq_live_rate_inputs.argtypes = [C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.peaq_batch_resample_range.argtypes = [vp, C.c_int, C.c_uint32, C.c_int, C.POINTER(RateSegment), vp, C.c_size_t,
                                                vp, C.c_size_t, vp]
        L.peaq_session_set_rates.argtypes = [vp, C.c_uint32, C.c_uint32]
        L.peaq_broker_set_rates.argtypes = [vp, C.c_uint32, C.c_uint32]
        if L.peaq_rate_segment_size() != C.sizeof(RateSegment):
            raise PeaqError(f"peaq_rate_segment is {L.peaq_rate_segment_size()} bytes in the library, "
                            f"{C.sizeof(RateSegment)} in this binding")
    if hasattr(L, "peaq_batch_estimate_delay"):      # (A/B runs load older variant libraries through PEAQ_AMD_LIB)
        L.peaq_batch_estimate_delay.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_size_t, u32p, u32p, C.c_uint32,
                                                C.c_uint32, vp, vp]
        L.peaq_align_workspace_bytes.restype = C.c_size_t
        L.peaq_align_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32]
        L.peaq_batch_cut.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t, u32p, u32p, vp, C.c_size_t, vp]
        L.peaq_aligned_lengths.restype = None
        L.peaq_aligned_lengths.argtypes = [C.c_int32, C.c_uint32, C.c_uint32, u32p, u32p, u32p]
        L.peaq_run_pair_aligned.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_uint32, C.c_uint32, fp, C.c_size_t,
                                            fp, C.c_size_t, C.POINTER(Delay), dp]
    L.peaq_pcm_sample_bytes.restype = C.c_size_t
    L.peaq_pcm_sample_bytes.argtypes = [C.c_int]
    L.peaq_feed_size.restype = C.c_size_t
    L.peaq_feed_size.argtypes = []
    L.peaq_batch_decode_pcm.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, u32p, C.c_uint32, vp, C.c_size_t, vp]
    L.peaq_batch_run_host.argtypes = [vp, C.c_int, C.c_double, C.POINTER(Feed), C.c_size_t, C.POINTER(HostPair), dp,
                                      C.POINTER(Delay)]
    L.peaq_feed_workspace_bytes.restype = C.c_size_t
    L.peaq_feed_workspace_bytes.argtypes = [C.POINTER(Feed), C.c_int, C.c_size_t, C.c_uint64]
    if hasattr(L, "peaq_batch_gather"):              # (A/B runs load older variant libraries through PEAQ_AMD_LIB)
        L.peaq_batch_gather.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, u32p, u32p, u32p, vp, C.c_size_t, vp]
        L.peaq_batch_run_host_refs.argtypes = [vp, C.c_int, C.c_double, C.POINTER(Feed), C.c_size_t, C.POINTER(HostSignal),
                                               C.c_size_t, C.POINTER(HostTest), dp, C.POINTER(Delay)]
        L.peaq_feed_refs_workspace_bytes.restype = C.c_size_t
        L.peaq_feed_refs_workspace_bytes.argtypes = [C.POINTER(Feed), C.c_int, C.c_size_t, C.c_size_t, C.c_uint64]
    if hasattr(L, "peaq_batch_measure_gain"):        # (A/B runs load older variant libraries through PEAQ_AMD_LIB)
        L.peaq_gain_size.restype = C.c_size_t
        L.peaq_gain_size.argtypes = []
        L.peaq_batch_measure_gain.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t, u32p, vp, C.c_size_t, u32p, u32p, C.c_int,
                                              C.c_double, vp, vp]
        L.peaq_gain_workspace_bytes.restype = C.c_size_t
        L.peaq_gain_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_uint32]
        L.peaq_batch_cut_scaled.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t, u32p, u32p, vp, vp, C.c_size_t, vp]
        L.peaq_run_pair_matched.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_uint32, C.c_uint32, C.c_int, C.c_double, fp,
                                            C.c_size_t, fp, C.c_size_t, C.POINTER(Delay), C.POINTER(Gain), dp]
        L.peaq_batch_run_host_matched.argtypes = [vp, C.c_int, C.c_double, C.POINTER(Feed), C.c_int, C.c_double, C.c_size_t,
                                                  C.POINTER(HostSignal), C.c_size_t, C.POINTER(HostTest), dp, C.POINTER(Delay),
                                                  C.POINTER(Gain)]
        L.peaq_feed_matched_workspace_bytes.restype = C.c_size_t
        L.peaq_feed_matched_workspace_bytes.argtypes = [C.POINTER(Feed), C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_uint64]
    if hasattr(L, "peaq_batch_refine_delay"):        # (A/B runs load older variant libraries through PEAQ_AMD_LIB)
        i32p = C.POINTER(C.c_int32)
        L.peaq_subdelay_size.restype = C.c_size_t
        L.peaq_subdelay_size.argtypes = []
        L.peaq_subsample_tables.argtypes = [dp, dp]
        L.peaq_batch_refine_delay.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_size_t, u32p, u32p, C.c_uint32, i32p, vp, vp]
        L.peaq_subdelay_workspace_bytes.restype = C.c_size_t
        L.peaq_subdelay_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_uint32]
        L.peaq_batch_cut_shifted.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t, u32p, u32p, u32p, i32p, vp, C.c_size_t, vp]
        L.peaq_run_pair_subsample.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_uint32, C.c_uint32, C.c_int, C.c_double, fp,
                                              C.c_size_t, fp, C.c_size_t, C.POINTER(Delay), C.POINTER(SubDelay),
                                              C.POINTER(Gain), dp]
    if hasattr(L, "peaq_batch_cut_drift"):           # (A/B runs load older variant libraries through PEAQ_AMD_LIB)
        i32p = C.POINTER(C.c_int32)
        L.peaq_drift_size.restype = C.c_size_t
        L.peaq_drift_size.argtypes = []
        L.peaq_drift_fit.argtypes = [dp, dp, C.POINTER(C.c_uint8), C.c_size_t, dp, dp]
        L.peaq_drift_index.restype = None
        L.peaq_drift_index.argtypes = [C.c_double, C.c_double, C.c_int64, C.POINTER(C.c_int64), i32p]
        L.peaq_drift_lengths.restype = None
        L.peaq_drift_lengths.argtypes = [C.c_int32, C.c_double, C.c_double, C.c_uint32, C.c_uint32, u32p, u32p, u32p]
        L.peaq_drift_windows.restype = C.c_uint32
        L.peaq_drift_windows.argtypes = [C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32]
        L.peaq_drift_workspace_bytes.restype = C.c_size_t
        L.peaq_drift_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32]
        L.peaq_batch_estimate_drift.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_size_t, u32p, u32p, C.c_uint32, i32p,
                                                C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_uint32, vp, vp,
                                                C.POINTER(Drift), vp]
        L.peaq_batch_cut_drift.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t, u32p, u32p, u32p, dp, dp, vp, C.c_size_t, vp]
        L.peaq_run_pair_drift.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                          C.c_double, fp, C.c_size_t, fp, C.c_size_t, C.POINTER(Delay), C.POINTER(Drift),
                                          C.POINTER(Gain), dp]
    if hasattr(L, "peaq_batch_cut_track"):           # (A/B runs load older variant libraries through PEAQ_AMD_LIB)
        i32p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
        L.peaq_track_size.restype = C.c_size_t
        L.peaq_track_size.argtypes = []
        L.peaq_track_fit.argtypes = [dp, u8p, C.c_uint32, C.c_uint32, C.c_double, C.POINTER(Track), dp, dp, dp]
        L.peaq_track_segment.restype = C.c_uint32
        L.peaq_track_segment.argtypes = [C.c_int64, C.c_uint32, C.c_uint32]
        L.peaq_track_index.restype = None
        L.peaq_track_index.argtypes = [C.c_uint32, C.c_uint32, dp, dp, C.c_int64, C.POINTER(C.c_int64), i32p]
        L.peaq_track_lengths.restype = None
        L.peaq_track_lengths.argtypes = [C.c_int32, C.c_uint32, C.c_uint32, dp, dp, C.c_uint32, C.c_uint32, u32p, u32p, u32p]
        L.peaq_batch_estimate_track.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_size_t, u32p, u32p, C.c_uint32, i32p,
                                                C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_uint32, vp, vp,
                                                C.POINTER(Drift), C.POINTER(Track), dp, C.c_uint32, dp, dp, vp]
        L.peaq_batch_cut_track.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t, u32p, u32p, u32p, C.c_uint32, u32p,
                                           C.c_uint32, dp, dp, vp, C.c_size_t, vp]
        L.peaq_run_pair_track.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                          C.c_double, fp, C.c_size_t, fp, C.c_size_t, C.POINTER(Delay), C.POINTER(Track),
                                          C.POINTER(Gain), dp]
    if hasattr(L, "peaq_batch_cut_pieces"):          # (A/B runs load older variant libraries through PEAQ_AMD_LIB)
        i32p = C.POINTER(C.c_int32)
        for f in (L.peaq_step_candidate_size, L.peaq_step_size, L.peaq_pieces_size):
            f.restype = C.c_size_t
            f.argtypes = []
        L.peaq_steps_workspace_bytes.restype = C.c_size_t
        L.peaq_steps_workspace_bytes.argtypes = [C.c_int, C.c_uint32]
        L.peaq_batch_locate_steps.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_size_t, u32p, u32p, C.c_uint32, i32p, C.c_int,
                                              C.POINTER(StepCandidate), vp, vp]
        L.peaq_steps_candidates.argtypes = [dp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double,
                                            C.POINTER(StepCandidate), u32p]
        L.peaq_steps_fit.argtypes = [dp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_double,
                                     C.POINTER(Step), C.c_uint32, C.POINTER(Pieces), u32p, dp, dp]
        L.peaq_pieces_index.restype = None
        L.peaq_pieces_index.argtypes = [C.c_uint32, u32p, dp, dp, C.c_int64, C.POINTER(C.c_int64), i32p]
        L.peaq_pieces_lengths.restype = None
        L.peaq_pieces_lengths.argtypes = [C.c_int32, C.c_uint32, u32p, dp, dp, C.c_uint32, C.c_uint32, u32p, u32p, u32p]
        L.peaq_batch_estimate_steps.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_size_t, u32p, u32p, C.c_uint32, i32p,
                                                C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_double,
                                                C.c_double, C.c_uint32, vp, vp, C.POINTER(Drift), C.POINTER(Track), dp,
                                                C.c_uint32, C.POINTER(Step), C.POINTER(Pieces), C.c_uint32, u32p, dp, dp, vp]
        L.peaq_batch_cut_pieces.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t, u32p, u32p, u32p, u32p, C.c_uint32, u32p,
                                            dp, dp, vp, C.c_size_t, vp]
        L.peaq_run_pair_steps.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                          C.c_double, fp, C.c_size_t, fp, C.c_size_t, C.POINTER(Delay), C.POINTER(Track),
                                          C.POINTER(Pieces), C.POINTER(Step), C.c_uint32, C.POINTER(Gain), dp]
    L.peaq_batch_last_timing.argtypes = [vp, C.POINTER(_Timing)]
    if hasattr(L, "peaq_calibrate"):                 # (A/B runs load older variant libraries through PEAQ_AMD_LIB)
        L.peaq_calibrate.argtypes = [vp, C.c_int, C.POINTER(_Calibration)]
        L.peaq_batch_last_clock.argtypes = [vp, dp]
    L.peaq_synth_fill.argtypes = [vp, C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_size_t, vp, vp, vp]
    L.peaq_debug_frontend.argtypes = [vp, C.c_int, C.c_int, C.c_double, vp, vp, C.c_uint32, C.c_uint32,
                                      C.c_int, dp]
    L.peaq_debug_filterbank.argtypes = [vp, C.c_int, C.c_double, vp, vp, C.c_uint32, C.c_uint32, C.c_int, C.c_int, dp]
    if hasattr(L, "peaq_debug_wave"):                # (A/B runs load older variant libraries through PEAQ_AMD_LIB)
        L.peaq_debug_wave.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_int, dp, C.c_int, dp, C.c_int, dp]
        L.peaq_debug_common_tables.argtypes = [dp, dp]
    if hasattr(L, "peaq_batch_decimate"):            # (A/B runs load older variant libraries through PEAQ_AMD_LIB)
        L.peaq_wide_delay_size.restype = C.c_size_t
        L.peaq_wide_factor.restype = C.c_uint32
        L.peaq_wide_factor.argtypes = [C.c_uint32]
        L.peaq_wide_taps.argtypes = [C.c_uint32, dp]
        L.peaq_batch_decimate.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t, u32p, C.c_uint32, C.c_uint32, C.c_int, vp,
                                          C.c_size_t, vp]
        L.peaq_batch_estimate_delay_wide.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_size_t, u32p, u32p, C.c_uint32,
                                                     C.c_uint32, C.c_int, C.c_uint32, C.POINTER(WideDelay), vp]
        L.peaq_wide_workspace_bytes.restype = C.c_size_t
        L.peaq_wide_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32]
        L.peaq_run_pair_wide.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, fp,
                                         C.c_size_t, fp, C.c_size_t, C.POINTER(WideDelay), dp]
    ip = C.POINTER(C.c_int)
    L.peaq_broker_create.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_int, C.POINTER(vp)]
    L.peaq_broker_create_multi.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, vp, C.c_int,
                                           C.POINTER(vp)]
    L.peaq_broker_devices.argtypes = [vp]
    if hasattr(L, "peaq_debug_broker_fail_shard"):
        L.peaq_debug_broker_fail_shard.argtypes = [vp, C.c_int, C.c_char_p]
    L.peaq_broker_stats_size.argtypes = []
    L.peaq_broker_stats_size.restype = C.c_size_t
    L.peaq_broker_destroy.argtypes = [vp]
    L.peaq_broker_destroy.restype = None
    L.peaq_broker_open.argtypes = [vp, ip]
    L.peaq_broker_close.argtypes = [vp, C.c_int]
    L.peaq_broker_push.argtypes = [vp, C.c_int, C.c_int, fp, C.c_size_t]
    L.peaq_broker_flush.argtypes = [vp, C.c_int]
    L.peaq_broker_tick.argtypes = [vp, C.POINTER(C.c_uint)]
    L.peaq_broker_results.argtypes = [vp, C.c_int, dp]
    L.peaq_broker_start.argtypes = [vp, C.c_uint]
    L.peaq_broker_stop.argtypes = [vp]
    L.peaq_broker_stats.argtypes = [vp, C.POINTER(_BrokerStats)]
    _LIB = L
    return L


def _check(rc):
    if rc != 0:
        raise PeaqError(f"libpeaq_amd error {rc}: {load_library().peaq_last_error().decode()}")


def _result_dict(row, advanced):
    n = 5 if advanced else 11
    return dict(movs=np.array(row[:n]), di=float(row[11]), odg=float(row[12]), totalsnr=float(row[13]),
                frames=int(row[14]), fb_blocks=int(row[15]))


_METER_FIELDS = ("index", "start", "length", "first_frame", "n_frames", "first_block", "n_blocks")


def _meter_dict(row, advanced=None):
    """a peaq_meter_reading as a dict; advanced = None: the row's own fields only (peaq_meter_readings leaves r alone)"""
    d = {k: int(getattr(row, k)) for k in _METER_FIELDS}
    if advanced is not None:
        d.update(_result_dict(np.array(row.r[:]), advanced))
    return d


def meter_frames(seconds):
    """peaq_meter_frames: seconds as FFT frames of the running stream, max(1, round(seconds * 48000 / 1024))"""
    f = C.c_uint32(0)
    _check(load_library().peaq_meter_frames(float(seconds), C.byref(f)))
    return f.value


def meter_windows(n_ref, n_test, window, hop=None):
    """peaq_meter_readings: the readings a metered stream of these lengths delivers up to and at its flush, as dicts of
    index, first_frame, n_frames, first_block, n_blocks and the equivalent batch window / span {start, length}
    (length 0: none has exactly these frames).  Host arithmetic only."""
    L = load_library()
    cfg = MeterConfig(int(window), int(window if hop is None else hop), 1)
    n = C.c_int(0)
    _check(L.peaq_meter_readings(int(n_ref), int(n_test), C.byref(cfg), None, 0, C.byref(n)))
    rows = (MeterReading * max(n.value, 1))()
    _check(L.peaq_meter_readings(int(n_ref), int(n_test), C.byref(cfg), rows, n.value, C.byref(n)))
    return [_meter_dict(rows[i]) for i in range(n.value)]


def meter_bands_workspace(window, hop=None, depth=64, advanced=False, channels=2):
    """peaq_meter_bands_workspace: the device bytes the band meter adds to a session of this geometry (a broker slot
    holds 8 frames of planes in place of 64).  Host arithmetic only; refuses what set_meter(..., bands=True) refuses."""
    cfg = MeterConfig(int(window), int(window if hop is None else hop), int(depth))
    n = C.c_size_t(0)
    _check(load_library().peaq_meter_bands_workspace(C.byref(cfg), int(bool(advanced)), int(channels), C.byref(n)))
    return n.value


def _meter_read(L, read, read_bands, advanced, channels, cap, bands):
    """the common body of Session.meter_read and Broker.meter_read; read / read_bands: the entry with its handle bound"""
    rows = (MeterReading * cap)()
    n, dropped = C.c_int(0), C.c_uint64(0)
    if not bands:
        _check(read(rows, int(cap), C.byref(n), C.byref(dropped)))
        return [_meter_dict(rows[i], advanced) for i in range(n.value)], dropped.value
    row = L.peaq_band_row(int(advanced))
    nb = L.peaq_band_count(int(advanced))
    band_rows = np.zeros((cap, channels, METER_BAND_ROWS, row))
    _check(read_bands(rows, band_rows.ctypes.data_as(C.POINTER(C.c_double)), int(cap), C.byref(n), C.byref(dropped)))
    out = []
    for i in range(n.value):
        d = _meter_dict(rows[i], advanced)
        d["bands"] = band_rows[i].copy()
        for k, name in enumerate(BAND_SUMMARY_ROWS[:METER_BAND_ROWS]):
            d[name] = d["bands"][:, k, :nb]
        d["counted"] = d["bands"][:, 0, nb].astype(np.int64)
        out.append(d)
    return out, dropped.value


def _align_config(max_lag, probe, watch):
    return LiveAlignConfig(int(max_lag or 0), int(probe or 0), int(watch or 0), 0)


def _live_delay_dict(d):
    return dict(acquired=bool(d.acquired), probe_ref=int(d.probe_ref), probe_test=int(d.probe_test),
                skip_ref=int(d.skip_ref), skip_test=int(d.skip_test), lag=int(d.d.lag), peak=float(d.d.peak),
                runner_up=float(d.d.runner_up), norm=float(d.d.norm))


def _watch_dict(w):
    if not w.n_frames:
        return None
    return dict(index=int(w.index), first_frame=int(w.first_frame), n_frames=int(w.n_frames), offset=int(w.offset),
                peak=float(w.peak), runner_up=float(w.runner_up), norm=float(w.norm), e_ref=float(w.e_ref),
                e_test=float(w.e_test), c=np.array(w.c[:]))


def live_align_plan(max_lag, have_ref, have_test, lag, probe=None):
    """peaq_live_align_plan: (probe_ref, probe_test, skip_ref, skip_test) of rule A for what the pads hold and a lag.
    Host arithmetic only."""
    cfg = _align_config(max_lag, probe, 0)
    out = [C.c_uint32(0) for _ in range(4)]
    _check(load_library().peaq_live_align_plan(C.byref(cfg), int(have_ref), int(have_test), int(lag),
                                               *[C.byref(o) for o in out]))
    return tuple(o.value for o in out)


def delay_watch_pick(c, e_ref, e_test):
    """peaq_delay_watch_pick: dict of offset, peak, runner_up, norm for a watch window's sums c[d + 31], d = -31 .. 31"""
    c = np.ascontiguousarray(c, dtype=np.float64)
    assert c.shape == (2 * WATCH_LAGS + 1,)
    offset, out = C.c_int32(0), [C.c_double(0) for _ in range(3)]
    _check(load_library().peaq_delay_watch_pick(c.ctypes.data_as(C.POINTER(C.c_double)), float(e_ref), float(e_test),
                                                C.byref(offset), *[C.byref(o) for o in out]))
    return dict(offset=offset.value, peak=out[0].value, runner_up=out[1].value, norm=out[2].value)


class Context:
    """One per process and GPU: owns the constant tables in HBM."""

    def __init__(self, device=0):
        self.L = load_library()
        self.h = C.c_void_p()
        _check(self.L.peaq_ctx_create(int(device), C.byref(self.h)))
        self.device = device

    def close(self):
        if self.h:
            self.L.peaq_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_settings(self, **changed):
        """the reference's settings.h switches by name (include/peaq_amd.h peaq_settings); unnamed ones get
        the shipped values, no argument restores all of them.  Applies to batch calls made and to sessions /
        brokers created afterwards."""
        st = Settings()
        self.L.peaq_settings_default(C.byref(st))
        for k, v in changed.items():
            if k not in dict(Settings._fields_):
                raise PeaqError(f"unknown setting {k}")
            setattr(st, k, int(v))
        _check(self.L.peaq_ctx_set_settings(self.h, C.byref(st)))

    def settings(self):
        st = Settings()
        _check(self.L.peaq_ctx_get_settings(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in Settings._fields_}

    def set_fir_fp64(self, enable):
        """advanced version: True = every stage FP64, FIR bank on the FP64 matrix instruction (the engine's default);
        False = the opt-in split-FP16 FIR (see include/peaq_amd.h PEAQ_FIR_*)"""
        _check(self.L.peaq_ctx_set_fir_fp64(self.h, int(bool(enable))))

    def set_fir_mode(self, mode):
        """'f32' | 'f64' | 'f16x3' (include/peaq_amd.h PEAQ_FIR_*)"""
        _check(self.L.peaq_ctx_set_fir_mode(self.h, {"f32": 0, "f64": 1, "f16x3": 2}[mode]))

    def fir_mode(self):
        return ("f32", "f64", "f16x3")[self.L.peaq_ctx_get_fir_mode(self.h)]

    def fir_fp64(self):
        return bool(self.L.peaq_ctx_get_fir_fp64(self.h))

    def last_timing(self):
        t = _Timing()
        _check(self.L.peaq_batch_last_timing(self.h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in _Timing._fields_}

    def last_clock_mhz(self):
        """shader clock while the last batch ran (peaq_batch_last_clock)"""
        if not hasattr(self.L, "peaq_batch_last_clock"):
            return 0.0
        v = C.c_double(0.)
        _check(self.L.peaq_batch_last_clock(self.h, C.byref(v)))
        return v.value

    def calibrate(self, iterations=0):
        """peaq_calibrate: shader clock and FP64 rate of this device under a fixed FP64 load (include/peaq_amd.h)"""
        if not hasattr(self.L, "peaq_calibrate"):
            return None
        t = _Calibration()
        _check(self.L.peaq_calibrate(self.h, int(iterations), C.byref(t)))
        return {k: getattr(t, k) for k, _ in _Calibration._fields_}


class Session:
    """Streaming session = one `peaq` element instance (host buffers in, results out)."""

    def __init__(self, ctx, advanced, channels, playback_level=92.0, rates=(48000, 48000)):
        """rates: the sampling rates of the (ref, test) pads, see set_rates"""
        self.ctx, self.advanced, self.channels = ctx, bool(advanced), channels
        self.L = ctx.L
        self.h = C.c_void_p()
        _check(self.L.peaq_session_create(ctx.h, int(advanced), int(channels), float(playback_level),
                                          C.byref(self.h)))
        if tuple(rates) != (48000, 48000):
            self.set_rates(*rates)

    def set_rates(self, rate_ref, rate_test=None):
        """peaq_session_set_rates: the pads take samples at these rates and convert them to 48 kHz on the device, as
        resample does for a whole signal (rate_test None: the same as rate_ref; 48000: that pad as it is).  Before the
        first push or right after reset() only; reset() keeps the rates."""
        _check(self.L.peaq_session_set_rates(self.h, int(rate_ref), int(rate_ref if rate_test is None else rate_test)))

    def push(self, pad, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        _check(self.L.peaq_session_push(self.h, int(pad), x.ctypes.data_as(C.POINTER(C.c_float)),
                                        x.size // self.channels))

    def push_ref(self, x):
        self.push(0, x)

    def push_test(self, x):
        self.push(1, x)

    def flush(self):
        _check(self.L.peaq_session_flush(self.h))

    def set_level(self, playback_level):
        _check(self.L.peaq_session_set_level(self.h, float(playback_level)))

    def results(self):
        out = np.zeros(RESULT_DOUBLES)
        _check(self.L.peaq_session_results(self.h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return _result_dict(out, self.advanced)

    def reset(self):
        """peaq_session_reset: the stream starts over; a meter that is set starts over with it"""
        _check(self.L.peaq_session_reset(self.h))

    def set_meter(self, window, hop=None, depth=64, bands=False):
        """peaq_session_set_meter: sliding-window readings of `window` FFT frames every `hop` (default: window), the
        `depth` newest kept (meter_frames converts seconds).  window = 0 or None switches the meter off.  Before the
        first push or right after reset() only.  bands: the band meter as well (peaq_session_set_meter_bands: at most
        METER_BANDS_MAX_OPEN windows open at once, depth at most METER_BANDS_MAX_DEPTH)."""
        if not window:
            _check(self.L.peaq_session_set_meter(self.h, None))
            self._meter_depth = 0
            return
        cfg = MeterConfig(int(window), int(window if hop is None else hop), int(depth))
        _check(self.L.peaq_session_set_meter(self.h, C.byref(cfg)))
        self._meter_depth = int(depth)
        if bands:
            self.set_meter_bands(True)

    def set_meter_bands(self, on=True):
        """peaq_session_set_meter_bands: the band rows of every reading on or off; after set_meter, which switches
        them off"""
        _check(self.L.peaq_session_set_meter_bands(self.h, int(bool(on))))

    def meter_read(self, cap=None, bands=False):
        """(readings, dropped): the delivered, not yet read readings, oldest first -- each a dict of the result's
        fields plus index, start, length, first_frame, n_frames, first_block, n_blocks -- and how many were lost since
        the previous read (peaq_session_meter_read).  cap: at most so many (default: the depth that was set).
        bands (peaq_session_meter_read_bands; the band meter must be on): every dict also has "bands", ndarray
        [channels, 4, row], its named views nmr_sum, nmr_max, nmr_disturbed, exc_ref_sum [channels, bands] and
        counted [channels], the window's counted frames."""
        cap = max(1, getattr(self, "_meter_depth", 0)) if cap is None else int(cap)
        return _meter_read(self.L, lambda *a: self.L.peaq_session_meter_read(self.h, *a),
                           lambda *a: self.L.peaq_session_meter_read_bands(self.h, *a), self.advanced, self.channels,
                           cap, bands)

    def set_align(self, max_lag, probe=None, watch=None):
        """peaq_session_set_align: hold the stream until both pads have `probe` samples (default 48000 + 2 max_lag),
        find the delay within +-max_lag and drop the early pad's head (max_lag 0 or None: no acquisition); watch the
        delay over tumbling windows of `watch` FFT frames (0 or None: no watch; meter_frames converts seconds).  Before
        the first push or right after reset() only."""
        cfg = _align_config(max_lag, probe, watch)
        _check(self.L.peaq_session_set_align(self.h, C.byref(cfg)))

    def align_read(self):
        """peaq_session_align_read: dict of acquired (False while the stream holds), probe_ref, probe_test, skip_ref,
        skip_test and the aligner's lag, peak, runner_up, norm"""
        d = LiveDelay()
        _check(self.L.peaq_session_align_read(self.h, C.byref(d)))
        return _live_delay_dict(d)

    def watch_read(self):
        """peaq_session_watch_read: the newest complete watch window as a dict (index, first_frame, n_frames, offset,
        peak, runner_up, norm, e_ref, e_test, c: array of 63), or None while no window is complete"""
        w = DelayWatch()
        _check(self.L.peaq_session_watch_read(self.h, C.byref(w)))
        return _watch_dict(w)

    def close(self):
        if self.h:
            self.L.peaq_session_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Broker:
    """Many live sessions (one per hosted `peaq` element), one batched launch per tick."""

    def __init__(self, ctx, channels, max_sessions, playback_level=92.0, advanced=False, devices=None, fir_mode=None,
                 rates=None):
        """devices = None: one broker on ctx's GPU.  devices = [ordinals]: peaq_broker_create_multi -- one device
        broker (with a context of its own) per entry, sessions dealt out to the least loaded; ctx only lends the
        loaded library then.  rates: the sampling rates of the (ref, test) pads of every session, see set_rates."""
        self.ctx, self.channels, self.advanced = ctx, channels, bool(advanced)
        self.L = ctx.L
        self.h = C.c_void_p()
        if devices is None:
            _check(self.L.peaq_broker_create(ctx.h, int(bool(advanced)), int(channels), float(playback_level),
                                             int(max_sessions), C.byref(self.h)))
        else:
            assert self.L.peaq_broker_stats_size() == C.sizeof(_BrokerStats)
            arr = (C.c_int * len(devices))(*[int(d) for d in devices])
            mode = -1 if fir_mode is None else FIR_MODES[fir_mode]
            _check(self.L.peaq_broker_create_multi(arr, len(devices), int(bool(advanced)), int(channels),
                                                   float(playback_level), int(max_sessions), None, mode, C.byref(self.h)))
        if rates is not None:
            self.set_rates(*rates)

    def set_rates(self, rate_ref, rate_test=None):
        """peaq_broker_set_rates: one pair of rates for all sessions of the broker (see Session.set_rates), before the
        first open() and before start()"""
        _check(self.L.peaq_broker_set_rates(self.h, int(rate_ref), int(rate_ref if rate_test is None else rate_test)))

    def devices(self):
        return int(self.L.peaq_broker_devices(self.h))

    def fail_shard(self, shard, message):
        """test hook (peaq_debug_broker_fail_shard): one device's share stops as after a device error"""
        _check(self.L.peaq_debug_broker_fail_shard(self.h, int(shard), message.encode()))

    def open(self):
        sid = C.c_int(-1)
        _check(self.L.peaq_broker_open(self.h, C.byref(sid)))
        return sid.value

    def close_session(self, sid):
        _check(self.L.peaq_broker_close(self.h, int(sid)))

    def push(self, sid, pad, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        _check(self.L.peaq_broker_push(self.h, int(sid), int(pad), x.ctypes.data_as(C.POINTER(C.c_float)),
                                       x.size // self.channels))

    def flush(self, sid):
        _check(self.L.peaq_broker_flush(self.h, int(sid)))

    def tick(self):
        n = C.c_uint(0)
        _check(self.L.peaq_broker_tick(self.h, C.byref(n)))
        return n.value

    def results(self, sid):
        out = np.zeros(RESULT_DOUBLES)
        _check(self.L.peaq_broker_results(self.h, int(sid), out.ctypes.data_as(C.POINTER(C.c_double))))
        return _result_dict(out, self.advanced)

    def set_meter(self, window, hop=None, depth=64, bands=False):
        """peaq_broker_set_meter: one geometry for all sessions of the broker (see Session.set_meter), before the first
        open() and before start().  bands: the band meter as well (peaq_broker_set_meter_bands)."""
        self._meter_depth = int(depth) if window else 0
        if not window:
            _check(self.L.peaq_broker_set_meter(self.h, None))
            return
        cfg = MeterConfig(int(window), int(window if hop is None else hop), int(depth))
        _check(self.L.peaq_broker_set_meter(self.h, C.byref(cfg)))
        if bands:
            self.set_meter_bands(True)

    def set_meter_bands(self, on=True):
        """peaq_broker_set_meter_bands: the band rows of every slot's readings on or off; after set_meter"""
        _check(self.L.peaq_broker_set_meter_bands(self.h, int(bool(on))))

    def meter_read(self, sid, cap=None, bands=False):
        """(readings, dropped) of session sid, as Session.meter_read: what was delivered up to the last tick; no tick
        is forced (peaq_broker_meter_read, with bands peaq_broker_meter_read_bands)"""
        cap = max(1, getattr(self, "_meter_depth", 0)) if cap is None else int(cap)
        return _meter_read(self.L, lambda *a: self.L.peaq_broker_meter_read(self.h, int(sid), *a),
                           lambda *a: self.L.peaq_broker_meter_read_bands(self.h, int(sid), *a), self.advanced,
                           self.channels, cap, bands)

    def set_align(self, max_lag, probe=None, watch=None):
        """peaq_broker_set_align: one configuration for all sessions of the broker (see Session.set_align), before the
        first open() and before start()"""
        cfg = _align_config(max_lag, probe, watch)
        _check(self.L.peaq_broker_set_align(self.h, C.byref(cfg)))

    def align_read(self, sid):
        """the delay of session sid, as Session.align_read (peaq_broker_align_read): as of the last tick; a session
        that still holds with its flush requested is ticked until it is acquired"""
        d = LiveDelay()
        _check(self.L.peaq_broker_align_read(self.h, int(sid), C.byref(d)))
        return _live_delay_dict(d)

    def watch_read(self, sid):
        """the newest complete watch window of session sid, as Session.watch_read (peaq_broker_watch_read): as of the
        last tick; no tick is forced"""
        w = DelayWatch()
        _check(self.L.peaq_broker_watch_read(self.h, int(sid), C.byref(w)))
        return _watch_dict(w)

    def start(self, period_us=2000):
        _check(self.L.peaq_broker_start(self.h, int(period_us)))

    def stop(self):
        _check(self.L.peaq_broker_stop(self.h))

    def stats(self):
        st = _BrokerStats()
        _check(self.L.peaq_broker_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in _BrokerStats._fields_}

    def close(self):
        if self.h:
            self.L.peaq_broker_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _torch_stream(stream):
    """context manager that makes `stream` (None, a torch.cuda.Stream or a raw hipStream_t) torch's current stream:
    tensors made inside are filled, and later recycled by the caching allocator, in that stream's order"""
    import contextlib
    import torch
    if stream is None:
        return contextlib.nullcontext()
    if not hasattr(stream, "cuda_stream"):
        stream = torch.cuda.ExternalStream(int(stream))
    return torch.cuda.stream(stream)


def _stream_ptr(stream):
    if stream is None:
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return C.c_void_p(int(getattr(stream, "cuda_stream", stream)))   # torch.cuda.Stream or a raw hipStream_t


def resample_supported(rate):
    """True if the device converter takes this sampling rate (peaq_resample_supported)"""
    return bool(load_library().peaq_resample_supported(int(rate)))


def resample_plan(rate):
    """peaq_resample_plan_info as a dict: what the device converter does for `rate` (host arithmetic, no GPU)"""
    pl = ResamplePlan()
    _check(load_library().peaq_resample_plan_info(int(rate), C.byref(pl)))
    return {k: getattr(pl, k) for k, _ in ResamplePlan._fields_}


def resampled_length(n, rate):
    """samples per channel at 48 kHz of n samples per channel at `rate` (peaq_resampled_length)"""
    L = load_library()
    v = L.peaq_resampled_length(int(n), int(rate))
    if v == 0 and n and L.peaq_last_error():
        raise PeaqError(L.peaq_last_error().decode())
    return int(v)


def resample(ctx, x, rate, n=None, out=None, stream=None):
    """Converts x, a CUDA float32 tensor [n_pairs, n_samples, channels] sampled at `rate`, to 48 kHz on the device
    (peaq_batch_resample).  n: optional per-pair lengths.  out: optional tensor [n_pairs, stride, channels] to write into
    (samples past a pair's converted length keep what they held); without it a zero-filled one with an even stride is
    made.  Returns (y, n_out): the 48 kHz tensor and the converted lengths (numpy uint32 [n_pairs])."""
    import torch
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 3
    n_pairs, stride, channels = x.shape
    a_n = None if n is None else np.ascontiguousarray(n, dtype=np.uint32)
    if out is None:
        longest = resampled_length(int(a_n.max()) if a_n is not None and len(a_n) else (stride if a_n is None else 0), rate)
        o_stride = max(longest, 2)
        with _torch_stream(stream):                    # the zero fill runs on the stream the converter runs on
            out = torch.zeros((n_pairs, o_stride + (o_stride & 1), channels), dtype=torch.float32, device=x.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 3
    assert out.shape[0] == n_pairs and out.shape[2] == channels
    n_out = np.zeros(n_pairs, dtype=np.uint32)
    u32p = C.POINTER(C.c_uint32)
    _check(ctx.L.peaq_batch_resample(ctx.h, channels, int(rate), n_pairs, C.c_void_p(x.data_ptr()), stride,
                                     a_n.ctypes.data_as(u32p) if a_n is not None else None, stride,
                                     C.c_void_p(out.data_ptr()), out.shape[1], n_out.ctypes.data_as(u32p),
                                     _stream_ptr(stream)))
    return out, n_out


RATE_OPEN = 2**64 - 1   # in_total of a segment whose stream has not ended
RANGE_TILE = 256         # outputs a workgroup of resample_range_kernel takes (kRangeTile, csrc/peaq_live_rate.hip)


def live_rate_ready(rate, n_have, ended=False):
    """converted samples a stream at `rate` can deliver once n_have raw samples have arrived (peaq_live_rate_ready, host
    arithmetic): not ended, the outputs whose taps all lie below n_have; ended, resampled_length without its limit"""
    v = C.c_uint64(0)
    _check(load_library().peaq_live_rate_ready(int(rate), int(n_have), int(bool(ended)), C.byref(v)))
    return v.value


def live_rate_span(rate, out_first, out_count):
    """(in_first, in_end): the raw samples the outputs [out_first, out_first + out_count) read (peaq_live_rate_inputs,
    host arithmetic)"""
    a, b = C.c_uint64(0), C.c_uint64(0)
    _check(load_library().peaq_live_rate_inputs(int(rate), int(out_first), int(out_count), C.byref(a), C.byref(b)))
    return a.value, b.value


def resample_range(ctx, x, rate, segments, out=None, stream=None):
    """Converts runs of outputs of streams sampled at `rate` (peaq_batch_resample_range).  x: CUDA float32 tensor
    [n_segments, in_stride, channels], row i holding the raw samples [in_base, in_base + in_have) of segment i's
    stream.  segments: one (out_first, out_count, in_base, in_have, in_total) each, in_total None (or RATE_OPEN) while
    the stream has not ended.  out: optional tensor [n_segments, out_stride, channels]; without it a zero-filled one
    as long as the longest out_count (at least 1).  Returns out; row i holds the outputs in its first out_count
    samples."""
    import torch
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 3
    n_seg, in_stride, channels = x.shape
    assert len(segments) == n_seg
    arr = (RateSegment * max(n_seg, 1))()
    for i, (out_first, out_count, in_base, in_have, in_total) in enumerate(segments):
        arr[i] = RateSegment(int(out_first), int(in_base), RATE_OPEN if in_total is None else int(in_total),
                             int(out_count), int(in_have))
    if out is None:
        with _torch_stream(stream):
            out = torch.zeros((n_seg, max([int(s[1]) for s in segments] + [1]), channels), dtype=torch.float32,
                              device=x.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 3
    assert out.shape[0] == n_seg and out.shape[2] == channels
    _check(ctx.L.peaq_batch_resample_range(ctx.h, channels, int(rate), n_seg, arr, C.c_void_p(x.data_ptr()), in_stride,
                                           C.c_void_p(out.data_ptr()), out.shape[1], _stream_ptr(stream)))
    return out


def _to_48k(ctx, ref, test, n_ref, n_test, rate, stream):
    """both buffers of a batch at `rate` -> (ref, test, n_ref, n_test) at 48 kHz with one common stride"""
    import torch
    assert ref.shape == test.shape
    n_pairs, stride, channels = ref.shape
    if n_ref is None:
        n_ref = n_test = np.full(n_pairs, stride, dtype=np.uint32)
    longest = max([resampled_length(int(v), rate) for v in set(np.asarray(n_ref).tolist()) | set(np.asarray(n_test).tolist())] + [2])
    with _torch_stream(stream):                        # filled, and given back to the allocator, in `stream`'s order
        bufs = [torch.zeros((n_pairs, longest + (longest & 1), channels), dtype=torch.float32, device=ref.device)
                for _ in (0, 1)]
    _, o_ref = resample(ctx, ref, rate, n_ref, out=bufs[0], stream=stream)
    _, o_test = resample(ctx, test, rate, n_test, out=bufs[1], stream=stream)
    return bufs[0], bufs[1], o_ref, o_test


def aligned_lengths(lag, n_ref, n_test):
    """(skip_ref, skip_test, n_common) for one pair's lag (peaq_aligned_lengths, host arithmetic)"""
    sr, st, n = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    load_library().peaq_aligned_lengths(int(lag), int(n_ref), int(n_test), C.byref(sr), C.byref(st), C.byref(n))
    return sr.value, st.value, n.value


def align_workspace_bytes(channels, n_pairs, n_max, max_lag):
    """scratch of estimate_delay for a shape (peaq_align_workspace_bytes)"""
    return int(load_library().peaq_align_workspace_bytes(int(channels), int(n_pairs), int(n_max), int(max_lag)))


def estimate_delay(ctx, ref, test, max_lag, n_ref=None, n_test=None, stream=None):
    """Delay of every pair of a batch (peaq_batch_estimate_delay): ref/test CUDA float32 [n_pairs, n_samples, channels],
    n_ref/n_test optional per-pair lengths.  Returns a dict of numpy arrays [n_pairs]: lag (int32; positive: the test
    signal is late), peak, runner_up, norm.  Synchronises the stream it ran on."""
    import torch
    assert ref.is_cuda and test.is_cuda and ref.dtype == torch.float32 and test.dtype == torch.float32
    assert ref.is_contiguous() and test.is_contiguous() and ref.shape == test.shape and ref.dim() == 3
    n_pairs, stride, channels = ref.shape
    assert (n_ref is None) == (n_test is None), "n_ref and n_test: both or neither"
    a_ref = a_test = None
    if n_ref is not None:
        a_ref = np.ascontiguousarray(n_ref, dtype=np.uint32)
        a_test = np.ascontiguousarray(n_test, dtype=np.uint32)
        assert a_ref.shape == (n_pairs,) and a_test.shape == (n_pairs,)
    with _torch_stream(stream):
        rec = torch.zeros((max(n_pairs, 1), C.sizeof(Delay)), dtype=torch.uint8, device=ref.device)
    u32p = C.POINTER(C.c_uint32)
    _check(ctx.L.peaq_batch_estimate_delay(ctx.h, channels, n_pairs, C.c_void_p(ref.data_ptr()),
                                           C.c_void_p(test.data_ptr()), stride,
                                           a_ref.ctypes.data_as(u32p) if a_ref is not None else None,
                                           a_test.ctypes.data_as(u32p) if a_test is not None else None,
                                           stride, int(max_lag), C.c_void_p(rec.data_ptr()), _stream_ptr(stream)))
    if stream is None:
        torch.cuda.current_stream(ref.device).synchronize()
    elif hasattr(stream, "synchronize"):
        stream.synchronize()
    else:
        torch.cuda.ExternalStream(int(stream)).synchronize()
    rows = rec.cpu().numpy()[:n_pairs].copy().view(
        np.dtype([("lag", "<i4"), ("reserved", "<i4"), ("peak", "<f8"), ("runner_up", "<f8"), ("norm", "<f8")]))[:, 0]
    return {k: np.ascontiguousarray(rows[k]) for k in ("lag", "peak", "runner_up", "norm")}


def cut(ctx, x, skip, n_keep, out=None, stream=None):
    """out[p, i] = x[p, skip[p] + i] for i < n_keep[p] (peaq_batch_cut); x: CUDA float32 [n_pairs, n_samples, channels].
    out: optional tensor [n_pairs, stride, channels] to write into (samples past n_keep[p] keep what they held); without
    it a zero-filled one with an even stride is made.  Returns out."""
    import torch
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 3
    n_pairs, stride, channels = x.shape
    a_skip = np.ascontiguousarray(skip, dtype=np.uint32)
    a_keep = np.ascontiguousarray(n_keep, dtype=np.uint32)
    assert a_skip.shape == (n_pairs,) and a_keep.shape == (n_pairs,)
    if out is None:
        o_stride = max(int(a_keep.max()) if n_pairs else 0, 2)
        with _torch_stream(stream):                    # the zero fill runs on the stream the copy runs on
            out = torch.zeros((n_pairs, o_stride + (o_stride & 1), channels), dtype=torch.float32, device=x.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 3
    assert out.shape[0] == n_pairs and out.shape[2] == channels
    u32p = C.POINTER(C.c_uint32)
    _check(ctx.L.peaq_batch_cut(ctx.h, channels, n_pairs, C.c_void_p(x.data_ptr()), stride, a_skip.ctypes.data_as(u32p),
                                a_keep.ctypes.data_as(u32p), C.c_void_p(out.data_ptr()), out.shape[1],
                                _stream_ptr(stream)))
    return out


def gather(ctx, x, src, skip=None, n_keep=None, out=None, stream=None):
    """out[p, i] = x[src[p], skip[p] + i] for i < n_keep[p] (peaq_batch_gather); x: CUDA float32 [n_rows, n_samples,
    channels], src: a row of x per output, any row any number of times.  skip: zeros without it; n_keep: what is left
    of the row behind the skip.  out: optional tensor [n_out, stride, channels] to write into (samples past n_keep[p]
    keep what they held); without it a zero-filled one with an even stride is made.  Returns out."""
    import torch
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 3
    n_rows, stride, channels = x.shape
    a_src = np.ascontiguousarray(src, dtype=np.uint32)
    assert a_src.ndim == 1
    n_out = len(a_src)
    a_skip = np.zeros(n_out, np.uint32) if skip is None else np.ascontiguousarray(skip, dtype=np.uint32)
    a_keep = (stride - np.minimum(a_skip, stride)).astype(np.uint32) if n_keep is None else np.ascontiguousarray(n_keep, dtype=np.uint32)
    assert a_skip.shape == (n_out,) and a_keep.shape == (n_out,)
    if out is None:
        o_stride = max(int(a_keep.max()) if n_out else 0, 2)
        with _torch_stream(stream):                    # the zero fill runs on the stream the copy runs on
            out = torch.zeros((n_out, o_stride + (o_stride & 1), channels), dtype=torch.float32, device=x.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 3
    assert out.shape[0] == n_out and out.shape[2] == channels
    u32p = C.POINTER(C.c_uint32)
    _check(ctx.L.peaq_batch_gather(ctx.h, channels, n_rows, n_out, C.c_void_p(x.data_ptr()), stride,
                                   a_src.ctypes.data_as(u32p), a_skip.ctypes.data_as(u32p), a_keep.ctypes.data_as(u32p),
                                   C.c_void_p(out.data_ptr()), out.shape[1], _stream_ptr(stream)))
    return out


def gain_mode(gain, per_channel=False):
    """PEAQ_GAIN_* of a name (None 'lsq' 'rms' 'polarity') or of the number itself, PEAQ_GAIN_PER_CHANNEL or-ed in"""
    if not isinstance(gain, (int, np.integer)):
        if gain not in GAIN_MODES:
            raise PeaqError(f"unknown gain mode {gain!r}: None, 'lsq', 'rms' or 'polarity'")
        gain = GAIN_MODES[gain]
    return int(gain) | (GAIN_PER_CHANNEL if per_channel else 0)


def gain_workspace_bytes(channels, n_pairs, n_max):
    """partial sums of measure_gain for a shape (peaq_gain_workspace_bytes)"""
    return int(load_library().peaq_gain_workspace_bytes(int(channels), int(n_pairs), int(n_max)))


def gain_records(rec, n_pairs=None):
    """a device record tensor of measure_gain (or a ctypes Gain array) as a dict of numpy arrays: gain, srr, stt, srt,
    flags [n_pairs, 2] and n [n_pairs]; synchronises the device the tensor is on"""
    if hasattr(rec, "is_cuda"):
        import torch
        torch.cuda.synchronize(rec.device)
        rows = rec.cpu().numpy().copy().view(GAIN_DTYPE)[:, 0]
    else:
        rows = np.frombuffer(bytes(rec), dtype=GAIN_DTYPE)
    rows = rows[:len(rows) if n_pairs is None else n_pairs]
    return {k: np.ascontiguousarray(rows[k]) for k in ("gain", "srr", "stt", "srt", "flags", "n")}


def measure_gain(ctx, ref, test, mode, skip_ref=None, skip_test=None, n=None, max_gain_db=40.0, per_channel=False,
                 stream=None):
    """Gain of every pair's test signal against its reference over n[p] samples from skip_ref[p] / skip_test[p] on
    (peaq_batch_measure_gain): ref/test CUDA float32 [n_pairs, n_samples, channels], each with its own n_samples.
    Without skips: zeros; without n: what both buffers hold behind their skips.  mode: 'lsq' 'rms' 'polarity' (or None:
    sums only).  Enqueues and returns (rec, read): the device record tensor (uint8 [n_pairs, 80], what cut_scaled
    takes) and a function that synchronises and returns the records as numpy arrays (gain_records)."""
    import torch
    for x in (ref, test):
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 3
    n_pairs, channels = ref.shape[0], ref.shape[2]
    assert test.shape[0] == n_pairs and test.shape[2] == channels
    a_sr = np.zeros(n_pairs, np.uint32) if skip_ref is None else np.ascontiguousarray(skip_ref, dtype=np.uint32)
    a_st = np.zeros(n_pairs, np.uint32) if skip_test is None else np.ascontiguousarray(skip_test, dtype=np.uint32)
    if n is None:
        a_n = np.minimum(ref.shape[1] - np.minimum(a_sr, ref.shape[1]), test.shape[1] - np.minimum(a_st, test.shape[1])).astype(np.uint32)
    else:
        a_n = np.ascontiguousarray(n, dtype=np.uint32)
    assert a_sr.shape == (n_pairs,) and a_st.shape == (n_pairs,) and a_n.shape == (n_pairs,)
    assert ctx.L.peaq_gain_size() == C.sizeof(Gain) == GAIN_DTYPE.itemsize
    with _torch_stream(stream):
        rec = torch.zeros((max(n_pairs, 1), C.sizeof(Gain)), dtype=torch.uint8, device=ref.device)
    u32p = C.POINTER(C.c_uint32)
    _check(ctx.L.peaq_batch_measure_gain(ctx.h, channels, n_pairs, C.c_void_p(ref.data_ptr()), ref.shape[1],
                                         a_sr.ctypes.data_as(u32p), C.c_void_p(test.data_ptr()), test.shape[1],
                                         a_st.ctypes.data_as(u32p), a_n.ctypes.data_as(u32p),
                                         gain_mode(mode, per_channel), float(max_gain_db), C.c_void_p(rec.data_ptr()),
                                         _stream_ptr(stream)))
    return rec, (lambda: gain_records(rec, n_pairs))


def cut_scaled(ctx, x, skip, n_keep, gain, out=None, stream=None):
    """cut with every pair's and channel's factor from the device records of measure_gain (peaq_batch_cut_scaled):
    out[p, i, c] = float32(float64(x[p, skip[p] + i, c]) * gain[p].gain[c]); a factor of exactly 1.0 moves the bits.
    gain: CUDA uint8 [n_pairs, 80].  out as for cut.  Returns out."""
    import torch
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 3
    n_pairs, stride, channels = x.shape
    a_skip = np.ascontiguousarray(skip, dtype=np.uint32)
    a_keep = np.ascontiguousarray(n_keep, dtype=np.uint32)
    assert a_skip.shape == (n_pairs,) and a_keep.shape == (n_pairs,)
    assert gain.is_cuda and gain.dtype == torch.uint8 and gain.is_contiguous() and gain.shape[0] >= n_pairs
    assert gain.shape[1] == C.sizeof(Gain)
    if out is None:
        o_stride = max(int(a_keep.max()) if n_pairs else 0, 2)
        with _torch_stream(stream):                    # the zero fill runs on the stream the copy runs on
            out = torch.zeros((n_pairs, o_stride + (o_stride & 1), channels), dtype=torch.float32, device=x.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 3
    assert out.shape[0] == n_pairs and out.shape[2] == channels
    u32p = C.POINTER(C.c_uint32)
    _check(ctx.L.peaq_batch_cut_scaled(ctx.h, channels, n_pairs, C.c_void_p(x.data_ptr()), stride,
                                       a_skip.ctypes.data_as(u32p), a_keep.ctypes.data_as(u32p),
                                       C.c_void_p(gain.data_ptr()), C.c_void_p(out.data_ptr()), out.shape[1],
                                       _stream_ptr(stream)))
    return out


def subsample_tables():
    """(corr [256, 33], shift [256, 65]): the two tables of the sub-sample stage exactly as uploaded
    (peaq_subsample_tables, host arithmetic, no GPU); row q + 128, column k + 16 / o + 32"""
    corr, shift = np.zeros((SUB_STEPS, 2 * SUB_LAGS + 1)), np.zeros((SUB_STEPS, 2 * SUB_HALF + 1))
    dp = C.POINTER(C.c_double)
    _check(load_library().peaq_subsample_tables(corr.ctypes.data_as(dp), shift.ctypes.data_as(dp)))
    return corr, shift


def subdelay_workspace_bytes(channels, n_pairs, n_max):
    """partial sums of refine_delay for a shape (peaq_subdelay_workspace_bytes)"""
    return int(load_library().peaq_subdelay_workspace_bytes(int(channels), int(n_pairs), int(n_max)))


def _sync_stream(stream, device):
    import torch
    if stream is None:
        torch.cuda.current_stream(device).synchronize()
    elif hasattr(stream, "synchronize"):
        stream.synchronize()
    else:
        torch.cuda.ExternalStream(int(stream)).synchronize()


def refine_delay(ctx, ref, test, lags, n_ref=None, n_test=None, stream=None):
    """The sub-sample part of every pair's delay around its integer lag (peaq_batch_refine_delay): ref/test CUDA float32
    [n_pairs, n_samples, channels], lags as estimate_delay's, n_ref/n_test optional per-pair lengths.  Returns a dict of
    numpy arrays [n_pairs]: lag, q (int32, grid point of 1/256 sample), frac (q / 256), peak, c0, flags (SUB_F_*).  The
    total delay is lag + frac; positive: the test signal is late.  Synchronises the stream it ran on."""
    import torch
    assert ref.is_cuda and test.is_cuda and ref.dtype == torch.float32 and test.dtype == torch.float32
    assert ref.is_contiguous() and test.is_contiguous() and ref.shape == test.shape and ref.dim() == 3
    n_pairs, stride, channels = ref.shape
    assert (n_ref is None) == (n_test is None), "n_ref and n_test: both or neither"
    a_ref = a_test = None
    if n_ref is not None:
        a_ref = np.ascontiguousarray(n_ref, dtype=np.uint32)
        a_test = np.ascontiguousarray(n_test, dtype=np.uint32)
        assert a_ref.shape == (n_pairs,) and a_test.shape == (n_pairs,)
    a_lag = np.ascontiguousarray(lags, dtype=np.int32)
    assert a_lag.shape == (n_pairs,)
    assert ctx.L.peaq_subdelay_size() == C.sizeof(SubDelay) == SUBDELAY_DTYPE.itemsize
    with _torch_stream(stream):
        rec = torch.zeros((max(n_pairs, 1), C.sizeof(SubDelay)), dtype=torch.uint8, device=ref.device)
    u32p = C.POINTER(C.c_uint32)
    _check(ctx.L.peaq_batch_refine_delay(ctx.h, channels, n_pairs, C.c_void_p(ref.data_ptr()), C.c_void_p(test.data_ptr()),
                                         stride, a_ref.ctypes.data_as(u32p) if a_ref is not None else None,
                                         a_test.ctypes.data_as(u32p) if a_test is not None else None, stride,
                                         a_lag.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(rec.data_ptr()),
                                         _stream_ptr(stream)))
    _sync_stream(stream, ref.device)
    rows = rec.cpu().numpy()[:n_pairs].copy().view(SUBDELAY_DTYPE)[:, 0]
    return {k: np.ascontiguousarray(rows[k]) for k in ("lag", "q", "frac", "peak", "c0", "flags")}


def cut_shifted(ctx, x, skip, n_keep, q, n_in=None, out=None, stream=None):
    """cut through the fractional-delay filter of every pair's grid point q[p] (peaq_batch_cut_shifted):
    out[p, i, c] = float32(sum_o shift_tab[q[p]][o] float64(x[p, skip[p] + i + o, c])), o = -32 .. 32; samples outside
    [0, n_in[p]) (without n_in: the buffer) contribute nothing; q[p] == 0 moves the bits.  out as for cut.  Returns out."""
    a_q = np.ascontiguousarray(q, dtype=np.int32)
    assert a_q.shape == (len(x),)
    return _cut_along(ctx, x, skip, n_keep, n_in, out, stream, lambda head, tail: ctx.L.peaq_batch_cut_shifted(
        *head, a_q.ctypes.data_as(C.POINTER(C.c_int32)), *tail))


def _cut_along(ctx, x, skip, n_keep, n_in, out, stream, call):
    """what cut_shifted, cut_drift, cut_track and cut_pieces share: x, skip, n_keep, n_in (default: the buffer) and out
    (default: zero-filled, even stride) as the four take them; call(head, tail) is the C entry between its leading
    arguments (ctx .. n_keep) and its trailing ones (d_out, out_stride, stream).  Returns out."""
    import torch
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 3
    n_pairs, stride, channels = x.shape
    a_skip = np.ascontiguousarray(skip, dtype=np.uint32)
    a_keep = np.ascontiguousarray(n_keep, dtype=np.uint32)
    a_in = np.full(n_pairs, stride, dtype=np.uint32) if n_in is None else np.ascontiguousarray(n_in, dtype=np.uint32)
    assert a_skip.shape == (n_pairs,) and a_keep.shape == (n_pairs,) and a_in.shape == (n_pairs,)
    if out is None:
        o_stride = max(int(a_keep.max()) if n_pairs else 0, 2)
        with _torch_stream(stream):                    # the zero fill runs on the stream the filter runs on
            out = torch.zeros((n_pairs, o_stride + (o_stride & 1), channels), dtype=torch.float32, device=x.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 3
    assert out.shape[0] == n_pairs and out.shape[2] == channels
    u32p = C.POINTER(C.c_uint32)
    _check(call((ctx.h, channels, n_pairs, C.c_void_p(x.data_ptr()), stride, a_in.ctypes.data_as(u32p),
                 a_skip.ctypes.data_as(u32p), a_keep.ctypes.data_as(u32p)),
                (C.c_void_p(out.data_ptr()), out.shape[1], _stream_ptr(stream))))
    return out


def drift_fit(d, x, valid=None):
    """(a, e, n_valid): the Theil-Sen line through the valid points (peaq_drift_fit, host arithmetic, no GPU)"""
    d = np.ascontiguousarray(d, dtype=np.float64)
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert d.ndim == 1 and d.shape == x.shape
    v = None
    if valid is not None:
        v = np.ascontiguousarray(valid, dtype=np.uint8)
        assert v.shape == d.shape
    a, e = C.c_double(0), C.c_double(0)
    dp = C.POINTER(C.c_double)
    n = load_library().peaq_drift_fit(d.ctypes.data_as(dp), x.ctypes.data_as(dp),
                                      v.ctypes.data_as(C.POINTER(C.c_uint8)) if v is not None else None, len(d),
                                      C.byref(a), C.byref(e))
    _check(min(n, 0))
    return a.value, e.value, n


def drift_index(a, e, i):
    """(m, phi): where output i of the drift cut reads (peaq_drift_index, host arithmetic, no GPU)"""
    m, phi = C.c_int64(0), C.c_int32(0)
    load_library().peaq_drift_index(float(a), float(e), int(i), C.byref(m), C.byref(phi))
    return m.value, phi.value


def drift_lengths(lag0, a, e, n_ref, n_test):
    """(skip_ref, skip_test, n_keep) for one pair's lag and line (peaq_drift_lengths, host arithmetic, no GPU)"""
    sr, st, n = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    load_library().peaq_drift_lengths(int(lag0), float(a), float(e), int(n_ref), int(n_test), C.byref(sr), C.byref(st),
                                      C.byref(n))
    return sr.value, st.value, n.value


def drift_windows(lag0, n_ref, n_test, window=DRIFT_WINDOW):
    """whole windows of one pair's aligned part (peaq_drift_windows)"""
    return int(load_library().peaq_drift_windows(int(lag0), int(n_ref), int(n_test), int(window)))


def drift_workspace_bytes(channels, n_pairs, window, w_max):
    """the two staging buffers of estimate_drift for a shape (peaq_drift_workspace_bytes)"""
    return int(load_library().peaq_drift_workspace_bytes(int(channels), int(n_pairs), int(window), int(w_max)))


def _drift_window(drift):
    """the window of a `drift=` keyword: True is the default window"""
    return DRIFT_WINDOW if drift is True else int(drift)


def estimate_drift(ctx, ref, test, lags, n_ref=None, n_test=None, window=DRIFT_WINDOW, R=None, min_corr=DRIFT_MIN_CORR,
                   max_e=DRIFT_MAX_E, stream=None):
    """Every pair's delay as a line a + e i in the coordinates its lag aligns (peaq_batch_estimate_drift): ref/test CUDA
    float32 [n_pairs, n_samples, channels], lags as estimate_delay's (over the whole signals), n_ref/n_test optional
    per-pair lengths.  window: samples per window; R: the windows' max_lag (default min(window // 4, 1024)).  Returns a
    dict of numpy arrays [n_pairs]: lag0, flags (DRIFT_F_*), a, e, ppm, resid_rms, n_windows, n_valid, and `windows`:
    the per-window records as a dict of arrays [n_pairs, w_max] (lag, peak, runner_up, norm of the delay records; q,
    sub_peak, c0, sub_flags of the sub-delay records).  Blocks until the records are there."""
    import torch
    assert ref.is_cuda and test.is_cuda and ref.dtype == torch.float32 and test.dtype == torch.float32
    assert ref.is_contiguous() and test.is_contiguous() and ref.shape == test.shape and ref.dim() == 3
    n_pairs, stride, channels = ref.shape
    assert (n_ref is None) == (n_test is None), "n_ref and n_test: both or neither"
    a_ref = a_test = None
    if n_ref is not None:
        a_ref = np.ascontiguousarray(n_ref, dtype=np.uint32)
        a_test = np.ascontiguousarray(n_test, dtype=np.uint32)
        assert a_ref.shape == (n_pairs,) and a_test.shape == (n_pairs,)
    a_lag = np.ascontiguousarray(lags, dtype=np.int32)
    assert a_lag.shape == (n_pairs,)
    window = int(window)
    R = min(window // 4, 1024) if R is None else int(R)
    L = ctx.L
    assert L.peaq_drift_size() == C.sizeof(Drift) == DRIFT_DTYPE.itemsize
    w_max = max([1] + [int(L.peaq_drift_windows(int(a_lag[p]), int(stride if a_ref is None else a_ref[p]),
                                                int(stride if a_test is None else a_test[p]), window))
                       for p in range(n_pairs)])
    with _torch_stream(stream):
        d_dl = torch.zeros((max(n_pairs, 1), w_max, C.sizeof(Delay)), dtype=torch.uint8, device=ref.device)
        d_sb = torch.zeros((max(n_pairs, 1), w_max, C.sizeof(SubDelay)), dtype=torch.uint8, device=ref.device)
    out = np.zeros(max(n_pairs, 1), dtype=DRIFT_DTYPE)
    u32p = C.POINTER(C.c_uint32)
    _check(L.peaq_batch_estimate_drift(ctx.h, channels, n_pairs, C.c_void_p(ref.data_ptr()), C.c_void_p(test.data_ptr()),
                                       stride, a_ref.ctypes.data_as(u32p) if a_ref is not None else None,
                                       a_test.ctypes.data_as(u32p) if a_test is not None else None, stride,
                                       a_lag.ctypes.data_as(C.POINTER(C.c_int32)), window, R, float(min_corr), float(max_e),
                                       w_max, C.c_void_p(d_dl.data_ptr()), C.c_void_p(d_sb.data_ptr()),
                                       out.ctypes.data_as(C.POINTER(Drift)), _stream_ptr(stream)))
    _sync_stream(stream, ref.device)
    res = {k: np.ascontiguousarray(out[k][:n_pairs]) for k in DRIFT_DTYPE.names}
    dl = d_dl.cpu().numpy()[:n_pairs].copy().view(DELAY_DTYPE)[:, :, 0]
    sb = d_sb.cpu().numpy()[:n_pairs].copy().view(SUBDELAY_DTYPE)[:, :, 0]
    res["windows"] = dict(lag=np.ascontiguousarray(dl["lag"]), peak=np.ascontiguousarray(dl["peak"]),
                          runner_up=np.ascontiguousarray(dl["runner_up"]), norm=np.ascontiguousarray(dl["norm"]),
                          q=np.ascontiguousarray(sb["q"]), sub_peak=np.ascontiguousarray(sb["peak"]),
                          c0=np.ascontiguousarray(sb["c0"]), sub_flags=np.ascontiguousarray(sb["flags"]))
    return res


def cut_drift(ctx, x, skip, n_keep, a, e, n_in=None, out=None, stream=None):
    """cut along every pair's line (peaq_batch_cut_drift): out[p, i, c] = float32(sum_o shift_tab[phi_i][o]
    float64(x[p, skip[p] + i + m_i + o, c])), o = -32 .. 32, (m_i, phi_i) = drift_index(a[p], e[p], i); samples outside
    [0, n_in[p]) (without n_in: the buffer) contribute nothing; a[p] == e[p] == 0 moves the bits.  out as for cut.
    Returns out."""
    a_a = np.ascontiguousarray(a, dtype=np.float64)
    a_e = np.ascontiguousarray(e, dtype=np.float64)
    assert a_a.shape == (len(x),) and a_e.shape == (len(x),)
    dp = C.POINTER(C.c_double)
    return _cut_along(ctx, x, skip, n_keep, n_in, out, stream, lambda head, tail: ctx.L.peaq_batch_cut_drift(
        *head, a_a.ctypes.data_as(dp), a_e.ctypes.data_as(dp), *tail))


def track_fit(d, valid=None, window=TRACK_WINDOW, max_e=TRACK_MAX_E):
    """The per-window delays d kept as a track (peaq_track_fit, host arithmetic, no GPU).  Returns a dict: the record's
    fields (flags, n_windows, n_valid, n_filled, n_segments, d_min, d_max, max_abs_e) and the arrays knots [W], a and e
    [max(W - 1, 1)]."""
    d = np.ascontiguousarray(d, dtype=np.float64)
    assert d.ndim == 1
    v = None
    if valid is not None:
        v = np.ascontiguousarray(valid, dtype=np.uint8)
        assert v.shape == d.shape
    W = len(d)
    knots, a, e = np.zeros(max(W, 1)), np.zeros(max(W - 1, 1)), np.zeros(max(W - 1, 1))
    rec = Track()
    dp = C.POINTER(C.c_double)
    _check(load_library().peaq_track_fit(d.ctypes.data_as(dp), v.ctypes.data_as(C.POINTER(C.c_uint8)) if v is not None else None,
                                         W, int(window), float(max_e), C.byref(rec), knots.ctypes.data_as(dp),
                                         a.ctypes.data_as(dp), e.ctypes.data_as(dp)))
    res = {k: getattr(rec, k) for k, _ in Track._fields_ if k != "lag0"}
    res.update(knots=knots[:W], a=a, e=e)
    return res


def track_segment(i, window, n_seg):
    """the segment output i belongs to (peaq_track_segment, host arithmetic, no GPU)"""
    return int(load_library().peaq_track_segment(int(i), int(window), int(n_seg)))


def track_index(window, a, e, i):
    """(m, phi): where output i of the track cut reads, a and e the pair's segments (peaq_track_index, host arithmetic)"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    e = np.ascontiguousarray(e, dtype=np.float64)
    assert a.ndim == 1 and a.shape == e.shape and len(a) >= 1
    m, phi = C.c_int64(0), C.c_int32(0)
    dp = C.POINTER(C.c_double)
    load_library().peaq_track_index(int(window), len(a), a.ctypes.data_as(dp), e.ctypes.data_as(dp), int(i), C.byref(m),
                                    C.byref(phi))
    return m.value, phi.value


def track_lengths(lag0, window, a, e, n_ref, n_test):
    """(skip_ref, skip_test, n_keep) for one pair's lag and segments (peaq_track_lengths, host arithmetic, no GPU)"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    e = np.ascontiguousarray(e, dtype=np.float64)
    assert a.ndim == 1 and a.shape == e.shape and len(a) >= 1
    sr, st, n = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    dp = C.POINTER(C.c_double)
    load_library().peaq_track_lengths(int(lag0), int(window), len(a), a.ctypes.data_as(dp), e.ctypes.data_as(dp), int(n_ref),
                                      int(n_test), C.byref(sr), C.byref(st), C.byref(n))
    return sr.value, st.value, n.value


def _track_window(track):
    """the window of a `track=` keyword: True is the default window"""
    return TRACK_WINDOW if track is True else int(track)


def estimate_track(ctx, ref, test, lags, n_ref=None, n_test=None, window=TRACK_WINDOW, R=None, min_corr=DRIFT_MIN_CORR,
                   max_e=TRACK_MAX_E, stream=None):
    """Every pair's delay as a track in the coordinates its lag aligns (peaq_batch_estimate_track); arguments as
    estimate_drift's.  Returns a dict of numpy arrays [n_pairs]: the fields of TRACK_DTYPE; knots [n_pairs, w_max]; a, e
    [n_pairs, seg_stride] (row p holds n_segments[p] segments); `windows`, the per-window records as estimate_drift's;
    and `drift`, the line's record as estimate_drift returns it (without windows).  Blocks until the records are there."""
    import torch
    assert ref.is_cuda and test.is_cuda and ref.dtype == torch.float32 and test.dtype == torch.float32
    assert ref.is_contiguous() and test.is_contiguous() and ref.shape == test.shape and ref.dim() == 3
    n_pairs, stride, channels = ref.shape
    assert (n_ref is None) == (n_test is None), "n_ref and n_test: both or neither"
    a_ref = a_test = None
    if n_ref is not None:
        a_ref = np.ascontiguousarray(n_ref, dtype=np.uint32)
        a_test = np.ascontiguousarray(n_test, dtype=np.uint32)
        assert a_ref.shape == (n_pairs,) and a_test.shape == (n_pairs,)
    a_lag = np.ascontiguousarray(lags, dtype=np.int32)
    assert a_lag.shape == (n_pairs,)
    window = int(window)
    R = min(window // 4, 1024) if R is None else int(R)
    L = ctx.L
    assert L.peaq_track_size() == C.sizeof(Track) == TRACK_DTYPE.itemsize
    w_max = max([1] + [int(L.peaq_drift_windows(int(a_lag[p]), int(stride if a_ref is None else a_ref[p]),
                                                int(stride if a_test is None else a_test[p]), window))
                       for p in range(n_pairs)])
    seg_stride = max(w_max - 1, 1)
    with _torch_stream(stream):
        d_dl = torch.zeros((max(n_pairs, 1), w_max, C.sizeof(Delay)), dtype=torch.uint8, device=ref.device)
        d_sb = torch.zeros((max(n_pairs, 1), w_max, C.sizeof(SubDelay)), dtype=torch.uint8, device=ref.device)
    out = np.zeros(max(n_pairs, 1), dtype=TRACK_DTYPE)
    line = np.zeros(max(n_pairs, 1), dtype=DRIFT_DTYPE)
    knots = np.zeros((max(n_pairs, 1), w_max))
    seg_a, seg_e = np.zeros((max(n_pairs, 1), seg_stride)), np.zeros((max(n_pairs, 1), seg_stride))
    u32p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    _check(L.peaq_batch_estimate_track(ctx.h, channels, n_pairs, C.c_void_p(ref.data_ptr()), C.c_void_p(test.data_ptr()),
                                       stride, a_ref.ctypes.data_as(u32p) if a_ref is not None else None,
                                       a_test.ctypes.data_as(u32p) if a_test is not None else None, stride,
                                       a_lag.ctypes.data_as(C.POINTER(C.c_int32)), window, R, float(min_corr), float(max_e),
                                       w_max, C.c_void_p(d_dl.data_ptr()), C.c_void_p(d_sb.data_ptr()),
                                       line.ctypes.data_as(C.POINTER(Drift)), out.ctypes.data_as(C.POINTER(Track)),
                                       knots.ctypes.data_as(dp), seg_stride, seg_a.ctypes.data_as(dp), seg_e.ctypes.data_as(dp),
                                       _stream_ptr(stream)))
    _sync_stream(stream, ref.device)
    res = {k: np.ascontiguousarray(out[k][:n_pairs]) for k in TRACK_DTYPE.names}
    res.update(knots=knots[:n_pairs], a=seg_a[:n_pairs], e=seg_e[:n_pairs], window=window)
    res["drift"] = {k: np.ascontiguousarray(line[k][:n_pairs]) for k in DRIFT_DTYPE.names}
    dl = d_dl.cpu().numpy()[:n_pairs].copy().view(DELAY_DTYPE)[:, :, 0]
    sb = d_sb.cpu().numpy()[:n_pairs].copy().view(SUBDELAY_DTYPE)[:, :, 0]
    res["windows"] = dict(lag=np.ascontiguousarray(dl["lag"]), peak=np.ascontiguousarray(dl["peak"]),
                          runner_up=np.ascontiguousarray(dl["runner_up"]), norm=np.ascontiguousarray(dl["norm"]),
                          q=np.ascontiguousarray(sb["q"]), sub_peak=np.ascontiguousarray(sb["peak"]),
                          c0=np.ascontiguousarray(sb["c0"]), sub_flags=np.ascontiguousarray(sb["flags"]))
    return res


def cut_track(ctx, x, skip, n_keep, window, n_seg, a, e, n_in=None, out=None, stream=None):
    """cut along every pair's track (peaq_batch_cut_track): as cut_drift, with (m_i, phi_i) = track_index(window,
    a[p, :n_seg[p]], e[p, :n_seg[p]], i); a, e: [n_pairs, seg_stride].  A pair whose segments are all (0, 0) has its bits
    moved.  Returns out."""
    a_seg = np.ascontiguousarray(n_seg, dtype=np.uint32)
    a_a = np.ascontiguousarray(a, dtype=np.float64)
    a_e = np.ascontiguousarray(e, dtype=np.float64)
    assert a_seg.shape == (len(x),) and a_a.ndim == 2 and a_a.shape[0] == len(x) and a_a.shape == a_e.shape
    u32p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    return _cut_along(ctx, x, skip, n_keep, n_in, out, stream, lambda head, tail: ctx.L.peaq_batch_cut_track(
        *head, int(window), a_seg.ctypes.data_as(u32p), a_a.shape[1], a_a.ctypes.data_as(dp), a_e.ctypes.data_as(dp), *tail))


def steps_workspace_bytes(n_cand, span_max):
    """bytes of chunk rows locate_steps keeps in the context (peaq_steps_workspace_bytes)"""
    return int(load_library().peaq_steps_workspace_bytes(int(n_cand), int(span_max)))


def _candidates_array(cand):
    """candidates as a STEP_CANDIDATE_DTYPE array: that, or rows (pair, lo, hi, LA, LB)"""
    if isinstance(cand, np.ndarray) and cand.dtype == STEP_CANDIDATE_DTYPE:
        return np.ascontiguousarray(cand)
    rows = [tuple(int(v) for v in r) for r in cand]
    return np.array(rows, dtype=STEP_CANDIDATE_DTYPE).reshape(len(rows))


def locate_steps(ctx, ref, test, lags, cand, n_ref=None, n_test=None, stream=None):
    """Where each candidate's delay steps from LA to LB (peaq_batch_locate_steps).  lags: every pair's lag0, which fixes
    its coordinates; cand: rows (pair, lo, hi, LA, LB) or a STEP_CANDIDATE_DTYPE array.  Returns a STEP_DTYPE array, one
    record per candidate.  Blocks until the records are there."""
    import torch
    assert ref.is_cuda and test.is_cuda and ref.dtype == torch.float32 and test.dtype == torch.float32
    assert ref.is_contiguous() and test.is_contiguous() and ref.shape == test.shape and ref.dim() == 3
    n_pairs, stride, channels = ref.shape
    assert (n_ref is None) == (n_test is None), "n_ref and n_test: both or neither"
    a_ref = a_test = None
    if n_ref is not None:
        a_ref = np.ascontiguousarray(n_ref, dtype=np.uint32)
        a_test = np.ascontiguousarray(n_test, dtype=np.uint32)
        assert a_ref.shape == (n_pairs,) and a_test.shape == (n_pairs,)
    a_lag = np.ascontiguousarray(lags, dtype=np.int32)
    assert a_lag.shape == (n_pairs,)
    cd = _candidates_array(cand)
    n_cand = len(cd)
    L = ctx.L
    assert L.peaq_step_size() == C.sizeof(Step) == STEP_DTYPE.itemsize
    assert L.peaq_step_candidate_size() == C.sizeof(StepCandidate) == STEP_CANDIDATE_DTYPE.itemsize
    with _torch_stream(stream):
        d_out = torch.zeros((max(n_cand, 1), C.sizeof(Step)), dtype=torch.uint8, device=ref.device)
    u32p = C.POINTER(C.c_uint32)
    _check(L.peaq_batch_locate_steps(ctx.h, channels, n_pairs, C.c_void_p(ref.data_ptr()), C.c_void_p(test.data_ptr()), stride,
                                     a_ref.ctypes.data_as(u32p) if a_ref is not None else None,
                                     a_test.ctypes.data_as(u32p) if a_test is not None else None, stride,
                                     a_lag.ctypes.data_as(C.POINTER(C.c_int32)), n_cand,
                                     cd.ctypes.data_as(C.POINTER(StepCandidate)), C.c_void_p(d_out.data_ptr()),
                                     _stream_ptr(stream)))
    _sync_stream(stream, ref.device)
    return d_out.cpu().numpy()[:n_cand].copy().view(STEP_DTYPE)[:, 0]


def steps_candidates(knots, window, n_common, pair=0, min_step=STEP_MIN_STEP, ratio=STEP_RATIO):
    """the segments of a track that look like a step, as a STEP_CANDIDATE_DTYPE array (peaq_steps_candidates, host
    arithmetic, no GPU)"""
    knots = np.ascontiguousarray(knots, dtype=np.float64)
    assert knots.ndim == 1
    W = len(knots)
    out = np.zeros(max(W - 1, 1), dtype=STEP_CANDIDATE_DTYPE)
    n = C.c_uint32(0)
    _check(load_library().peaq_steps_candidates(knots.ctypes.data_as(C.POINTER(C.c_double)), W, int(window), int(n_common),
                                                int(pair), float(min_step), float(ratio),
                                                out.ctypes.data_as(C.POINTER(StepCandidate)), C.byref(n)))
    return out[:n.value].copy()


def steps_fit(knots, window, n_common, steps, min_step=STEP_MIN_STEP, ratio=STEP_RATIO, min_gain=STEP_MIN_GAIN,
              max_e=TRACK_MAX_E):
    """One pair's track rebuilt as pieces (peaq_steps_fit, host arithmetic, no GPU).  steps: the STEP_DTYPE records
    locate_steps wrote for steps_candidates(knots, ...).  Returns a dict: the record's fields (flags, n_candidates,
    n_accepted, n_pieces, max_abs_e), the arrays b, a, e [n_pieces], and `steps`, the records with STEP_F_WEAK set where
    one was not accepted."""
    knots = np.ascontiguousarray(knots, dtype=np.float64)
    assert knots.ndim == 1
    W = len(knots)
    st = np.array(steps, dtype=STEP_DTYPE).reshape(-1).copy()
    room = max(W - 1, 1) + len(st)
    b, a, e = np.zeros(room, np.uint32), np.zeros(room), np.zeros(room)
    rec = Pieces()
    dp = C.POINTER(C.c_double)
    _check(load_library().peaq_steps_fit(knots.ctypes.data_as(dp), W, int(window), int(n_common), float(min_step), float(ratio),
                                         float(min_gain), float(max_e), st.ctypes.data_as(C.POINTER(Step)), len(st),
                                         C.byref(rec), b.ctypes.data_as(C.POINTER(C.c_uint32)), a.ctypes.data_as(dp),
                                         e.ctypes.data_as(dp)))
    res = {k: getattr(rec, k) for k, _ in Pieces._fields_}
    n = rec.n_pieces
    res.update(b=b[:n], a=a[:n], e=e[:n], steps=st)
    return res


def _pieces_arrays(b, a, e):
    b = np.ascontiguousarray(b, dtype=np.uint32)
    a = np.ascontiguousarray(a, dtype=np.float64)
    e = np.ascontiguousarray(e, dtype=np.float64)
    assert b.ndim == 1 and b.shape == a.shape == e.shape and len(b) >= 1
    return b, a, e


def pieces_index(b, a, e, i):
    """(m, phi): where output i of the pieces cut reads (peaq_pieces_index, host arithmetic)"""
    b, a, e = _pieces_arrays(b, a, e)
    m, phi = C.c_int64(0), C.c_int32(0)
    dp = C.POINTER(C.c_double)
    load_library().peaq_pieces_index(len(b), b.ctypes.data_as(C.POINTER(C.c_uint32)), a.ctypes.data_as(dp), e.ctypes.data_as(dp),
                                     int(i), C.byref(m), C.byref(phi))
    return m.value, phi.value


def pieces_lengths(lag0, b, a, e, n_ref, n_test):
    """(skip_ref, skip_test, n_keep) for one pair's lag and pieces (peaq_pieces_lengths, host arithmetic, no GPU)"""
    b, a, e = _pieces_arrays(b, a, e)
    sr, st, n = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    dp = C.POINTER(C.c_double)
    load_library().peaq_pieces_lengths(int(lag0), len(b), b.ctypes.data_as(C.POINTER(C.c_uint32)), a.ctypes.data_as(dp),
                                       e.ctypes.data_as(dp), int(n_ref), int(n_test), C.byref(sr), C.byref(st), C.byref(n))
    return sr.value, st.value, n.value


def _steps_window(steps):
    """the window of a `steps=` keyword: True is the default window"""
    return TRACK_WINDOW if steps is True else int(steps)


def estimate_steps(ctx, ref, test, lags, n_ref=None, n_test=None, window=TRACK_WINDOW, R=None, min_corr=DRIFT_MIN_CORR,
                   max_e=TRACK_MAX_E, min_step=STEP_MIN_STEP, ratio=STEP_RATIO, min_gain=STEP_MIN_GAIN, stream=None):
    """Every pair's delay as pieces: its track, the steps located in it, the track rebuilt around them
    (peaq_batch_estimate_steps); arguments as estimate_track's.  Returns a dict: `track`, the fields of TRACK_DTYPE
    [n_pairs]; knots [n_pairs, w_max]; `steps`, STEP_DTYPE [n_pairs, steps_stride] (row p holds n_candidates[p]
    records); the fields of PIECES_DTYPE [n_pairs]; b, a, e [n_pairs, piece_stride] (row p holds n_pieces[p] pieces);
    `drift` as estimate_track's.  Blocks until the records are there."""
    import torch
    assert ref.is_cuda and test.is_cuda and ref.dtype == torch.float32 and test.dtype == torch.float32
    assert ref.is_contiguous() and test.is_contiguous() and ref.shape == test.shape and ref.dim() == 3
    n_pairs, stride, channels = ref.shape
    assert (n_ref is None) == (n_test is None), "n_ref and n_test: both or neither"
    a_ref = a_test = None
    if n_ref is not None:
        a_ref = np.ascontiguousarray(n_ref, dtype=np.uint32)
        a_test = np.ascontiguousarray(n_test, dtype=np.uint32)
        assert a_ref.shape == (n_pairs,) and a_test.shape == (n_pairs,)
    a_lag = np.ascontiguousarray(lags, dtype=np.int32)
    assert a_lag.shape == (n_pairs,)
    window = int(window)
    R = min(window // 4, 1024) if R is None else int(R)
    L = ctx.L
    assert L.peaq_step_size() == C.sizeof(Step) == STEP_DTYPE.itemsize
    assert L.peaq_pieces_size() == C.sizeof(Pieces) == PIECES_DTYPE.itemsize
    w_max = max([1] + [int(L.peaq_drift_windows(int(a_lag[p]), int(stride if a_ref is None else a_ref[p]),
                                                int(stride if a_test is None else a_test[p]), window))
                       for p in range(n_pairs)])
    steps_stride = max(w_max - 1, 1)
    piece_stride = 2 * steps_stride
    rows = max(n_pairs, 1)
    with _torch_stream(stream):
        d_dl = torch.zeros((rows, w_max, C.sizeof(Delay)), dtype=torch.uint8, device=ref.device)
        d_sb = torch.zeros((rows, w_max, C.sizeof(SubDelay)), dtype=torch.uint8, device=ref.device)
    track = np.zeros(rows, dtype=TRACK_DTYPE)
    line = np.zeros(rows, dtype=DRIFT_DTYPE)
    knots = np.zeros((rows, w_max))
    steps = np.zeros((rows, steps_stride), dtype=STEP_DTYPE)
    pieces = np.zeros(rows, dtype=PIECES_DTYPE)
    b = np.zeros((rows, piece_stride), dtype=np.uint32)
    a, e = np.zeros((rows, piece_stride)), np.zeros((rows, piece_stride))
    u32p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    _check(L.peaq_batch_estimate_steps(ctx.h, channels, n_pairs, C.c_void_p(ref.data_ptr()), C.c_void_p(test.data_ptr()),
                                       stride, a_ref.ctypes.data_as(u32p) if a_ref is not None else None,
                                       a_test.ctypes.data_as(u32p) if a_test is not None else None, stride,
                                       a_lag.ctypes.data_as(C.POINTER(C.c_int32)), window, R, float(min_corr), float(max_e),
                                       float(min_step), float(ratio), float(min_gain), w_max, C.c_void_p(d_dl.data_ptr()),
                                       C.c_void_p(d_sb.data_ptr()), line.ctypes.data_as(C.POINTER(Drift)),
                                       track.ctypes.data_as(C.POINTER(Track)), knots.ctypes.data_as(dp), steps_stride,
                                       steps.ctypes.data_as(C.POINTER(Step)), pieces.ctypes.data_as(C.POINTER(Pieces)),
                                       piece_stride, b.ctypes.data_as(u32p), a.ctypes.data_as(dp), e.ctypes.data_as(dp),
                                       _stream_ptr(stream)))
    _sync_stream(stream, ref.device)
    res = {k: np.ascontiguousarray(pieces[k][:n_pairs]) for k in PIECES_DTYPE.names}
    res["track"] = {k: np.ascontiguousarray(track[k][:n_pairs]) for k in TRACK_DTYPE.names}
    res["drift"] = {k: np.ascontiguousarray(line[k][:n_pairs]) for k in DRIFT_DTYPE.names}
    res.update(knots=knots[:n_pairs], steps=steps[:n_pairs], b=b[:n_pairs], a=a[:n_pairs], e=e[:n_pairs], window=window)
    return res


def cut_pieces(ctx, x, skip, n_keep, n_pieces, b, a, e, n_in=None, out=None, stream=None):
    """cut along every pair's pieces (peaq_batch_cut_pieces): as cut_track, with (m_i, phi_i) = pieces_index(b[p,
    :n_pieces[p]], a[p, :n_pieces[p]], e[p, :n_pieces[p]], i); b, a, e: [n_pairs, piece_stride].  A pair whose pieces are
    all (0, 0) has its bits moved.  Returns out."""
    a_np = np.ascontiguousarray(n_pieces, dtype=np.uint32)
    a_b = np.ascontiguousarray(b, dtype=np.uint32)
    a_a = np.ascontiguousarray(a, dtype=np.float64)
    a_e = np.ascontiguousarray(e, dtype=np.float64)
    assert a_np.shape == (len(x),) and a_a.ndim == 2 and a_a.shape[0] == len(x) and a_a.shape == a_e.shape == a_b.shape
    u32p, dp = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    return _cut_along(ctx, x, skip, n_keep, n_in, out, stream, lambda head, tail: ctx.L.peaq_batch_cut_pieces(
        *head, a_np.ctypes.data_as(u32p), a_a.shape[1], a_b.ctypes.data_as(u32p), a_a.ctypes.data_as(dp), a_e.ctypes.data_as(dp),
        *tail))


def wide_factor(max_offset):
    """the decimation factor of a wide search of +-max_offset samples, a power of two in 2 .. 64; 0: max_offset is
    outside 1 .. 2^20 (peaq_wide_factor, host arithmetic, no GPU)"""
    return int(load_library().peaq_wide_factor(int(max_offset) if 0 <= int(max_offset) <= 0xFFFFFFFF else 0))


def wide_taps(M):
    """the decimator's 16 M + 1 taps exactly as uploaded, float64, tap j = -8M first (peaq_wide_taps, no GPU)"""
    M = int(M)
    h = np.zeros(16 * M + 1 if 0 < M <= 64 else 1)
    n = load_library().peaq_wide_taps(M, h.ctypes.data_as(C.POINTER(C.c_double)))
    if n < 0:
        _check(n)
    assert n == len(h)
    return h


def wide_mode(mode):
    """PEAQ_WIDE_* of a name ('waveform' 'envelope') or of the number itself"""
    return WIDE_MODES[mode] if isinstance(mode, str) else int(mode)


def wide_workspace_bytes(channels, n_pairs, n_max, max_offset):
    """the staging of estimate_delay_wide for a shape (peaq_wide_workspace_bytes)"""
    return int(load_library().peaq_wide_workspace_bytes(int(channels), int(n_pairs), int(n_max), int(max_offset)))


def decimate(ctx, x, M, mode, n=None, out=None, stream=None):
    """The mono sum of x (its magnitude with mode 'envelope', and then less its mean), low-passed and decimated by M
    (peaq_batch_decimate): x CUDA float32 [n_pairs, n_samples, channels], n optional per-pair lengths.  out: optional
    tensor [n_pairs, stride] to write into (entries past ceil (n / M) keep what they held); without it a zero-filled one
    with an even stride is made.  Returns (y, n_dec): the tensor and the decimated lengths (numpy uint32 [n_pairs])."""
    import torch
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 3
    n_pairs, stride, channels = x.shape
    M = int(M)
    a_n = None if n is None else np.ascontiguousarray(n, dtype=np.uint32)
    assert a_n is None or a_n.shape == (n_pairs,)
    lens = np.full(n_pairs, stride, dtype=np.uint64) if a_n is None else a_n.astype(np.uint64)
    n_dec = ((lens + max(M, 1) - 1) // max(M, 1)).astype(np.uint32)
    if out is None:
        o_stride = max(int(n_dec.max()) if n_pairs else 0, 2)
        with _torch_stream(stream):                    # the zero fill runs on the stream the filter runs on
            out = torch.zeros((n_pairs, o_stride + (o_stride & 1)), dtype=torch.float32, device=x.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 2 and out.shape[0] == n_pairs
    _check(ctx.L.peaq_batch_decimate(ctx.h, channels, n_pairs, C.c_void_p(x.data_ptr()), stride,
                                     a_n.ctypes.data_as(C.POINTER(C.c_uint32)) if a_n is not None else None, stride, M,
                                     wide_mode(mode), C.c_void_p(out.data_ptr()), out.shape[1], _stream_ptr(stream)))
    return out, n_dec


def estimate_delay_wide(ctx, ref, test, max_offset, mode="envelope", max_lag=4096, n_ref=None, n_test=None, stream=None):
    """Delay of every pair of a batch within +-max_offset samples (up to 2^20), coarse to fine
    (peaq_batch_estimate_delay_wide): decimate, estimate_delay on the decimated copies, cut by the coarse lag,
    estimate_delay with max_lag on the cut pair.  Arguments as estimate_delay's.  Returns a dict of numpy arrays
    [n_pairs]: lag (int32; positive: the test signal is late), coarse_lag, factor, flags (WIDE_F_*), and fine and coarse,
    the two stages' records as estimate_delay's dicts (coarse's lag counts decimated samples).  Blocks."""
    import torch
    assert ref.is_cuda and test.is_cuda and ref.dtype == torch.float32 and test.dtype == torch.float32
    assert ref.is_contiguous() and test.is_contiguous() and ref.shape == test.shape and ref.dim() == 3
    n_pairs, stride, channels = ref.shape
    assert (n_ref is None) == (n_test is None), "n_ref and n_test: both or neither"
    a_ref = a_test = None
    if n_ref is not None:
        a_ref = np.ascontiguousarray(n_ref, dtype=np.uint32)
        a_test = np.ascontiguousarray(n_test, dtype=np.uint32)
        assert a_ref.shape == (n_pairs,) and a_test.shape == (n_pairs,)
    assert ctx.L.peaq_wide_delay_size() == C.sizeof(WideDelay) == WIDE_DELAY_DTYPE.itemsize
    rows = np.zeros(max(n_pairs, 1), dtype=WIDE_DELAY_DTYPE)
    u32p = C.POINTER(C.c_uint32)
    _check(ctx.L.peaq_batch_estimate_delay_wide(ctx.h, channels, n_pairs, C.c_void_p(ref.data_ptr()),
                                                C.c_void_p(test.data_ptr()), stride,
                                                a_ref.ctypes.data_as(u32p) if a_ref is not None else None,
                                                a_test.ctypes.data_as(u32p) if a_test is not None else None, stride,
                                                int(max_offset), wide_mode(mode), int(max_lag),
                                                rows.ctypes.data_as(C.POINTER(WideDelay)), _stream_ptr(stream)))
    rows = rows[:n_pairs]
    out = {k: np.ascontiguousarray(rows[k]) for k in ("lag", "coarse_lag", "factor", "flags")}
    for stage in ("fine", "coarse"):
        out[stage] = {k: np.ascontiguousarray(rows[stage][k]) for k in ("lag", "peak", "runner_up", "norm")}
    return out


def _need_wide(wide, align, drift=False, track=False, steps=False):
    if wide is None:
        return
    if align is None:
        raise ValueError("wide= requires align= (a max_lag): the wide estimate ends in a fine search of that range")
    for name, given in (("drift", drift), ("track", track), ("steps", steps)):
        if given:
            raise ValueError("wide= and %s= exclude each other for now: the windows around a wide lag are not covered" % name)


def _need_align(subsample, align, drift=False, track=False, steps=False):
    if steps and drift:
        raise PeaqError("steps= and drift= exclude each other: the pieces are the lines, one or two per window")
    if steps and track:
        raise PeaqError("steps= and track= exclude each other: the pieces are the track's segments, cut where a step was located")
    if steps and subsample:
        raise PeaqError("steps= and subsample=True exclude each other: the track's knots carry the sub-sample part")
    if steps and align is None:
        raise PeaqError("steps= requires align= (a max_lag): the track is measured around an integer lag")
    if track and drift:
        raise PeaqError("track= and drift= exclude each other: the track's segments are the lines, one per window")
    if track and subsample:
        raise PeaqError("track= and subsample=True exclude each other: the track's knots carry the sub-sample part")
    if track and align is None:
        raise PeaqError("track= requires align= (a max_lag): the track is measured around an integer lag")
    if subsample and drift:
        raise PeaqError("drift= and subsample=True exclude each other: the line's offset a carries the sub-sample part")
    if subsample and align is None:
        raise PeaqError("subsample=True requires align= (a max_lag): the sub-sample estimate refines an integer lag")
    if drift and align is None:
        raise PeaqError("drift= requires align= (a max_lag): the line is fitted around an integer lag")


def align(ctx, ref, test, lags, n_ref=None, n_test=None, stream=None, gain=None, gain_per_channel=False, max_gain_db=40.0,
          subsample=False, drift=False, track=False, steps=False):
    """Cuts both buffers of a batch to each pair's common, aligned part for the given lags (aligned_lengths, cut).
    gain: 'lsq' 'rms' 'polarity': the test signal's gain is measured over that part and applied in its cut
    (measure_gain, cut_scaled); the record tensor is kept as align.last_gain.
    subsample: the sub-sample part of each pair's delay is estimated around its lag (refine_delay, records kept as
    align.last_subdelay) and the test signal is cut through the shift filter (cut_shifted); a gain is then measured on
    the two CUT buffers and applied into a further buffer.
    drift: True or a window: each pair's delay is fitted as a line around its lag (estimate_drift, records kept as
    align.last_drift), both signals are cut to drift_lengths and the test signal is resampled along the line
    (cut_drift); a gain is then measured on the two CUT buffers, as with subsample, which drift excludes.
    track: True or a window: each pair's delay is kept as a track of per-window delays around its lag (estimate_track,
    records kept as align.last_track), both signals are cut to track_lengths and the test signal is resampled along the
    track (cut_track); a gain is then measured on the two CUT buffers.  Excludes drift and subsample.
    steps: True or a window: as track, with the steps of the delay located inside their windows and the track rebuilt as
    pieces that jump there (estimate_steps, records kept as align.last_steps; pieces_lengths; cut_pieces).  Excludes
    track, drift and subsample.
    Returns (ref', test', n', n'): two new tensors with one common stride and the common lengths (numpy uint32)."""
    if steps:
        _need_align(subsample, 0, drift, track, steps)
        return _align_steps(ctx, ref, test, lags, n_ref, n_test, stream, gain, gain_per_channel, max_gain_db,
                            _steps_window(steps))
    if track:
        _need_align(subsample, 0, drift, track)
        return _align_track(ctx, ref, test, lags, n_ref, n_test, stream, gain, gain_per_channel, max_gain_db,
                            _track_window(track))
    if drift:
        return _align_drift(ctx, ref, test, lags, n_ref, n_test, stream, gain, gain_per_channel, max_gain_db,
                            _drift_window(drift), subsample)
    n_pairs, stride, _ = ref.shape
    assert (n_ref is None) == (n_test is None), "n_ref and n_test: both or neither"
    a_ref = np.full(n_pairs, stride, dtype=np.uint32) if n_ref is None else np.asarray(n_ref, dtype=np.uint32)
    a_test = np.full(n_pairs, stride, dtype=np.uint32) if n_test is None else np.asarray(n_test, dtype=np.uint32)
    cuts = np.array([aligned_lengths(int(lags[p]), int(a_ref[p]), int(a_test[p])) for p in range(n_pairs)],
                    dtype=np.uint32).reshape(n_pairs, 3)
    import torch
    o_stride = max(int(cuts[:, 2].max()) if n_pairs else 0, 2)
    with _torch_stream(stream):
        bufs = [torch.zeros((n_pairs, o_stride + (o_stride & 1), ref.shape[2]), dtype=torch.float32, device=ref.device)
                for _ in range(3 if subsample and gain is not None else 2)]
    n = np.ascontiguousarray(cuts[:, 2])
    if subsample:
        sub = refine_delay(ctx, ref, test, lags, n_ref, n_test, stream=stream)
        align.last_subdelay = sub
        cut(ctx, ref, cuts[:, 0], n, out=bufs[0], stream=stream)
        cut_shifted(ctx, test, cuts[:, 1], n, sub["q"], n_in=a_test, out=bufs[1], stream=stream)
        if gain is not None:
            rec, _ = measure_gain(ctx, bufs[0], bufs[1], gain, None, None, n, max_gain_db=max_gain_db,
                                  per_channel=gain_per_channel, stream=stream)
            cut_scaled(ctx, bufs[1], np.zeros(n_pairs, np.uint32), n, rec, out=bufs[2], stream=stream)
            align.last_gain = rec
            return bufs[0], bufs[2], n, n.copy()
    elif gain is None:
        cut(ctx, ref, cuts[:, 0], cuts[:, 2], out=bufs[0], stream=stream)
        cut(ctx, test, cuts[:, 1], cuts[:, 2], out=bufs[1], stream=stream)
    else:
        rec, _ = measure_gain(ctx, ref, test, gain, cuts[:, 0], cuts[:, 1], cuts[:, 2], max_gain_db=max_gain_db,
                              per_channel=gain_per_channel, stream=stream)
        cut(ctx, ref, cuts[:, 0], cuts[:, 2], out=bufs[0], stream=stream)
        cut_scaled(ctx, test, cuts[:, 1], cuts[:, 2], rec, out=bufs[1], stream=stream)
        align.last_gain = rec
    return bufs[0], bufs[1], n, n.copy()


def _align_drift(ctx, ref, test, lags, n_ref, n_test, stream, gain, gain_per_channel, max_gain_db, window, subsample=False):
    """align(..., drift=window)"""
    if subsample:
        _need_align(True, 0, True)
    return _align_along(
        ctx, ref, test, lags, n_ref, n_test, stream, gain, gain_per_channel, max_gain_db, "last_drift",
        lambda: estimate_drift(ctx, ref, test, lags, n_ref, n_test, window=window, stream=stream),
        lambda dr, p, nr, nt: drift_lengths(int(lags[p]), dr["a"][p], dr["e"][p], nr, nt),
        lambda dr, skip, n, a_test, out: cut_drift(ctx, test, skip, n, dr["a"], dr["e"], n_in=a_test, out=out, stream=stream))


def _align_track(ctx, ref, test, lags, n_ref, n_test, stream, gain, gain_per_channel, max_gain_db, window):
    """align(..., track=window)"""
    def lengths(tr, p, nr, nt):
        k = tr["n_segments"][p]
        return track_lengths(int(lags[p]), window, tr["a"][p, :k], tr["e"][p, :k], nr, nt)
    return _align_along(
        ctx, ref, test, lags, n_ref, n_test, stream, gain, gain_per_channel, max_gain_db, "last_track",
        lambda: estimate_track(ctx, ref, test, lags, n_ref, n_test, window=window, stream=stream), lengths,
        lambda tr, skip, n, a_test, out: cut_track(ctx, test, skip, n, window, tr["n_segments"], tr["a"], tr["e"], n_in=a_test,
                                                   out=out, stream=stream))


def _align_steps(ctx, ref, test, lags, n_ref, n_test, stream, gain, gain_per_channel, max_gain_db, window):
    """align(..., steps=window)"""
    def lengths(st, p, nr, nt):
        k = st["n_pieces"][p]
        return pieces_lengths(int(lags[p]), st["b"][p, :k], st["a"][p, :k], st["e"][p, :k], nr, nt)
    return _align_along(
        ctx, ref, test, lags, n_ref, n_test, stream, gain, gain_per_channel, max_gain_db, "last_steps",
        lambda: estimate_steps(ctx, ref, test, lags, n_ref, n_test, window=window, stream=stream), lengths,
        lambda st, skip, n, a_test, out: cut_pieces(ctx, test, skip, n, st["n_pieces"], st["b"], st["a"], st["e"], n_in=a_test,
                                                    out=out, stream=stream))


def _align_along(ctx, ref, test, lags, n_ref, n_test, stream, gain, gain_per_channel, max_gain_db, keep, estimate, lengths,
                 cut_test):
    """what align(..., drift=), (..., track=) and (..., steps=) share.  estimate(): the stage's records, kept as
    align.<keep>; lengths(records, p, n_ref, n_test): pair p's (skip_ref, skip_test, n_keep); cut_test(records, skip,
    n_keep, n_test, out): the stage's cut of the test buffer.  The reference is cut plainly; a gain is measured on the
    two CUT buffers and applied into a third."""
    import torch
    n_pairs, stride, _ = ref.shape
    assert (n_ref is None) == (n_test is None), "n_ref and n_test: both or neither"
    a_ref = np.full(n_pairs, stride, dtype=np.uint32) if n_ref is None else np.asarray(n_ref, dtype=np.uint32)
    a_test = np.full(n_pairs, stride, dtype=np.uint32) if n_test is None else np.asarray(n_test, dtype=np.uint32)
    est = estimate()
    setattr(align, keep, est)
    cuts = np.array([lengths(est, p, int(a_ref[p]), int(a_test[p])) for p in range(n_pairs)],
                    dtype=np.uint32).reshape(n_pairs, 3)
    o_stride = max(int(cuts[:, 2].max()) if n_pairs else 0, 2)
    with _torch_stream(stream):
        bufs = [torch.zeros((n_pairs, o_stride + (o_stride & 1), ref.shape[2]), dtype=torch.float32, device=ref.device)
                for _ in range(3 if gain is not None else 2)]
    n = np.ascontiguousarray(cuts[:, 2])
    cut(ctx, ref, cuts[:, 0], n, out=bufs[0], stream=stream)
    cut_test(est, cuts[:, 1], n, a_test, bufs[1])
    if gain is not None:
        rec, _ = measure_gain(ctx, bufs[0], bufs[1], gain, None, None, n, max_gain_db=max_gain_db,
                              per_channel=gain_per_channel, stream=stream)
        cut_scaled(ctx, bufs[1], np.zeros(n_pairs, np.uint32), n, rec, out=bufs[2], stream=stream)
        align.last_gain = rec
        return bufs[0], bufs[2], n, n.copy()
    return bufs[0], bufs[1], n, n.copy()


def _aligned(ctx, ref, test, n_ref, n_test, max_lag, stream, gain=None, gain_per_channel=False, max_gain_db=40.0,
             subsample=False, drift=False, track=False, steps=False, wide=None, wide_mode="envelope"):
    """the `align=`, `gain=` and `subsample=` keywords of batch_run / batch_trajectory / batch_trace: estimate (without
    align: lags of 0; with wide: the wide estimate, its records kept as align.last_wide), then refine, match and cut"""
    _need_align(subsample, max_lag, drift, track, steps)
    _need_wide(wide, max_lag, drift, track, steps)
    if wide is not None:
        align.last_wide = estimate_delay_wide(ctx, ref, test, wide, wide_mode, max_lag, n_ref, n_test, stream=stream)
        lags = align.last_wide["lag"]
    elif max_lag is not None:
        lags = estimate_delay(ctx, ref, test, max_lag, n_ref, n_test, stream=stream)["lag"]
    else:
        lags = np.zeros(ref.shape[0], dtype=np.int32)
    if steps:
        return align(ctx, ref, test, lags, n_ref, n_test, stream=stream, gain=gain, gain_per_channel=gain_per_channel,
                     max_gain_db=max_gain_db, steps=steps)
    if track:
        return align(ctx, ref, test, lags, n_ref, n_test, stream=stream, gain=gain, gain_per_channel=gain_per_channel,
                     max_gain_db=max_gain_db, track=track)
    if drift:
        return align(ctx, ref, test, lags, n_ref, n_test, stream=stream, gain=gain, gain_per_channel=gain_per_channel,
                     max_gain_db=max_gain_db, drift=drift)
    if subsample:
        return align(ctx, ref, test, lags, n_ref, n_test, stream=stream, gain=gain, gain_per_channel=gain_per_channel,
                     max_gain_db=max_gain_db, subsample=True)
    if gain is None:
        return align(ctx, ref, test, lags, n_ref, n_test, stream=stream)
    return align(ctx, ref, test, lags, n_ref, n_test, stream=stream, gain=gain, gain_per_channel=gain_per_channel,
                 max_gain_db=max_gain_db)


def _batch_front(ctx, ref, test, n_ref, n_test, rate, align, stream, gain=None, gain_per_channel=False, max_gain_db=40.0,
                 subsample=False, drift=False, track=False, steps=False, both_lengths=True, wide=None, wide_mode="envelope"):
    """The front the batch_* functions share: convert to 48 kHz, align / match / cut as the keywords ask (_aligned has
    the order of precedence), hold the tensors against what the library takes, make the host length arrays.
    both_lengths=False (batch_run, batch_trajectory): n_ref without n_test is left to numpy and the library.
    Returns ref, test, a_ref, a_test and the two length arguments of the library's entry."""
    import torch
    if int(rate) != 48000:
        ref, test, n_ref, n_test = _to_48k(ctx, ref, test, n_ref, n_test, rate, stream)
    _need_align(subsample, align, drift, track, steps)
    _need_wide(wide, align, drift, track, steps)
    if steps or track or drift or subsample or gain is not None or align is not None:
        ref, test, n_ref, n_test = _aligned(ctx, ref, test, n_ref, n_test, align, stream, gain, gain_per_channel, max_gain_db,
                                            subsample=bool(subsample), drift=drift, track=track, steps=steps, wide=wide,
                                            wide_mode=wide_mode)
    assert ref.is_cuda and test.is_cuda and ref.dtype == torch.float32 and test.dtype == torch.float32
    assert ref.is_contiguous() and test.is_contiguous() and ref.shape == test.shape and ref.dim() == 3
    if both_lengths:
        assert (n_ref is None) == (n_test is None), "n_ref and n_test: both or neither"
    a_ref = a_test = None
    if n_ref is not None:
        a_ref = np.ascontiguousarray(n_ref, dtype=np.uint32)
        a_test = np.ascontiguousarray(n_test, dtype=np.uint32)
    u32p = C.POINTER(C.c_uint32)
    len_args = (a_ref.ctypes.data_as(u32p) if a_ref is not None else None,
                a_test.ctypes.data_as(u32p) if a_test is not None else None)
    return ref, test, a_ref, a_test, len_args


def _pair_counts(n_pairs, stride, a_ref, a_test, filter_bank=False):
    """frames (filter_bank: blocks) of every pair of a batch, counted once per distinct pair of lengths"""
    lens = [(stride, stride)] * n_pairs if a_ref is None else list(zip(a_ref.tolist(), a_test.tolist()))
    cnt = {rt: frame_count(*rt, filter_bank) for rt in set(lens)}
    return np.array([cnt[rt] for rt in lens], dtype=np.uint32)


def _host_pair(ref, test):
    """the two signals of a run_pair_* call as the library takes them: the arrays, their channel count and the four
    arguments of the entry"""
    ref = np.ascontiguousarray(ref, dtype=np.float32)
    test = np.ascontiguousarray(test, dtype=np.float32)
    assert test.shape[1] == ref.shape[1]
    fp = C.POINTER(C.c_float)
    return ref, test, ref.shape[1], (ref.ctypes.data_as(fp), len(ref), test.ctypes.data_as(fp), len(test))


def _lens_48k(ref, test, rate):
    """the lengths a run_pair_* call's signals have at 48 kHz"""
    if int(rate) == 48000:
        return [len(ref), len(test)]
    return [resampled_length(len(ref), rate), resampled_length(len(test), rate)]


def _delay_dict(rec):
    return dict(lag=int(rec.lag), peak=rec.peak, runner_up=rec.runner_up, norm=rec.norm)


def batch_run(ctx, advanced, ref, test, n_ref=None, n_test=None, playback_level=92.0, results=None,
              stream=None, sync=True, rate=48000, align=None, gain=None, gain_per_channel=False, max_gain_db=40.0,
              subsample=False, drift=False, track=False, steps=False, wide=None, wide_mode="envelope"):
    """ref/test: CUDA float32 tensors [n_pairs, n_samples, channels] (contiguous).
    wide: a max_offset in 48 kHz samples (up to 2^20), with align: every pair's lag comes from the wide estimate, coarse
    to fine with align as the fine stage's range (estimate_delay_wide; wide_mode 'envelope' or 'waveform';
    align.last_wide), and goes into the cut as before; gain and subsample work with it unchanged.  Excludes drift, track
    and steps.
    steps: True or a window, with align: as track, with the steps of every pair's delay located and the test signal cut
    along pieces that jump there (estimate_steps, cut_pieces; align.last_steps).  Excludes track, drift and subsample.
    track: True or a window, with align: every pair's delay is kept as a track of per-window delays and the test signal
    is resampled along it (estimate_track, cut_track; align.last_track); a gain is then measured after that cut.
    Excludes drift and subsample.
    drift: True or a window, with align: every pair's delay is fitted as a line and the test signal is resampled along
    it (estimate_drift, cut_drift; align.last_drift); a gain is then measured after that cut.  Excludes subsample.
    subsample: with align, the sub-sample part of every pair's delay is estimated and removed from the test signal too
    (refine_delay, cut_shifted; align.last_subdelay); a gain is then measured after the shift.
    gain: 'lsq' 'rms' 'polarity': the test signal's level (polarity) is matched to the reference's over the common part,
    after the alignment if there is one (measure_gain, cut_scaled); gain_per_channel, max_gain_db as measure_gain's.
    n_ref/n_test: optional per-pair lengths (samples per channel).
    rate: sampling rate of ref/test; anything but 48000 is converted on the device first (resample).
    align: a max_lag in 48 kHz samples: every pair's delay is estimated and both signals are cut to their common,
    aligned part first (estimate_delay, align), after the rate conversion.
    Returns a list of result dicts (sync=True) or the device result tensor."""
    import torch
    ref, test, a_ref, a_test, len_args = _batch_front(ctx, ref, test, n_ref, n_test, rate, align, stream, gain,
                                                      gain_per_channel, max_gain_db, subsample, drift, track, steps,
                                                      both_lengths=False, wide=wide, wide_mode=wide_mode)
    n_pairs, stride, channels = ref.shape
    if results is None:
        results = torch.empty((n_pairs, RESULT_DOUBLES), dtype=torch.float64, device=ref.device)
    _check(ctx.L.peaq_batch_run(ctx.h, int(bool(advanced)), channels, float(playback_level), n_pairs,
                                C.c_void_p(ref.data_ptr()), C.c_void_p(test.data_ptr()), stride, *len_args,
                                stride, C.c_void_p(results.data_ptr()), _stream_ptr(stream)))
    if not sync:
        return results
    torch.cuda.synchronize(ref.device)
    rows = results.cpu().numpy()
    return [_result_dict(r, advanced) for r in rows]


def batch_trajectory(ctx, advanced, ref, test, interval, n_points, n_ref=None, n_test=None, playback_level=92.0,
                     stream=None, sync=True, rate=48000, align=None, gain=None, gain_per_channel=False, max_gain_db=40.0,
                     subsample=False):
    """Readings every `interval` samples per channel through each pair (peaq_batch_run_trajectory): point k of pair p
    is what a session pushed the first min((k + 1) interval, n) samples of each signal reads, unflushed.
    ref/test, rate and align as for batch_run; `interval` counts samples at 48 kHz whatever the rate.  Returns
    (points, results): lists of result dicts, points[p][k], (sync=True) or the device tensors [n_pairs, n_points, 16]
    and [n_pairs, 16]."""
    import torch
    ref, test, a_ref, a_test, len_args = _batch_front(ctx, ref, test, n_ref, n_test, rate, align, stream, gain,
                                                      gain_per_channel, max_gain_db, subsample, both_lengths=False)
    n_pairs, stride, channels = ref.shape
    n_points = int(n_points)
    points = torch.empty((n_pairs, max(n_points, 1), RESULT_DOUBLES), dtype=torch.float64, device=ref.device)
    results = torch.empty((n_pairs, RESULT_DOUBLES), dtype=torch.float64, device=ref.device)
    _check(ctx.L.peaq_batch_run_trajectory(ctx.h, int(bool(advanced)), channels, float(playback_level), n_pairs,
                                           C.c_void_p(ref.data_ptr()), C.c_void_p(test.data_ptr()), stride, *len_args,
                                           stride, int(interval), n_points, C.c_void_p(points.data_ptr()),
                                           C.c_void_p(results.data_ptr()), _stream_ptr(stream)))
    if not sync:
        return points, results
    torch.cuda.synchronize(ref.device)
    pts = points.cpu().numpy()
    return ([[_result_dict(r, advanced) for r in row] for row in pts],
            [_result_dict(r, advanced) for r in results.cpu().numpy()])


def run_pair_trajectory(ctx, advanced, ref, test, interval, n_points, playback_level=92.0, rate=48000):
    """peaq_run_pair_trajectory: one whole pair from host memory (numpy float32 [n, channels]);
    returns (points, result) as result dicts.  rate other than 48000: the pair is converted on the device first and
    read through batch_trajectory (interval in 48 kHz samples)."""
    ref = np.ascontiguousarray(ref, dtype=np.float32)
    test = np.ascontiguousarray(test, dtype=np.float32)
    ch = ref.shape[1]
    assert test.shape[1] == ch
    if int(rate) != 48000:
        import torch
        n = max(len(ref), len(test), 1)
        both = np.zeros((2, n, ch), dtype=np.float32)
        both[0, :len(ref)], both[1, :len(test)] = ref, test
        d = torch.from_numpy(both).cuda(ctx.device)
        pts, res = batch_trajectory(ctx, advanced, d[0:1], d[1:2], interval, n_points, [len(ref)], [len(test)],
                                    playback_level, rate=rate)
        return pts[0], res[0]
    pts = np.zeros((max(int(n_points), 1), RESULT_DOUBLES))
    out = np.zeros(RESULT_DOUBLES)
    dp = C.POINTER(C.c_double)
    _check(ctx.L.peaq_run_pair_trajectory(ctx.h, int(bool(advanced)), ch, float(playback_level),
                                          ref.ctypes.data_as(C.POINTER(C.c_float)), len(ref),
                                          test.ctypes.data_as(C.POINTER(C.c_float)), len(test),
                                          int(interval), int(n_points), pts.ctypes.data_as(dp), out.ctypes.data_as(dp)))
    return [_result_dict(r, bool(advanced)) for r in pts], _result_dict(out, bool(advanced))


def _check_trace_sizes(L):
    fb, bb = C.c_size_t(0), C.c_size_t(0)
    L.peaq_trace_sizes(C.byref(fb), C.byref(bb))
    if (fb.value, bb.value) != (C.sizeof(FrameTrace), C.sizeof(BlockTrace)) or \
            (fb.value, bb.value) != (FRAME_TRACE_DTYPE.itemsize, BLOCK_TRACE_DTYPE.itemsize):
        raise PeaqError(f"the library's trace records are {fb.value} and {bb.value} bytes, this binding's "
                        f"{C.sizeof(FrameTrace)} and {C.sizeof(BlockTrace)}")


def frame_count(n_ref, n_test, filter_bank=False):
    """frames (filter_bank: blocks) of a pair with these lengths, the flush's included (peaq_frame_count)"""
    return int(load_library().peaq_frame_count(int(n_ref), int(n_test), int(bool(filter_bank))))


def batch_trace(ctx, advanced, ref, test, n_ref=None, n_test=None, playback_level=92.0, rate=48000, align=None,
                stream=None, sync=True, d_frames=None, d_blocks=None, gain=None, gain_per_channel=False, max_gain_db=40.0,
                subsample=False):
    """The MOV layer's values of every frame and block of every pair, in the run that scores them
    (peaq_batch_run_trace).  ref/test, n_ref/n_test, rate and align as for batch_run.  d_frames / d_blocks: optional
    record tensors to write into (CUDA uint8 [n_pairs, stride, 128] / [.., 96]; records past a pair's count keep what
    they held); without them zero-filled ones of the longest pair's count are made.
    Returns a dict: d_frames / d_blocks, the record tensors (CUDA uint8 [n_pairs, stride, 128] / [n_pairs, stride, 96],
    zero-filled past each pair's count; d_blocks None in the basic version), d_results [n_pairs, 16], n_frames /
    n_blocks (numpy, the counts per pair), and with sync=True frames / blocks (numpy structured views of the records by
    field name, FRAME_TRACE_DTYPE / BLOCK_TRACE_DTYPE, [n_pairs, stride]) and results (result dicts)."""
    import torch
    _check_trace_sizes(ctx.L)
    ref, test, a_ref, a_test, len_args = _batch_front(ctx, ref, test, n_ref, n_test, rate, align, stream, gain,
                                                      gain_per_channel, max_gain_db, subsample)
    n_pairs, stride, channels = ref.shape
    n_frames = _pair_counts(n_pairs, stride, a_ref, a_test)
    n_blocks = _pair_counts(n_pairs, stride, a_ref, a_test, True) if advanced else np.zeros(n_pairs, dtype=np.uint32)
    f_stride = max(int(n_frames.max()) if n_pairs else 0, 1)
    b_stride = max(int(n_blocks.max()) if n_pairs else 0, 1)
    with _torch_stream(stream):                        # the zero fill runs on the stream the batch runs on
        if d_frames is None:
            d_frames = torch.zeros((n_pairs, f_stride, C.sizeof(FrameTrace)), dtype=torch.uint8, device=ref.device)
        if d_blocks is None and advanced:
            d_blocks = torch.zeros((n_pairs, b_stride, C.sizeof(BlockTrace)), dtype=torch.uint8, device=ref.device)
        results = torch.empty((n_pairs, RESULT_DOUBLES), dtype=torch.float64, device=ref.device)
    for t, size in ((d_frames, C.sizeof(FrameTrace)),) + (((d_blocks, C.sizeof(BlockTrace)),) if advanced else ()):
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 3
        assert t.shape[0] == n_pairs and t.shape[2] == size
    f_stride, b_stride = d_frames.shape[1], d_blocks.shape[1] if advanced else 0
    _check(ctx.L.peaq_batch_run_trace(ctx.h, int(bool(advanced)), channels, float(playback_level), n_pairs,
                                      C.c_void_p(ref.data_ptr()), C.c_void_p(test.data_ptr()), stride, *len_args, stride,
                                      C.c_void_p(d_frames.data_ptr()), f_stride,
                                      C.c_void_p(d_blocks.data_ptr()) if advanced else None, b_stride,
                                      C.c_void_p(results.data_ptr()), _stream_ptr(stream)))
    out = dict(d_frames=d_frames, d_blocks=d_blocks if advanced else None, d_results=results, n_frames=n_frames, n_blocks=n_blocks)
    if not sync:
        return out
    torch.cuda.synchronize(ref.device)
    out["frames"] = d_frames.cpu().numpy().view(FRAME_TRACE_DTYPE)[:, :, 0]
    out["blocks"] = d_blocks.cpu().numpy().view(BLOCK_TRACE_DTYPE)[:, :, 0] if advanced else None
    out["results"] = [_result_dict(r, advanced) for r in results.cpu().numpy()]
    return out


def run_pair_trace(ctx, advanced, ref, test, playback_level=92.0, rate=48000, align=None):
    """peaq_run_pair_trace: one whole pair from host memory (numpy float32 [n, channels]), sampled at `rate`, aligned
    first with align = a max_lag in 48 kHz samples.  Returns a dict: frames / blocks (numpy structured arrays
    FRAME_TRACE_DTYPE / BLOCK_TRACE_DTYPE of the counts written; blocks None in the basic version), result (a result
    dict) and, with align, delay."""
    ref, test, ch, pair_args = _host_pair(ref, test)
    _check_trace_sizes(ctx.L)
    lens = _lens_48k(ref, test, rate)
    f_cap = max(frame_count(*lens), 1)
    b_cap = max(frame_count(*lens, True), 1) if advanced else 0
    frames = np.zeros(f_cap, dtype=FRAME_TRACE_DTYPE)
    blocks = np.zeros(b_cap, dtype=BLOCK_TRACE_DTYPE) if advanced else None
    nf, nb, rec, out = C.c_uint32(0), C.c_uint32(0), Delay(), np.zeros(RESULT_DOUBLES)
    _check(ctx.L.peaq_run_pair_trace(ctx.h, int(bool(advanced)), ch, float(playback_level), int(rate),
                                     0 if align is None else int(align), *pair_args,
                                     C.c_void_p(frames.ctypes.data), f_cap, C.byref(nf),
                                     C.c_void_p(blocks.ctypes.data) if advanced else None, b_cap, C.byref(nb),
                                     C.byref(rec), out.ctypes.data_as(C.POINTER(C.c_double))))
    res = dict(frames=frames[:nf.value], blocks=blocks[:nb.value] if advanced else None,
               result=_result_dict(out, bool(advanced)))
    if align is not None:
        res["delay"] = _delay_dict(rec)
    return res


def _planes_mask(planes, table, what):
    if isinstance(planes, (int, np.integer)):
        return int(planes)
    if isinstance(planes, str):
        planes = [planes]
    unknown = [p for p in planes if p not in table]
    if unknown:
        raise PeaqError(f"unknown {what} {unknown[0]!r} (one of {', '.join(table)})")
    mask = 0
    for p in planes:
        mask |= table[p]
    return mask


def _planes_dict(rows, mask, table, n_bands):
    """rows [..., n_planes, row] -> {name: [..., n_bands]} in the order of the slots, the pad column (if any) removed"""
    names = [name for name, bit in table.items() if mask & bit]
    return {name: rows[..., k, :n_bands] for k, name in enumerate(names)}


def _band_tables(entry, n):
    fc, second = np.zeros(n), np.zeros(n)
    dp = C.POINTER(C.c_double)
    _check(entry(fc.ctypes.data_as(dp), second.ctypes.data_as(dp)))
    return fc, second


def band_planes_mask(planes):
    """a PEAQ_BAND_* mask from plane names (BAND_PLANES; one name, or several in any order) or from a mask"""
    return _planes_mask(planes, BAND_PLANES, "band plane")


def band_tables(advanced):
    """(fc, mask_diff): the centre frequencies in Hz and the mask_diff factors of the 109 (advanced: 55) bands of the
    FFT path (peaq_band_tables; host only)"""
    L, adv = load_library(), int(bool(advanced))
    return _band_tables(lambda *a: L.peaq_band_tables(adv, *a), L.peaq_band_count(adv))


def fb_band_planes_mask(planes):
    """a PEAQ_FB_BAND_* mask from plane names (FB_BAND_PLANES; one name, or several in any order) or from a mask"""
    return _planes_mask(planes, FB_BAND_PLANES, "filter-bank band plane")


def fb_band_tables():
    """(fc, internal_noise): the centre frequencies in Hz and the internal noise of the 40 bands of the filter-bank
    path (peaq_fb_band_tables; host only)"""
    L = load_library()
    return _band_tables(L.peaq_fb_band_tables, L.peaq_fb_band_count())


def pattern_band_planes_mask(planes):
    """a PEAQ_PAT_BAND_* mask from plane names (PATTERN_BAND_PLANES; one name, or several in any order) or from a mask"""
    return _planes_mask(planes, PATTERN_BAND_PLANES, "pattern band plane")


def pattern_band_tables():
    """(fc, internal_noise): the centre frequencies in Hz and the internal noise of the 109 bands of the basic
    version's FFT path (peaq_pattern_band_tables; host only)"""
    L = load_library()
    return _band_tables(L.peaq_pattern_band_tables, L.peaq_band_count(0))


# What tells the three band-row outputs apart (FFT bands, filter-bank bands, pattern bands; _batch_band_rows and
# _run_pair_band_rows are their common bodies): the plane table, its word in messages and its valid bits; whether a row
# is a filter-bank block (else an FFT frame); the version it runs in (None: the entry takes `advanced`); (L, adv) ->
# (band count, row width in doubles); the library entry less its prefix; the tables function and its second key.
_BandRows = collections.namedtuple("_BandRows", "planes what all_bits blocks advanced shape entry tables second")
_BAND_ROWS = dict(
    fft=_BandRows(BAND_PLANES, "band plane", 31, False, None, lambda L, adv: (L.peaq_band_count(adv), L.peaq_band_row(adv)),
                  "bands", band_tables, "mask_diff"),
    fb=_BandRows(FB_BAND_PLANES, "filter-bank band plane", 0x1FFF, True, True, lambda L, adv: (L.peaq_fb_band_count(),) * 2,
                 "fb_bands", lambda adv: fb_band_tables(), "internal_noise"),
    pattern=_BandRows(PATTERN_BAND_PLANES, "pattern band plane", 0x1FFF, False, False,
                      lambda L, adv: (L.peaq_band_count(0), L.peaq_band_row(0)), "pattern_bands",
                      lambda adv: pattern_band_tables(), "internal_noise"))


def _batch_band_rows(kind, ctx, advanced, ref, test, planes, n_ref, n_test, playback_level, rate, align, stream, sync, d_bands):
    """batch_bands, batch_fb_bands and batch_pattern_bands (their docstrings have the arguments and what is returned)"""
    import torch
    k = _BAND_ROWS[kind]
    mask = _planes_mask(planes, k.planes, k.what)
    ref, test, a_ref, a_test, len_args = _batch_front(ctx, ref, test, n_ref, n_test, rate, align, stream)
    n_pairs, stride, channels = ref.shape
    counts = _pair_counts(n_pairs, stride, a_ref, a_test, k.blocks)
    adv = int(bool(advanced)) if k.advanced is None else int(k.advanced)
    (n_bands, row), n_planes = k.shape(ctx.L, adv), bin(mask & k.all_bits).count("1")
    with _torch_stream(stream):                        # the zero fill runs on the stream the batch runs on
        if d_bands is None:
            d_bands = torch.zeros((n_pairs, max(int(counts.max()) if n_pairs else 0, 1), channels, max(n_planes, 1), row),
                                  dtype=torch.float64, device=ref.device)
        results = torch.empty((n_pairs, RESULT_DOUBLES), dtype=torch.float64, device=ref.device)
    assert d_bands.is_cuda and d_bands.dtype == torch.float64 and d_bands.is_contiguous() and d_bands.dim() == 5
    assert d_bands.shape[0] == n_pairs and tuple(d_bands.shape[2:]) == (channels, max(n_planes, 1), row)
    _check(getattr(ctx.L, "peaq_batch_run_" + k.entry)(
        ctx.h, *((adv,) if k.advanced is None else ()), channels, float(playback_level), n_pairs,
        C.c_void_p(ref.data_ptr()), C.c_void_p(test.data_ptr()), stride, *len_args, stride, mask,
        C.c_void_p(d_bands.data_ptr()), d_bands.shape[1], C.c_void_p(results.data_ptr()), _stream_ptr(stream)))
    fc, second = k.tables(adv)
    out = {"d_bands": d_bands, "d_results": results, "counts": counts, "fc": fc, k.second: second, "planes": mask}
    if not sync:
        return out
    torch.cuda.synchronize(ref.device)
    out.update(_planes_dict(d_bands.cpu().numpy(), mask, k.planes, n_bands))
    out["results"] = [_result_dict(r, advanced if k.advanced is None else k.advanced) for r in results.cpu().numpy()]
    return out


def _run_pair_band_rows(kind, ctx, advanced, ref, test, planes, playback_level, rate, align):
    """run_pair_bands, run_pair_fb_bands and run_pair_pattern_bands"""
    k = _BAND_ROWS[kind]
    ref, test, ch, pair_args = _host_pair(ref, test)
    mask = _planes_mask(planes, k.planes, k.what)
    adv = int(bool(advanced)) if k.advanced is None else int(k.advanced)
    cap = max(frame_count(*_lens_48k(ref, test, rate), k.blocks), 1)
    n_bands, row = k.shape(ctx.L, adv)
    rows = np.zeros((cap, ch, max(bin(mask & k.all_bits).count("1"), 1), row))
    n, rec, out = C.c_uint32(0), Delay(), np.zeros(RESULT_DOUBLES)
    _check(getattr(ctx.L, "peaq_run_pair_" + k.entry)(
        ctx.h, *((adv,) if k.advanced is None else ()), ch, float(playback_level), int(rate),
        0 if align is None else int(align), *pair_args, mask, C.c_void_p(rows.ctypes.data), cap, C.byref(n), C.byref(rec),
        out.ctypes.data_as(C.POINTER(C.c_double))))
    fc, second = k.tables(adv)
    res = {**_planes_dict(rows[:n.value], mask, k.planes, n_bands), "result": _result_dict(out, bool(adv)), "fc": fc,
           k.second: second, "planes": mask}
    if align is not None:
        res["delay"] = _delay_dict(rec)
    return res


def batch_bands(ctx, advanced, ref, test, planes=("nmr",), n_ref=None, n_test=None, playback_level=92.0, rate=48000,
                align=None, stream=None, sync=True, d_bands=None):
    """The FFT path's values per frame, channel and band of every pair, in the run that scores them
    (peaq_batch_run_bands).  planes: names of BAND_PLANES (or a PEAQ_BAND_* mask); ref/test, n_ref/n_test, rate and
    align as for batch_run.  d_bands: an optional CUDA float64 tensor [n_pairs, stride, channels, n_planes, row] to
    write into (rows past a pair's count keep what they held); without it a zero-filled one of the longest pair's
    count is made.
    Returns a dict: every requested plane by name, np.ndarray [pairs, frames_max, channels, bands] (the pad column
    removed), counts (numpy, frames per pair), results (result dicts), fc and mask_diff (band_tables), planes (the
    mask), and d_bands / d_results, the device tensors.  sync=False: the device tensors, counts, fc, mask_diff and
    planes only."""
    return _batch_band_rows("fft", ctx, advanced, ref, test, planes, n_ref, n_test, playback_level, rate, align, stream,
                            sync, d_bands)


def run_pair_bands(ctx, advanced, ref, test, planes=("nmr",), playback_level=92.0, rate=48000, align=None):
    """peaq_run_pair_bands: one whole pair from host memory (numpy float32 [n, channels]), sampled at `rate`, aligned
    first with align = a max_lag in 48 kHz samples.  Returns a dict: every requested plane by name, np.ndarray
    [frames, channels, bands], result (a result dict), fc, mask_diff, planes (the mask) and, with align, delay."""
    return _run_pair_band_rows("fft", ctx, advanced, ref, test, planes, playback_level, rate, align)


def batch_fb_bands(ctx, ref, test, planes=("noiseloud",), n_ref=None, n_test=None, playback_level=92.0, rate=48000,
                   align=None, stream=None, sync=True, d_bands=None):
    """The filter-bank path's values per block, channel and band of every pair, in the run that scores them in the
    advanced version (peaq_batch_run_fb_bands).  planes: names of FB_BAND_PLANES (or a PEAQ_FB_BAND_* mask); ref/test,
    n_ref/n_test, rate and align as for batch_run.  d_bands: an optional CUDA float64 tensor [n_pairs, stride, channels,
    n_planes, 40] to write into (rows past a pair's count keep what they held); without it a zero-filled one of the
    longest pair's count is made.
    Returns a dict: every requested plane by name, np.ndarray [pairs, blocks_max, channels, 40], counts (numpy, blocks
    per pair), results (result dicts), fc and internal_noise (fb_band_tables), planes (the mask), and d_bands /
    d_results, the device tensors.  sync=False: the device tensors, counts, fc, internal_noise and planes only."""
    return _batch_band_rows("fb", ctx, True, ref, test, planes, n_ref, n_test, playback_level, rate, align, stream, sync,
                            d_bands)


def run_pair_fb_bands(ctx, ref, test, planes=("noiseloud",), playback_level=92.0, rate=48000, align=None):
    """peaq_run_pair_fb_bands: one whole pair from host memory (numpy float32 [n, channels]), sampled at `rate`, aligned
    first with align = a max_lag in 48 kHz samples.  Returns a dict: every requested plane by name, np.ndarray
    [blocks, channels, 40], result (a result dict), fc, internal_noise, planes (the mask) and, with align, delay."""
    return _run_pair_band_rows("fb", ctx, True, ref, test, planes, playback_level, rate, align)


def batch_pattern_bands(ctx, ref, test, planes=("noiseloud",), n_ref=None, n_test=None, playback_level=92.0, rate=48000,
                        align=None, stream=None, sync=True, d_bands=None):
    """The pattern layer's values per frame, channel and band of every pair, in the run that scores them in the basic
    version (peaq_batch_run_pattern_bands).  planes: names of PATTERN_BAND_PLANES (or a PEAQ_PAT_BAND_* mask); ref/test,
    n_ref/n_test, rate and align as for batch_run.  d_bands: an optional CUDA float64 tensor [n_pairs, stride, channels,
    n_planes, 110] to write into (rows past a pair's count keep what they held); without it a zero-filled one of the
    longest pair's count is made.
    Returns a dict: every requested plane by name, np.ndarray [pairs, frames_max, channels, 109] (the pad column
    removed), counts (numpy, frames per pair), results (result dicts), fc and internal_noise (pattern_band_tables),
    planes (the mask), and d_bands / d_results, the device tensors.  sync=False: the device tensors, counts, fc,
    internal_noise and planes only."""
    return _batch_band_rows("pattern", ctx, False, ref, test, planes, n_ref, n_test, playback_level, rate, align, stream,
                            sync, d_bands)


def run_pair_pattern_bands(ctx, ref, test, planes=("noiseloud",), playback_level=92.0, rate=48000, align=None):
    """peaq_run_pair_pattern_bands: one whole pair from host memory (numpy float32 [n, channels]), sampled at `rate`,
    aligned first with align = a max_lag in 48 kHz samples.  Returns a dict: every requested plane by name, np.ndarray
    [frames, channels, 109], result (a result dict), fc, internal_noise, planes (the mask) and, with align, delay."""
    return _run_pair_band_rows("pattern", ctx, False, ref, test, planes, playback_level, rate, align)


def _band_summary_views(rows, n_bands):
    """rows [..., R, row] (peaq_batch_run_band_summary) -> the named views [..., n_bands] and `counted` [...]: every
    view is its row over the row's denominator (entry n_bands), NaN where that is 0; moddiff1 / moddiff2 carry the
    factor 100 / n_bands, so that their sum over the bands is the channel's AvgModDiff."""
    rows = np.asarray(rows)

    def ratio(k, scale=1.0):
        den = rows[..., k, n_bands:n_bands + 1]
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(den != 0., scale * rows[..., k, :n_bands] / den, np.nan)

    out = dict(counted=rows[..., 0, n_bands].astype(np.int64), nmr_mean=ratio(0), nmr_disturbed=ratio(2),
               exc_ref_mean=ratio(3))
    out["nmr_max"] = np.where(rows[..., 1, n_bands:n_bands + 1] != 0., rows[..., 1, :n_bands], np.nan)
    if rows.shape[-2] > 4:
        out.update(exc_test_mean=ratio(4), moddiff1=ratio(5, 100. / n_bands), moddiff2=ratio(6, 100. / n_bands),
                   noiseloud_mean=ratio(7))
    return out


def batch_band_summary(ctx, advanced, ref, test, n_ref=None, n_test=None, playback_level=92.0, rate=48000, align=None,
                       d_summary=None, results=None, stream=None, sync=True):
    """Every pair's per-band summary, reduced over the pair's counted frames on the device in the run that scores the
    batch (peaq_batch_run_band_summary; include/peaq_amd.h has the rows and which frames count).  ref/test,
    n_ref/n_test, rate and align as for batch_bands.  d_summary: an optional CUDA float64 tensor [n_pairs (or more),
    channels, R, row] to write into (pairs past the batch keep what they held); results: an optional CUDA float64
    tensor [n_pairs, RESULT_DOUBLES].
    Returns a dict: rows, np.ndarray [pairs, channels, R, row] (BAND_SUMMARY_ROWS in row order, the denominators in
    the last entry of each row); the named views nmr_mean, nmr_max, nmr_disturbed (a fraction), exc_ref_mean and, in the
    basic version, exc_test_mean, moddiff1, moddiff2 (their sum over the bands is the channel's AvgModDiff) and
    noiseloud_mean, each [pairs, channels, bands] and NaN where its denominator is 0; counted [pairs, channels]; fc
    (band_tables); results (result dicts); and d_summary / d_results, the device tensors.  sync=False: the device
    tensors and fc only."""
    import torch
    advanced = bool(advanced)
    ref, test, a_ref, a_test, len_args = _batch_front(ctx, ref, test, n_ref, n_test, rate, align, stream)
    n_pairs, stride, channels = ref.shape
    n_bands, row, n_rows = ctx.L.peaq_band_count(advanced), ctx.L.peaq_band_row(advanced), ctx.L.peaq_band_summary_rows(advanced)
    with _torch_stream(stream):
        if d_summary is None:
            d_summary = torch.empty((n_pairs, channels, n_rows, row), dtype=torch.float64, device=ref.device)
        if results is None:
            results = torch.empty((n_pairs, RESULT_DOUBLES), dtype=torch.float64, device=ref.device)
    assert d_summary.is_cuda and d_summary.dtype == torch.float64 and d_summary.is_contiguous() and d_summary.dim() == 4
    assert d_summary.shape[0] >= n_pairs and tuple(d_summary.shape[1:]) == (channels, n_rows, row)
    assert results.is_cuda and results.dtype == torch.float64 and results.is_contiguous()
    _check(ctx.L.peaq_batch_run_band_summary(ctx.h, int(advanced), channels, float(playback_level), n_pairs,
                                             C.c_void_p(ref.data_ptr()), C.c_void_p(test.data_ptr()), stride,
                                             *len_args, stride, C.c_void_p(d_summary.data_ptr()), C.c_void_p(results.data_ptr()),
                                             _stream_ptr(stream)))
    fc, _ = band_tables(advanced)
    out = dict(d_summary=d_summary, d_results=results, fc=fc)
    if not sync:
        return out
    torch.cuda.synchronize(ref.device)
    rows = d_summary[:n_pairs].cpu().numpy()
    out.update(rows=rows, **_band_summary_views(rows, n_bands))
    out["results"] = [_result_dict(r, advanced) for r in results.cpu().numpy()]
    return out


def run_pair_band_summary(ctx, advanced, ref, test, playback_level=92.0, rate=48000, align=None):
    """peaq_run_pair_band_summary: one whole pair from host memory (numpy float32 [n, channels]), sampled at `rate`,
    aligned first with align = a max_lag in 48 kHz samples.  Returns a dict: rows [channels, R, row], the named views of
    batch_band_summary [channels, bands], counted [channels], fc, result (a result dict) and, with align, delay."""
    ref, test, ch, pair_args = _host_pair(ref, test)
    advanced = bool(advanced)
    n_bands, row, n_rows = ctx.L.peaq_band_count(advanced), ctx.L.peaq_band_row(advanced), ctx.L.peaq_band_summary_rows(advanced)
    rows = np.zeros((ch, n_rows, row))
    rec, out = Delay(), np.zeros(RESULT_DOUBLES)
    _check(ctx.L.peaq_run_pair_band_summary(ctx.h, int(advanced), ch, float(playback_level), int(rate),
                                            0 if align is None else int(align), *pair_args,
                                            C.c_void_p(rows.ctypes.data), C.byref(rec),
                                            out.ctypes.data_as(C.POINTER(C.c_double))))
    fc, _ = band_tables(advanced)
    res = dict(rows=rows, fc=fc, result=_result_dict(out, advanced), **_band_summary_views(rows, n_bands))
    if align is not None:
        res["delay"] = _delay_dict(rec)
    return res


def window_frames(n_ref, n_test, start, length):
    """(first, count): the FFT frames the window {start, length} covers of a pair with these lengths (peaq_window_frames;
    samples per channel at 48 kHz)"""
    first, count = C.c_uint32(0), C.c_uint32(0)
    _check(load_library().peaq_window_frames(int(n_ref), int(n_test), int(start), int(length), C.byref(first),
                                             C.byref(count)))
    return first.value, count.value


def sliding_windows(n, length, hop=None):
    """[start, length] rows (np.uint32 [k, 2]) of the windows of `length` samples every `hop` (default: length) that
    cover [0, n): all of the same length but the last, which ends at n"""
    n, length = int(n), int(length)
    hop = length if hop is None else int(hop)
    assert n > 0 and length > 0 and hop > 0
    rows, start = [], 0
    while True:
        rows.append((start, min(length, n - start)))
        if start + length >= n:
            break
        start += hop
    return np.array(rows, dtype=np.uint32).reshape(-1, 2)


def _windows_array(windows):
    w = np.ascontiguousarray(windows, dtype=np.uint32).reshape(-1, 2)
    return w, C.c_void_p(w.ctypes.data) if len(w) else None


def _batch_spans(entry_name, advanced, ctx, ref, test, spans, n_ref, n_test, playback_level, rate, align, stream, sync,
                 d_spans, results, gain, gain_per_channel, max_gain_db, subsample):
    """batch_windows (peaq_batch_run_windows, basic version) and batch_adv_spans (peaq_batch_run_adv_spans)"""
    import torch
    ref, test, a_ref, a_test, len_args = _batch_front(ctx, ref, test, n_ref, n_test, rate, align, stream, gain,
                                                      gain_per_channel, max_gain_db, subsample)
    n_pairs, stride, channels = ref.shape
    w, w_ptr = _windows_array(spans)
    with _torch_stream(stream):
        if d_spans is None:
            d_spans = torch.empty((n_pairs, max(len(w), 1), RESULT_DOUBLES), dtype=torch.float64, device=ref.device)
        if results is None:
            results = torch.empty((n_pairs, RESULT_DOUBLES), dtype=torch.float64, device=ref.device)
    assert d_spans.is_cuda and d_spans.dtype == torch.float64 and d_spans.is_contiguous()
    assert tuple(d_spans.shape) == (n_pairs, max(len(w), 1), RESULT_DOUBLES)
    assert results.is_cuda and results.dtype == torch.float64 and results.is_contiguous()
    _check(getattr(ctx.L, entry_name)(ctx.h, channels, float(playback_level), n_pairs, C.c_void_p(ref.data_ptr()),
                                      C.c_void_p(test.data_ptr()), stride, *len_args, stride, w_ptr, len(w),
                                      C.c_void_p(d_spans.data_ptr()), C.c_void_p(results.data_ptr()),
                                      _stream_ptr(stream)))
    if not sync:
        return d_spans, results
    torch.cuda.synchronize(ref.device)
    return ([[_result_dict(r, advanced) for r in row] for row in d_spans.cpu().numpy()],
            [_result_dict(r, advanced) for r in results.cpu().numpy()])


def _run_pair_spans(entry_name, advanced, key, ctx, ref, test, spans, playback_level, rate, align):
    """run_pair_windows (peaq_run_pair_windows, basic version) and run_pair_adv_spans (peaq_run_pair_adv_spans)"""
    ref, test, ch, pair_args = _host_pair(ref, test)
    w, w_ptr = _windows_array(spans)
    rows = np.zeros((max(len(w), 1), RESULT_DOUBLES))
    rec, out = Delay(), np.zeros(RESULT_DOUBLES)
    _check(getattr(ctx.L, entry_name)(ctx.h, ch, float(playback_level), int(rate), 0 if align is None else int(align),
                                      *pair_args, w_ptr, len(w), C.c_void_p(rows.ctypes.data), C.byref(rec),
                                      out.ctypes.data_as(C.POINTER(C.c_double))))
    res = {key: [_result_dict(r, advanced) for r in rows[:len(w)]], "result": _result_dict(out, advanced)}
    if align is not None:
        res["delay"] = _delay_dict(rec)
    return res


def batch_windows(ctx, ref, test, windows, n_ref=None, n_test=None, playback_level=92.0, rate=48000, align=None,
                  stream=None, sync=True, d_windows=None, results=None, gain=None, gain_per_channel=False,
                  max_gain_db=40.0, subsample=False):
    """The score of time windows inside every pair, in the run that scores the batch (peaq_batch_run_windows, basic
    version; include/peaq_amd.h has which frames a window covers and what its reading is: a view into the running
    stream, not a cold start).  windows: [start, length] rows in samples per channel at 48 kHz, shared by all pairs
    (sliding_windows makes them).  ref/test, n_ref/n_test, rate, align, gain and subsample as for batch_trace.
    d_windows / results: optional CUDA float64 tensors [n_pairs, n_windows, 16] / [n_pairs, 16] to write into.
    Returns (windows, results): lists of result dicts, windows[p][w], (sync=True) or the device tensors."""
    return _batch_spans("peaq_batch_run_windows", False, ctx, ref, test, windows, n_ref, n_test, playback_level, rate,
                        align, stream, sync, d_windows, results, gain, gain_per_channel, max_gain_db, subsample)


def run_pair_windows(ctx, ref, test, windows, playback_level=92.0, rate=48000, align=None):
    """peaq_run_pair_windows: one whole pair from host memory (numpy float32 [n, channels]), sampled at `rate`, aligned
    first with align = a max_lag in 48 kHz samples; the windows count 48 kHz samples of the signals as scored.  Returns
    a dict: windows (result dicts, one per window), result (a result dict) and, with align, delay."""
    return _run_pair_spans("peaq_run_pair_windows", False, "windows", ctx, ref, test, windows, playback_level, rate, align)


def span_blocks(n_ref, n_test, start, length):
    """(first, count): the filter-bank blocks the span {start, length} covers of a pair with these lengths
    (peaq_span_blocks; samples per channel at 48 kHz).  Its FFT frames are window_frames'."""
    first, count = C.c_uint32(0), C.c_uint32(0)
    _check(load_library().peaq_span_blocks(int(n_ref), int(n_test), int(start), int(length), C.byref(first),
                                           C.byref(count)))
    return first.value, count.value


def batch_adv_spans(ctx, ref, test, spans, n_ref=None, n_test=None, playback_level=92.0, rate=48000, align=None,
                    stream=None, sync=True, d_spans=None, results=None, gain=None, gain_per_channel=False,
                    max_gain_db=40.0, subsample=False):
    """The score of time spans inside every pair in the advanced version, in the run that scores the batch
    (peaq_batch_run_adv_spans; include/peaq_amd.h has which frames and blocks a span covers and what its reading is: a
    view into the running stream, not a cold start).  spans: [start, length] rows in samples per channel at 48 kHz,
    shared by all pairs (sliding_windows makes them).  The other arguments as for batch_windows.
    d_spans / results: optional CUDA float64 tensors [n_pairs, n_spans, 16] / [n_pairs, 16] to write into.
    Returns (spans, results): lists of result dicts, spans[p][s], (sync=True) or the device tensors."""
    return _batch_spans("peaq_batch_run_adv_spans", True, ctx, ref, test, spans, n_ref, n_test, playback_level, rate,
                        align, stream, sync, d_spans, results, gain, gain_per_channel, max_gain_db, subsample)


def run_pair_adv_spans(ctx, ref, test, spans, playback_level=92.0, rate=48000, align=None):
    """peaq_run_pair_adv_spans: one whole pair from host memory (numpy float32 [n, channels]), sampled at `rate`, aligned
    first with align = a max_lag in 48 kHz samples; the spans count 48 kHz samples of the signals as scored.  Returns a
    dict: spans (result dicts, one per span), result (a result dict) and, with align, delay."""
    return _run_pair_spans("peaq_run_pair_adv_spans", True, "spans", ctx, ref, test, spans, playback_level, rate, align)


def _fb_band_summary_views(rows, n_bands=40):
    """rows [..., 7, 42] (peaq_batch_run_fb_band_summary) -> the named views [..., n_bands] and `counted` [...]:
    exc_ref_mean, exc_test_mean, moddiff (row 2 over the sum of W) and lindist_mean are their row over the row's
    denominator (entry n_bands); moddiff_sq_share, noiseloud_sq_share and missing_sq_share are their row over its sum
    over the bands -- the band's share of the square the MOV averages.  A view is NaN where its denominator is 0."""
    rows = np.asarray(rows)

    def ratio(k):
        den = rows[..., k, n_bands:n_bands + 1]
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(den != 0., rows[..., k, :n_bands] / den, np.nan)

    def share(k):
        den = rows[..., k, :n_bands].sum(axis=-1, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(den != 0., rows[..., k, :n_bands] / den, np.nan)

    return dict(counted=rows[..., 0, n_bands].astype(np.int64), exc_ref_mean=ratio(0), exc_test_mean=ratio(1),
                moddiff=ratio(2), moddiff_sq_share=share(3), noiseloud_sq_share=share(4), missing_sq_share=share(5),
                lindist_mean=ratio(6))


def batch_fb_band_summary(ctx, ref, test, n_ref=None, n_test=None, playback_level=92.0, rate=48000, align=None,
                          d_summary=None, results=None, stream=None, sync=True):
    """Every pair's per-band summary of the filter-bank path (the 40 bands behind RmsModDiff, RmsNoiseLoudAsym and
    AvgLinDist), reduced over the pair's counted blocks on the device in the run that scores the batch in the advanced
    version (peaq_batch_run_fb_band_summary; include/peaq_amd.h has the rows and which blocks count).  ref/test,
    n_ref/n_test, rate and align as for batch_fb_bands.  d_summary: an optional CUDA float64 tensor [n_pairs (or more),
    channels, 7, 42] to write into (pairs past the batch keep what they held); results: an optional CUDA float64 tensor
    [n_pairs, RESULT_DOUBLES].
    Returns a dict: rows, np.ndarray [pairs, channels, 7, 42] (FB_BAND_SUMMARY_ROWS in row order, the denominator in
    entry 40 of each row); the named views exc_ref_mean, exc_test_mean, moddiff, moddiff_sq_share, noiseloud_sq_share,
    missing_sq_share and lindist_mean, each [pairs, channels, 40] and NaN where its denominator is 0; counted [pairs,
    channels]; fc (fb_band_tables); results (result dicts); and d_summary / d_results, the device tensors.  sync=False:
    the device tensors and fc only."""
    import torch
    ref, test, a_ref, a_test, len_args = _batch_front(ctx, ref, test, n_ref, n_test, rate, align, stream)
    n_pairs, stride, channels = ref.shape
    n_bands, row, n_rows = ctx.L.peaq_fb_band_count(), ctx.L.peaq_fb_band_summary_row(), ctx.L.peaq_fb_band_summary_rows()
    with _torch_stream(stream):
        if d_summary is None:
            d_summary = torch.empty((n_pairs, channels, n_rows, row), dtype=torch.float64, device=ref.device)
        if results is None:
            results = torch.empty((n_pairs, RESULT_DOUBLES), dtype=torch.float64, device=ref.device)
    assert d_summary.is_cuda and d_summary.dtype == torch.float64 and d_summary.is_contiguous() and d_summary.dim() == 4
    assert d_summary.shape[0] >= n_pairs and tuple(d_summary.shape[1:]) == (channels, n_rows, row)
    assert results.is_cuda and results.dtype == torch.float64 and results.is_contiguous()
    _check(ctx.L.peaq_batch_run_fb_band_summary(ctx.h, channels, float(playback_level), n_pairs,
                                                C.c_void_p(ref.data_ptr()), C.c_void_p(test.data_ptr()), stride,
                                                *len_args, stride, C.c_void_p(d_summary.data_ptr()),
                                                C.c_void_p(results.data_ptr()), _stream_ptr(stream)))
    fc, _ = fb_band_tables()
    out = dict(d_summary=d_summary, d_results=results, fc=fc)
    if not sync:
        return out
    torch.cuda.synchronize(ref.device)
    rows = d_summary[:n_pairs].cpu().numpy()
    out.update(rows=rows, **_fb_band_summary_views(rows, n_bands))
    out["results"] = [_result_dict(r, True) for r in results.cpu().numpy()]
    return out


def run_pair_fb_band_summary(ctx, ref, test, playback_level=92.0, rate=48000, align=None):
    """peaq_run_pair_fb_band_summary: one whole pair from host memory (numpy float32 [n, channels]), sampled at `rate`,
    aligned first with align = a max_lag in 48 kHz samples.  Returns a dict: rows [channels, 7, 42], the named views of
    batch_fb_band_summary [channels, 40], counted [channels], fc, result (a result dict) and, with align, delay."""
    ref, test, ch, pair_args = _host_pair(ref, test)
    n_bands, row, n_rows = ctx.L.peaq_fb_band_count(), ctx.L.peaq_fb_band_summary_row(), ctx.L.peaq_fb_band_summary_rows()
    rows = np.zeros((ch, n_rows, row))
    rec, out = Delay(), np.zeros(RESULT_DOUBLES)
    _check(ctx.L.peaq_run_pair_fb_band_summary(ctx.h, ch, float(playback_level), int(rate),
                                               0 if align is None else int(align), *pair_args,
                                               C.c_void_p(rows.ctypes.data), C.byref(rec),
                                               out.ctypes.data_as(C.POINTER(C.c_double))))
    fc, _ = fb_band_tables()
    res = dict(rows=rows, fc=fc, result=_result_dict(out, True), **_fb_band_summary_views(rows, n_bands))
    if align is not None:
        res["delay"] = _delay_dict(rec)
    return res


def _gain_dict(rec):
    return dict(gain=list(rec.gain), srr=list(rec.srr), stt=list(rec.stt), srt=list(rec.srt), flags=list(rec.flags), n=int(rec.n))


def _subdelay_dict(rec):
    return dict(lag=int(rec.lag), q=int(rec.q), frac=rec.frac, peak=rec.peak, c0=rec.c0, flags=int(rec.flags))


def run_pair(ctx, advanced, ref, test, playback_level=92.0, rate=48000, align=None, gain=None, gain_per_channel=False,
             max_gain_db=40.0, subsample=False, drift=False, track=False, steps=False, wide=None, wide_mode="envelope"):
    """one whole pair from host memory (peaq_run_pair): ref/test numpy float32 [n, channels]; sampled at a `rate`
    other than 48000 they are converted on the device first (peaq_run_pair_rate).  align: a max_lag in 48 kHz samples:
    the pair is aligned on the device first (peaq_run_pair_aligned) and the result dict carries the record as `delay`.
    drift: True or a window, with align: peaq_run_pair_drift; the result dict carries the line's record as `drift`.
    track: True or a window, with align: peaq_run_pair_track; the result dict carries the track's record as `track`.
    steps: True or a window, with align: peaq_run_pair_steps; the result dict carries the track's record as `track`, the
    pieces' as `pieces` and the located steps, a STEP_DTYPE array, as `steps`.
    wide: a max_offset in 48 kHz samples (up to 2^20), with align: peaq_run_pair_wide, the lag found coarse to fine with
    align as the fine stage's range; the result dict carries the fine stage's record with the total lag as `delay` and
    the whole record as `wide`.  Excludes gain, subsample, drift, track and steps here."""
    ref = np.ascontiguousarray(ref, dtype=np.float32)
    test = np.ascontiguousarray(test, dtype=np.float32)
    ch = ref.shape[1]
    assert test.shape[1] == ch
    out = np.zeros(RESULT_DOUBLES)
    _need_align(subsample, align, drift, track, steps)
    _need_wide(wide, align, drift, track, steps)
    if wide is not None:                               # peaq_run_pair_wide; the records as `delay`, `wide`
        if gain is not None or subsample:
            raise ValueError("run_pair: wide= is not taken with gain= or subsample=True (batch_run takes them)")
        wrec = WideDelay()
        _check(ctx.L.peaq_run_pair_wide(ctx.h, int(bool(advanced)), ch, float(playback_level), int(rate), int(wide),
                                        WIDE_MODES[wide_mode] if isinstance(wide_mode, str) else int(wide_mode), int(align),
                                        ref.ctypes.data_as(C.POINTER(C.c_float)), len(ref),
                                        test.ctypes.data_as(C.POINTER(C.c_float)), len(test), C.byref(wrec),
                                        out.ctypes.data_as(C.POINTER(C.c_double))))
        res = _result_dict(out, bool(advanced))
        res["delay"] = dict(_delay_dict(wrec.fine), lag=int(wrec.lag))
        res["wide"] = dict(lag=int(wrec.lag), coarse_lag=int(wrec.coarse_lag), factor=int(wrec.factor), flags=int(wrec.flags),
                           fine=_delay_dict(wrec.fine), coarse=_delay_dict(wrec.coarse))
        return res
    if steps:                                          # peaq_run_pair_steps; `delay`, `track`, `pieces`, `steps`, `gain`
        rec, trec, prec, grec = Delay(), Track(), Pieces(), Gain()
        window = _steps_window(steps)
        found = np.zeros(max(max(len(ref), len(test)) // max(window, 1), 1), dtype=STEP_DTYPE)
        _check(ctx.L.peaq_run_pair_steps(ctx.h, int(bool(advanced)), ch, float(playback_level), int(rate), int(align),
                                         window, gain_mode(gain, gain_per_channel), float(max_gain_db),
                                         ref.ctypes.data_as(C.POINTER(C.c_float)), len(ref),
                                         test.ctypes.data_as(C.POINTER(C.c_float)), len(test), C.byref(rec),
                                         C.byref(trec), C.byref(prec), found.ctypes.data_as(C.POINTER(Step)), len(found),
                                         C.byref(grec), out.ctypes.data_as(C.POINTER(C.c_double))))
        res = _result_dict(out, bool(advanced))
        res["delay"] = _delay_dict(rec)
        res["track"] = {k: getattr(trec, k) for k, _ in Track._fields_}
        res["pieces"] = {k: getattr(prec, k) for k, _ in Pieces._fields_}
        res["steps"] = found[:min(len(found), prec.n_candidates)].copy()
        if gain is not None:
            res["gain"] = _gain_dict(grec)
        return res
    if track:                                          # peaq_run_pair_track; the records as `delay`, `track`, `gain`
        rec, trec, grec = Delay(), Track(), Gain()
        _check(ctx.L.peaq_run_pair_track(ctx.h, int(bool(advanced)), ch, float(playback_level), int(rate), int(align),
                                         _track_window(track), gain_mode(gain, gain_per_channel), float(max_gain_db),
                                         ref.ctypes.data_as(C.POINTER(C.c_float)), len(ref),
                                         test.ctypes.data_as(C.POINTER(C.c_float)), len(test), C.byref(rec),
                                         C.byref(trec), C.byref(grec), out.ctypes.data_as(C.POINTER(C.c_double))))
        res = _result_dict(out, bool(advanced))
        res["delay"] = _delay_dict(rec)
        res["track"] = {k: getattr(trec, k) for k, _ in Track._fields_}
        if gain is not None:
            res["gain"] = _gain_dict(grec)
        return res
    if drift:                                          # peaq_run_pair_drift; the records as `delay`, `drift`, `gain`
        rec, drec, grec = Delay(), Drift(), Gain()
        _check(ctx.L.peaq_run_pair_drift(ctx.h, int(bool(advanced)), ch, float(playback_level), int(rate), int(align),
                                         _drift_window(drift), gain_mode(gain, gain_per_channel), float(max_gain_db),
                                         ref.ctypes.data_as(C.POINTER(C.c_float)), len(ref),
                                         test.ctypes.data_as(C.POINTER(C.c_float)), len(test), C.byref(rec),
                                         C.byref(drec), C.byref(grec), out.ctypes.data_as(C.POINTER(C.c_double))))
        res = _result_dict(out, bool(advanced))
        res["delay"] = _delay_dict(rec)
        res["drift"] = dict(lag0=int(drec.lag0), flags=int(drec.flags), a=drec.a, e=drec.e, ppm=drec.ppm,
                            resid_rms=drec.resid_rms, n_windows=int(drec.n_windows), n_valid=int(drec.n_valid))
        if gain is not None:
            res["gain"] = _gain_dict(grec)
        return res
    if subsample:                                      # peaq_run_pair_subsample; the records as `delay`, `subdelay`, `gain`
        rec, srec, grec = Delay(), SubDelay(), Gain()
        _check(ctx.L.peaq_run_pair_subsample(ctx.h, int(bool(advanced)), ch, float(playback_level), int(rate), int(align),
                                             gain_mode(gain, gain_per_channel), float(max_gain_db),
                                             ref.ctypes.data_as(C.POINTER(C.c_float)), len(ref),
                                             test.ctypes.data_as(C.POINTER(C.c_float)), len(test), C.byref(rec),
                                             C.byref(srec), C.byref(grec), out.ctypes.data_as(C.POINTER(C.c_double))))
        res = _result_dict(out, bool(advanced))
        res["delay"] = _delay_dict(rec)
        res["subdelay"] = _subdelay_dict(srec)
        if gain is not None:
            res["gain"] = _gain_dict(grec)
        return res
    if gain is not None:                               # peaq_run_pair_matched; the result dict carries the record as `gain`
        rec, grec = Delay(), Gain()
        _check(ctx.L.peaq_run_pair_matched(ctx.h, int(bool(advanced)), ch, float(playback_level), int(rate),
                                           0 if align is None else int(align), gain_mode(gain, gain_per_channel),
                                           float(max_gain_db), ref.ctypes.data_as(C.POINTER(C.c_float)), len(ref),
                                           test.ctypes.data_as(C.POINTER(C.c_float)), len(test), C.byref(rec), C.byref(grec),
                                           out.ctypes.data_as(C.POINTER(C.c_double))))
        res = _result_dict(out, bool(advanced))
        res["gain"] = _gain_dict(grec)
        if align is not None:
            res["delay"] = _delay_dict(rec)
        return res
    if align is not None:
        rec = Delay()
        _check(ctx.L.peaq_run_pair_aligned(ctx.h, int(bool(advanced)), ch, float(playback_level), int(rate), int(align),
                                           ref.ctypes.data_as(C.POINTER(C.c_float)), len(ref),
                                           test.ctypes.data_as(C.POINTER(C.c_float)), len(test), C.byref(rec),
                                           out.ctypes.data_as(C.POINTER(C.c_double))))
        res = _result_dict(out, bool(advanced))
        res["delay"] = _delay_dict(rec)
        return res
    if int(rate) != 48000:
        _check(ctx.L.peaq_run_pair_rate(ctx.h, int(bool(advanced)), ch, float(playback_level), int(rate),
                                        ref.ctypes.data_as(C.POINTER(C.c_float)), len(ref),
                                        test.ctypes.data_as(C.POINTER(C.c_float)), len(test),
                                        out.ctypes.data_as(C.POINTER(C.c_double))))
        return _result_dict(out, bool(advanced))
    _check(ctx.L.peaq_run_pair(ctx.h, int(bool(advanced)), ch, float(playback_level),
                               ref.ctypes.data_as(C.POINTER(C.c_float)), len(ref),
                               test.ctypes.data_as(C.POINTER(C.c_float)), len(test),
                               out.ctypes.data_as(C.POINTER(C.c_double))))
    return _result_dict(out, bool(advanced))


def pcm_format(format):
    """PEAQ_PCM_* of a name ('u8' 's16' 's24' 's32' 'f32' 'f64') or of the number itself"""
    return PCM_FORMATS[format] if isinstance(format, str) else int(format)


def pcm_sample_bytes(format):
    """bytes per sample of a format, 0 for an unknown one (peaq_pcm_sample_bytes)"""
    return int(load_library().peaq_pcm_sample_bytes(pcm_format(format)))


def decode_pcm(ctx, raw, format, channels, n=None, out=None, stream=None):
    """Decodes a batch in a file's own sample format on the device (peaq_batch_decode_pcm).  raw: CUDA uint8 tensor
    [pairs, stride * channels * sample_bytes], pair p's samples from its row's first byte on.  n: optional per-pair lengths
    (samples per channel; without them every pair has `stride`).  out: optional float32 tensor [pairs, out_stride, channels]
    to write into (samples past a pair's length keep what they held); without it a zero-filled one with an even stride
    is made.  Returns out."""
    import torch
    fmt = pcm_format(format)
    sb = pcm_sample_bytes(fmt)
    assert raw.is_cuda and raw.dtype == torch.uint8 and raw.is_contiguous() and raw.dim() == 2 and sb
    n_pairs, row = raw.shape
    assert row % (channels * sb) == 0, "a row is stride * channels * sample_bytes bytes"
    stride = row // (channels * sb)
    a_n = None if n is None else np.ascontiguousarray(n, dtype=np.uint32)
    if out is None:
        o_stride = max(stride, 2)
        with _torch_stream(stream):                    # the zero fill runs on the stream the decoder runs on
            out = torch.zeros((n_pairs, o_stride + (o_stride & 1), channels), dtype=torch.float32, device=raw.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 3
    assert out.shape[0] == n_pairs and out.shape[2] == channels
    u32p = C.POINTER(C.c_uint32)
    _check(ctx.L.peaq_batch_decode_pcm(ctx.h, fmt, int(channels), n_pairs, C.c_void_p(raw.data_ptr()), stride,
                                       a_n.ctypes.data_as(u32p) if a_n is not None else None, stride,
                                       C.c_void_p(out.data_ptr()), out.shape[1], _stream_ptr(stream)))
    return out


def make_feed(format, channels, rate=48000, align=None, chunk_pairs=0):
    """a peaq_feed (include/peaq_amd.h) with this library's struct_size"""
    return Feed(C.sizeof(Feed), pcm_format(format), int(channels), int(rate), 0 if align is None else int(align),
                int(chunk_pairs))


def feed_workspace_bytes(feed, advanced, n_pairs, n_max):
    """staging, device buffers and workspaces of a run_host call (peaq_feed_workspace_bytes)"""
    return int(load_library().peaq_feed_workspace_bytes(C.byref(feed), int(bool(advanced)), int(n_pairs), int(n_max)))


def _run_host_rows(ctx, advanced, pairs, format, channels, rate, align, chunk_pairs, playback_level):
    """peaq_batch_run_host on numpy arrays -> (rows float64 [n_pairs, 16], the Delay records or None)"""
    fmt = pcm_format(format)
    unit = pcm_sample_bytes(fmt) * int(channels)
    assert unit, "unknown sample format"
    keep, rows = [], (HostPair * max(len(pairs), 1))()
    for p, pair in enumerate(pairs):
        for i, x in enumerate(pair):
            x = np.asarray(x)
            assert x.dtype == PCM_DTYPES[fmt], f"pair {p}: {x.dtype} is not the dtype of this format ({PCM_DTYPES[fmt]})"
            if not x.flags.c_contiguous:
                x = np.ascontiguousarray(x)
            assert x.nbytes % unit == 0, f"pair {p}: not a whole number of samples per channel"
            keep.append(x)                             # (the arrays stay alive until the call has returned)
            setattr(rows[p], ("ref", "test")[i], x.ctypes.data if x.nbytes else None)
            setattr(rows[p], ("n_ref", "n_test")[i], x.nbytes // unit)
    feed = make_feed(fmt, channels, rate, align, chunk_pairs)
    out = np.zeros((max(len(pairs), 1), RESULT_DOUBLES))
    rec = (Delay * max(len(pairs), 1))() if align is not None else None
    _check(ctx.L.peaq_batch_run_host(ctx.h, int(bool(advanced)), float(playback_level), C.byref(feed), len(pairs), rows,
                                     out.ctypes.data_as(C.POINTER(C.c_double)), rec))
    del keep
    return out[:len(pairs)], rec


def run_host(ctx, advanced, pairs, format, channels, rate=48000, align=None, chunk_pairs=0, playback_level=92.0,
             gain=None, gain_per_channel=False, max_gain_db=40.0):
    """Scores a list of pairs that sit in host memory in a file's own sample format (peaq_batch_run_host): upload, decode,
    rate conversion, alignment and scoring on the device, chunk by chunk.  pairs: [(ref, test)] numpy arrays in the
    file's dtype (PCM_DTYPES; S24: the bytes), interleaved, any shape; they may be unaligned views.  rate: sampling rate
    of all of them.  align: a max_lag in 48 kHz samples.  Returns the result dicts in list order, and with `align`
    (results, delays): delays a dict of numpy arrays lag / peak / runner_up / norm as estimate_delay's.  gain: as
    run_host_refs's, which scores the pairs then, one test per reference."""
    if gain is not None:
        return run_host_refs(ctx, advanced, [p[0] for p in pairs], [p[1] for p in pairs], list(range(len(pairs))), format,
                             channels, rate=rate, align=align, chunk_pairs=chunk_pairs, playback_level=playback_level,
                             gain=gain, gain_per_channel=gain_per_channel, max_gain_db=max_gain_db)
    out, rec = _run_host_rows(ctx, advanced, pairs, format, channels, rate, align, chunk_pairs, playback_level)
    res = [_result_dict(r, bool(advanced)) for r in out]
    if align is None:
        return res
    delays = {k: np.array([getattr(rec[p], k) for p in range(len(pairs))], dtype=np.int32 if k == "lag" else np.float64)
              for k in ("lag", "peak", "runner_up", "norm")}
    return res, delays


def _delay_arrays(rec, n):
    return {k: np.array([getattr(rec[p], k) for p in range(n)], dtype=np.int32 if k == "lag" else np.float64)
            for k in ("lag", "peak", "runner_up", "norm")}


def feed_refs_workspace_bytes(feed, advanced, n_refs, n_tests, n_max):
    """staging, device buffers and workspaces of a run_host_refs call (peaq_feed_refs_workspace_bytes)"""
    return int(load_library().peaq_feed_refs_workspace_bytes(C.byref(feed), int(bool(advanced)), int(n_refs), int(n_tests),
                                                             int(n_max)))


def _run_host_refs_rows(ctx, advanced, refs, tests, ref_index, format, channels, rate, align, chunk_pairs, playback_level,
                        gain=None, gain_per_channel=False, max_gain_db=40.0):
    """peaq_batch_run_host_refs (with gain: peaq_batch_run_host_matched) on numpy arrays -> (rows float64 [n_tests, 16],
    the Delay records or None[, the Gain records]); a reference may be None (no buffer, no samples)"""
    fmt = pcm_format(format)
    unit = pcm_sample_bytes(fmt) * int(channels)
    assert unit, "unknown sample format"
    assert len(ref_index) == len(tests), "one reference index per test"
    keep = []

    def fill(row, x, what):
        if x is None:
            row.data, row.n = None, 0
            return
        x = np.asarray(x)
        assert x.dtype == PCM_DTYPES[fmt], f"{what}: {x.dtype} is not the dtype of this format ({PCM_DTYPES[fmt]})"
        if not x.flags.c_contiguous:
            x = np.ascontiguousarray(x)
        assert x.nbytes % unit == 0, f"{what}: not a whole number of samples per channel"
        keep.append(x)                                 # (the arrays stay alive until the call has returned)
        row.data, row.n = (x.ctypes.data if x.nbytes else None), x.nbytes // unit

    r_rows, t_rows = (HostSignal * max(len(refs), 1))(), (HostTest * max(len(tests), 1))()
    for r, x in enumerate(refs):
        fill(r_rows[r], x, f"reference {r}")
    for t, x in enumerate(tests):
        fill(t_rows[t], x, f"test {t}")
        t_rows[t].ref = int(ref_index[t])
    feed = make_feed(fmt, channels, rate, align, chunk_pairs)
    out = np.zeros((max(len(tests), 1), RESULT_DOUBLES))
    rec = (Delay * max(len(tests), 1))() if align is not None else None
    if gain is not None:
        grec = (Gain * max(len(tests), 1))()
        _check(ctx.L.peaq_batch_run_host_matched(ctx.h, int(bool(advanced)), float(playback_level), C.byref(feed),
                                                 gain_mode(gain, gain_per_channel), float(max_gain_db), len(refs), r_rows,
                                                 len(tests), t_rows, out.ctypes.data_as(C.POINTER(C.c_double)), rec, grec))
        del keep
        return out[:len(tests)], rec, grec
    _check(ctx.L.peaq_batch_run_host_refs(ctx.h, int(bool(advanced)), float(playback_level), C.byref(feed), len(refs), r_rows,
                                          len(tests), t_rows, out.ctypes.data_as(C.POINTER(C.c_double)), rec))
    del keep
    return out[:len(tests)], rec


def run_host_refs(ctx, advanced, refs, tests, ref_index, format, channels, rate=48000, align=None, chunk_pairs=0,
                  playback_level=92.0, gain=None, gain_per_channel=False, max_gain_db=40.0):
    """run_host for tests that share references (peaq_batch_run_host_refs): tests[t] is scored against
    refs[ref_index[t]], and a reference is uploaded, decoded and converted once per chunk, not once per test -- keep the
    tests of a reference next to each other.  A reference no test names may be None.  Returns what run_host returns for
    the pairs (refs[ref_index[t]], tests[t]), bit for bit.  gain: 'lsq' 'rms' 'polarity': every test's level is matched
    to its reference's on the device (peaq_batch_run_host_matched), and the gain records (gain_records) are returned
    last: (results, gains) or (results, delays, gains)."""
    if gain is not None:
        out, rec, grec = _run_host_refs_rows(ctx, advanced, refs, tests, ref_index, format, channels, rate, align, chunk_pairs,
                                             playback_level, gain, gain_per_channel, max_gain_db)
        res = [_result_dict(r, bool(advanced)) for r in out]
        gains = gain_records(grec, len(tests))
        return (res, gains) if align is None else (res, _delay_arrays(rec, len(tests)), gains)
    out, rec = _run_host_refs_rows(ctx, advanced, refs, tests, ref_index, format, channels, rate, align, chunk_pairs,
                                   playback_level)
    res = [_result_dict(r, bool(advanced)) for r in out]
    return res if align is None else (res, _delay_arrays(rec, len(tests)))


def run_files(ctx, advanced, files, align=None, chunk_pairs=0, playback_level=92.0, share_refs=True, gain=None,
              gain_per_channel=False, max_gain_db=40.0):
    """Scores a list of (ref_path, test_path) RIFF/WAVE files: the data chunks are read as they are (wavio.read_wav_raw),
    the pairs grouped by (format, channels, rate) and each group run through run_host_refs: within a group every distinct
    reference path (compared as the exact string) is read once and the tests are ordered by reference (a stable sort), so
    that a reference shared by several pairs is uploaded once per chunk.  share_refs=False: every line's reference is
    read again and the group goes through run_host.  Returns the result dicts in list order, and with `align`
    (results, delays), delays a list of dicts.  ValueError, naming the file, if the two files of a pair differ in
    channels, rate or format.  gain: as run_host_refs's; the gain records come last, a list of dicts."""
    from . import wavio
    groups, loaded, read = {}, [], {}
    for p, (ref_path, test_path) in enumerate(files):
        key = str(ref_path)
        r = read.get(key) if share_refs else None
        if r is None:
            r = wavio.read_wav_raw(ref_path)
            read[key] = r
        t = wavio.read_wav_raw(test_path)
        for what, a, b in (("format", r[1], t[1]), ("channel count", r[2], t[2]), ("rate", r[3], t[3])):
            if a != b:
                raise ValueError(f"{test_path}: {what} {b} differs from {ref_path}'s ({a})")
        loaded.append((r[0], t[0], key))
        groups.setdefault((r[1], r[2], r[3]), []).append(p)
    results, delays, gains = [None] * len(files), [None] * len(files), [None] * len(files)
    gkw = {} if gain is None else dict(gain=gain, gain_per_channel=gain_per_channel, max_gain_db=max_gain_db)
    for (fmt, channels, rate), members in groups.items():
        as_array = lambda b: np.frombuffer(b, dtype=PCM_DTYPES[fmt])   # noqa: E731
        if share_refs:
            index = {}
            for p in members:
                index.setdefault(loaded[p][2], len(index))
            members = sorted(members, key=lambda p: index[loaded[p][2]])
            refs = [None] * len(index)
            for p in members:
                refs[index[loaded[p][2]]] = as_array(loaded[p][0])
            got = run_host_refs(ctx, advanced, refs, [as_array(loaded[p][1]) for p in members],
                                [index[loaded[p][2]] for p in members], fmt, channels, rate=rate, align=align,
                                chunk_pairs=chunk_pairs, playback_level=playback_level, **gkw)
        else:
            arrays = [(as_array(loaded[p][0]), as_array(loaded[p][1])) for p in members]
            got = run_host(ctx, advanced, arrays, fmt, channels, rate=rate, align=align, chunk_pairs=chunk_pairs,
                           playback_level=playback_level, **gkw)
        gn = None
        if gain is not None:
            got, gn = (got[0], got[-1]) if align is None else (got[:2], got[-1])
        res, dl = got if align is not None else (got, None)
        for i, p in enumerate(members):
            results[p] = res[i]
            if dl is not None:
                delays[p] = {k: dl[k][i].item() for k in dl}
            if gn is not None:
                gains[p] = {k: gn[k][i].tolist() for k in gn}
    out = (results, delays) if align is not None else results
    if gain is None:
        return out
    return out + (gains,) if align is not None else (out, gains)


def synth_fill(ctx, seed0, n_pairs, channels, n_samples, device="cuda:0", stream=None, out=None):
    """-> (ref, test) CUDA tensors [n_pairs, n_samples, channels] of include/peaq_synth.h pairs
    seed0 .. seed0 + n_pairs - 1.  out=(ref, test): refill existing buffers (their first n_pairs
    rows) instead of allocating -- how a GPU's share is consumed in waves."""
    import torch
    if out is not None:
        ref, test = out
        assert ref.is_cuda and ref.is_contiguous() and test.is_contiguous() and ref.shape == test.shape
        assert ref.shape[0] >= n_pairs and ref.shape[1] == n_samples and ref.shape[2] == channels
    else:
        ref = torch.empty((n_pairs, n_samples, channels), dtype=torch.float32, device=device)
        test = torch.empty_like(ref)
    _check(ctx.L.peaq_synth_fill(ctx.h, int(seed0) & 0xFFFFFFFF, n_pairs, channels, n_samples, n_samples,
                                 C.c_void_p(ref.data_ptr()), C.c_void_p(test.data_ptr()), _stream_ptr(stream)))
    return ref, test


def debug_frontend(ctx, bands, ref, test, n_frames, playback_level=92.0, n_ref=None, n_test=None):
    """Stage-level access: per-frame front-end records of ONE pair.
    ref/test: CUDA float32 [n, channels] (may differ in length); n_ref/n_test: the signals' lengths where the tensors
    are longer (a signal of no samples is a tensor with something behind it: an empty tensor has no address).
    -> np [frames, channels, 576]"""
    import torch
    assert ref.is_cuda and test.is_cuda and ref.is_contiguous() and test.is_contiguous()
    channels = ref.shape[1]
    n_ref = ref.shape[0] if n_ref is None else int(n_ref)
    n_test = test.shape[0] if n_test is None else int(n_test)
    assert 0 <= n_ref <= ref.shape[0] and 0 <= n_test <= test.shape[0] and test.shape[1] == channels
    out = np.zeros((n_frames, channels, RECORD_DOUBLES))
    torch.cuda.synchronize()
    _check(ctx.L.peaq_debug_frontend(ctx.h, bands, channels, float(playback_level), C.c_void_p(ref.data_ptr()),
                                     C.c_void_p(test.data_ptr()), n_ref, n_test, n_frames,
                                     out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


RAW_RECORD_DOUBLES = 352


def debug_select_frontend(ctx, two_waves):
    """Development switch of the basic front end: 0 = the one-wave kernel, 1 = the two-wave kernel, -1 = what
    PEAQ_AMD_FE says.  -> the previous selection"""
    ctx.L.peaq_debug_select_frontend.argtypes = [C.c_int]
    ctx.L.peaq_debug_select_frontend.restype = C.c_int
    return ctx.L.peaq_debug_select_frontend(int(two_waves))


def debug_frontend_pairs(ctx, ref, test, n_ref, n_test, frames_per_launch, n_frames, playback_level=92.0):
    """Stage-level access: the basic front end over several pairs as the batch path launches it.
    ref/test: CUDA float32 [pairs, stride, channels]; n_ref/n_test: samples per pair.
    -> np [pairs, n_frames, channels, 352], the records as the kernels exchange them"""
    import torch
    assert ref.is_cuda and test.is_cuda and ref.is_contiguous() and test.is_contiguous() and ref.shape == test.shape
    n_pairs, stride, channels = ref.shape
    nr = (C.c_uint32 * n_pairs)(*[int(v) for v in n_ref])
    nt = (C.c_uint32 * n_pairs)(*[int(v) for v in n_test])
    out = np.zeros((n_pairs, n_frames, channels, RAW_RECORD_DOUBLES))
    ctx.L.peaq_debug_frontend_pairs.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t,
                                                C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_int, C.c_int,
                                                C.POINTER(C.c_double)]
    ctx.L.peaq_debug_frontend_pairs.restype = C.c_int
    torch.cuda.synchronize()
    _check(ctx.L.peaq_debug_frontend_pairs(ctx.h, channels, float(playback_level), C.c_void_p(ref.data_ptr()),
                                           C.c_void_p(test.data_ptr()), n_pairs, stride, nr, nt, int(frames_per_launch),
                                           int(n_frames), out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def debug_filterbank(ctx, ref, test, n_blocks, blocks_per_launch=320, playback_level=92.0):
    """Stage-level access to the filter-bank ear model of ONE pair.
    ref/test: CUDA float32 [n, channels].  -> np [blocks, channels, 168]"""
    import torch
    assert ref.is_cuda and test.is_cuda and ref.is_contiguous() and test.is_contiguous()
    channels = ref.shape[1]
    out = np.zeros((n_blocks, channels, 168))
    torch.cuda.synchronize()
    _check(ctx.L.peaq_debug_filterbank(ctx.h, channels, float(playback_level), C.c_void_p(ref.data_ptr()),
                                       C.c_void_p(test.data_ptr()), ref.shape[0], test.shape[0], n_blocks,
                                       blocks_per_launch, out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


BACKEND_DEBUG_DOUBLES = 912
BACKEND_DEBUG_VECTORS = ["exc_ref", "exc_test", "adapted_ref", "adapted_test", "mod_ref", "mod_test",
                         "avgloud_ref", "avgloud_test"]
BACKEND_DEBUG_MOVS = ["moddiff1", "moddiff2", "tempwt", "noiseloud", "nmr_mean", "nmr_max", "p_detect", "steps"]


def debug_backend(ctx, records):
    """Stage-level access to the stateful back end (basic version, fresh state).
    records: np [frames, channels, 576] front-end records (from debug_frontend, or hand-built).
    -> (dict name -> np [frames, channels, 109] for BACKEND_DEBUG_VECTORS plus 'loudness' [frames, channels, 2] and
        'mov' (dict name -> np [frames, channels] for BACKEND_DEBUG_MOVS; the last two: channel 0 only),
        result dict after the last frame)"""
    rec = np.ascontiguousarray(records, dtype=np.float64)
    n_frames, channels, width = rec.shape
    assert width == RECORD_DOUBLES
    out = np.zeros((n_frames, channels, BACKEND_DEBUG_DOUBLES))
    res = np.zeros(RESULT_DOUBLES)
    dp = C.POINTER(C.c_double)
    _check(ctx.L.peaq_debug_backend(ctx.h, channels, n_frames, rec.ctypes.data_as(dp), out.ctypes.data_as(dp),
                                    res.ctypes.data_as(dp)))
    d = {name: out[:, :, 112 * i: 112 * i + 109] for i, name in enumerate(BACKEND_DEBUG_VECTORS)}
    d["loudness"] = out[:, :, 896:898]
    # the MOV layer's per-frame values before accumulation (include/peaq_amd.h, PEAQ_DEBUG_BACKEND_DOUBLES)
    d["mov"] = dict(zip(BACKEND_DEBUG_MOVS, np.moveaxis(out[:, :, 904:912], 2, 0)))
    return d, _result_dict(res, False)


ADVANCED_DEBUG_BLOCK = ["rmsmoddiff", "tempwt", "noiseloud", "missing", "lindist", "loudness_ref", "loudness_test"]
ADVANCED_DEBUG_FRAME = ["segnmr_db", "nmr_mean"]


def debug_backend_advanced(ctx, fb_records, fft_records):
    """Stage-level access to the advanced version's MOV layer (fresh state).
    fb_records: np [blocks, channels, 168] (debug_filterbank); fft_records: np [frames, channels, 576] (debug_frontend
    with 55 bands).  -> (dict name -> np [blocks, channels] for ADVANCED_DEBUG_BLOCK, dict name -> np [frames, channels]
    for ADVANCED_DEBUG_FRAME, result dict after the last block and frame): the values of EVERY block / frame before
    accumulation (include/peaq_amd.h, peaq_debug_backend_advanced)."""
    fb = np.ascontiguousarray(fb_records, dtype=np.float64)
    ff = np.ascontiguousarray(fft_records, dtype=np.float64)
    n_blocks, channels, w = fb.shape
    n_frames, ch2, w2 = ff.shape
    assert w == 168 and w2 == RECORD_DOUBLES and ch2 == channels
    ob = np.zeros((n_blocks, channels, 8))
    of = np.zeros((n_frames, channels, 2))
    res = np.zeros(RESULT_DOUBLES)
    dp = C.POINTER(C.c_double)
    _check(ctx.L.peaq_debug_backend_advanced(ctx.h, channels, n_blocks, fb.ctypes.data_as(dp), n_frames, ff.ctypes.data_as(dp),
                                             ob.ctypes.data_as(dp), of.ctypes.data_as(dp), res.ctypes.data_as(dp)))
    return (dict(zip(ADVANCED_DEBUG_BLOCK, np.moveaxis(ob[:, :, :7], 2, 0))),
            dict(zip(ADVANCED_DEBUG_FRAME, np.moveaxis(of, 2, 0))), _result_dict(res, True))


def debug_backend_plain(ctx, fft_records, frames_per_launch=None, fb_records=None, blocks_per_launch=None):
    """The shipped instantiations of the back ends on records, from a fresh state, cut into launches of
    frames_per_launch frames (and blocks_per_launch blocks); None = one launch.  fb_records None: basic version
    (fft_records np [frames, channels, 576], 109 bands); else the advanced version (55-band fft_records and
    fb_records np [blocks, channels, 168]).  -> result dict (include/peaq_amd.h, peaq_debug_backend_plain)."""
    ff = np.ascontiguousarray(fft_records, dtype=np.float64)
    n_frames, channels, w = ff.shape
    assert w == RECORD_DOUBLES
    adv = fb_records is not None
    dp = C.POINTER(C.c_double)
    fb, n_blocks = None, 0
    if adv:
        fb = np.ascontiguousarray(fb_records, dtype=np.float64)
        n_blocks = fb.shape[0]
        assert fb.shape[1:] == (channels, 168)
    res = np.zeros(RESULT_DOUBLES)
    _check(ctx.L.peaq_debug_backend_plain(ctx.h, int(adv), channels, n_frames, ff.ctypes.data_as(dp),
                                          int(frames_per_launch or n_frames), n_blocks,
                                          fb.ctypes.data_as(dp) if adv else None, int(blocks_per_launch or max(n_blocks, 1)),
                                          res.ctypes.data_as(dp)))
    return _result_dict(res, adv)


# planes in / out of the ops of peaq_debug_wave (include/peaq_amd.h); every other op is 1 -> 1
WAVE_OP_PLANES = {"div_fast": (2, 1), "pow_pos": (2, 1), "pow_tab": (2, 1), "pow_logtab": (2, 1),
                  "log_nonneg_n5": (5, 5), "exp_fast_n5": (5, 5), "wave_sum2": (2, 2), "wave_sum4": (4, 4),
                  "rows_transpose4": (4, 4), "wave_prefix_geometric_z": (3, 3), "dft4": (8, 8), "dft8": (16, 16),
                  "dft16": (32, 32)}


def debug_wave(ctx, op, inputs, params=()):
    """The primitives of csrc/peaq_wave.h on their own (peaq_debug_wave, include/peaq_amd.h).
    inputs: float64 [n] or [planes, n]; params: the op's scalar parameters (m of the geometric scans).
    -> np float64 [planes_out, n] ([n] for an op with one output plane); for the
    cross-lane ops every 64 consecutive elements are one wave and the output is what each lane holds."""
    x = np.ascontiguousarray(inputs, dtype=np.float64)
    flat = x.ndim == 1
    if flat:
        x = x[None, :]
    assert x.ndim == 2
    planes_out = WAVE_OP_PLANES.get(op, (1, 1))[1]
    out = np.zeros((planes_out, x.shape[1]))
    par = np.ascontiguousarray(params, dtype=np.float64).reshape(-1)
    dp = C.POINTER(C.c_double)
    _check(ctx.L.peaq_debug_wave(ctx.h, op.encode(), x.shape[1], x.shape[0], x.ctypes.data_as(dp), len(par),
                                 par.ctypes.data_as(dp) if len(par) else None, planes_out, out.ctypes.data_as(dp)))
    return out[0] if planes_out == 1 else out


def debug_common_tables():
    """-> (log_tab [130, 2], exp_tab [64]): the tables of log_tab / exp_tab as every context uploads them (host only)"""
    lt, et = np.zeros((130, 2)), np.zeros(64)
    dp = C.POINTER(C.c_double)
    _check(load_library().peaq_debug_common_tables(lt.ctypes.data_as(dp), et.ctypes.data_as(dp)))
    return lt, et

"""gstpeaq_amd -- MI355X-native PEAQ (ITU-R BS.1387) engine behind the plugin
surface of HSU-ANT/gstpeaq.

The product is the C-ABI shared library ``libpeaq_amd.so`` (include/peaq_amd.h)
built from gstpeaq_amd/csrc (hand-written HIP for gfx950).  This Python package
is only the thin ctypes binding used by the tests and by bench.py; PyTorch is
used for device memory and streams, nothing else.  There is no CPU fallback:
every entry point raises if the HIP library or the GPU is missing.
"""
from .capi import (Broker, Context, PeaqError, Session, batch_run, batch_trajectory, build_library, debug_backend, debug_frontend, debug_filterbank, debug_wave, debug_common_tables, run_pair,  # noqa: F401
                   run_pair_trajectory, library_path, load_library, synth_fill, resample, resample_plan, resampled_length, resample_supported,
                   estimate_delay, cut, align, aligned_lengths, align_workspace_bytes, Delay,
                   decode_pcm, run_host, run_files, make_feed, feed_workspace_bytes, pcm_format, pcm_sample_bytes, Feed, HostPair,
                   gather, run_host_refs, feed_refs_workspace_bytes, HostSignal, HostTest,
                   Gain, measure_gain, cut_scaled, gain_workspace_bytes, gain_records, gain_mode, GAIN_DTYPE, GAIN_MODES,
                   GAIN_PER_CHANNEL, GAIN_F_SILENT, GAIN_F_NONFINITE, GAIN_F_ZERO, GAIN_F_RANGE,
                   SubDelay, refine_delay, cut_shifted, subsample_tables, subdelay_workspace_bytes, SUBDELAY_DTYPE, SUB_STEPS,
                   SUB_LAGS, SUB_HALF, SUB_F_NONE, SUB_F_EDGE,
                   Track, TRACK_DTYPE, TRACK_F_NONE, TRACK_F_RANGE, TRACK_MAX_E, TRACK_MAX_STEP, TRACK_MAX_SEGMENTS_PER_CALL,
                   TRACK_WINDOW, track_fit, track_segment, track_index, track_lengths, estimate_track, cut_track,
                   Step, StepCandidate, Pieces, STEP_DTYPE, STEP_CANDIDATE_DTYPE, PIECES_DTYPE, STEP_F_NONE, STEP_F_SPAN, STEP_F_WEAK, STEP_MAX_SPAN, STEP_MAX_L, STEP_MIN_STEP, STEP_RATIO, STEP_MIN_GAIN,
                   PIECES_F_RANGE, PIECES_MAX_PER_PAIR, PIECES_MAX_PER_CALL, locate_steps, steps_candidates, steps_fit, pieces_index, pieces_lengths, estimate_steps, cut_pieces, steps_workspace_bytes,
                   Drift, estimate_drift, cut_drift, drift_lengths, drift_fit, drift_index, drift_windows, drift_workspace_bytes,
                   DRIFT_DTYPE, DRIFT_F_NONE, DRIFT_F_RANGE, DRIFT_WINDOW, DRIFT_MIN_CORR, DRIFT_MAX_E, DRIFT_MAX_WINDOWS,
                   WideDelay, WIDE_DELAY_DTYPE, WIDE_WAVEFORM, WIDE_ENVELOPE, WIDE_MODES, WIDE_CHUNK, WIDE_MAX_OFFSET, WIDE_F_NONE,
                   WIDE_F_RANGE, WIDE_F_EDGE, wide_factor, wide_taps, wide_workspace_bytes, decimate, estimate_delay_wide,
                   PCM_FORMATS, PCM_DTYPES,
                   batch_trace, run_pair_trace, frame_count, FrameTrace, BlockTrace, FRAME_TRACE_DTYPE, BLOCK_TRACE_DTYPE,
                   TRACE_ABOVE, TRACE_MOD_OPEN, TRACE_LOUD_OPEN, TRACE_FLUSH,
                   batch_bands, run_pair_bands, band_tables, band_planes_mask, BAND_PLANES,
                   batch_fb_bands, run_pair_fb_bands, fb_band_tables, fb_band_planes_mask, FB_BAND_PLANES,
                   batch_pattern_bands, run_pair_pattern_bands, pattern_band_tables, pattern_band_planes_mask,
                   PATTERN_BAND_PLANES,
                   batch_band_summary, run_pair_band_summary, BAND_SUMMARY_ROWS,
                   batch_fb_band_summary, run_pair_fb_band_summary, FB_BAND_SUMMARY_ROWS,
                   batch_windows, run_pair_windows, window_frames, sliding_windows, WINDOWS_MAX,
                   MOV_NAMES_BASIC, MOV_NAMES_ADVANCED)

__all__ = ["Broker", "Context", "PeaqError", "Session", "batch_run", "batch_trajectory", "build_library", "debug_backend", "debug_frontend", "debug_filterbank", "debug_wave", "debug_common_tables", "run_pair",
           "run_pair_trajectory", "library_path", "load_library", "synth_fill", "resample", "resample_plan", "resampled_length",
           "resample_supported", "estimate_delay", "cut", "align", "aligned_lengths", "align_workspace_bytes", "Delay",
           "decode_pcm", "run_host", "run_files", "make_feed", "feed_workspace_bytes", "pcm_format", "pcm_sample_bytes", "Feed",
           "HostPair", "PCM_FORMATS", "PCM_DTYPES", "gather", "run_host_refs", "feed_refs_workspace_bytes", "HostSignal", "HostTest",
           "batch_trace", "run_pair_trace", "frame_count", "FrameTrace", "BlockTrace", "FRAME_TRACE_DTYPE", "BLOCK_TRACE_DTYPE",
           "TRACE_ABOVE", "TRACE_MOD_OPEN", "TRACE_LOUD_OPEN", "TRACE_FLUSH",
           "batch_bands", "run_pair_bands", "band_tables", "band_planes_mask", "BAND_PLANES",
           "batch_fb_bands", "run_pair_fb_bands", "fb_band_tables", "fb_band_planes_mask", "FB_BAND_PLANES",
           "batch_pattern_bands", "run_pair_pattern_bands", "pattern_band_tables", "pattern_band_planes_mask",
           "PATTERN_BAND_PLANES",
           "batch_band_summary", "run_pair_band_summary", "BAND_SUMMARY_ROWS",
           "batch_fb_band_summary", "run_pair_fb_band_summary", "FB_BAND_SUMMARY_ROWS",
           "batch_windows", "run_pair_windows", "window_frames", "sliding_windows", "WINDOWS_MAX",
           "Gain", "measure_gain", "cut_scaled", "gain_workspace_bytes", "gain_records", "gain_mode", "GAIN_DTYPE", "GAIN_MODES",
           "GAIN_PER_CHANNEL", "GAIN_F_SILENT", "GAIN_F_NONFINITE", "GAIN_F_ZERO", "GAIN_F_RANGE",
           "SubDelay", "refine_delay", "cut_shifted", "subsample_tables", "subdelay_workspace_bytes", "SUBDELAY_DTYPE", "SUB_STEPS",
           "SUB_LAGS", "SUB_HALF", "SUB_F_NONE", "SUB_F_EDGE",
           "Track", "TRACK_DTYPE", "TRACK_F_NONE", "TRACK_F_RANGE", "TRACK_MAX_E", "TRACK_MAX_STEP",
           "TRACK_MAX_SEGMENTS_PER_CALL", "TRACK_WINDOW", "track_fit", "track_segment", "track_index", "track_lengths",
           "estimate_track", "cut_track",
           "Step", "StepCandidate", "Pieces", "STEP_DTYPE", "STEP_CANDIDATE_DTYPE", "PIECES_DTYPE", "STEP_F_NONE", "STEP_F_SPAN", "STEP_F_WEAK", "STEP_MAX_SPAN", "STEP_MAX_L", "STEP_MIN_STEP", "STEP_RATIO", "STEP_MIN_GAIN",
           "PIECES_F_RANGE", "PIECES_MAX_PER_PAIR", "PIECES_MAX_PER_CALL", "locate_steps", "steps_candidates", "steps_fit", "pieces_index", "pieces_lengths", "estimate_steps", "cut_pieces", "steps_workspace_bytes",
           "Drift", "estimate_drift", "cut_drift", "drift_lengths", "drift_fit", "drift_index", "drift_windows",
           "drift_workspace_bytes", "DRIFT_DTYPE", "DRIFT_F_NONE", "DRIFT_F_RANGE", "DRIFT_WINDOW", "DRIFT_MIN_CORR",
           "DRIFT_MAX_E", "DRIFT_MAX_WINDOWS",
           "WideDelay", "WIDE_DELAY_DTYPE", "WIDE_WAVEFORM", "WIDE_ENVELOPE", "WIDE_MODES", "WIDE_CHUNK", "WIDE_MAX_OFFSET",
           "WIDE_F_NONE", "WIDE_F_RANGE", "WIDE_F_EDGE", "wide_factor", "wide_taps", "wide_workspace_bytes", "decimate",
           "estimate_delay_wide",
           "MOV_NAMES_BASIC", "MOV_NAMES_ADVANCED"]

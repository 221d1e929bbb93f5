/* peaq_amd.h -- C ABI of the MI355X-native PEAQ engine (libpeaq_amd.so).
 *
 * This is the drop-in boundary of SURVEY.md 8(b): everything the `peaq`
 * GStreamer element of HSU-ANT/gstpeaq calls below its adapters -- ear models,
 * level/pattern adaptation, modulation patterns, MOV calculators, MOV
 * accumulators and the neural network (reference src/{fftearmodel,fbearmodel,
 * earmodel,leveladapter,modpatt,movs,movaccum,nn}.c) -- is replaced by batched
 * HIP kernels for gfx950 behind the entry points declared here.  Plain C,
 * plain pointers and sizes; no GLib, GStreamer or torch types.
 *
 * Two ways in:
 *   session API  one handle per element instance / per (ref,test) stream; the
 *                element's pad_chain / change_state / get_property call it
 *                (gstpeaq_amd/gst/gstpeaq_amd.c is that element).
 *   batch API    N whole (ref,test) pairs resident in device memory, the shape
 *                of BASELINE.json configs 2-4.
 *
 * All functions return PEAQ_OK (0) or a negative error; peaq_last_error()
 * gives the message of the calling thread's last failure.  The reference's DSP
 * calls cannot fail (SURVEY.md 8(b) "error convention"); device/allocation
 * errors are new and map to GST_FLOW_ERROR in the element.
 */
#ifndef PEAQ_AMD_H
#define PEAQ_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PEAQ_OK            0
#define PEAQ_ERR_ARG      -1   /* bad argument */
#define PEAQ_ERR_DEVICE   -2   /* HIP runtime error (no GPU, launch failure, ...) */
#define PEAQ_ERR_NOMEM    -3
#define PEAQ_ERR_STATE    -4   /* call not valid in the handle's current state */

#define PEAQ_MOVS_BASIC     11  /* order = enum _MovBasic, gstpeaq.c:95-108 */
#define PEAQ_MOVS_ADVANCED   5  /* order = enum _MovAdvanced, gstpeaq.c:86-93 */

/* One result record per pair (batch API) -- 16 doubles.
 * movs[] holds 11 (basic) or 5 (advanced) values, the rest is 0. */
typedef struct {
  double movs[PEAQ_MOVS_BASIC];
  double di;          /* peaq_calculate_di_basic/_advanced, nn.c:187,304 */
  double odg;         /* peaq_calculate_odg, nn.c:372 */
  double totalsnr;    /* element property "totalsnr", gstpeaq.c:493-497 */
  double frames;      /* FFT frame-pairs processed (frame_counter, gstpeaq.c:920) */
  double fb_blocks;   /* filter-bank blocks processed (advanced; gstpeaq.c:1009) */
} peaq_result;

const char *peaq_last_error (void);
/* Number of frames the element processes for signals of n_ref / n_test samples per
 * channel: full frames while both adapters hold one (do_processing,
 * gstpeaq.c:596-611) plus ONE zero-padded frame if anything is left on either
 * side (do_flush, :716-745).  filter_bank = 0: FFT frames (2048 / hop 1024);
 * 1: filter-bank blocks (192 / 192).  Pure host arithmetic, no GPU needed. */
uint32_t peaq_frame_count (uint64_t n_ref, uint64_t n_test, int filter_bank);
/* "x.y.z gfx950" */
const char *peaq_version (void);

/* ---- device context -------------------------------------------------------
 * Owns the constant tables in HBM (Hann window, ear weights, band tables,
 * twiddles, filter-bank impulse responses -- what the reference builds in
 * fftearmodel.c:160-173,240-257,693-788, fbearmodel.c:188-225,
 * earmodel.c:279-323) for one GPU.  Thread-safe; create one per process/GPU. */
typedef struct peaq_ctx peaq_ctx;
int peaq_ctx_create (int device_ordinal, peaq_ctx **out);
void peaq_ctx_destroy (peaq_ctx *ctx);
int peaq_ctx_device (const peaq_ctx *ctx);
/* ---- the reference's readings of BS.1387 as run-time switches ---------------
 * The reference is compiled with ONE value for each of six interpretation
 * switches (src/settings.h:47-97); a context carries them as data.  The
 * defaults (peaq_settings_default, or passing NULL) are the values the reference
 * ships with, and every golden of the default build pins exactly those.
 * A change applies to batch calls made, and to sessions and brokers CREATED,
 * afterwards.  Each field replaces the settings.h macro of the same name. */
typedef struct peaq_settings {
  int swap_mod_patts_for_noise_loudness_movs;   /* settings.h:47  default 1  (movs.c:566-575, 693-703) */
  int center_ehs_correlation_window;            /* settings.h:56  default 0  (movs.c:1362-1368) */
  int ehs_subtract_dc_before_window;            /* settings.h:66  default 1  (movs.c:1409-1433) */
  int use_floor_for_steps_above_threshold;      /* settings.h:76  default 0  (movs.c:1256-1260) */
  int clamp_movs;                               /* settings.h:86  default 0  (nn.c:202-207, 320-325) */
  int swap_slope_filter_coefficients;           /* settings.h:97  default 0  (fbearmodel.c:335-339) */
} peaq_settings;
void peaq_settings_default (peaq_settings *s);
int peaq_ctx_set_settings (peaq_ctx *ctx, const peaq_settings *s);
int peaq_ctx_get_settings (const peaq_ctx *ctx, peaq_settings *s);

/* Advanced version only: the arithmetic of the filter-bank ear model's front half
 * (fbearmodel.c:327-435: the 40 complex FIR filters, the level-dependent slopes, the upward spreading).
 *   PEAQ_FIR_F64 (default): the reference's double arithmetic -- v_mfma_f64_16x16x4_f64 and FP64 vector
 *       instructions throughout; follows the oracle to 1e-9 per block (tests/gpu_common.py, column "default").
 *       Bands 0..23 are evaluated in the block-sum form of DESIGN.md section 10 (a third of the reference's
 *       multiply-adds), bands 24..39 as plain sums.
 *   PEAQ_FIR_F16X3 (opt-in, 1.5x the throughput of the default on MI355X): the FIR bank on
 *       v_mfma_f32_16x16x32_f16 with signal and coefficients split into a high and a low FP16 part and three
 *       products per term (about 22 bits), FP32 accumulation; slopes and upward spreading in FP32, the slope
 *       filter (the one recurrence along the stream) FP64.  Tolerances this mode is held to by the parity suite
 *       (tests/gpu_common.py, column "f16x3"): MOVs 2e-6 relative, DI and ODG 1e-6 against the real reference's
 *       goldens; per-block excitation 1e-4; a stream cut into launches in different ways (session, broker,
 *       batch) agrees with itself to 1e-9.  Measured max |dODG| against the FP64 engine: 5e-7 over 39 advanced
 *       cases (profiles/r02_precision_ledger.json), 6e-6 over 4096 ten-second pairs (bench.py,
 *       advanced.reduced_precision_f16x3).  No range limit: a signal whose filtered peak leaves the FP16
 *       headroom (30 dB above full scale) runs at its own power-of-two scale.
 *   PEAQ_FIR_F32 (opt-in): the FIR bank on v_mfma_f32_16x16x4_f32 (5e-8), everything after it FP64.
 * peaq_ctx_set_fir_fp64(ctx, 0) selects PEAQ_FIR_F16X3, (ctx, 1) PEAQ_FIR_F64; the environment variables
 * PEAQ_AMD_FIR=f64|f16x3|f32 and PEAQ_AMD_FIR_FP64=1|0 set the mode at context creation.  peaq_version() names
 * the default.  Until release 0.2.0 the default was PEAQ_FIR_F16X3.  The basic version and everything
 * downstream of the spreading are FP64 in every mode.  Applies to the launches that follow.
 * Non-finite input samples (NaN / Inf in a float stream): the reference's DC-rejection filters are recursive
 * (fbearmodel.c:289-303), so one such sample makes every later filter-bank output of that signal NaN there, and it
 * does here; what differs is only how far BACK it reaches inside the launch that contains it -- PEAQ_FIR_F64
 * evaluates the long filters through running sums that are re-anchored once per launch (up to 840 blocks), so the
 * blocks of that launch in front of the sample may read NaN as well.  Finite input is assumed, as by the reference. */
#define PEAQ_FIR_F32   0
#define PEAQ_FIR_F64   1
#define PEAQ_FIR_F16X3 2
int peaq_ctx_set_fir_mode (peaq_ctx *ctx, int mode);
int peaq_ctx_get_fir_mode (const peaq_ctx *ctx);
int peaq_ctx_set_fir_fp64 (peaq_ctx *ctx, int enable);
int peaq_ctx_get_fir_fp64 (const peaq_ctx *ctx);

/* ---- session API ------------------------------------------------------------
 * Replaces, per element instance: g_object_new(PEAQ_TYPE_FFTEARMODEL /
 * _FILTERBANKEARMODEL) gstpeaq.c:364-365, peaq_movaccum_new x11 :376,
 * "number-of-bands"/"playback-level" :481-526, peaq_movaccum_set_mode :528-557,
 * _set_channels :580-584, alloc_per_channel_data :442-473.
 * `channels` is what set_caps learns (1 or 2); changing caps or the `advanced`
 * property means destroying and re-creating the session, as the reference
 * re-allocates all per-channel state there (gstpeaq.c:519,559,575,586). */
typedef struct peaq_session peaq_session;
int peaq_session_create (peaq_ctx *ctx, int advanced, int channels,
                         double playback_level_db, peaq_session **out);
void peaq_session_destroy (peaq_session *s);

/* pad_chain (gstpeaq.c:614-661): append interleaved F32 samples
 * (n = samples per channel) to the ref (pad 0) or test (pad 1) adapter and
 * process every frame that both adapters now hold (do_processing :596-611:
 * FFT frames 2048/1024; advanced additionally filter-bank blocks 192/192).
 * The data is copied before the call returns (SURVEY.md 8(b) ownership).
 * Processing is asynchronous on the session's HIP stream. */
int peaq_session_push (peaq_session *s, int pad, const float *interleaved, size_t n);

/* change_state PAUSED->READY (gstpeaq.c:764-776): one zero-padded frame from
 * whatever is left in the adapters (do_flush :716-745); leftovers may differ
 * between ref and test. */
int peaq_session_flush (peaq_session *s);

/* get_property "di"/"odg" (gstpeaq.c:484-492 -> calculate_di_* :1013-1063,
 * calculate_odg :1066-1078): callable at any time, idempotent.  movs receives
 * 11 or 5 values (may be NULL).  NaN-on-empty-accumulator behaviour of the
 * reference is preserved. */
int peaq_session_results (peaq_session *s, peaq_result *out);

/* set_property "playback_level" (gstpeaq.c:508-515 -> fftearmodel.c:305-314,
 * fbearmodel.c:249-254): the level factors of both ear models change, no state
 * does -- exactly what the reference's ear models do when the property changes
 * mid-stream.  The new level holds for the FFT frames and filter-bank blocks
 * that are processed by the pushes and the flush AFTER the call, whatever their
 * samples' age: samples that were pushed earlier and still wait for the other
 * pad (do_processing, gstpeaq.c:596-611) take it, frames and blocks that an
 * earlier push processed keep theirs.  What they left behind -- the smeared
 * excitation, the pattern layer's adapters, the filter bank's high-pass state
 * and the filtered samples the next blocks' FIR windows reach back into -- stays
 * as computed at the old level, as in the reference.  Callable at any time, also
 * before the first push (then the same as creating the session at that level)
 * and after the flush (no result changes).  A level outside 0 .. 130, NaN or a
 * NULL session: PEAQ_ERR_ARG, level and stream as before.
 * (tests/test_gpu_level_steps.py, against the reference driven along the same
 * schedules of pushes and level changes.) */
int peaq_session_set_level (peaq_session *s, double playback_level_db);

/* explicit reset (the reference never resets, gstpeaq.c:357-361; the element
 * does not call this): the stream starts over -- adapters, ear-model states,
 * pattern layer, accumulators, counters, a meter or an alignment that is set.
 * The playback level is NOT part of the stream: the level last set with
 * peaq_session_set_level (or the one of peaq_session_create) stays, so a reset
 * session equals a session created at that level. */
int peaq_session_reset (peaq_session *s);

/* ---- meter: sliding-window scores of a live stream ---------------------------------------------------------------------
 * peaq_session_results reads DI / ODG / totalsnr accumulated since sample 0: the score of a file, but no meter -- after
 * ten minutes it hardly moves whatever happens to the signal.  The meter reads the running stream the way
 * peaq_batch_run_windows / peaq_batch_run_adv_spans (below) read a finished pair: "how good were the last five seconds",
 * continuously, on the device behind the session's own launches, and without disturbing the stream.
 *
 * Geometry, in FFT frames of the running stream (1024 samples per channel at 48 kHz apart; peaq_meter_frames converts
 * seconds: max (1, round (seconds * 48000 / 1024))): a window of W = window_frames, a hop of H = hop_frames, a depth of
 * D = depth kept readings; W >= 1, H >= 1, K = ceil (W / H) <= 64 windows open at once, 1 <= D <= 4096.
 *   Frames.  Window k = 0, 1, 2, .. covers frames [a_k, b_k) = [k H, k H + W) of the stream; the flush frame counts as
 *            a frame like any other.
 *   Blocks (advanced version).  With start_k = a_k ? 1024 (a_k + 1) : 0 and e_k = 1024 (b_k + 1), the filter-bank
 *            blocks [start_k / 192, e_k / 192); a window that takes the stream's last frame takes all blocks to the
 *            last, the flush block included.
 * The reading of a window is exactly what the sections "windows" (basic version) and "spans" (advanced version) below
 * define for those frames and blocks: the read-out of accumulators reset just before the window's first unit and then
 * given what the stream's own accumulators are given in the window's units -- the same tentative / normal turns,
 * values, weights and gates --, the energies of totalsnr summed over those frames only.  A view into the running
 * stream, IN CONTEXT, not a cold start.  `frames` / `fb_blocks` of the record are the window's counts.
 *
 *   Delivery while streaming.  Window k is delivered once frame b_k - 1 has run and, in the advanced version, block
 *            e_k / 192 - 1 as well: both need the samples up to e_k on both pads.
 *   Delivery at the flush.  T = peaq_frame_count frames are then known.  Every window with b_k <= T is delivered, then
 *            one more: the oldest window with a_k < T < b_k, over frames [a_k, T) and the blocks to the end.  Younger
 *            open windows are discarded.
 *   Ring.    A delivered reading never changes.  The D newest delivered readings are kept; a reader that falls behind
 *            loses the oldest, and the loss is counted.
 *   Off is the default, and then nothing of a session's launches changes.
 *
 * Correspondence to the batch, with n = min (n_ref, n_test), m = max (n_ref, n_test): the reading of a window that does
 * not reach the stream's end is that of the batch window / span {start_k, e_k - start_k} of the pair; that of a window
 * that reaches it (the cut one, or a complete one whose last frame is the flush frame) is that of {start_k, m - start_k}.
 * Two corners have no sample window with exactly these frames: a complete window with e_k == m (the batch rule would add
 * the flush frame) and a window with start_k >= m, which holds only the flush frame.  peaq_meter_readings lists a finished
 * stream's readings by host arithmetic alone -- for every row its index k, first frame and frame count, first block and
 * block count, and the equivalent {start, length}, length == 0 in the two corners --; it leaves `r` of the rows
 * untouched, fills at most `cap` rows (rows may be NULL when cap is 0) and returns the count of all rows in *n.
 *
 * peaq_session_set_meter: NULL or window_frames == 0 switches the meter off.  Accepted only before the first push or
 * right after peaq_session_reset; otherwise, and for a geometry outside the limits above, PEAQ_ERR_ARG before a device
 * is touched, the message naming entry and value.  Workspace: (K + D + 2) snapshots of 2184 bytes and one launch's trace
 * records (64 frames of 128 bytes, 120 blocks of 96 bytes); PEAQ_ERR_NOMEM where that cannot be reserved.
 * peaq_session_meter_read: the delivered, not yet read readings, oldest first, at most `cap` of them (the rest stays
 * for the next call); *n_read their count; *dropped (may be NULL) the readings lost since the previous call because
 * more than D were delivered between two reads.  While the stream runs, a row's {start, length} is {start_k, e_k -
 * start_k}.  It waits for the session's enqueued work and changes nothing of the stream.  With the meter off:
 * PEAQ_ERR_ARG.  peaq_session_reset restarts the meter: the index starts at 0 again, unread readings are gone.  After
 * peaq_session_flush the list of readings is complete; it stays readable until the reset.
 * peaq_meter_frames refuses a NULL pointer and seconds that are negative, not a number or above 1e6 (PEAQ_ERR_ARG);
 * 0 seconds gives 1 frame.
 *
 * The broker (below): peaq_broker_set_meter sets ONE geometry for all sessions of the broker, because it shapes the
 * launch; accepted before the first peaq_broker_open and before peaq_broker_start (PEAQ_ERR_ARG otherwise), and for a
 * broker made by peaq_broker_create_multi in every shard.  A tick then adds one small kernel behind each back-end
 * launch, no copy and no wait: geometry and flush counts ride in the metadata rows the tick uploads anyway.  While a
 * metered session streams, a tick takes its filter-bank blocks no further than the frame after the last FFT frame
 * taken, so both paths stay at one sample horizon (nothing waits that would not wait for that frame anyway); its end
 * result is then that of the same stream cut into other launches.  peaq_broker_meter_read returns what was delivered up
 * to the last tick enqueued -- it waits for that tick and does not force one.  Closing a slot and opening it again
 * starts a fresh meter.  Workspace per slot: (K + D + 2) snapshots and a tick's trace records (8 frames, 48 blocks). */
typedef struct peaq_meter_config {
  uint32_t window_frames, hop_frames, depth;
} peaq_meter_config;
typedef struct peaq_meter_reading {
  uint64_t index;            /* k */
  uint64_t start, length;    /* the equivalent batch window / span in samples per channel; length 0: none (see above) */
  uint32_t first_frame, n_frames, first_block, n_blocks;
  peaq_result r;
} peaq_meter_reading;
size_t peaq_meter_reading_size (void);  /* sizeof (peaq_meter_reading) in THIS library, as peaq_broker_stats_size */
int peaq_meter_frames (double seconds, uint32_t *frames);
int peaq_meter_readings (uint64_t n_ref, uint64_t n_test, const peaq_meter_config *cfg,
                        peaq_meter_reading *rows, int cap, int *n);
int peaq_session_set_meter (peaq_session *s, const peaq_meter_config *cfg);
int peaq_session_meter_read (peaq_session *s, peaq_meter_reading *out, int cap, int *n_read, uint64_t *dropped);

/* ---- meter: band rows ---------------------------------------------------------------------------------------------------
 * The meter says in which window the score was lost; the band rows say in which band.  With the band meter on, every
 * reading carries rows 0 .. 3 of the band summary ("per-band summary" below), reduced on the device over the window's
 * frames: per band the sum of the noise-to-mask ratio, its maximum, the count of frames in which it is above 1.5 dB,
 * and the sum of the reference excitation -- a noise-to-mask spectrum per window, in the basic version (109 bands) and
 * the advanced version (55 bands).
 *
 * Counted frames.  Window k covers frames [a_k, b_k) = [k H, k H + W), cut at T at the flush, as above.  Let A_k be
 *   those of its frames that have PEAQ_TRACE_ABOVE -- the frame trace's flag: over all channels, the flush frame
 *   included.  The counted frames of the window are min A_k .. max A_k inclusive, none if A_k is empty: frames below the
 *   boundary in between count, a leading run before the first frame above it does not, a trailing run is dropped.
 *   This is what accumulators that start fresh at a_k count, and the rule of peaq_batch_run_band_summary with "the
 *   pair's frames" read as "the window's frames".
 * Rows.  peaq_meter_band_rows () = 4 rows per channel, each of row = peaq_band_row (advanced) doubles, with the meaning
 *   and order of PEAQ_BAND_SUMMARY_NMR_SUM, _NMR_MAX, _NMR_DISTURBED, _EXC_REF_SUM.  Sums are FP64 in frame order.
 *   Entry nb = peaq_band_count (advanced) of every row is the number of counted frames; a window without a counted
 *   frame reads 0 everywhere.  The values per frame are those of the running stream, in context, as the meter's scores
 *   are: those peaq_batch_run_bands gives for the planes PEAQ_BAND_NMR and PEAQ_BAND_EXC_REF in the window's frames.
 *
 * peaq_session_set_meter_bands (s, on): accepted where peaq_session_set_meter is, and it needs a meter that is set;
 * peaq_session_set_meter switches it off again, so the order is always meter, then bands.  Every open window keeps its
 * rows twice (the running rows, and the rows as they were at the last frame above the boundary), so with bands on the
 * geometry is limited to K = ceil (W / H) <= 16 and depth <= 256: outside that, PEAQ_ERR_ARG before a device is touched,
 * the message naming entry and value; PEAQ_ERR_NOMEM where the workspace cannot be reserved.  Off is the default, and
 * with bands off a metered session's and a broker's launches are exactly what they are without this section.
 * peaq_session_meter_read_bands: peaq_session_meter_read, with the same single cursor, that also fills
 *   rows[((i * channels + c) * 4 + k) * row + b]  for reading i, channel c, row k, entry b;
 * `rows` holds cap * channels * 4 * row doubles (NULL only with cap 0).  peaq_session_meter_read goes on working with
 * bands on and just does not copy rows.  With bands off: PEAQ_ERR_ARG.  peaq_session_reset restarts the rows with the
 * meter.
 * peaq_meter_bands_workspace: host arithmetic only; the device bytes the band meter adds to a session,
 *   *bytes = 8 channels (K (8 row + 2) + 4 (D + 2) row + 2 * 64 row)
 * -- per open window and channel the running and the saved rows and a status word, D + 2 delivered sets, and the two
 * planes of one launch's 64 frames --; a broker slot holds a tick's 8 frames in place of the 64.  It refuses a NULL
 * pointer, channels other than 1 or 2 and what peaq_session_set_meter_bands refuses for a geometry (PEAQ_ERR_ARG).
 * The broker: peaq_broker_set_meter_bands for every slot of the broker, every shard of a peaq_broker_create_multi broker
 * included -- accepted where peaq_broker_set_meter is, after it --, and peaq_broker_meter_read_bands; closing a slot
 * and opening it again starts fresh rows.  A tick adds one more small kernel behind the FFT back end; no new rows of
 * metadata, no copy, no wait. */
int peaq_meter_band_rows (void);
int peaq_meter_bands_workspace (const peaq_meter_config *cfg, int advanced, int channels, size_t *bytes);
int peaq_session_set_meter_bands (peaq_session *s, int on);
int peaq_session_meter_read_bands (peaq_session *s, peaq_meter_reading *out, double *rows, int cap, int *n_read,
                                   uint64_t *dropped);

/* ---- live alignment: find the chain's delay, align the pads, watch it move ---------------------------------------------
 * A monitored chain -- a codec, a link, a processor between the reference pad and the test pad -- has a delay, and PEAQ
 * takes the two signals as sample-aligned ("time alignment on the device" below, the batch side's cure).  Two things for a
 * live stream, both off by default; with both off nothing of a session's launches or a broker's ticks changes.
 *
 * Rule A, acquisition (max_lag != 0).  No frame and no block of the stream is taken until both pads hold at least `probe`
 *   samples per channel (0: 48000 + 2 max_lag), or the flush is called (session) or requested (broker).  At that moment,
 *   with have_ref / have_test what the pads hold: probe_ref = min (have_ref, probe), probe_test = min (have_test, probe);
 *   `d` is the record of peaq_batch_estimate_delay for one pair of those leading samples with this max_lag -- the same
 *   kernels, the same arg-max rule, bit for bit (a pad that holds nothing has the record that entry documents for an
 *   empty signal: all zero).  skip_* follow peaq_aligned_lengths: for lag >= 0 the test pad drops its first `lag`
 *   samples, for lag < 0 the reference pad drops -lag; a skip stops at what the pad holds; nothing is cut at the tail --
 *   a live stream ends when it ends, and the flush pads the leftovers as it always does.  From then on the stream behaves
 *   as a plain stream that was fed ref[skip_ref:] and test[skip_test:], the STREAM AS SCORED: framing, flush, the `frames`
 *   and `fb_blocks` counts and, with a meter, its frame indices, {start, length} and end-of-stream totals all count the
 *   stream as scored.  One device wait per stream, at its start, inside the push or flush that completes the probe.
 *   A silent or non-finite probe gives the aligner's lag = 0 with norm 0 or NaN: the stream then runs unaligned and the
 *   caller sees why in `d`.  Nothing retries; retrying is the caller's business, with peaq_session_reset.
 *   peaq_live_align_plan is rule A's arithmetic on the host, no device: the probe lengths and the skips for a lag
 *   (output pointers may be NULL).  PEAQ_ERR_ARG for a configuration that set_align would refuse, max_lag == 0, or
 *   |lag| > max_lag.
 *
 * Rule B, watch (watch_frames = W != 0).  r[n], t[n]: the mono sums in double of the stream as scored, as the aligner
 *   defines them.  Watch window k covers the whole FFT frames [k W, (k + 1) W); the flush frame is never counted and an
 *   incomplete last window is discarded.  For d = -31 .. 31:
 *     c[d] = sum r[n] t[n + d] over n = 1024 k W + 512 .. 1024 (k + 1) W + 511,
 *     e_ref = sum r[n]^2, e_test = sum t[n]^2 over the same n
 *   (every n + d lies inside the frame that owns n, so the watch reads only what the stream's launches have staged).
 *   norm = sqrt (e_ref e_test); offset = the d with the largest |c[d]|, values within 1e-12 norm of the largest counting
 *   as tied, ties to the smaller |d|, then to the positive d -- the aligner's rule; peak = c[offset]; runner_up = the
 *   largest |c| over the other lags.  A window with norm == 0 reads offset 0, peak 0, runner_up 0; one whose sums are not
 *   all finite reads the same with norm NaN.  peaq_delay_watch_pick is this rule on the host (PEAQ_ERR_ARG for a NULL c;
 *   the output pointers may be NULL).
 *   Arithmetic: samples FP32 as stored, then FP64; per frame a fixed order, frames added in frame order from 0 at each
 *   window's first frame.  A window's record does not depend on how pushes cut the stream into launches and is the same
 *   bit for bit from run to run; every c[d], e_ref, e_test is within 1e-9 norm of the exact sum (1024 W products, W <=
 *   65536: the derived bound is far below that).  The watch reports and never touches the stream.
 *
 * peaq_session_set_align: NULL, or max_lag == 0 && watch_frames == 0, switches both off.  Accepted only before the first
 * push or right after peaq_session_reset; otherwise, and for max_lag > 16384, a probe (after the default is filled in)
 * outside max_lag + 2048 .. 1 << 20, watch_frames > 65536 or reserved != 0: PEAQ_ERR_ARG before a device is touched, the
 * message naming entry and value.  The probe buffers are reserved here: PEAQ_ERR_NOMEM where that fails.
 * peaq_session_align_read (acquisition set) and peaq_session_watch_read (watch set) wait for the session's enqueued work
 * and change nothing; with their half off: PEAQ_ERR_ARG.  While the stream still holds, align_read gives acquired = 0
 * and everything else zero.  watch_read gives the newest complete window -- n_frames == 0 and everything else zero while
 * there is none --, is idempotent, and `index` tells whether the window is new.  peaq_session_reset starts over: the
 * stream holds again, the watch is at index 0 with nothing complete.
 *
 * The broker (below): peaq_broker_set_align sets ONE configuration for all sessions of the broker, accepted where
 * peaq_broker_set_meter is -- before the first peaq_broker_open and before peaq_broker_start, PEAQ_ERR_ARG otherwise --
 * and for a broker made by peaq_broker_create_multi in every shard.  No tick waits on the device for an estimate: a tick
 * finds the held slots whose probe is there (or whose flush has been requested), stages the probes of at most 8 of them
 * -- the rest wait for later ticks --, and enqueues ONE peaq_batch_estimate_delay over them and the copy of its records
 * to pinned memory; the next tick, after the wait for the previous tick's staging that every tick begins with, reads the
 * records and releases those streams, whose first units ride in that tick.  A stream's first result is therefore two
 * ticks later than without acquisition, more where over 8 streams start at once.  peaq_broker_push does not count a held
 * stream's samples up to `probe` towards its back-pressure limit.  peaq_broker_results and peaq_broker_align_read on a
 * slot that still holds with its flush requested tick until it is acquired (results: until it is drained); otherwise the
 * reads report what the last tick enqueued has left, wait for it, and force none.  The watch adds two small kernels
 * behind a tick's front-end launch over its FFT pairs, no copy and no wait: the whole-frame counts ride in one more
 * metadata row, uploaded with the watch on only.  A window's record is the same bit for bit between a session and a
 * broker slot.  Closing a slot and opening it again starts over. */
typedef struct peaq_live_align_config {
  uint32_t max_lag;       /* 0: no acquisition; else 1 .. 16384 as peaq_batch_estimate_delay */
  uint32_t probe;         /* samples per channel held on each pad for the estimate; 0: 48000 + 2 max_lag */
  uint32_t watch_frames;  /* W: 0 = no watch; else 1 .. 65536 FFT frames per watch window */
  uint32_t reserved;      /* 0 */
} peaq_live_align_config;
typedef struct peaq_live_delay {
  int32_t  acquired;               /* 0: still holding (everything else zero), 1: done */
  uint32_t probe_ref, probe_test;  /* samples the estimate saw */
  uint32_t skip_ref, skip_test;    /* samples dropped from the head of each pad */
  uint32_t reserved;
  struct { int32_t lag, reserved; double peak, runner_up, norm; } d;   /* peaq_delay, the aligner's own record */
} peaq_live_delay;
typedef struct peaq_delay_watch {
  uint64_t index;                  /* k of the newest complete window; valid only if n_frames != 0 */
  uint32_t first_frame, n_frames;  /* k W, W (n_frames 0: no window complete yet) */
  int32_t  offset;  int32_t reserved;
  double   peak, runner_up, norm, e_ref, e_test;
  double   c[63];                  /* c[d + 31], d = -31 .. 31 */
} peaq_delay_watch;
size_t peaq_live_delay_size (void);     /* the struct sizes in THIS library, as peaq_meter_reading_size */
size_t peaq_delay_watch_size (void);
int peaq_live_align_plan (const peaq_live_align_config *cfg, uint64_t have_ref, uint64_t have_test, int32_t lag,
                          uint32_t *probe_ref, uint32_t *probe_test, uint32_t *skip_ref, uint32_t *skip_test);
int peaq_delay_watch_pick (const double c[63], double e_ref, double e_test, int32_t *offset, double *peak,
                           double *runner_up, double *norm);
int peaq_session_set_align (peaq_session *s, const peaq_live_align_config *cfg);
int peaq_session_align_read (peaq_session *s, peaq_live_delay *out);
int peaq_session_watch_read (peaq_session *s, peaq_delay_watch *out);

/* ---- broker: many live sessions, one launch per tick -------------------------
 * Replaces, for a process hosting MANY `peaq` elements (BASELINE.json
 * configs[5]), the per-element device work of pad_chain -> do_processing
 * (gstpeaq.c:596-640): every element owns a session SLOT of one shared broker;
 * push only queues on the host, and each tick runs the frames that became
 * ready in all sessions as ONE batched front-end + back-end launch.  The
 * result of a session is identical to that of a peaq_session fed the same
 * stream (basic and advanced version).  All entry points are thread-safe. */
typedef struct peaq_broker peaq_broker;
typedef struct peaq_broker_stats_t {
  uint64_t ticks;        /* ticks executed (including idle ones)             */
  uint64_t launches;     /* ticks that launched device work                  */
  uint64_t frames;       /* FFT frames (per session, not per channel) run    */
  uint32_t max_active;   /* most sessions served by a single launch          */
  uint32_t worker_failed;/* the tick thread stopped on a device error        */
  /* Timing, in microseconds, over the ticks that launched device work (max, and the 99th percentile from a
   * histogram with 9 % resolution).  A session's LATENCY is the time from "a whole frame (block) of both pads
   * sits in its FIFO" (or its flush was requested) to "the device work of the tick that took it is complete",
   * i.e. wait for the next tick + that tick's host part + its device part: what the reference does inside
   * pad_chain (gstpeaq.c:614-661) the broker does at most one tick period later. */
  double   tick_host_us_max, tick_host_us_p99, tick_host_us_mean;        /* scan + staging copies + enqueue           */
  double   tick_device_us_max, tick_device_us_p99, tick_device_us_mean;  /* copies and kernels of one tick on the GPU */
  double   latency_us_max, latency_us_p99, latency_us_mean;
  uint64_t latency_samples;                         /* (session, tick) pairs behind the latency figures */
} peaq_broker_stats_t;
int  peaq_broker_create  (peaq_ctx *ctx, int advanced, int channels, double playback_level_db,
                          int max_sessions, peaq_broker **out);
/* The same over SEVERAL GPUs of a node (BASELINE.json configs[4] on an 8-GPU box): one device broker -- its own
 * context, slots, launch stream and tick thread -- per entry of `devices` (an ordinal may appear more than once:
 * two brokers on that GPU); a session is opened on the device that holds the fewest, stays there, and every call
 * below is forwarded by its id.  Sessions never exchange anything (gstpeaq.c:110-139: all state is per element), so
 * the devices' ticks are independent.  `settings` NULL = the reference's shipped values, `fir_mode` < 0 = the
 * engine's default (PEAQ_FIR_*).  max_sessions is rounded up to a multiple of the device count.  peaq_broker_stats
 * adds the counts up over the devices and reports the worst device's times. */
int  peaq_broker_create_multi (const int *devices, int n_devices, int advanced, int channels,
                               double playback_level_db, int max_sessions, const peaq_settings *settings,
                               int fir_mode, peaq_broker **out);
int  peaq_broker_devices (const peaq_broker *b);                       /* 1 for peaq_broker_create's */
/* Test hook: puts one device's share of a multi-device broker (shard 0 .. devices - 1 in the order of `devices`; 0 of a
 * plain broker) into the state a device error during one of its ticks leaves it in -- stopped for good, `message` kept
 * as its error.  What must hold then (tests/test_gpu_broker.py): peaq_broker_tick still ticks every other device and
 * returns this device's error; sessions on the other devices run to their results; every call on a session of the
 * failed device reports that device's own message. */
int  peaq_debug_broker_fail_shard (peaq_broker *b, int shard, const char *message);
void peaq_broker_destroy (peaq_broker *b);
int  peaq_broker_open    (peaq_broker *b, int *session_id);            /* gst_peaq_init / READY->PAUSED      */
int  peaq_broker_close   (peaq_broker *b, int session_id);             /* finalize                           */
int  peaq_broker_push    (peaq_broker *b, int session_id, int pad, const float *interleaved, size_t n_samples);
int  peaq_broker_flush   (peaq_broker *b, int session_id);             /* EOS: do_flush on the next tick     */
int  peaq_broker_tick    (peaq_broker *b, unsigned *n_active);         /* one batched launch, any thread     */
int  peaq_broker_results (peaq_broker *b, int session_id, peaq_result *out);  /* drains this session first   */
int  peaq_broker_start   (peaq_broker *b, unsigned period_us);         /* own tick thread (0 = 2000 us)      */
int  peaq_broker_stop    (peaq_broker *b);
int  peaq_broker_stats   (peaq_broker *b, peaq_broker_stats_t *out);
int  peaq_broker_set_meter (peaq_broker *b, const peaq_meter_config *cfg);     /* see "meter" above */
int  peaq_broker_meter_read (peaq_broker *b, int session_id, peaq_meter_reading *out, int cap, int *n_read,
                             uint64_t *dropped);
int  peaq_broker_set_meter_bands (peaq_broker *b, int on);                       /* see "meter: band rows" above */
int  peaq_broker_meter_read_bands (peaq_broker *b, int session_id, peaq_meter_reading *out, double *rows, int cap,
                                   int *n_read, uint64_t *dropped);
int  peaq_broker_set_align (peaq_broker *b, const peaq_live_align_config *cfg);   /* see "live alignment" above */
int  peaq_broker_align_read (peaq_broker *b, int session_id, peaq_live_delay *out);
int  peaq_broker_watch_read (peaq_broker *b, int session_id, peaq_delay_watch *out);
size_t peaq_broker_stats_size (void);   /* sizeof (peaq_broker_stats_t) in THIS library: a caller built against another
                                         * header compares before it hands over a buffer */

/* ---- batch API ------------------------------------------------------------
 * n_pairs whole pairs, inputs already in device memory as interleaved F32
 * [pair][sample][channel] with a fixed stride of `pair_stride` samples between
 * pairs.  n_ref / n_test give each pair's length in samples per channel (host
 * arrays of n_pairs entries; NULL = every pair has n_uniform samples).  Each
 * pair is framed and flushed exactly as one element run would be (full frames
 * + one zero-padded frame).  d_results: device array of n_pairs peaq_result.
 * `stream` is a hipStream_t (NULL = default stream); the call enqueues work
 * and returns, results are valid after the stream is synchronised. */
int peaq_batch_run (peaq_ctx *ctx, int advanced, int channels, double playback_level_db,
                    int n_pairs, const float *d_ref, const float *d_test, size_t pair_stride,
                    const uint32_t *n_ref, const uint32_t *n_test, uint32_t n_uniform,
                    peaq_result *d_results, void *stream);

/* Scratch the batch path needs for a given shape, in bytes (it is allocated
 * lazily inside the context and reused across calls). */
size_t peaq_batch_workspace_bytes (int advanced, int channels, int n_pairs, uint32_t n_max);

/* ---- trajectories: readings at fixed intervals through each pair -----------
 * The element's di / odg / totalsnr properties can be read at any time during a
 * stream (gstpeaq.c:484-497).  peaq_batch_run_trajectory takes such readings
 * every `interval` samples per channel (48 kHz) of every pair, in ONE batch run:
 *
 *   Point k (0 <= k < n_points) of pair p is exactly what peaq_session_results
 *   returns for a session that has been pushed the first
 *   min((k+1) interval, n_ref[p]) reference samples and the first
 *   min((k+1) interval, n_test[p]) test samples, and has NOT been flushed.
 *   With a = min((k+1) interval, n_ref[p], n_test[p]) that session has
 *   processed F(a) = a >= 2048 ? (a - 2048) / 1024 + 1 : 0 FFT frames
 *   (do_processing, gstpeaq.c:596-611) and, in the advanced version,
 *   B(a) = a / 192 filter-bank blocks.  The point's record carries
 *   frames = F(a), fb_blocks = B(a) (0 in basic) and the MOVs, DI, ODG and
 *   totalsnr of that state: tentative accumulators read their saved values,
 *   accumulators that are still empty read NaN, as in the reference.  Points
 *   past the end of both signals all hold the final UNFLUSHED reading.
 *
 * d_points: device array [n_pairs][n_points] of peaq_result.  d_results (may be
 * NULL): the flushed end result of every pair, bit for bit what peaq_batch_run
 * writes for the same inputs.  Arguments otherwise as for peaq_batch_run, and
 * the context's settings and FIR mode apply as they do there.  Returns
 * PEAQ_ERR_ARG for interval == 0, n_points < 1 or d_points == NULL, and
 * PEAQ_ERR_NOMEM when the snapshot scratch (n_pairs x n_points x about 2.2 KB)
 * cannot be reserved. */
int peaq_batch_run_trajectory (peaq_ctx *ctx, int advanced, int channels, double playback_level_db,
                               int n_pairs, const float *d_ref, const float *d_test, size_t pair_stride,
                               const uint32_t *n_ref, const uint32_t *n_test, uint32_t n_uniform,
                               uint32_t interval, int n_points,
                               peaq_result *d_points,   /* device, [n_pairs][n_points] */
                               peaq_result *d_results,  /* device, [n_pairs], may be NULL */
                               void *stream);
/* peaq_batch_workspace_bytes plus the snapshot scratch of n_points readings per pair. */
size_t peaq_batch_trajectory_workspace_bytes (int advanced, int channels, int n_pairs, uint32_t n_max, int n_points);

/* ---- traces: the MOV layer's values of every frame and block --------------------
 * A result says how good an item is, a trajectory how the reading developed; a trace says WHERE the score was lost:
 * peaq_batch_run_trace writes, in the same run that scores the batch, one record per FFT frame of every pair and, in
 * the advanced version, one per filter-bank block.
 *
 *   Frame record f of pair p holds the MOV layer's values of that frame BEFORE accumulation (the functions of movs.c
 *   named at the fields), computed for every frame whether or not the gates of gstpeaq.c let the accumulators see
 *   them; `flags` says which gates were open, so that a caller can reproduce what was counted:
 *     PEAQ_TRACE_ABOVE      the reference was above the data-boundary threshold in this frame / block
 *                           (is_frame_above_threshold, gstpeaq.c:1081-1099): the accumulators were NOT set tentative
 *     PEAQ_TRACE_MOD_OPEN   frame >= 24 (block >= 125): gstpeaq.c:871 / :988 let the modulation differences through
 *     PEAQ_TRACE_LOUD_OPEN  gstpeaq.c:880-881 / :996-997 let the noise loudness through: frame >= 24 and
 *                           frame - 3 >= loudness_reached_frame (block >= 125 and block - 13 >= ...), the subtraction
 *                           and the comparison unsigned, the frame in which the gate of :841-845 opens included
 *     PEAQ_TRACE_FLUSH      the zero-padded frame / block of the flush (gstpeaq.c:716-745)
 *   The frame records of the advanced version (its 55-band path has neither gate) carry ABOVE and FLUSH only.
 *   Pair p has peaq_frame_count (n_ref[p], n_test[p], 0) frame records, d_frames[p * frame_stride + f], and
 *   peaq_frame_count (n_ref[p], n_test[p], 1) block records, d_blocks[p * block_stride + b]; `frame` / `block` is the
 *   index.  Entries of the arrays past a pair's count are left untouched.
 *
 * d_results (may be NULL): bit for bit what peaq_batch_run writes for the same inputs.  Arguments otherwise as for
 * peaq_batch_run; the context's settings and FIR mode apply as they do there.  PEAQ_ERR_ARG, before any device is
 * touched and with a message that names the value: d_frames NULL or not 16-byte aligned (the records go out as
 * 16-byte stores; so d_blocks), a stride below the longest pair's count, d_blocks NULL in the advanced version or
 * non-NULL in the basic version, and everything peaq_batch_run refuses.  Trace and trajectory are separate calls. */
#define PEAQ_TRACE_ABOVE      1u
#define PEAQ_TRACE_MOD_OPEN   2u
#define PEAQ_TRACE_LOUD_OPEN  4u
#define PEAQ_TRACE_FLUSH      8u

typedef struct {            /* 128 bytes, one per (pair, FFT frame) */
  double   ch[2][6];        /* basic, per channel: ModDiff1, ModDiff2, TempWt (movs.c:205-254, with the factor 100 the
                             * accumulators see), noise loudness (:354-371), mean and maximum of the band noise-to-mask
                             * ratios, linear (:971-1023).  advanced (55-band path), per channel: 10 log10 of the mean
                             * band NMR (:1010-1020), that mean, four zeros.  mono: ch[1] is zero */
  double   p_detect, steps; /* basic: detection probability and steps above threshold of the frame, all channels
                             * (:1224-1276); advanced: 0 */
  uint32_t flags, frame;
  double   reserved;        /* 0 */
} peaq_frame_trace;

typedef struct {            /* 96 bytes, one per (pair, filter-bank block); advanced only */
  double   ch[2][5];        /* RmsModDiff and its weight (movs.c:205-254, :243-244), noise loudness and
                             * missing-components term of RmsNoiseLoudAsym (:551-577), AvgLinDist (:679-706).
                             * mono: ch[1] is zero */
  uint32_t flags, block;
  double   reserved;        /* 0 */
} peaq_block_trace;

int peaq_batch_run_trace (peaq_ctx *ctx, int advanced, int channels, double playback_level_db, int n_pairs,
                          const float *d_ref, const float *d_test, size_t pair_stride,
                          const uint32_t *n_ref, const uint32_t *n_test, uint32_t n_uniform,
                          peaq_frame_trace *d_frames, size_t frame_stride,     /* device, [n_pairs][frame_stride] */
                          peaq_block_trace *d_blocks, size_t block_stride,     /* device; advanced: required, basic: must be NULL */
                          peaq_result *d_results /* device, [n_pairs], may be NULL */, void *stream);
/* sizeof of both records in THIS library (returns the frame record's; either pointer may be NULL): a caller built
 * against another header compares before it hands over a buffer, as with peaq_broker_stats_size */
size_t peaq_trace_sizes (size_t *frame_bytes, size_t *block_bytes);
/* (peaq_run_pair_trace, the same for one pair from host memory: after peaq_run_pair_aligned below) */

/* ---- band traces: the FFT path's values per frame, channel and BAND ----------------
 * A frame trace says in which frames the score was lost; a band trace says at which frequency: peaq_batch_run_bands
 * writes, in the same run that scores the batch, the values the FFT back end has per critical band before it reduces
 * them to the frame trace's mean, maximum and probability -- a noise-to-mask spectrogram and what goes with it.
 * `planes` selects them (FP64, before accumulation, for every frame of the pair, the flush frame included):
 *     PEAQ_BAND_NMR       r = noise * mask_diff / exc_ref (movs.c:1002-1022), linear; its mean over the bands is the
 *                         frame trace's ch[c][4], its maximum ch[c][5]                          basic, advanced (55 bands)
 *     PEAQ_BAND_EXC_REF   the smeared reference excitation (fftearmodel.c:496-504), the denominator above; the masking
 *                         threshold is exc_ref / mask_diff                                       basic, advanced
 *     PEAQ_BAND_EXC_TEST  the smeared test excitation                                            basic
 *     PEAQ_BAND_DETECT    the channel's detection exponent x = (e / s)^b (movs.c:1239-1253): the band's probability is
 *                         1 - 2^-x, the frame's 1 - 2^-(sum_b max_c x)                           basic
 *     PEAQ_BAND_STEPS     the channel's steps above threshold q = |trunc e| / s (:1256-1260;
 *                         use_floor_for_steps_above_threshold applies); the frame's: sum_b max_c q   basic
 *   The 55-band path of the advanced version computes neither the test excitation nor the detection terms; the
 *   filter-bank path's 40 bands have a trace of their own (peaq_batch_run_fb_bands, below).
 *
 * Layout: the value of plane slot k -- the rank of the plane's bit among the set bits of `planes` -- sits at
 *   d_bands[((((p * frame_stride + f) * channels + c) * n_planes + k) * row) + b],  row = peaq_band_row (advanced),
 * b < peaq_band_count (advanced); the row's last entry (b = 109 of 110, 55 of 56) is written 0.  Pair p has
 * peaq_frame_count (n_ref[p], n_test[p], 0) frames; rows past a pair's count are left untouched.  peaq_band_tables
 * (host only, no device) gives the bands' centre frequencies in Hz and the mask_diff factors of the ratio above.
 *
 * d_results (may be NULL): bit for bit what peaq_batch_run writes for the same inputs; the context's settings and, in
 * the advanced version (whose filter-bank side runs as in peaq_batch_run), its FIR mode apply as they do there.
 * PEAQ_ERR_ARG, before any device is touched and with a message that names the value: planes zero or with a bit above
 * 16, a plane the version does not have, d_bands NULL or not 16-byte aligned (the rows go out as 16-byte stores), a
 * frame_stride below the longest pair's count, and everything peaq_batch_run refuses.  Band trace, trace and
 * trajectory are separate calls. */
#define PEAQ_BAND_NMR       1u
#define PEAQ_BAND_EXC_REF   2u
#define PEAQ_BAND_EXC_TEST  4u
#define PEAQ_BAND_DETECT    8u
#define PEAQ_BAND_STEPS    16u

int peaq_band_count (int advanced);      /* 109 / 55 */
int peaq_band_row (int advanced);        /* 110 / 56: doubles per row, the count rounded up to even */
int peaq_band_tables (int advanced, double *fc /* [count] */, double *mask_diff /* [count] */);   /* host only */
int peaq_batch_run_bands (peaq_ctx *ctx, int advanced, int channels, double playback_level_db, int n_pairs,
                          const float *d_ref, const float *d_test, size_t pair_stride,
                          const uint32_t *n_ref, const uint32_t *n_test, uint32_t n_uniform,
                          uint32_t planes, double *d_bands /* device */, size_t frame_stride,
                          peaq_result *d_results /* device, [n_pairs], may be NULL */, void *stream);
/* (peaq_run_pair_bands, the same for one pair from host memory: after peaq_run_pair_trace below) */

/* ---- band traces of the filter-bank path: its values per block, channel and BAND ----------------
 * Three of the advanced version's five MOVs come from the filter-bank path (RmsModDiff, RmsNoiseLoudAsym, AvgLinDist);
 * the block trace gives their five values per block and channel, peaq_batch_run_fb_bands the 40 per-band terms those
 * are summed from and the patterns they are made of -- in the same run that scores the batch.  There is no `advanced`
 * argument: the path exists in the advanced version only.  `planes` selects (FP64, before accumulation, for every
 * block of the pair, the flush block included, whatever the gates of gstpeaq.c:988/996 let the accumulators see -- the
 * block trace's convention).  With n the band's internal noise, er / et the excitations after time smearing
 * (fbearmodel.c:371-395), ur / ut the unsmeared ones, ar / at the level- and pattern-adapted patterns
 * (leveladapter.c:331-336), mr / mt the modulations (modpatt.c:245-247), lr the reference's average loudness
 * (modpatt.c:240-243) and, movs.c:709-743,
 *   T (alpha, f, m_ref, m_test, e_ref, e_test) =
 *       (n / stest)^0.23 ((1 + max (stest e_test - sref e_ref, 0) / (n + sref e_ref beta))^0.23 - 1),
 *       sref = f m_ref + 1, stest = f m_test + 1, beta = exp (-alpha (e_test - e_ref) / e_ref):
 *     PEAQ_FB_BAND_MODDIFF     |mr - mt| / (1 + mr)                                   (movs.c:224-251)
 *     PEAQ_FB_BAND_MODWT       lr / (lr + n^0.3)
 *     PEAQ_FB_BAND_NOISELOUD   T (2.5, 0.3, mr, mt, ar, at)
 *     PEAQ_FB_BAND_MISSING     T (1.5, 0.15, mt, mr, at, ar); with swap_mod_patts_for_noise_loudness_movs = 0:
 *                              T (1.5, 0.15, mr, mt, at, ar)
 *     PEAQ_FB_BAND_LINDIST     T (1.5, 0.15, mr, mr, ar, er); with the switch 0 the second modulation is mt
 *     PEAQ_FB_BAND_UNSM_REF / _UNSM_TEST / _EXC_REF / _EXC_TEST / _ADAPT_REF / _ADAPT_TEST / _MOD_REF / _MOD_TEST
 *                              ur, ut, er, et, ar, at, mr, mt
 *   With the block record of the same pair (peaq_block_trace, sums over the 40 bands):
 *     ch[c][0] = 100 / sqrt (40) sum MODDIFF      ch[c][1] = sum MODWT
 *     ch[c][2] = 0.6 sum NOISELOUD, and 0 where that is below 0.1
 *     ch[c][3] = 0.6 sum MISSING                  ch[c][4] = 0.6 sum LINDIST
 *
 * Layout: the value of plane slot k -- the rank of the plane's bit among the set bits of `planes` -- sits at
 *   d_bands[((((p * block_stride + b) * channels + c) * n_planes + k) * 40) + band].
 * Pair p has peaq_frame_count (n_ref[p], n_test[p], 1) blocks; rows past a pair's count are left untouched.
 * peaq_fb_band_tables (host only, no device) gives the bands' centre frequencies in Hz and their internal noise; either
 * pointer may be NULL, not both.
 *
 * d_results (may be NULL): bit for bit what peaq_batch_run writes for the same inputs in the advanced version; the
 * context's settings and FIR mode apply as they do there.  PEAQ_ERR_ARG, before a context or a device is touched and
 * with a message that names the value: planes zero or with a bit above 0x1000, d_bands NULL or not 16-byte aligned, a
 * block_stride below the longest pair's count, and everything peaq_batch_run refuses.  A run of its own, like the band
 * trace, the trace and the trajectory. */
#define PEAQ_FB_BAND_MODDIFF     0x0001u
#define PEAQ_FB_BAND_MODWT       0x0002u
#define PEAQ_FB_BAND_NOISELOUD   0x0004u
#define PEAQ_FB_BAND_MISSING     0x0008u
#define PEAQ_FB_BAND_LINDIST     0x0010u
#define PEAQ_FB_BAND_UNSM_REF    0x0020u
#define PEAQ_FB_BAND_UNSM_TEST   0x0040u
#define PEAQ_FB_BAND_EXC_REF     0x0080u
#define PEAQ_FB_BAND_EXC_TEST    0x0100u
#define PEAQ_FB_BAND_ADAPT_REF   0x0200u
#define PEAQ_FB_BAND_ADAPT_TEST  0x0400u
#define PEAQ_FB_BAND_MOD_REF     0x0800u
#define PEAQ_FB_BAND_MOD_TEST    0x1000u

int peaq_fb_band_count (void);           /* 40 */
int peaq_fb_band_tables (double *fc /* [40] */, double *internal_noise /* [40] */);   /* host only */
int peaq_batch_run_fb_bands (peaq_ctx *ctx, int channels, double playback_level_db, int n_pairs,
                             const float *d_ref, const float *d_test, size_t pair_stride,
                             const uint32_t *n_ref, const uint32_t *n_test, uint32_t n_uniform,
                             uint32_t planes, double *d_bands /* device */, size_t block_stride,
                             peaq_result *d_results /* device, [n_pairs], may be NULL */, void *stream);
/* (peaq_run_pair_fb_bands, the same for one pair from host memory: after peaq_run_pair_bands below) */

/* ---- band traces of the pattern layer: the basic version's modulation and noise-loudness terms per BAND ----------
 * Most of the basic version's ODG is made of pattern-layer MOVs (WinModDiff1, AvgModDiff1, AvgModDiff2, RmsNoiseLoud);
 * the frame trace gives their four values per frame and channel, peaq_batch_run_pattern_bands the 109 per-band terms
 * those are summed from and the patterns they are made of -- in the same run that scores the batch.  There is no
 * `advanced` argument: the 55-band FFT path of the advanced version computes neither (its pattern MOVs come from the
 * filter bank, peaq_batch_run_fb_bands above).  `planes` selects (FP64, before accumulation, for every frame of the
 * pair, the flush frame included, whatever the gates of gstpeaq.c:871 / :880-881 let the accumulators see -- the frame
 * trace's convention).  With n the band's internal noise, ur / ut the unsmeared excitations, er / et the excitations
 * after time smearing (fftearmodel.c:496-504), ar / at the level- and pattern-adapted patterns (leveladapter.c:331-336),
 * mr / mt the modulations (modpatt.c:245-247) and lr the reference's average loudness (modpatt.c:240-243):
 *     PEAQ_PAT_BAND_MODDIFF1    |mr - mt| / (1 + mr)                                   (movs.c:224-251)
 *     PEAQ_PAT_BAND_MODDIFF2    w |mr - mt| / (0.01 + mr), w = 1 where mt >= mr, else 0.1
 *     PEAQ_PAT_BAND_MODWT       lr / (lr + 100 n^0.3)
 *     PEAQ_PAT_BAND_NOISELOUD   (n / stest)^0.23 ((1 + max (stest at - sref ar, 0) / (n + sref ar beta))^0.23 - 1),
 *                               sref = 0.15 mr + 0.5, stest = 0.15 mt + 0.5, beta = exp (-1.5 (at - ar) / ar)
 *                               (movs.c:709-743 as gstpeaq.c:880-886 calls it); exactly 0 where stest at < sref ar
 *     PEAQ_PAT_BAND_UNSM_REF / _UNSM_TEST / _EXC_REF / _EXC_TEST / _ADAPT_REF / _ADAPT_TEST / _MOD_REF / _MOD_TEST /
 *     _AVGLOUD_REF              ur, ut, er, et, ar, at, mr, mt, lr; EXC_REF and EXC_TEST are bit for bit the planes of
 *                               the same name of peaq_batch_run_bands
 *   With the frame record of the same pair (peaq_frame_trace, basic version; sums over the 109 bands):
 *     ch[c][0] = 100 / 109 sum MODDIFF1           ch[c][1] = 100 / 109 sum MODDIFF2
 *     ch[c][2] = sum MODWT                        ch[c][3] = 24 / 109 sum NOISELOUD
 *   None of the six switches of peaq_settings touches these planes in the basic version
 *   (swap_mod_patts_for_noise_loudness_movs acts in the filter-bank path only).
 *
 * Layout: that of peaq_batch_run_bands for the basic version.  The value of plane slot k -- the rank of the plane's bit
 * among the set bits of `planes` -- sits at
 *   d_bands[((((p * frame_stride + f) * channels + c) * n_planes + k) * 110) + b],  b < 109;
 * the row's last entry (b = 109) is written 0.  Pair p has peaq_frame_count (n_ref[p], n_test[p], 0) frames; rows past
 * a pair's count are left untouched.  peaq_pattern_band_tables (host only, no device) gives the bands' centre
 * frequencies in Hz and their internal noise; either pointer may be NULL, not both.
 *
 * d_results (may be NULL): bit for bit what peaq_batch_run writes for the same inputs in the basic version; the
 * context's settings apply as they do there.  PEAQ_ERR_ARG, before a context or a device is touched and with a message
 * that names the value: planes zero or with a bit above 0x1000, d_bands NULL or not 16-byte aligned (the rows go out as
 * 16-byte stores), a frame_stride below the longest pair's count, and everything peaq_batch_run refuses.  A run of its
 * own, like the other band traces, the trace and the trajectory. */
#define PEAQ_PAT_BAND_MODDIFF1     0x0001u
#define PEAQ_PAT_BAND_MODDIFF2     0x0002u
#define PEAQ_PAT_BAND_MODWT        0x0004u
#define PEAQ_PAT_BAND_NOISELOUD    0x0008u
#define PEAQ_PAT_BAND_UNSM_REF     0x0010u
#define PEAQ_PAT_BAND_UNSM_TEST    0x0020u
#define PEAQ_PAT_BAND_EXC_REF      0x0040u
#define PEAQ_PAT_BAND_EXC_TEST     0x0080u
#define PEAQ_PAT_BAND_ADAPT_REF    0x0100u
#define PEAQ_PAT_BAND_ADAPT_TEST   0x0200u
#define PEAQ_PAT_BAND_MOD_REF      0x0400u
#define PEAQ_PAT_BAND_MOD_TEST     0x0800u
#define PEAQ_PAT_BAND_AVGLOUD_REF  0x1000u

int peaq_pattern_band_tables (double *fc /* [109] */, double *internal_noise /* [109] */);   /* host only */
int peaq_batch_run_pattern_bands (peaq_ctx *ctx, int channels, double playback_level_db, int n_pairs,
                                  const float *d_ref, const float *d_test, size_t pair_stride,
                                  const uint32_t *n_ref, const uint32_t *n_test, uint32_t n_uniform,
                                  uint32_t planes, double *d_bands /* device */, size_t frame_stride,
                                  peaq_result *d_results /* device, [n_pairs], may be NULL */, void *stream);
/* (peaq_run_pair_pattern_bands, the same for one pair from host memory: after peaq_run_pair_fb_bands below) */

/* ---- band summary: the band traces' values reduced over time on the device, one small row set per pair ----------
 * A result says how good an item is, a trajectory how the reading developed, a frame trace in which frames the score
 * was lost, the band traces at which frequency -- at rows per frame.  "In which bands does this coder lose, per item"
 * needs 109 numbers per item, not 109 per frame: peaq_batch_run_band_summary reduces the per-band values over the
 * pair's frames in the run that scores the batch, under the accumulators' own gates, and writes R =
 * peaq_band_summary_rows (advanced) rows of row = peaq_band_row (advanced) doubles per pair and channel:
 *   d_summary[((p * channels + c) * R + k) * row + b],  b < nb = peaq_band_count (advanced); entry b = nb of every row
 *   holds that row's denominator.
 *
 * Counted frames.  PEAQ_TRACE_ABOVE is defined as in the frame trace (over all channels, flush frame included).  With
 * A the set of the pair's frames that have it, the counted frames are min A .. max A inclusive -- frames in between
 * that are not above the data boundary count too -- and none if A is empty.  That is what the reference's
 * accumulators count (movaccum.c:317-362): nothing before the first frame above the boundary, and a trailing
 * tentative run dropped.
 *
 * Rows.  r, er, et are the values of PEAQ_BAND_NMR / _EXC_REF / _EXC_TEST, the other terms those of PEAQ_PAT_BAND_*:
 *   k  PEAQ_BAND_SUMMARY_     value at band b < nb                                             entry nb
 *   0  NMR_SUM                sum over the counted frames of r[b], FP64, in frame order         their number n
 *   1  NMR_MAX                max over the counted frames of r[b]; 0 if none                    n
 *   2  NMR_DISTURBED          number of counted frames with r[b] > 1.41253754462275 (1.5 dB,    n
 *                             the RelDistFrames threshold, per band)
 *   3  EXC_REF_SUM            sum over the counted frames of er[b]                              n
 *   4  EXC_TEST_SUM           sum over the counted frames of et[b]                              n
 *   5  MODDIFF1_WSUM          sum over the counted frames >= 24 (PEAQ_TRACE_MOD_OPEN) of         sum of those W
 *                             W MODDIFF1[b], W = sum_b MODWT[b] of that frame and channel
 *                             (the frame trace's ch[c][2])
 *   6  MODDIFF2_WSUM          the same with MODDIFF2                                            sum of those W
 *   7  NOISELOUD_SUM          sum over the counted frames with PEAQ_TRACE_LOUD_OPEN of          their number
 *                             NOISELOUD[b]
 * The advanced version (its 55-band path) has rows 0 .. 3; rows 4 .. 7 exist in the basic version only.  A pair with no
 * counted frame reads 0 everywhere, denominators included.  With the MOVs of the same pair (basic version):
 *   TotalNMR_B   = mean_c 10 log10 (sum_b row0 / (109 n))
 *   AvgModDiff1_B = mean_c (100 / 109) sum_b row5 / (sum of W);  AvgModDiff2_B likewise with row 6
 *   sum_b row0 / nb is the sum, over the counted frames, of the frame trace's ch[c][4] (basic) / ch[c][1] (advanced)
 *   max_b row2 <= (number of disturbed counted frames of the channel) <= sum_b row2
 *
 * The call writes every row of the n_pairs pairs completely (no plane mask: a whole summary is 14 KB per stereo pair);
 * memory past them is left untouched.  d_summary is working memory of the call while it runs -- the pairs' running
 * rows live there between the launches -- and valid after the stream has been synchronised.  The context keeps a
 * second array of the same size (the rows as they were when a pair last turned tentative), reserved on the first such
 * call: PEAQ_ERR_NOMEM if that fails.
 *
 * d_results (may be NULL): bit for bit what peaq_batch_run writes for the same inputs.  PEAQ_ERR_ARG, before a context
 * or a device is touched and with a message that names the value: d_summary NULL or not 16-byte aligned, and everything
 * peaq_batch_run refuses.  A run of its own, like the band traces, the trace and the trajectory.  The filter-bank
 * path's 40 bands have a summary of their own: peaq_batch_run_fb_band_summary, below. */
#define PEAQ_BAND_SUMMARY_NMR_SUM        0
#define PEAQ_BAND_SUMMARY_NMR_MAX        1
#define PEAQ_BAND_SUMMARY_NMR_DISTURBED  2
#define PEAQ_BAND_SUMMARY_EXC_REF_SUM    3
#define PEAQ_BAND_SUMMARY_EXC_TEST_SUM   4   /* basic version only, like the three below */
#define PEAQ_BAND_SUMMARY_MODDIFF1_WSUM  5
#define PEAQ_BAND_SUMMARY_MODDIFF2_WSUM  6
#define PEAQ_BAND_SUMMARY_NOISELOUD_SUM  7

int peaq_band_summary_rows (int advanced);            /* 8 / 4 */
int peaq_batch_run_band_summary (peaq_ctx *ctx, int advanced, int channels, double playback_level_db, int n_pairs,
                                 const float *d_ref, const float *d_test, size_t pair_stride,
                                 const uint32_t *n_ref, const uint32_t *n_test, uint32_t n_uniform,
                                 double *d_summary /* device */, peaq_result *d_results /* device, may be NULL */,
                                 void *stream);
/* (peaq_run_pair_band_summary, the same for one pair from host memory: after peaq_run_pair_pattern_bands below) */

/* ---- band summary of the filter-bank path: the 40 bands behind RmsModDiff, RmsNoiseLoudAsym and AvgLinDist -------
 * Three of the advanced version's five MOVs come from the filter-bank path.  peaq_batch_run_fb_band_summary reduces
 * the term planes of peaq_batch_run_fb_bands over the pair's blocks in the run that scores the batch, under the
 * accumulators' own gates, and writes peaq_fb_band_summary_rows () = 7 rows of peaq_fb_band_summary_row () = 42
 * doubles per pair and channel (advanced version only: there is no `advanced` argument):
 *   d_summary[((p * channels + c) * 7 + k) * 42 + b],  b < 40; entry 40 of every row holds that row's denominator,
 *   entry 41 is written 0.  A stereo pair takes 4704 bytes.
 *
 * Counted blocks.  PEAQ_TRACE_ABOVE is defined as in the block trace (any reference channel, flush block included).
 * With A the set of the pair's blocks that have it, the counted blocks are min A .. max A inclusive -- blocks in
 * between that are below the data boundary count too -- and none if A is empty: what the reference's accumulators
 * count (movaccum.c:317-362), as for the frames of peaq_batch_run_band_summary.
 *
 * Rows.  The plane names are those of PEAQ_FB_BAND_*.  Per block and channel W = sum_b MODWT[b] (the block trace's
 * ch[c][1]), D = sum_b MODDIFF[b], L = the block trace's ch[c][2] (0.6 sum_b NOISELOUD[b], and 0 where that is below
 * 0.1), M = ch[c][3] (0.6 sum_b MISSING[b]):
 *   k  PEAQ_FB_BAND_SUMMARY_  value at band b < 40                                              entry 40
 *   0  EXC_REF_SUM            sum over the counted blocks of EXC_REF[b], FP64, in block order    their number n
 *   1  EXC_TEST_SUM           the same of EXC_TEST[b]                                           n
 *   2  MODDIFF_WSUM           sum over the counted blocks with PEAQ_TRACE_MOD_OPEN (>= 125) of   sum of those W
 *                             W MODDIFF[b]
 *   3  MODDIFF_SQ             sum over the same blocks of W^2 D MODDIFF[b]: the band's share    sum of those W^2
 *                             of the square RmsModDiff averages
 *   4  NOISELOUD_SQ           sum over the counted blocks with PEAQ_TRACE_LOUD_OPEN of          their number m
 *                             L NOISELOUD[b] (0 for a block whose L is floored to 0)
 *   5  MISSING_SQ             sum over the same blocks of M MISSING[b]                          m
 *   6  LINDIST_SUM            sum over the same blocks of LINDIST[b]                            m
 * A pair with no counted block reads 0 everywhere, denominators included.  The context's
 * swap_mod_patts_for_noise_loudness_movs acts on MISSING and LINDIST as in the band trace.  With the MOVs of the same
 * call (order of the advanced version: 0, 1, 4):
 *   RmsModDiff_A       = mean_c (100 / sqrt 40) sqrt (sum_b row3 / row3[40])
 *   RmsNoiseLoudAsym_A = mean_c (sqrt (0.6 sum_b row4 / m) + 0.5 sqrt (0.6 sum_b row5 / m))
 *   AvgLinDist_A       = mean_c 0.6 sum_b row6 / m
 *   sum_b row2 is the sum over the same blocks of W D; per block, from the block trace: ch[c][1] ch[c][0] sqrt 40 / 100
 *
 * Every row of the n_pairs pairs is written completely; memory past them is left untouched.  d_summary is working
 * memory of the call while it runs and valid after the stream has been synchronised; the context's second array (the
 * rows as they were when a pair last turned tentative) is the one peaq_batch_run_band_summary uses: PEAQ_ERR_NOMEM if
 * it cannot be reserved, before anything is enqueued.
 *
 * d_results (may be NULL): bit for bit what peaq_batch_run writes for the same inputs in the advanced version; the
 * context's settings and FIR mode apply as they do there.  PEAQ_ERR_ARG, before a context or a device is touched:
 * d_summary NULL or not 16-byte aligned (the address is in the message), and everything peaq_batch_run refuses.  A run
 * of its own, like the other band outputs. */
#define PEAQ_FB_BAND_SUMMARY_EXC_REF_SUM   0
#define PEAQ_FB_BAND_SUMMARY_EXC_TEST_SUM  1
#define PEAQ_FB_BAND_SUMMARY_MODDIFF_WSUM  2
#define PEAQ_FB_BAND_SUMMARY_MODDIFF_SQ    3
#define PEAQ_FB_BAND_SUMMARY_NOISELOUD_SQ  4
#define PEAQ_FB_BAND_SUMMARY_MISSING_SQ    5
#define PEAQ_FB_BAND_SUMMARY_LINDIST_SUM   6

int peaq_fb_band_summary_rows (void);                 /* 7 */
int peaq_fb_band_summary_row (void);                  /* 42: doubles per row */
int peaq_batch_run_fb_band_summary (peaq_ctx *ctx, int channels, double playback_level_db, int n_pairs,
                                    const float *d_ref, const float *d_test, size_t pair_stride,
                                    const uint32_t *n_ref, const uint32_t *n_test, uint32_t n_uniform,
                                    double *d_summary /* device */, peaq_result *d_results /* device, may be NULL */,
                                    void *stream);
/* (peaq_run_pair_fb_band_summary, the same for one pair from host memory: after peaq_run_pair_band_summary below) */

/* ---- windows: the score of a stretch of each pair, replayed on the device (basic version) -------------------------
 * "The worst five seconds", "ODG per scene", a sliding short-term ODG: the reading of the frames a time window covers,
 * as a full result record.  A trajectory point cannot give it (it averages everything since sample 0, and two points
 * cannot be subtracted: WinModDiff1, ADB, MFPD and the tentative/saved logic are no differences of sums, the network is
 * not linear), and the frame trace leaves bandwidths, EHS, energies, accumulation and read-out to the caller.
 *
 * A window {start, length} counts samples per channel at 48 kHz.  With n = min (n_ref, n_test), m = max (n_ref,
 * n_test), T = peaq_frame_count (n_ref, n_test, 0), F (a) = a >= 2048 ? (a - 2048) / 1024 + 1 : 0 (the trajectory's F)
 * and e = start + length in 64 bits, its frames are [first, end):
 *     first = start >= m ? T : F (min (start, n)),      end = e >= m ? T : F (min (e, n)),      count = end - first
 * -- a window that reaches the end of the longer signal takes the flush frame.  peaq_window_frames returns exactly this
 * (host arithmetic only; first / count may be NULL, not both), and the device uses the same rule.
 *
 * The reading of a window is what peaq_session_results would return if
 *   - the 11 accumulators had been reset to their initial state just before frame `first` (status initial, every field
 *     zero, the AVG_WINDOW history at its NaN sentinels),
 *   - they had then been given, for the frames first .. end - 1 in order, exactly what the pair's own accumulators are
 *     given in those frames: the same tentative / normal turns, the same values and weights, the same gates, and
 *   - the two energies of totalsnr had been summed over those frames only.
 * Everything below the accumulators is the pair's own, IN CONTEXT: time smearing, level and pattern adaptation, the
 * modulation filters, the gate that keeps the first 24 frames out of the modulation MOVs and the loudness gate are
 * where the running stream has them.  A window is a view into the running stream, NOT a cold-start score of the
 * excerpt: for that, score the excerpt as a pair of its own -- a pair_stride view into the same buffers through
 * peaq_batch_run -- whose ear models, adaptation and gates then start cold, at the price of one front end per window.
 * `frames` of a window's record is count, `fb_blocks` 0.  An empty window (count == 0) reads what the read-out of an
 * untouched accumulator set reads, like a trajectory point before the first frame.
 * It follows (same operations, same order, from 0 + x): a window {0, L} with L < m is bit for bit point k of
 * peaq_batch_run_trajectory with (k + 1) interval == L; a window {0, L} with L >= m is bit for bit d_results; and
 * d_results is bit for bit peaq_batch_run's.
 *
 * windows (HOST, n_windows of them, 1 .. PEAQ_WINDOWS_MAX, none of length 0) are shared by all pairs; d_windows
 * (device, 16-byte aligned) receives [n_pairs][n_windows] records; d_results may be NULL.  The other arguments, the
 * refusals (PEAQ_ERR_ARG before a context or a device is touched, the message naming entry and value), stream and
 * workspace rules are peaq_batch_run's; PEAQ_ERR_NOMEM when the scratch cannot be reserved --
 * peaq_batch_windows_workspace_bytes: per pair a 128-byte trace record per frame and a 2184-byte snapshot per window on
 * top of the plain run's.  The call is a run of its own, like the traces and the trajectory.  There is no `advanced`
 * argument: the advanced version's windows are peaq_batch_run_adv_spans below. */
typedef struct { uint32_t start, length; } peaq_window;   /* samples per channel at 48 kHz */
#define PEAQ_WINDOWS_MAX 4096
int peaq_window_frames (uint32_t n_ref, uint32_t n_test, uint32_t start, uint32_t length,
                        uint32_t *first, uint32_t *count);
int peaq_batch_run_windows (peaq_ctx *ctx, int channels, double playback_level_db, int n_pairs,
                            const float *d_ref, const float *d_test, size_t pair_stride,
                            const uint32_t *n_ref, const uint32_t *n_test, uint32_t n_uniform,
                            const peaq_window *windows /* host, shared by all pairs */, int n_windows,
                            peaq_result *d_windows /* device, [n_pairs][n_windows] */,
                            peaq_result *d_results /* device, [n_pairs], may be NULL */, void *stream);
size_t peaq_batch_windows_workspace_bytes (int channels, int n_pairs, uint32_t n_max, int n_windows);
/* (peaq_run_pair_windows, the same for one pair from host memory: after peaq_run_pair_fb_band_summary below) */

/* ---- spans: the score of a stretch of each pair in the advanced version, replayed on the device ----------------------
 * The same reading as the section above gives for the basic version, for the advanced one.  The advanced version has
 * two feeds with two units: the 55-band FFT path in frames of 2048 samples every 1024 (SegmentalNMR, EHS, the energies of
 * totalsnr) and the filter-bank path in blocks of 192 samples (RmsModDiff, RmsNoiseLoudAsym, AvgLinDist).
 *
 * A span {start, length} is a peaq_window: samples per channel at 48 kHz.  With n = min (n_ref, n_test), m = max (n_ref,
 * n_test) and e = start + length in 64 bits:
 *   Frames.  [first, end) exactly as peaq_window_frames gives them: F, T = peaq_frame_count (n_ref, n_test, 0).
 *   Blocks.  With B (a) = a / 192 (the trajectory's B) and TB = peaq_frame_count (n_ref, n_test, 1), [first_b, end_b):
 *     first_b = start >= m ? TB : B (min (start, n)),   end_b = e >= m ? TB : B (min (e, n)),   count_b = end_b - first_b
 * -- a span that reaches the end of the longer signal takes the flush frame and the flush block.  peaq_span_blocks
 * returns exactly the block rule (host arithmetic only; first / count may be NULL, not both), and the device uses the
 * same function.
 *
 * The reading of a span is what peaq_session_results of an advanced session would return if
 *   - the five accumulators had been reset to their initial state just before frame `first` / block `first_b` (status
 *     initial, every field zero),
 *   - SegmentalNMR and EHS had then been given, for the frames first .. end - 1 in order, and RmsModDiff,
 *     RmsNoiseLoudAsym and AvgLinDist, for the blocks first_b .. end_b - 1 in order, exactly what the pair's own
 *     accumulators are given in those frames and blocks: the same tentative / normal turns (from the frame's, the
 *     block's own data-boundary flag), the same values and weights, the same gates, and
 *   - the two energies of totalsnr had been summed over those frames only.
 * What each accumulator is given (PEAQ_TRACE_* are the flags of the unit's trace record):
 *     RmsModDiff        block   when PEAQ_TRACE_MOD_OPEN    the block record's ch[c][0], weight ch[c][1]
 *     RmsNoiseLoudAsym  block   when PEAQ_TRACE_LOUD_OPEN   ch[c][2] and ch[c][3] (noise loudness, missing components)
 *     AvgLinDist        block   when PEAQ_TRACE_LOUD_OPEN   ch[c][4], weight 1
 *     SegmentalNMR      frame   always                      the frame record's ch[c][0], weight 1
 *     EHS               frame   when either signal has its energy bit in any channel    1000 ehs, weight 1
 * Everything below the accumulators is the pair's own, IN CONTEXT: both ear models, time smearing, level and pattern
 * adaptation, the modulation filters, the gate that keeps the first 125 blocks out of the filter-bank MOVs and the
 * loudness gate are where the running stream has them.  A span is a view into the running stream, NOT a cold-start
 * score of the excerpt: for that, score the excerpt as a pair of its own -- a pair_stride view into the same buffers
 * through peaq_batch_run -- whose ear models, adaptation and gates then start cold, at the price of both front ends per
 * span (every row of such a view, pair_stride samples from its first one, has to lie inside the caller's allocation: the
 * kernels may read a row beyond the pair's length, so the last pair needs that much room behind it).  `frames` of a span's record is end - first, `fb_blocks` is count_b.  An empty span reads what the read-out of an
 * untouched accumulator set reads, like a trajectory point before the first frame.
 * It follows (same operations, same order, from 0 + x; default FP64 engine): a span {0, L} with L < m is bit for bit
 * point k of peaq_batch_run_trajectory (advanced = 1) with (k + 1) interval == L; a span {0, L} with L >= m is bit for
 * bit d_results; and d_results is bit for bit peaq_batch_run's.
 *
 * spans (HOST, n_spans of them, 1 .. PEAQ_WINDOWS_MAX, none of length 0) are shared by all pairs; d_spans (device,
 * 16-byte aligned) receives [n_pairs][n_spans] records; d_results may be NULL.  The other arguments, the refusals
 * (PEAQ_ERR_ARG before a context or a device is touched, the message naming entry and value), stream and workspace rules
 * are peaq_batch_run's; PEAQ_ERR_NOMEM when the scratch cannot be reserved, before anything is enqueued --
 * peaq_batch_adv_spans_workspace_bytes: peaq_batch_workspace_bytes (1, ..) plus, per pair, a 128-byte trace record per
 * frame, a 96-byte trace record per block and a 2184-byte snapshot per span, plus 8 bytes per span.  The call is a run of
 * its own, like the traces, the trajectory and the basic version's windows. */
int peaq_span_blocks (uint32_t n_ref, uint32_t n_test, uint32_t start, uint32_t length,
                      uint32_t *first, uint32_t *count);
int peaq_batch_run_adv_spans (peaq_ctx *ctx, int channels, double playback_level_db, int n_pairs,
                              const float *d_ref, const float *d_test, size_t pair_stride,
                              const uint32_t *n_ref, const uint32_t *n_test, uint32_t n_uniform,
                              const peaq_window *spans /* host, shared by all pairs */, int n_spans,
                              peaq_result *d_spans /* device, [n_pairs][n_spans] */,
                              peaq_result *d_results /* device, [n_pairs], may be NULL */, void *stream);
size_t peaq_batch_adv_spans_workspace_bytes (int channels, int n_pairs, uint32_t n_max, int n_spans);
/* (peaq_run_pair_adv_spans, the same for one pair from host memory: after peaq_run_pair_windows below) */

/* Timing of the last peaq_batch_run on this context, measured with HIP events
 * on `stream`: total milliseconds, and milliseconds / launch count of the
 * dominant kernel (the FFT ear-model front end).  Valid after the stream has
 * been synchronised.  Used by bench.py for the roofline line. */
typedef struct {
  float total_ms;
  float frontend_ms;      /* sum over launches of the front-end kernel */
  int   frontend_launches;
  float backend_ms;
  int   backend_launches;
  float fb_ms;            /* advanced: filter-bank kernels */
  int   fb_launches;
} peaq_batch_timing;
int peaq_batch_last_timing (peaq_ctx *ctx, peaq_batch_timing *out);
/* The shader clock (MHz) the device held while the last batch ran: one workgroup of every back-end launch reads the
 * shader-clock counter and the constant-rate counter around its own lifetime -- beside the front end of the next chunk,
 * i.e. under the step's own load; 0 before the first batch.  With peaq_calibrate() what lets a throughput number be
 * read as "this library at this clock". */
int peaq_batch_last_clock (peaq_ctx *ctx, double *shader_clock_mhz);

/* One whole pair from HOST memory (interleaved F32, n samples per channel each): upload + the batch path
 * with one pair + result.  For callers that hold both signals completely (gstpeaq_amd/cli/peaq.c); same
 * framing, flush and results as a session fed with the same samples (gstpeaq.c:596-611, 716-745). */
int peaq_run_pair (peaq_ctx *ctx, int advanced, int channels, double playback_level_db,
                   const float *ref, size_t n_ref, const float *test, size_t n_test, peaq_result *out);
/* The same with the n_points readings of peaq_batch_run_trajectory into `points` (host, n_points records);
 * `out` (may be NULL) receives the flushed end result. */
int peaq_run_pair_trajectory (peaq_ctx *ctx, int advanced, int channels, double playback_level_db,
                              const float *ref, size_t n_ref, const float *test, size_t n_test,
                              uint32_t interval, int n_points, peaq_result *points /* host */, peaq_result *out);

/* ---- sample-rate conversion to 48 kHz on the device -----------------------------
 * The ear models are defined for 48 kHz only (earmodel.c:43) and every entry point above takes 48 kHz.  The
 * reference's CLI puts `audioresample` in front of the element (peaq.c:154-209); gstpeaq_amd/cli/peaq.c stands in for
 * it with a Kaiser-windowed sinc interpolator (resample_to_48k) whose parameters are the measured ones of that
 * `audioresample`.  peaq_batch_resample is the same converter for whole batches resident in device memory: same
 * filter, same tap table (built on the host in double, once per rate and context), same output length, samples in
 * FP32, taps and accumulation in FP64 in the tap order j = 0 .. 2K-1, one rounding to FP32 at the end -- the CLI's
 * samples up to the rounding of the FP64 sum (the device contracts multiply and add; |difference| <= one FP32 ulp).
 *
 *   g = gcd (48000, rate), L = 48000 / g, M = rate / g.  Output sample m sits at input position
 *   t_m = m M / L - 1/8: a delay of one eighth of an INPUT sample, audioresample's.
 *   y[m] = sum_j h_p[j] x[n_first + j], j = 0 .. 2K-1, p = (m M) mod L,
 *   n_first = (m M) div L + floor (p / L - 1/8) - K + 1; taps outside [0, n) contribute nothing.
 *   rate < 48000: cutoff 0.94 x 0.5, half width 32.15, Kaiser beta 8.49; rate > 48000: cutoff
 *   0.921 x 0.5 x 48000 / rate, half width 4 ceil (64 rate / 48000 / 8), beta 8.41; K = ceil (half width) + 1.
 *   Length: n samples per channel become n ? floor ((n - 1) x 48000 / rate) + 1 : 0, evaluated in double as
 *   the CLI does (the last output sample is the last one whose position does not pass the last input sample).
 *
 * Supported rates: 8000 <= rate <= 384000 with L <= 4096, 48000 itself excluded (nothing to convert: hand the
 * buffers straight on) -- 8, 11.025, 16, 22.05, 24, 32, 44.1, 88.2, 96, 176.4 and 192 kHz among them.  Every other
 * rate is PEAQ_ERR_ARG with a message that names it.  Non-finite input samples: the device evaluates a few
 * zero-valued taps beside each filter's 2K (fewer than 4 ceil (rate / 48000) + 4), so an Inf or NaN reaches that many more
 * output samples than in the CLI. */
int      peaq_resample_supported (uint32_t rate);              /* 1 if peaq_batch_resample takes this rate, else 0 */
/* Samples per channel at 48 kHz of n samples per channel at `rate` (any rate > 0, supported or not).  A length that
 * does not fit uint32_t, or rate 0, returns 0 with peaq_last_error() set (the message is cleared on success). */
uint32_t peaq_resampled_length   (uint64_t n, uint32_t rate);
/* Converts one buffer of the batch layout -- interleaved F32 [pair][sample][channel], `in_stride` samples per channel
 * between pairs, lengths n_in (host array of n_pairs entries; NULL = n_uniform each) -- into d_out of the same layout
 * with `out_stride` samples between pairs.  n_out (host, may be NULL) receives each pair's converted length, valid
 * on return.  Samples of d_out between a pair's converted length and out_stride are left untouched.  out_stride
 * smaller than the longest converted signal, a pair longer than in_stride, a length that does not fit uint32_t,
 * channels other than 1 or 2, more than 65535 pairs, NULL buffers and unsupported rates are PEAQ_ERR_ARG.  Enqueues
 * on `stream` and returns, like peaq_batch_run, and synchronises nothing: per-pair lengths travel through one of four
 * pinned staging slots and are copied on `stream` itself; only the fifth call in a row with lengths waits, for the
 * FIRST one's kernel.  (The first call for a rate on a context builds and uploads that rate's table, synchronously.)
 * Call it for the reference and for the test buffer and hand the results and n_out to peaq_batch_run /
 * peaq_batch_run_trajectory (whose `interval` stays in 48 kHz samples). */
int peaq_batch_resample (peaq_ctx *ctx, int channels, uint32_t rate, int n_pairs,
                         const float *d_in, size_t in_stride, const uint32_t *n_in, uint32_t n_uniform,
                         float *d_out, size_t out_stride, uint32_t *n_out /* host, may be NULL */, void *stream);
/* What the device converter does for `rate`, computed on the host (no device needed): the reduced ratio, the filter
 * length, which kernel takes the rate and what its workgroups need -- what tests/test_resample_budgets.py holds to
 * the ceilings of DESIGN.md 10, and what tools/resample_cost.py counts work with. */
typedef struct peaq_resample_plan {
  uint32_t L, M;              /* 48000 / g, rate / g */
  uint32_t taps;              /* 2K */
  int      tiled;             /* 1: resample_tile_kernel (both tiles fit a CU's LDS), 0: resample_any_kernel */
  uint32_t period_out, period_in;  /* tiled: L' = c L outputs and M' = c M inputs per lane */
  uint32_t zero_taps;         /* tiled: taps evaluated beside the 2K per output, all zero (union of four phases' windows) */
  uint32_t lds_bytes;         /* tiled: dynamic LDS of one workgroup (512 threads) */
  uint64_t table_bytes;       /* the tap table in device memory */
  double   max_sum_abs_taps;  /* max over the phases of sum_j |h_p[j]|: the factor in the bound of the sum's rounding error */
} peaq_resample_plan;
int peaq_resample_plan_info (uint32_t rate, peaq_resample_plan *out);
/* peaq_run_pair for host signals sampled at `rate`: upload, convert both on the device, the one-pair path.
 * rate == 48000 is peaq_run_pair itself. */
int peaq_run_pair_rate (peaq_ctx *ctx, int advanced, int channels, double playback_level_db, uint32_t rate,
                        const float *ref, size_t n_ref, const float *test, size_t n_test, peaq_result *out);

/* ---- live rate conversion: the converter above, window by window ----------------------------------------------------
 * Output sample m of the converter depends on m and on the 2K input samples n_first (m) .. last (m) alone:
 *   n_first (m) = (m M) div L + (8 p < L ? -1 : 0) - K + 1, p = (m M) mod L;   last (m) = n_first (m) + 2K - 1
 * (L, M, K, h_p as in "sample-rate conversion" above; both are non-decreasing in m).  So a stream can be converted a
 * window at a time, from whatever raw samples are there, and gives exactly the samples peaq_batch_resample gives for
 * the whole stream.
 *
 * peaq_live_rate_ready: how many converted samples a stream of which n_have raw samples (per channel) have arrived can
 *   deliver.  Not ended: the count of outputs m with last (m) < n_have -- a prefix, since last is non-decreasing --, in
 *   closed form: with A = 8 L (n_have - K) + L, 0 if A <= 0, else (A - 1) div (8 M) + 1.  Ended: the converter's own
 *   length, peaq_resampled_length (n_have, rate), without the limit of 32 bits.  The first never passes the second
 *   (m M < L (n_have - K) + L / 8 implies m M <= L (n_have - 1)), and holds back the outputs whose taps reach within K
 *   samples of the end: 36 at 44.1 kHz, 50 at 32 kHz, 32 at 96 kHz, 144 at 11.025 kHz, 198 at 8 kHz at most, under 5 ms.
 * peaq_live_rate_inputs: the raw samples [in_first, in_end) the outputs [out_first, out_first + out_count) read,
 *   in_first = max (0, n_first (out_first)), in_end = last (out_first + out_count - 1) + 1 (the end of the stream does
 *   not clamp it: the caller knows where that is); out_count == 0: in_end = in_first.
 *   (Named _inputs, not _span: "spans" are the advanced version's scored stretches further up.)
 * Both are host arithmetic, need no device, and refuse rate 48000 and every rate peaq_resample_supported does not take
 * with PEAQ_ERR_ARG and a message that names the rate; positions past 2^62 / 48000 are PEAQ_ERR_ARG as well.
 *
 * peaq_batch_resample_range converts n_segments segments in one launch.  Segment i reads row i of d_in -- interleaved
 * F32, `in_stride` samples per channel between rows, holding the raw samples [in_base, in_base + in_have) of its stream
 * -- and writes the outputs m = out_first .. out_first + out_count - 1 to row i of d_out (`out_stride` between rows;
 * what lies behind out_count is left as it is).  Each output is acc = fma (h_p[j], (double) x[n_first + j], acc) from
 * acc = 0 with j ascending, rounded once to FP32: the chain of both kernels of peaq_batch_resample, so that for finite
 * input the samples are bit for bit those of peaq_batch_resample over the whole stream at the same indices.  Taps
 * outside [0, in_total) are absent (in_total: the stream's length once it has ended, UINT64_MAX before).  A tap inside
 * the stream that the row does not hold is PEAQ_ERR_ARG, found on the host before anything is enqueued; so are outputs
 * past the ended stream's converted length, out_count > out_stride, in_have > in_stride, an unsupported rate, rate ==
 * 48000, channels other than 1 or 2, more than 65535 segments and NULL buffers.  Positions are 64-bit throughout (a
 * 44.1 kHz stream passes 2^32 samples in 27 hours).  Enqueues on `stream` and synchronises nothing: the segments travel
 * through the pinned slots peaq_batch_resample's lengths travel through, under the same rule.  (The first call for a
 * rate on a context uploads that rate's plain tap table, synchronously.)
 * One kernel, resample_range_kernel: a workgroup of 256 threads takes 256 consecutive outputs of one segment, stages
 * their raw span (all channels) in LDS once, and each lane runs one output's chain, its tap row read from the plain
 * [L][2K] table.  No atomics, a fixed order. */
typedef struct peaq_rate_segment {
  uint64_t out_first;  /* outputs m in [out_first, out_first + out_count) ...              */
  uint64_t in_base;    /* ... from a row that holds raw samples [in_base, in_base + in_have) */
  uint64_t in_total;   /* the stream's length once it has ended, UINT64_MAX before          */
  uint32_t out_count, in_have;
} peaq_rate_segment;
size_t peaq_rate_segment_size (void);   /* the struct's size in THIS library, as peaq_meter_reading_size */
int peaq_live_rate_ready (uint32_t rate, uint64_t n_have, int ended, uint64_t *ready);
int peaq_live_rate_inputs (uint32_t rate, uint64_t out_first, uint32_t out_count, uint64_t *in_first, uint64_t *in_end);
int peaq_batch_resample_range (peaq_ctx *ctx, int channels, uint32_t rate, int n_segments,
                               const peaq_rate_segment *seg /* host */, const float *d_in, size_t in_stride,
                               float *d_out, size_t out_stride, void *stream);
/* Sessions.  peaq_session_set_rates gives each pad a rate: 48000 leaves the pad as it is, any other rate the converter
 * takes makes it a RATED pad, whose pushes are raw samples at that rate.  A rated session IS the plain session fed
 * each pad's peaq_batch_resample'd stream, whatever the pushes were: bit for bit in the basic version, and in the
 * advanced version as far as one stream cut into other launches is the same.  The host FIFO of a rated pad holds raw
 * samples; every count of the stream -- what is ready to be framed, frames, blocks, the meter's frames, {start,
 * length} and totals, and with live alignment `probe`, `max_lag`, the probe lengths and the skips that
 * peaq_session_align_read reports -- is in CONVERTED samples, through peaq_live_rate_ready of what has arrived.  Each
 * launch uploads the raw span of its window (peaq_live_rate_inputs) and one launch of the range converter writes the
 * window where the copy would have put it -- two segments, the two pads, where they share a rate --; an acquisition
 * converts the probes the same way in front of peaq_batch_estimate_delay.  Everything behind is untouched.  Windows
 * overlap by a hop, so a launch converts up to 1024 outputs that the launch before converted, and in the advanced
 * version frames and blocks each convert their own window.  peaq_session_flush ends the stream: the outputs held back
 * are delivered with the taps past the end absent, as peaq_batch_resample has them.  After it a push on a rated pad is
 * PEAQ_ERR_STATE until peaq_session_reset, which keeps the rates.  Accepted where peaq_session_set_meter is, before
 * the first push or right after peaq_session_reset; otherwise, and for an unsupported rate, PEAQ_ERR_ARG with a
 * message that names entry and rate.
 * The broker.  peaq_broker_set_rates sets ONE pair of rates for all sessions of the broker, because they size the
 * pinned staging: accepted where peaq_broker_set_meter is, for a broker made by peaq_broker_create_multi in every
 * shard; brokers of more than 65535 sessions are refused.  A tick uploads the raw samples of its windows and runs one
 * launch of the range converter per path and rated pad over the tick's segments, in front of the front end; the
 * probes of an acquisition likewise.  With both rates 48000 a tick enqueues exactly what it enqueues without the call.
 * Every slot is its rated session.  peaq_broker_flush ends the slot's stream; a later push on a rated pad is
 * PEAQ_ERR_STATE until the slot is closed and opened again. */
int peaq_session_set_rates (peaq_session *s, uint32_t rate_ref, uint32_t rate_test);
int peaq_broker_set_rates (peaq_broker *b, uint32_t rate_ref, uint32_t rate_test);

/* ---- time alignment on the device ------------------------------------------------
 * PEAQ compares frame against frame and takes the two signals as sample-aligned (BS.1387; the reference has no
 * aligner).  A codec's output is late by its own delay; these entry points find that delay and cut both signals to
 * their common, aligned part, as a stage in front of peaq_batch_run / peaq_batch_run_trajectory.  Integer lags only
 * here (the constant sub-sample part: "sub-sample delay on the device", a constant drift: "constant drift on the
 * device", a delay that bends: "delay track on the device", all further down), one lag per pair for
 * all channels; level and polarity are matched by the stage further down ("level and polarity matching on the device").
 *
 *   For one pair with n_ref / n_test samples per channel:
 *   r[n] = sum_c (double) ref[n][c], t[n] likewise: the mono sum, no 1 / channels factor.
 *   c[d] = sum_n r[n] t[n + d] over all n with 0 <= n < n_ref and 0 <= n + d < n_test, for every integer d in
 *   [-D, D], D = max_lag, 1 <= D <= 16384 (anything else: PEAQ_ERR_ARG with a message that names it).
 *   lag = the d with the largest |c[d]|; ties go to the smaller |d|, then to the positive one.  Positive lag: the
 *   test signal is late, test[n + lag] belongs to ref[n].  The absolute value lets a polarity-inverted test signal
 *   align too; the sign shows in `peak`.
 *   peak = c[lag] (signed), runner_up = the largest |c[d]| over d != lag, norm = sqrt (sum r^2 sum t^2) over the
 *   whole signals.  A pair in which either signal is empty or all zero gets lag = 0, peak = runner_up = 0 (and norm 0).
 *   Arithmetic: samples FP32 as stored, everything after the conversion in FP64.  c is evaluated in the blocked
 *   frequency-domain form (1024-point FP64 transforms over blocks of 512 samples, exact for linear correlation);
 *   every c[d] used is within 1e-9 norm of the exact sum, peak and runner_up with it.
 *   The arg-max is taken over these computed values, and values of |c| within 1e-12 norm of the largest count as
 *   tied with it (the transforms' rounding, some 1e-14 norm, gives the lags of an exact tie different last bits; the
 *   tolerance is what makes the tie rule hold for them).  So `lag` IS the exact arg-max whenever the exact largest
 *   |c| leads every other by more than 1e-12 norm; where two are closer than that, the smaller |d| wins even if the
 *   other is the larger by that little, and runner_up may then equal or pass |peak| by up to 1e-12 norm.
 *   A pair with a NaN or infinite sample (or whose sum r^2 sum t^2 is not finite) has no estimate: lag = 0,
 *   peak = runner_up = 0 and norm = NaN, which is how a caller tells it from silence (norm 0).  The record of a pair
 *   does not depend on the other pairs of the call and is the same bit for bit run to run. */
typedef struct {
  int32_t lag;
  int32_t reserved;
  double  peak;
  double  runner_up;
  double  norm;
} peaq_delay;
/* Batch layout and lengths as for peaq_batch_run (n_ref / n_test: host arrays, both or neither; NULL = n_uniform).
 * d_out: device array of n_pairs peaq_delay.  Enqueues on `stream` and returns; lengths travel as
 * peaq_batch_resample's do.  The scratch (peaq_align_workspace_bytes) lives in the context and is reused across
 * calls; a call on another stream waits, on the device, for the previous call's kernels.  channels other than 1 or
 * 2, more than 65535 pairs, NULL buffers, a pair longer than pair_stride: PEAQ_ERR_ARG. */
int peaq_batch_estimate_delay (peaq_ctx *ctx, int channels, int n_pairs,
                               const float *d_ref, const float *d_test, size_t pair_stride,
                               const uint32_t *n_ref, const uint32_t *n_test, uint32_t n_uniform,
                               uint32_t max_lag, peaq_delay *d_out /* device, [n_pairs] */, void *stream);
/* Scratch of peaq_batch_estimate_delay for a shape, in bytes (n_max: the longest signal of either side).  Pairs are
 * taken in groups, so it stops growing with n_pairs at about 1 GiB.  0 for no pairs or a max_lag out of range. */
size_t peaq_align_workspace_bytes (int channels, int n_pairs, uint32_t n_max, uint32_t max_lag);
/* out[p][i][c] = in[p][skip[p] + i][c] for i < n_keep[p]; samples of d_out past n_keep[p] are left as they were.
 * skip / n_keep: host arrays of n_pairs entries (pinned staging, copied on `stream`).  d_out must not overlap d_in.
 * A pair whose skip + n_keep passes in_stride, an out_stride below the longest n_keep, NULL buffers or arrays,
 * channels other than 1 or 2, more than 65535 pairs: PEAQ_ERR_ARG. */
int peaq_batch_cut (peaq_ctx *ctx, int channels, int n_pairs,
                    const float *d_in, size_t in_stride, const uint32_t *skip /* host */, const uint32_t *n_keep /* host */,
                    float *d_out, size_t out_stride, void *stream);
/* What to cut for a lag (host arithmetic): lag >= 0: the reference keeps its start, the test signal drops its first
 * `lag` samples; lag < 0: the reference drops -lag, the test signal keeps its start (a skip stops at its signal's
 * length).  Both are then cut to n_common = min (n_ref - skip_ref, n_test - skip_test). */
void peaq_aligned_lengths (int32_t lag, uint32_t n_ref, uint32_t n_test,
                           uint32_t *skip_ref, uint32_t *skip_test, uint32_t *n_common);
/* One pair from HOST memory: upload, conversion of both to 48 kHz on the device if rate != 48000, estimate, cut, then
 * the one-pair path of peaq_run_pair.  The lag counts 48 kHz samples (after the conversion).  delay (host, may be
 * NULL) receives the record. */
int peaq_run_pair_aligned (peaq_ctx *ctx, int advanced, int channels, double playback_level_db, uint32_t rate,
                           uint32_t max_lag, const float *ref, size_t n_ref, const float *test, size_t n_test,
                           peaq_delay *delay /* host */, peaq_result *out);
/* peaq_batch_run_trace (above) for one pair from HOST memory, records into host arrays: upload, conversion of both
 * signals to 48 kHz on the device if rate != 48000, alignment as in peaq_run_pair_aligned if max_lag != 0 (0: none; delay, may be NULL, receives the
 * record, zeroed without alignment), then peaq_batch_run_trace with one pair.  n_frames / n_blocks (may be NULL)
 * receive the counts written -- those of the signals as scored, after conversion and cut; frame_cap / block_cap are
 * the arrays' sizes in records, and a cap below the count is PEAQ_ERR_ARG with both numbers in the message
 * (peaq_frame_count of the two 48 kHz lengths is always enough: the cut only shortens).  blocks: required in the
 * advanced version, NULL in the basic one.  out (may be NULL): the pair's result. */
int peaq_run_pair_trace (peaq_ctx *ctx, int advanced, int channels, double playback_level_db,
                         uint32_t rate, uint32_t max_lag,
                         const float *ref, size_t n_ref, const float *test, size_t n_test,
                         peaq_frame_trace *frames /* host */, size_t frame_cap, uint32_t *n_frames,
                         peaq_block_trace *blocks /* host */, size_t block_cap, uint32_t *n_blocks,
                         peaq_delay *delay /* host */, peaq_result *out);
/* peaq_batch_run_bands (above) for one pair from HOST memory, rows into a host array [frame_cap][channels][n_planes][row]:
 * upload, conversion, alignment and counts as in peaq_run_pair_trace.  n_frames (may be NULL) receives the count of
 * frames written; a frame_cap below it is PEAQ_ERR_ARG with both numbers in the message.  out (may be NULL): the
 * pair's result. */
int peaq_run_pair_bands (peaq_ctx *ctx, int advanced, int channels, double playback_level_db,
                         uint32_t rate, uint32_t max_lag,
                         const float *ref, size_t n_ref, const float *test, size_t n_test, uint32_t planes,
                         double *bands /* host */, size_t frame_cap, uint32_t *n_frames,
                         peaq_delay *delay /* host */, peaq_result *out);
/* peaq_batch_run_fb_bands (above) for one pair from HOST memory, rows into a host array
 * [block_cap][channels][n_planes][40]: upload, conversion and alignment as in peaq_run_pair_bands.  n_blocks (may be
 * NULL) receives the count of blocks written; a block_cap below it is PEAQ_ERR_ARG with both numbers in the message.
 * out (may be NULL): the pair's result. */
int peaq_run_pair_fb_bands (peaq_ctx *ctx, int channels, double playback_level_db,
                            uint32_t rate, uint32_t max_lag,
                            const float *ref, size_t n_ref, const float *test, size_t n_test, uint32_t planes,
                            double *bands /* host */, size_t block_cap, uint32_t *n_blocks,
                            peaq_delay *delay /* host */, peaq_result *out);
/* peaq_batch_run_pattern_bands (above) for one pair from HOST memory, rows into a host array
 * [frame_cap][channels][n_planes][110]: upload, conversion, alignment and counts as in peaq_run_pair_bands.  n_frames
 * (may be NULL) receives the count of frames written; a frame_cap below it is PEAQ_ERR_ARG with both numbers in the
 * message.  out (may be NULL): the pair's result. */
int peaq_run_pair_pattern_bands (peaq_ctx *ctx, int channels, double playback_level_db,
                                 uint32_t rate, uint32_t max_lag,
                                 const float *ref, size_t n_ref, const float *test, size_t n_test, uint32_t planes,
                                 double *bands /* host */, size_t frame_cap, uint32_t *n_frames,
                                 peaq_delay *delay /* host */, peaq_result *out);
/* peaq_batch_run_band_summary (above) for one pair from HOST memory, rows into a host array
 * [channels][peaq_band_summary_rows (advanced)][peaq_band_row (advanced)]: upload, conversion and alignment as in
 * peaq_run_pair_pattern_bands; the rows are those of the signals as scored, after conversion and cut.  out (may be
 * NULL): the pair's result. */
int peaq_run_pair_band_summary (peaq_ctx *ctx, int advanced, int channels, double playback_level_db,
                                uint32_t rate, uint32_t max_lag,
                                const float *ref, size_t n_ref, const float *test, size_t n_test,
                                double *summary /* host */, peaq_delay *delay /* host */, peaq_result *out);
/* peaq_batch_run_fb_band_summary (above) for one pair from HOST memory, rows into a host array [channels][7][42]:
 * upload, conversion and alignment as in peaq_run_pair_band_summary.  out (may be NULL): the pair's result. */
int peaq_run_pair_fb_band_summary (peaq_ctx *ctx, int channels, double playback_level_db,
                                   uint32_t rate, uint32_t max_lag,
                                   const float *ref, size_t n_ref, const float *test, size_t n_test,
                                   double *summary /* host */, peaq_delay *delay /* host */, peaq_result *out);
/* peaq_batch_run_windows (above) for one pair from HOST memory, the n_windows records into a host array: upload,
 * conversion and alignment as in peaq_run_pair_trace; the windows count 48 kHz samples of the signals as scored, after
 * conversion and cut.  out (may be NULL): the pair's result. */
int peaq_run_pair_windows (peaq_ctx *ctx, int channels, double playback_level_db,
                           uint32_t rate, uint32_t max_lag,
                           const float *ref, size_t n_ref, const float *test, size_t n_test,
                           const peaq_window *windows, int n_windows, peaq_result *out_windows /* host */,
                           peaq_delay *delay /* host */, peaq_result *out);
/* peaq_batch_run_adv_spans (above) for one pair from HOST memory, the n_spans records into a host array: upload,
 * conversion and alignment as in peaq_run_pair_windows; the spans count 48 kHz samples of the signals as scored, after
 * conversion and cut.  out (may be NULL): the pair's result. */
int peaq_run_pair_adv_spans (peaq_ctx *ctx, int channels, double playback_level_db,
                             uint32_t rate, uint32_t max_lag,
                             const float *ref, size_t n_ref, const float *test, size_t n_test,
                             const peaq_window *spans, int n_spans, peaq_result *out_spans /* host */,
                             peaq_delay *delay /* host */, peaq_result *out);

/* ---- PCM from host memory: device decoder and host-fed batch ------------------------
 * Corpora are 16- or 24-bit PCM files in host memory; the batch entry points above take interleaved F32 in device
 * memory.  peaq_batch_decode_pcm converts a batch in the file's own sample format on the device, and
 * peaq_batch_run_host scores a list of pairs that sit in host memory in that format: upload, decode, rate conversion,
 * alignment and scoring, chunk by chunk, the next chunk's upload beside the running chunk's kernels.
 *
 * The decoded sample is bit for bit what gstpeaq_amd/cli/peaq.c (wav_read) and gstpeaq_amd/wavio.py (read_wav)
 * produce: the value in double, divided, rounded ONCE to FP32.  U8, S16 and S24 are exact; S32 and F64 round to
 * nearest even; an F64 beyond the FP32 range becomes +-Inf as the C cast does; F32 copies the bits (NaN payloads too). */
#define PEAQ_PCM_U8  0   /* unsigned 8 bit            (x - 128) / 128        */
#define PEAQ_PCM_S16 1   /* little endian             x / 32768              */
#define PEAQ_PCM_S24 2   /* packed, 3 bytes, LE       x / 8388608            */
#define PEAQ_PCM_S32 3   /*                           x / 2147483648         */
#define PEAQ_PCM_F32 4   /* IEEE float, bits copied as they are              */
#define PEAQ_PCM_F64 5   /* IEEE double, one rounding to FP32 (nearest even) */
size_t peaq_pcm_sample_bytes (int format);          /* 1 2 3 4 4 8; 0 for an unknown format */
/* d_in: the batch layout in the file's own sample format, interleaved [pair][sample][channel]; pair p starts at BYTE
 * p * in_stride * channels * sample_bytes, so with S24 (and U8, S16) pair bases fall on any byte phase.  d_in itself
 * must be at least 4-byte aligned.  Lengths as for peaq_batch_resample: n_in (host array of n_pairs entries, through
 * pinned staging slots; NULL = n_uniform each).  d_out: interleaved F32 with out_stride samples per channel between
 * pairs; samples of d_out past a pair's length are left untouched.  Enqueues on `stream` and synchronises nothing.
 * PEAQ_ERR_ARG, before any device is touched and with the offending value in the message: an unknown format,
 * channels other than 1 or 2, more than 65535 pairs, NULL buffers, a d_in that is not 4-byte aligned, a pair longer
 * than in_stride, an out_stride below the longest pair. */
int peaq_batch_decode_pcm (peaq_ctx *ctx, int format, int channels, int n_pairs,
                           const void *d_in, size_t in_stride, const uint32_t *n_in, uint32_t n_uniform,
                           float *d_out, size_t out_stride, void *stream);

typedef struct { const void *ref, *test; uint64_t n_ref, n_test; } peaq_host_pair;   /* samples per channel */
typedef struct peaq_feed {
  uint32_t struct_size;     /* sizeof (peaq_feed) of the CALLER; anything else than this library's: PEAQ_ERR_ARG */
  int      format, channels;
  uint32_t rate;            /* 48000, or a rate peaq_resample_supported takes */
  uint32_t align_max_lag;   /* 0: no alignment; else 1..16384 as peaq_batch_estimate_delay */
  uint32_t chunk_pairs;     /* 0: the library chooses; else pairs per chunk (1..65535) */
} peaq_feed;
size_t peaq_feed_size (void);
/* results[p] is bit for bit what this sequence writes for pair p, whatever the chunking and whatever the other pairs
 * of the call are: (1) peaq_batch_decode_pcm of both buffers; (2) if rate != 48000, peaq_batch_resample of both;
 * (3) if align_max_lag, peaq_batch_estimate_delay, peaq_aligned_lengths and peaq_batch_cut of both -- delays[p]
 * (host, may be NULL) is that record, its lag in 48 kHz samples; without alignment delays[] is zeroed; (4)
 * peaq_batch_run with the context's settings and FIR mode.  Source buffers may be pageable and unaligned.  Synchronous:
 * returns when `results` (host, n_pairs records) is complete.  On a device error it stops, starts nothing more, waits
 * for what runs and returns the error.
 * Pipeline: pairs are taken in chunks; a chunk's raw bytes are packed into one of two pinned staging sets at the
 * chunk's own stride (its longest signal) and copied on a copy stream, decode through score run on a compute stream,
 * events order the two, results come back per chunk.  Chunk size: as many pairs as fit PEAQ_FEED_BUDGET_BYTES (4 GiB)
 * of staging plus device buffers -- per pair four raw signals in pinned memory (two sets), four in device memory, two
 * decoded F32 signals, two converted ones if rate != 48000 and two cut ones if aligned; the batch and aligner
 * workspaces are their own (peaq_feed_workspace_bytes counts them) --, never more than 65535, and a pair that alone
 * exceeds the budget runs as a chunk of one.  All buffers live in the context, are reused across calls and freed with
 * it.  The copy into the staging set is shared by PEAQ_FEED_DEFAULT_THREADS (8) host threads, started per chunk;
 * the environment variable PEAQ_AMD_FEED_THREADS = 1 .. 16 sets another count (anything else: PEAQ_ERR_ARG that names
 * it); the count never follows the machine's CPU count.
 * PEAQ_ERR_ARG before any device is touched: a wrong struct_size, an unknown format, channels other than 1 or 2, a
 * rate the device converter does not take, align_max_lag above 16384, chunk_pairs above 65535, a playback level
 * outside 0..130, NULL arguments, a pair with samples but no buffer, a pair of more than 2^32 - 1 samples (before or
 * after the conversion). */
#define PEAQ_FEED_BUDGET_BYTES   ((size_t) 4 << 30)
#define PEAQ_FEED_DEFAULT_THREADS 8
int peaq_batch_run_host (peaq_ctx *ctx, int advanced, double playback_level_db, const peaq_feed *feed,
                         size_t n_pairs, const peaq_host_pair *pairs,
                         peaq_result *results /* host, [n_pairs] */, peaq_delay *delays /* host, may be NULL */);
/* Staging, device buffers and the batch (and aligner) workspace of a call of n_pairs pairs of at most n_max samples
 * per channel (at the feed's rate), in bytes; 0 for a feed peaq_batch_run_host would refuse. */
size_t peaq_feed_workspace_bytes (const peaq_feed *feed, int advanced, size_t n_pairs, uint64_t n_max);

/* ---- one reference, many tests: gather and the host-fed batch with shared references ------------------------
 * Codec and listening-test corpora are one reference against K coded versions.  peaq_batch_run_host_refs takes the
 * references and the tests as two lists, each test naming its reference, and uploads, decodes and rate-converts a
 * reference once per chunk instead of once per test; peaq_batch_gather is the device copy that then puts it in front of
 * every test that names it.
 *
 * out[p][i][c] = in[src[p]][skip[p] + i][c]  for i < n_keep[p], p < n_out; samples of d_out past n_keep[p] untouched.
 * d_in holds n_rows signals, in_stride samples per channel apart; src / skip / n_keep: host arrays of n_out entries
 * (pinned staging slots, copied on `stream`, as peaq_batch_cut's).  A row may be named by any number of outputs, or none.
 * It is peaq_batch_cut with a source index: with src[p] = p and n_rows = n_out it writes bit for bit what
 * peaq_batch_cut writes.  Bits are moved as they are, NaN payloads included.  Enqueues on `stream` and synchronises
 * nothing.  PEAQ_ERR_ARG, before any device is touched and with the offending value in the message: a src[p] that is
 * not below n_rows, a skip[p] + n_keep[p] that passes in_stride, an out_stride below the longest n_keep, NULL buffers or
 * arrays, channels other than 1 or 2, n_out or n_rows above 65535, a d_out that overlaps d_in. */
int peaq_batch_gather (peaq_ctx *ctx, int channels, int n_rows, int n_out,
                       const float *d_in, size_t in_stride,
                       const uint32_t *src /* host */, const uint32_t *skip /* host */, const uint32_t *n_keep /* host */,
                       float *d_out, size_t out_stride, void *stream);

typedef struct { const void *data; uint64_t n; } peaq_host_signal;                    /* samples per channel */
typedef struct { const void *data; uint64_t n; uint32_t ref, reserved; } peaq_host_test;   /* ref: index into refs[] */
/* results[t] and delays[t] are bit for bit what peaq_batch_run_host writes for the pair { refs[tests[t].ref], tests[t] }
 * with the same feed, whatever the chunking, the order of the tests, and the other tests and references of the call.
 * Pipeline: as peaq_batch_run_host's (two streams, two staging sets, the same packing threads and error handling; one
 * call of either kind per context at a time).  Tests are taken in the caller's order, in chunks; feed->chunk_pairs
 * counts tests.  A chunk's staging set holds its tests and each distinct reference the chunk names, once; on the
 * device: decode the tests, decode the references once each; if rate != 48000 convert the tests, convert the
 * references once each; peaq_batch_gather the references into the pair layout; if aligned estimate the delays and cut
 * (the reference's cut is a gather with each test's skip); peaq_batch_run.
 * A reference named by tests of two chunks is uploaded in both: the saving is there when the tests of a reference
 * stand next to each other in tests[], so sort by reference where the order is free.  A reference nobody names is
 * never touched, and its data may be NULL.
 * Chunk size: PEAQ_FEED_BUDGET_BYTES as for peaq_batch_run_host, with a reference counted once per chunk -- its raw
 * bytes in two pinned sets and two device buffers, its decoded signal, its converted one if rate != 48000 -- and a test
 * as a pair there less the reference's four raw signals (the reference's copy in the pair layout stays per test).
 * PEAQ_ERR_ARG before any device is touched: what peaq_batch_run_host refuses, a tests[t].ref that is not below n_refs
 * (the message names t and the index), a named reference with samples but no buffer. */
int peaq_batch_run_host_refs (peaq_ctx *ctx, int advanced, double playback_level_db, const peaq_feed *feed,
                              size_t n_refs, const peaq_host_signal *refs,
                              size_t n_tests, const peaq_host_test *tests,
                              peaq_result *results /* host, [n_tests] */, peaq_delay *delays /* host, may be NULL */);
/* peaq_feed_workspace_bytes for a call of n_tests tests that name n_refs references, none longer than n_max samples
 * per channel, a chunk taken to name as many distinct references as it can; 0 for a feed it would refuse, no tests or
 * no references. */
size_t peaq_feed_refs_workspace_bytes (const peaq_feed *feed, int advanced, size_t n_refs, size_t n_tests, uint64_t n_max);

/* ---- level and polarity matching on the device ------------------------------------------------
 * PEAQ compares loudness patterns, so a test signal that is a few dB quieter than its reference, or inverted, is
 * scored as degraded.  This stage sits between delay estimation and the cut: peaq_batch_measure_gain measures each
 * pair's gain over the aligned part of the UNCUT buffers, and peaq_batch_cut_scaled applies it to the test signal
 * inside the copy the cut makes anyway.  The record stays on the device between the two.  Not done, here or anywhere:
 * DC offset removal, time-varying or per-band gain (fractional delay: the stage after this one); the reference signal
 * is never changed.
 *
 *   For pair p and channel c, with the host arrays skip_ref[p], skip_test[p], n[p]:
 *   r_i = (double) ref[p][skip_ref[p] + i][c], t_i = (double) test[p][skip_test[p] + i][c], i < n[p];
 *   Srr = sum r_i^2, Stt = sum t_i^2, Srt = sum r_i t_i, in FP64 (the products are exact: 24 x 24 bits).
 *   Order: a workgroup covers PEAQ_GAIN_CHUNK samples per channel and writes one partial per sum; there a lane adds at
 *   most 16 terms one after the other, then a fixed tree over the 256 lanes (8 levels); a second kernel adds the
 *   pair's partials, a lane every 256th in chunk order (at most 4096 for 2^32 - 1 samples), then the same tree.  No
 *   floating-point atomics, and the order depends on the index within the pair alone, never on an address.  A term
 *   passes at most 15 + 8 + 4095 + 8 additions, so |S - exact| <= 4126 * 2^-53 * sum |term| < 1e-12 sum |term| for
 *   every length up to 2^32 - 1.  The record of a pair does not depend on the other pairs of the call or on where its
 *   buffers lie, and is the same bit for bit run to run.
 *   The gain g is derived in FP64 by the IEEE quotient and square root on the record's own sums (mode below); without
 *   PEAQ_GAIN_PER_CHANNEL the sums of channel 0 and 1 are added first (0 first) and both channels get that g.
 *   A channel that cannot be matched is flagged and keeps gain = 1.0: the pair is scored unmatched and the flags say
 *   why.  Checked in this order, the first that holds: NONFINITE, SILENT, ZERO, RANGE.  RANGE is evaluated as |g|
 *   outside [10^(-max_gain_db / 20), 10^(max_gain_db / 20)], the two bounds computed once per call in FP64 (pow);
 *   a g of 0 or Inf is out of range.  PEAQ_GAIN_OFF measures the sums and the first two flags and leaves g = 1.0. */
#define PEAQ_GAIN_CHUNK     4096   /* samples per channel per workgroup of the measure kernel */
#define PEAQ_GAIN_OFF       0
#define PEAQ_GAIN_LSQ       1   /* g = Srt / Stt: minimises sum (r - g t)^2; negative for an inverted test signal */
#define PEAQ_GAIN_RMS       2   /* g = +-sqrt (Srr / Stt), the sign of Srt (+ for Srt == 0): equal energy */
#define PEAQ_GAIN_POLARITY  3   /* g = +-1, the sign of Srt: nothing but the inversion is undone */
#define PEAQ_GAIN_PER_CHANNEL 0x10   /* or-ed in: each channel its own g; otherwise the sums of channel 0 and 1
                                        are added (0 first) and both channels get one g */
#define PEAQ_GAIN_F_SILENT     1   /* Stt == 0 (or n == 0) */
#define PEAQ_GAIN_F_NONFINITE  2   /* a sum is NaN or Inf */
#define PEAQ_GAIN_F_ZERO       4   /* LSQ with Srt == 0: g would be 0 */
#define PEAQ_GAIN_F_RANGE      8   /* |20 log10 |g|| > max_gain_db */
typedef struct {                   /* 80 bytes */
  double   gain[2];                /* the factor APPLIED; 1.0 for a flagged channel; [1] = [0] for mono */
  double   srr[2], stt[2], srt[2]; /* per channel as measured; [1] = 0 for mono */
  uint32_t flags[2];               /* per channel; both alike without PER_CHANNEL */
  uint32_t n, reserved;
} peaq_gain;
size_t peaq_gain_size (void);
/* d_ref / d_test: interleaved F32 in the batch layout, each with its own stride (samples per channel between pairs).
 * skip_ref / skip_test / n: host arrays of n_pairs entries (pinned staging slots, copied on `stream`, as
 * peaq_batch_cut's).  d_out: device array of n_pairs peaq_gain.  Enqueues on `stream` and returns.  The partials
 * (peaq_gain_workspace_bytes) live in the context and are reused; a call on another stream waits, on the device, for
 * the previous call's kernels.  max_gain_db: 0 < x <= 120 (checked for every mode).
 * PEAQ_ERR_ARG, before any device is touched and with the offending value in the message: an unknown mode or flag
 * bit, max_gain_db out of range or NaN, channels other than 1 or 2, more than 65535 pairs, NULL buffers or arrays, a
 * pair whose skip + n passes its stride. */
int peaq_batch_measure_gain (peaq_ctx *ctx, int channels, int n_pairs,
                             const float *d_ref, size_t ref_stride, const uint32_t *skip_ref /* host */,
                             const float *d_test, size_t test_stride, const uint32_t *skip_test /* host */,
                             const uint32_t *n /* host */, int mode, double max_gain_db,
                             peaq_gain *d_out /* device, [n_pairs] */, void *stream);
/* Partials of peaq_batch_measure_gain for a shape, in bytes: 48 per chunk and pair.  Pairs are taken in groups, so
 * it stops growing with n_pairs at 256 MiB (or one pair's partials, if those are more).  0 for no pairs. */
size_t peaq_gain_workspace_bytes (int channels, int n_pairs, uint32_t n_max);
/* peaq_batch_cut with a factor per pair and channel, read from the device records:
 * out[p][i][c] = (float) ((double) in[p][skip[p] + i][c] * d_gain[p].gain[c]), rounded once (mono: gain[0]).  Where
 * the factor is exactly 1.0 the bits are moved as they are, NaN payloads included: a pair left unmatched is bit for
 * bit peaq_batch_cut's output.  Samples of d_out past n_keep[p] are left as they were.  Refusals as peaq_batch_cut's,
 * and a NULL d_gain. */
int peaq_batch_cut_scaled (peaq_ctx *ctx, int channels, int n_pairs,
                           const float *d_in, size_t in_stride, const uint32_t *skip /* host */, const uint32_t *n_keep /* host */,
                           const peaq_gain *d_gain /* device, [n_pairs] */, float *d_out, size_t out_stride, void *stream);
/* peaq_run_pair_aligned with the stage in it: upload, conversion to 48 kHz if rate != 48000, estimate if max_lag != 0
 * (0: no alignment, skips 0 and n = min (n_ref, n_test); delay is zeroed), peaq_batch_measure_gain over the common
 * part, cut of the reference, peaq_batch_cut_scaled of the test signal, the one-pair path.  gain (host, may be NULL)
 * receives the record.  mode PEAQ_GAIN_OFF scores what peaq_run_pair_aligned scores. */
int peaq_run_pair_matched (peaq_ctx *ctx, int advanced, int channels, double playback_level_db, uint32_t rate,
                           uint32_t max_lag, int mode, double max_gain_db,
                           const float *ref, size_t n_ref, const float *test, size_t n_test,
                           peaq_delay *delay /* host */, peaq_gain *gain /* host */, peaq_result *out);
/* peaq_batch_run_host_refs with the stage in it (plain pairs: one test per reference).  peaq_feed keeps its size, so
 * the two values are arguments.  results[t] is bit for bit what this sequence writes, whatever the chunking and order:
 * decode; convert if rate != 48000; gather; if align_max_lag, estimate and peaq_aligned_lengths (otherwise skips 0 and
 * n = min (n_ref, n_test)); peaq_batch_measure_gain over the common part; the reference's cut (a gather with each
 * test's skip); peaq_batch_cut_scaled of the test; peaq_batch_run.  gains (host, may be NULL): the records.  With
 * mode PEAQ_GAIN_OFF it is peaq_batch_run_host_refs itself (gains zeroed).  Refuses what that refuses, an unknown
 * mode and a max_gain_db out of range. */
int peaq_batch_run_host_matched (peaq_ctx *ctx, int advanced, double playback_level_db, const peaq_feed *feed,
                                 int mode, double max_gain_db,
                                 size_t n_refs, const peaq_host_signal *refs, size_t n_tests, const peaq_host_test *tests,
                                 peaq_result *results /* host, [n_tests] */, peaq_delay *delays /* host, may be NULL */,
                                 peaq_gain *gains /* host, may be NULL */);
/* peaq_feed_refs_workspace_bytes for peaq_batch_run_host_matched: with a mode other than PEAQ_GAIN_OFF the cut buffers
 * (also without alignment), the records and the partials are counted. */
size_t peaq_feed_matched_workspace_bytes (const peaq_feed *feed, int advanced, int mode, size_t n_refs, size_t n_tests,
                                          uint64_t n_max);

/* ---- sub-sample delay on the device ------------------------------------------------
 * A codec, a resampler or a DA/AD loop rarely delays by a whole number of 48 kHz samples, and the residue the integer
 * aligner leaves -- up to half a sample -- is scored as coding noise.  This stage sits behind peaq_batch_estimate_delay:
 * peaq_batch_refine_delay finds the constant sub-sample part of each pair's delay on a grid of 1 / PEAQ_SUB_STEPS
 * samples around the given integer lag, and peaq_batch_cut_shifted is peaq_batch_cut of the test signal through the
 * fractional-delay filter of that grid point.  Only the test signal is ever shifted; the reference is never changed.
 * With lag < 0 the test signal keeps skip = 0 and is still shifted by q.  A delay that grows steadily is the next
 * stage's ("constant drift on the device"), one that bends the one after ("delay track on the device").  Steps of the
 * delay sharper than a window of the track are the stage's after that ("delay steps on the device").  Not done, here
 * or anywhere: shifts finer than the grid, and the host-fed pipelines (peaq_batch_run_host*, the CLI's --list), which align to whole samples only.
 *
 *   w_H (x) = I0 (beta sqrt (1 - (x / H)^2)) / I0 (beta) for |x| < H, else 0; beta = 8.49, the converter's Kaiser window.
 *   sinc (x) = sin (pi x) / (pi x), sinc (0) = 1.  I0 is evaluated in double by the Chebyshev expansions of the Cephes
 *   library (what numpy.i0 evaluates): a table rebuilt from these formulas with numpy agrees to 1e-15 absolute.
 *   Two tables, built on the host in double once per process and uploaded once per context (peaq_subsample_tables
 *   hands out exactly what is uploaded), q in [-128, 127], k in [-16, 16], o in [-32, 32]:
 *     corr_tab[q + 128][k + 16]  = sinc (q / 256 - k) w_17 (q / 256 - k)
 *     shift_tab[q + 128][o + 32] = sinc (o - q / 256) w_33 (o - q / 256); row q = 0 is the exact unit impulse by
 *     construction, not by evaluating sin (pi o).
 *
 *   Estimate, per pair, with the integer lag of peaq_batch_estimate_delay (a host array):
 *   c_k = sum_n r[n] t[n + lag + k], r and t the FP64 mono sums as there, over all n with both indices inside their
 *   signals, for k in [-16, 16]: direct time-domain sums in a fixed order, built the way the gain stage builds its
 *   sums.  A workgroup covers 4096 n; there a lane adds at most 16 terms of one k one after the other (each term one
 *   fused multiply-add), then a fixed tree over the 256 lanes; a second kernel adds the pair's partials, a lane every
 *   256th in chunk order, then the same tree.  No floating-point atomics; the order depends on the index within the
 *   pair alone.  |c_k - exact| < 1e-12 sum |term| for every length up to 2^32 - 1 (the gain stage's count of additions).
 *   s = the sign of c_0 (+ for 0); v (q) = s sum_k c_k corr_tab[q][k], summed in the order k = -16 .. 16 in FP64, every
 *   product and every sum rounded on its own; q = the grid point with the largest v, values within 1e-12 max_k |c_k| of
 *   the largest counting as tied, ties to the smaller |q|, then to the positive one.  The total delay is lag + q / 256;
 *   positive still means that the test signal is late.
 *   The record of a pair does not depend on the other pairs of the call or on where its buffers lie, and is the same
 *   bit for bit run to run. */
#define PEAQ_SUB_STEPS   256   /* grid steps per sample */
#define PEAQ_SUB_LAGS    16    /* R: integer lags on each side of the given one */
#define PEAQ_SUB_HALF    32    /* K: the shift filter has 2 K + 1 = 65 taps */
#define PEAQ_SUB_F_NONE  1     /* no estimate: every c_k is 0, the overlap is empty (|lag| reaches a signal's length), or a
                                  sum is not finite; q = 0 and peak = 0 */
#define PEAQ_SUB_F_EDGE  2     /* q is -128 or 127: the maximum is not inside the interval, the integer lag is
                                  probably off by one */
typedef struct {               /* 40 bytes */
  int32_t  lag;                /* as given */
  int32_t  q;                  /* grid point, -128 .. 127 */
  double   frac;               /* q / 256 */
  double   peak;               /* v (q) s: the interpolated correlation at lag + frac, signed */
  double   c0;                 /* c_0 */
  uint32_t flags;
  uint32_t reserved;
} peaq_subdelay;
size_t peaq_subdelay_size (void);
/* corr: [256][33] doubles, shift: [256][65] doubles, the two tables exactly as uploaded; either may be NULL (both:
 * PEAQ_ERR_ARG).  Host only, no device. */
int peaq_subsample_tables (double *corr, double *shift);
/* Batch layout and lengths as for peaq_batch_estimate_delay (n_ref / n_test: host arrays, both or neither; NULL =
 * n_uniform); lag: host array of n_pairs entries.  All per-pair arrays travel through pinned staging slots, copied on
 * `stream`, as peaq_batch_cut's.  d_out: device array of n_pairs peaq_subdelay.  Enqueues on `stream` and returns,
 * synchronising nothing (a context's FIRST call of this stage copies the two tables to its device, blocking, once).
 * The partials (peaq_subdelay_workspace_bytes) live in the context and are reused; a call on another stream waits, on
 * the device, for the previous call's kernels.  A lag whose magnitude reaches either signal's length is no error: the
 * pair gets PEAQ_SUB_F_NONE.
 * PEAQ_ERR_ARG, before any device is touched and with the offending value in the message: channels other than 1 or
 * 2, more than 65535 pairs, NULL buffers, a NULL lag, n_ref without n_test, a pair longer than pair_stride. */
int peaq_batch_refine_delay (peaq_ctx *ctx, int channels, int n_pairs,
                             const float *d_ref, const float *d_test, size_t pair_stride,
                             const uint32_t *n_ref, const uint32_t *n_test, uint32_t n_uniform,
                             const int32_t *lag /* host */, peaq_subdelay *d_out /* device, [n_pairs] */, void *stream);
/* Partials and sums of peaq_batch_refine_delay for a shape, in bytes: 264 per chunk of 4096 reference samples and
 * pair, and 264 more per pair.  Pairs are taken in groups, so it stops growing with n_pairs at 256 MiB (or one pair's
 * row, if that is more).  0 for no pairs. */
size_t peaq_subdelay_workspace_bytes (int channels, int n_pairs, uint32_t n_max);
/* peaq_batch_cut through the shift filter of each pair's grid point q[p] (host array):
 * out[p][i][c] = (float) sum_{o = -32 .. 32} shift_tab[q[p]][o] (double) in[p][skip[p] + i + o][c] for i < n_keep[p]:
 * fused multiply-adds in the order o = -32 .. 32 in FP64, rounded once to FP32.  A tap whose index falls outside
 * [0, n_in[p]) contributes nothing.  Samples of d_out past n_keep[p] are left as they were.  A pair with q[p] == 0 has
 * its bits moved as they are, NaN payloads included: that output is bit for bit peaq_batch_cut's.
 * Refusals as peaq_batch_cut's (with the offending value in the message), and: a q outside [-128, 127], an n_in beyond
 * in_stride, a NULL n_in or q. */
int peaq_batch_cut_shifted (peaq_ctx *ctx, int channels, int n_pairs,
                            const float *d_in, size_t in_stride, const uint32_t *n_in /* host */,
                            const uint32_t *skip /* host */, const uint32_t *n_keep /* host */, const int32_t *q /* host */,
                            float *d_out, size_t out_stride, void *stream);
/* peaq_run_pair_matched with the stage in it, in this order: upload; conversion to 48 kHz if rate != 48000; estimate
 * (max_lag at least 1 is required); refine; plain cut of the reference; shifted cut of the test signal; if mode is not
 * PEAQ_GAIN_OFF, peaq_batch_measure_gain on the two CUT buffers with skips of 0 and peaq_batch_cut_scaled into a second
 * buffer; the one-pair path.  Measuring the gain after the shift is the point of the order: a residue of tau samples
 * lowers Srt by sinc (tau), which biases the LSQ gain.  delay, subdelay and gain (host) may be NULL. */
int peaq_run_pair_subsample (peaq_ctx *ctx, int advanced, int channels, double playback_level_db, uint32_t rate,
                             uint32_t max_lag, int mode, double max_gain_db,
                             const float *ref, size_t n_ref, const float *test, size_t n_test,
                             peaq_delay *delay /* host */, peaq_subdelay *subdelay /* host */, peaq_gain *gain /* host */,
                             peaq_result *out);

/* ---- wide delay search on the device ------------------------------------------------
 * peaq_batch_estimate_delay searches max_lag <= 16384 samples, 341 ms.  Recordings through a loopback that start
 * seconds apart, files with a leader of silence, material that passed a broadcast chain lie beyond that, and every
 * later stage starts from the integer lag.  This stage finds such an offset coarse to fine: both signals are decimated
 * by a power of two M so that the offset fits the aligner's range on the decimated copies, the aligner runs there, both
 * signals are cut by the coarse lag, and the aligner runs again on the cut pair with its usual range.
 *
 *   M = peaq_wide_factor (max_offset): the smallest power of two in 2 .. 64 with ceil (max_offset / M) <= 16384;
 *   max_offset in 1 .. 1048576 (2^20 samples, 21.8 s), anything else has no factor (0).
 *   h[j] = (0.75 / M) sinc (0.75 j / M) I0 (5.65 sqrt (1 - (j / 8M)^2)) / I0 (5.65) for j = -8M .. 8M,
 *   sinc (x) = sin (pi x) / (pi x), sinc (0) = 1: 16 M + 1 taps, a Kaiser window of about 60 dB, passband to about
 *   0.26 / M, stopband from about 0.49 / M cycles per sample.  Built in FP64 on the host: 0.75 j / M is exact, the
 *   sine's argument is reduced to [-1/2, 1/2] half turns exactly, I0 (x) = sum_k ((x / 2)^2k / k!^2) is summed in
 *   ascending k until a term no longer changes the sum; h[-j] is h[j]'s bits.  Every tap is within 1e-15 h[0] of the
 *   formula.  peaq_wide_taps hands out exactly what is uploaded.
 *
 *   peaq_batch_decimate, per pair with n samples per channel:
 *   s[i] = sum_c (double) in[i][c]: the aligner's mono sum, no 1 / channels factor.
 *   u = s (PEAQ_WIDE_WAVEFORM) or u = |s| (PEAQ_WIDE_ENVELOPE).
 *   y[k] = sum_{j = -8M .. 8M} h[j] u[k M + j] for k < n_dec = ceil (n / M): fused multiply-adds in the order
 *   j = -8M .. 8M in FP64, starting from 0.  A tap whose index falls outside [0, n) contributes nothing.  The filter is
 *   zero-phase: both signals of a pair are treated alike and the lag has no bias.
 *   Waveform: out[k] = (float) y[k].  Envelope: out[k] = (float) (y[k] - m), m = (sum_k y[k]) / n_dec in FP64: the
 *   correlation of two non-negative envelopes is otherwise a pedestal whose maximum is at the largest overlap.  The
 *   sum of m: a lane of 256 adds every 256th y one after the other, k ascending, then a fixed tree over the 256 lanes
 *   (the wave, then (0 + 1) + (2 + 3) over the four waves); no floating-point atomics.
 *   Entries of d_out past n_dec are left as they were.  A pair's output does not depend on the other pairs of the call
 *   and is the same bit for bit run to run.  A workgroup computes PEAQ_WIDE_CHUNK consecutive outputs of one pair.
 *   Envelope mode waits for m: y is kept in FP64 in the context's scratch (pairs in groups below 256 MiB, or one
 *   pair's row) and a second kernel subtracts. */
#define PEAQ_WIDE_WAVEFORM   0
#define PEAQ_WIDE_ENVELOPE   1
#define PEAQ_WIDE_CHUNK      248       /* outputs per workgroup of the decimator */
#define PEAQ_WIDE_MAX_OFFSET 1048576   /* 2^20 samples */
#define PEAQ_WIDE_F_NONE  1  /* the coarse stage had no estimate (coarse.norm 0 or NaN): coarse_lag = 0, the fine stage
                                ran on the pair cut at lag 0 (signals of one length: the pair as it is), so lag is the
                                plain estimate */
#define PEAQ_WIDE_F_RANGE 2  /* |coarse.lag| == ceil (max_offset / factor): the offset may lie outside max_offset */
#define PEAQ_WIDE_F_EDGE  4  /* |fine.lag| == max_lag: coarse and fine stage disagree */
typedef struct {            /* 80 bytes */
  int32_t  lag;             /* coarse_lag + fine.lag: positive = the test signal is late, as peaq_delay's */
  int32_t  coarse_lag;      /* coarse.lag * factor, input samples */
  uint32_t factor, flags;
  peaq_delay fine;          /* the record of the pair cut by coarse_lag */
  peaq_delay coarse;        /* the record of the decimated pair; its lag counts decimated samples */
} peaq_wide_delay;
size_t peaq_wide_delay_size (void);
/* Host only, no device.  0: max_offset is outside 1 .. PEAQ_WIDE_MAX_OFFSET. */
uint32_t peaq_wide_factor (uint32_t max_offset);
/* h: room for 16 M + 1 doubles, h[0] being the tap j = -8M.  Returns the count, 16 M + 1; an M that is not a power of
 * two in 2 .. 64, or h NULL: PEAQ_ERR_ARG.  Host only, no device. */
int peaq_wide_taps (uint32_t M, double *h);
/* d_in: [n_pairs][in_stride][channels] as peaq_batch_cut's; n_in: host array of per-pair lengths (pinned staging,
 * copied on `stream`), NULL = n_uniform for all.  d_out: device, MONO, [n_pairs][out_stride].  Enqueues on `stream` and
 * returns (a context's first call with a factor copies that factor's taps to its device, blocking, once).
 * PEAQ_ERR_ARG, before any device is touched and with the offending value in the message: an M that peaq_wide_taps
 * refuses, a mode other than 0 or 1, an out_stride below the longest n_dec, a pair longer than in_stride, NULL buffers,
 * channels other than 1 or 2, more than 65535 pairs. */
int peaq_batch_decimate (peaq_ctx *ctx, int channels, int n_pairs, const float *d_in, size_t in_stride,
                         const uint32_t *n_in /* host, NULL = n_uniform */, uint32_t n_uniform,
                         uint32_t M, int mode, float *d_out /* device, mono, [n_pairs][out_stride] */,
                         size_t out_stride, void *stream);
/* The wide estimate IS this composition of the entries above, bit for bit; batch layout and lengths as for
 * peaq_batch_estimate_delay:
 *   1. peaq_batch_decimate of both signals with M = peaq_wide_factor (max_offset) and `mode`;
 *   2. peaq_batch_estimate_delay on the two mono buffers with the lengths n_dec and max_lag = ceil (max_offset / M);
 *   3. the records are read; coarse_lag = coarse.lag M, or 0 under PEAQ_WIDE_F_NONE;
 *   4. peaq_batch_cut of both signals by peaq_aligned_lengths (coarse_lag, n_ref, n_test) into staging buffers;
 *   5. peaq_batch_estimate_delay on the staging with the common lengths and `max_lag`;
 *   6. the records are read; lag = coarse_lag + fine.lag, and the flags.
 * A pair whose common part is empty gets the estimator's all-zero fine record and lag = coarse_lag.  Pairs are taken
 * in groups whose staging (peaq_wide_workspace_bytes) stays below 1 GiB, or is one pair's; a pair's record does not
 * depend on its group.  out: HOST array of n_pairs records.  The call BLOCKS, as peaq_batch_estimate_drift does.
 * Envelope mode finds material that has nothing below 24000 / M Hz, which waveform mode cannot; neither finds
 * periodic material (a tone), which defeats any correlation search.
 * PEAQ_ERR_ARG, before any device is touched and with the offending value in the message: a max_offset that
 * peaq_wide_factor refuses, a mode other than 0 or 1, max_lag outside 1 .. 16384, and everything
 * peaq_batch_estimate_delay refuses. */
int peaq_batch_estimate_delay_wide (peaq_ctx *ctx, int channels, int n_pairs, const float *d_ref, const float *d_test,
                                    size_t pair_stride, const uint32_t *n_ref, const uint32_t *n_test, uint32_t n_uniform,
                                    uint32_t max_offset, int mode, uint32_t max_lag /* fine stage, 1 .. 16384 */,
                                    peaq_wide_delay *out /* HOST, [n_pairs] */, void *stream);
/* The call's own staging for a shape, in bytes (n_max: the longest signal of either side): per pair of a group the
 * two cut buffers, the two decimated buffers and the two records.  It stops growing with n_pairs at 1 GiB (or one
 * pair's share).  The scratch of the stages it calls (peaq_align_workspace_bytes, the decimator's FP64 rows) lives in
 * the context and comes on top.  0 for no pairs, channels other than 1 or 2 or a max_offset without a factor. */
size_t peaq_wide_workspace_bytes (int channels, int n_pairs, uint32_t n_max, uint32_t max_offset);
/* peaq_run_pair_aligned with the wide estimate in the plain one's place: upload, conversion to 48 kHz if rate != 48000,
 * peaq_batch_estimate_delay_wide, cut of both signals by delay->lag, the one-pair path.  The lag counts 48 kHz samples.
 * The result is bit for bit peaq_run_pair on the two signals cut by hand.  delay (host, may be NULL) receives the
 * record. */
int peaq_run_pair_wide (peaq_ctx *ctx, int advanced, int channels, double playback_level_db, uint32_t rate,
                        uint32_t max_offset, int mode, uint32_t max_lag, const float *ref, size_t n_ref,
                        const float *test, size_t n_test, peaq_wide_delay *delay /* host */, peaq_result *out);

/* ---- constant drift on the device ------------------------------------------------
 * Material that passed through a second clock (a DA/AD loop, a USB or Bluetooth device) has a delay that grows
 * steadily: at 100 ppm by 48 samples over 10 s.  One lag leaves most of such an item misaligned, and PEAQ scores that as
 * distortion.  This stage models the delay of a pair as ONE straight line, fits it robustly from per-window delays that
 * the two stages above measure, and resamples the test signal along it through shift_tab.  Only the test signal is
 * changed.  A delay that is no straight line is the next stage's ("delay track on the device").  Steps of the delay
 * sharper than a window of that track are the stage's after it ("delay steps on the device").  Not done, here or
 * anywhere: the host-fed pipelines
 * (peaq_batch_run_host*, the CLI's --list), which align to whole samples only.
 *
 *   Coordinates.  lag0 = the pair's lag from peaq_batch_estimate_delay over the whole signals; peaq_aligned_lengths
 *   (lag0, ...) gives skip_ref, skip_test and n_common; A_ref[i] = ref[skip_ref + i], A_test[i] = test[skip_test + i].
 *   The model: A_test at position i + a + e i belongs to A_ref[i].
 *   Windows.  W = n_common / window whole windows, 4096 <= window <= 2^20; window w is [w window, (w + 1) window) of
 *   A_ref and of A_test.  Its delay record is what peaq_batch_estimate_delay writes for that pair of slices with
 *   max_lag = R (1 <= R <= window / 4, R <= 16384), its sub-delay record what peaq_batch_refine_delay writes for the
 *   slices and that lag: the stage copies the slices (peaq_batch_gather) and calls those two entry points, so the
 *   records are theirs bit for bit.  d_w = lag_w + q_w / 256, x_w = w window + window / 2.
 *   A window is valid when its norm is finite and > 0, its sub-delay flags are 0 and |peak_w| >= min_corr norm_w (peak
 *   and norm of the DELAY record).
 *   Fit (host, FP64, every operation rounded on its own): Theil-Sen.  e = the median of (d_j - d_i) / (x_j - x_i) over
 *   all valid i < j; a = the median of d_w - e x_w over the valid w; a median is the middle one of the sorted doubles,
 *   the mean of the two middle ones for an even count.  resid_rms = sqrt (sum (d_w - a - e x_w)^2 / n_valid), summed
 *   in the order of w.  Fewer than 3 valid windows: PEAQ_DRIFT_F_NONE, a = e = 0.  |e| > max_e (0 < max_e <= 1e-3):
 *   PEAQ_DRIFT_F_RANGE, a = e = 0 (resid_rms stays that of the fitted line).  A pair's record depends on nothing but
 *   the pair and repeats bit for bit. */
#define PEAQ_DRIFT_MIN_WINDOW   4096u
#define PEAQ_DRIFT_MAX_WINDOW   (1u << 20)
#define PEAQ_DRIFT_MAX_WINDOWS  4096u   /* windows of one pair (the fit looks at every pair of them) */
#define PEAQ_DRIFT_MAX_E        1e-3
#define PEAQ_DRIFT_MAX_A        1048576.   /* |a| peaq_batch_cut_drift takes */
#define PEAQ_DRIFT_F_NONE   1   /* fewer than 3 valid windows */
#define PEAQ_DRIFT_F_RANGE  2   /* |e| > max_e */
typedef struct {               /* 48 bytes */
  int32_t  lag0;               /* as given */
  uint32_t flags;
  double   a, e;               /* samples, samples per sample */
  double   ppm;                /* 1e6 e */
  double   resid_rms;          /* samples */
  uint32_t n_windows, n_valid;
} peaq_drift;
size_t peaq_drift_size (void);
/* Host only.  The fit above over the n points (d[w], x[w]) with valid[w] != 0 (valid == NULL: all); n <=
 * PEAQ_DRIFT_MAX_WINDOWS.  Returns the number of valid points; with fewer than 3, *a = *e = 0.  PEAQ_ERR_ARG: NULL d,
 * x, a or e, an n beyond the limit. */
int peaq_drift_fit (const double *d, const double *x, const uint8_t *valid, size_t n, double *a, double *e);
/* Host only.  Where output i of the drift cut reads: g = (int64) rint (256 fma (e, (double) i, a)), to nearest even;
 * *m = floor ((g + 128) / 256); *phi = g - 256 m, in [-128, 127].  The device evaluates the same FP64 operations. */
void peaq_drift_index (double a, double e, int64_t i, int64_t *m, int32_t *phi);
/* Host only.  skip_ref, skip_test: peaq_aligned_lengths (lag0, ...)'s.  *n_keep: the largest count <= n_common such
 * that skip_test + i + m_i < n_test for every i < n_keep, i.e. no kept output is centred behind the test signal's end
 * (i + m_i never decreases with i, so these are the first n_keep).  An output centred before the test signal's first
 * sample -- at most the first -a of them, and only where skip_test < -a -- is kept: its taps outside the signal
 * contribute nothing, as in peaq_batch_cut_shifted. */
void peaq_drift_lengths (int32_t lag0, double a, double e, uint32_t n_ref, uint32_t n_test,
                         uint32_t *skip_ref, uint32_t *skip_test, uint32_t *n_keep);
/* Windows of a pair: n_common / window (0 for a window out of range). */
uint32_t peaq_drift_windows (int32_t lag0, uint32_t n_ref, uint32_t n_test, uint32_t window);
/* Batch layout and lengths as for peaq_batch_estimate_delay; lag0: host array.  d_win_delay / d_win_sub: device arrays
 * [n_pairs][w_max] that receive the per-window records, row p holding peaq_drift_windows of pair p and, behind them,
 * the records of empty slices (lag 0, norm 0; PEAQ_SUB_F_NONE).  out: HOST array of n_pairs records.  The call BLOCKS: it
 * copies the slices into two staging buffers of its own (peaq_drift_workspace_bytes; allocated and freed by the call),
 * runs peaq_batch_estimate_delay on them, reads the lags, runs peaq_batch_refine_delay, reads both record arrays and
 * fits.  Pairs are taken in groups of at most 1 GiB of staging (or one pair's), which is fewer than 65535 window slots.
 * PEAQ_ERR_ARG, before any device is touched and with the offending value in the message: a window, R, min_corr (0 ..
 * 1) or max_e out of range, a w_max of 0, beyond PEAQ_DRIFT_MAX_WINDOWS or below a pair's windows, channels other than
 * 1 or 2, more than 65535 pairs, NULL buffers or arrays, n_ref without n_test, a pair longer than pair_stride. */
int peaq_batch_estimate_drift (peaq_ctx *ctx, int channels, int n_pairs,
                               const float *d_ref, const float *d_test, size_t pair_stride,
                               const uint32_t *n_ref, const uint32_t *n_test, uint32_t n_uniform,
                               const int32_t *lag0 /* host */, uint32_t window, uint32_t R, double min_corr, double max_e,
                               uint32_t w_max, peaq_delay *d_win_delay /* device */, peaq_subdelay *d_win_sub /* device */,
                               peaq_drift *out /* host, [n_pairs] */, void *stream);
/* The two staging buffers of a call, in bytes: 2 x window x channels x 4 per window slot, w_max slots per pair, the
 * pairs of one group.  The aligner's and the sub-sample stage's own scratch for the slices (peaq_align_workspace_bytes,
 * peaq_subdelay_workspace_bytes with n_pairs x w_max "pairs" of `window` samples) comes on top.  0 for arguments the
 * call would refuse. */
size_t peaq_drift_workspace_bytes (int channels, int n_pairs, uint32_t window, uint32_t w_max);
/* peaq_batch_cut of the test signal along each pair's line (a[p], e[p]: host arrays of doubles):
 * out[p][i][c] = (float) sum_{o = -32 .. 32} shift_tab[phi_i][o] (double) in[p][skip[p] + i + m_i + o][c] for
 * i < n_keep[p], (m_i, phi_i) = peaq_drift_index (a[p], e[p], i): fused multiply-adds in the order o = -32 .. 32 in
 * FP64, rounded once to FP32.  A tap whose index falls outside [0, n_in[p]) contributes nothing.  Samples of d_out past
 * n_keep[p] are left as they were.  With e[p] == 0 and a[p] = q / 256, q in [-128, 127], the output is bit for bit
 * peaq_batch_cut_shifted's; a pair with a[p] == 0 and e[p] == 0 has its bits moved as they are (peaq_batch_cut's) and, like
 * peaq_batch_cut_shifted at q == 0, does not look at n_in[p]: it copies what the buffer holds.
 * Refusals as peaq_batch_cut_shifted's, and: an a or e that is not finite, |a| > PEAQ_DRIFT_MAX_A, |e| >
 * PEAQ_DRIFT_MAX_E, NULL a or e. */
int peaq_batch_cut_drift (peaq_ctx *ctx, int channels, int n_pairs,
                          const float *d_in, size_t in_stride, const uint32_t *n_in /* host */,
                          const uint32_t *skip /* host */, const uint32_t *n_keep /* host */,
                          const double *a /* host */, const double *e /* host */,
                          float *d_out, size_t out_stride, void *stream);
/* peaq_run_pair_subsample with this stage in the sub-sample stage's place, in this order: upload; conversion to 48 kHz
 * if rate != 48000; estimate (max_lag at least 1); peaq_batch_estimate_drift (window, R = min (window / 4, 1024),
 * min_corr 0.5, max_e 1e-3); peaq_drift_lengths; plain cut of the reference to n_keep; drift cut of the test signal; if
 * mode is not PEAQ_GAIN_OFF, the gain measured AFTER the drift cut on the two cut buffers and applied into a second
 * buffer; the one-pair path.  A flagged record (a = e = 0) scores what peaq_run_pair_aligned scores.  delay, drift and
 * gain (host) may be NULL. */
int peaq_run_pair_drift (peaq_ctx *ctx, int advanced, int channels, double playback_level_db, uint32_t rate,
                         uint32_t max_lag, uint32_t window, int mode, double max_gain_db,
                         const float *ref, size_t n_ref, const float *test, size_t n_test,
                         peaq_delay *delay /* host */, peaq_drift *drift /* host */, peaq_gain *gain /* host */,
                         peaq_result *out);

/* ---- delay track on the device ------------------------------------------------
 * Material that passed two clocks one after the other, a loop whose clock wanders, a player that re-synchronised once:
 * their delay bends or steps, and one line leaves part of the item misaligned.  This stage keeps the per-window delays
 * that the drift stage measures as a TRACK -- a knot per window, a line from every knot to the next -- and resamples
 * the test signal along it through shift_tab.  Only the test signal is changed.  A step sharper than a window is spread over
 * the window it falls in, or flags the pair: locating it is the next stage's ("delay steps on the device").  Not done,
 * here or anywhere: the host-fed pipelines
 * (peaq_batch_run_host*, the CLI's --list), which align to whole samples only.
 *
 *   Coordinates, windows, d_w = lag_w + q_w / 256, x_w = w window + window / 2 (the integer half) and the validity rule
 *   are those of "constant drift on the device".  The fit takes d[W], valid[W], window and max_e; host, FP64, every
 *   operation rounded on its own.  line (u1, u2, x1, x2, x0) = u1 + (u1 - u2) / (x1 - x2) * (x0 - x1).
 *   1. V_0 < ... < V_{nv-1} are the valid windows, u_j = d[V_j].  nv == 0: PEAQ_TRACK_F_NONE, every knot and segment 0.
 *   2. Outliers (nv >= 3; else t = u): a running median of three over the raw u.  t_j = med3 (u_{j-1}, u_j, u_{j+1})
 *      inside; t_0 = med3 (u_0, u_1, line (u_1, u_2, x_{V_1}, x_{V_2}, x_{V_0})) and the mirror image at the other end;
 *      med3 is the middle one by value.  Values on a line (a constant drift) pass unchanged, as does the inside of any
 *      monotone sequence (an end of one moves at most onto the line through its two neighbours); a step survives,
 *      one wild window does not.
 *   3. Knots: s_w = t_j at w = V_j; between V_j and V_{j+1} s_w = line (t_j, t_{j+1}, x_{V_j}, x_{V_{j+1}}, x_w); before
 *      the first and behind the last valid window that one's value.  n_filled counts the invalid windows.
 *   4. Segments: S = max (W - 1, 1); e_k = (s_{k+1} - s_k) / (double) window, a_k = s_k - e_k x_k; W == 1: e_0 = 0, a_0 =
 *      s_0.  Output i belongs to segment k (i) = i < window / 2 ? 0 : min ((i - window / 2) / window, S - 1), integers:
 *      the first and the last segment extend to the ends of the pair.
 *   5. Range: any |e_k| > max_e (0 < max_e <= PEAQ_TRACK_MAX_E): PEAQ_TRACK_F_RANGE, every a_k and e_k 0 (the pair is cut
 *      as peaq_batch_cut cuts it); the knots, d_min, d_max and max_abs_e stay readable.
 *   6. Output i reads at peaq_drift_index (a_{k (i)}, e_{k (i)}, i): the same FP64 operations on host and device.
 *   A pair's record depends on nothing but the pair and repeats bit for bit. */
#define PEAQ_TRACK_MAX_E       0.015625   /* 1 / 64 */
#define PEAQ_TRACK_MAX_STEP    0.00390625 /* 1 / 256: how far two segments may be apart where they meet, for the cut */
#define PEAQ_TRACK_F_NONE   1   /* no valid window */
#define PEAQ_TRACK_F_RANGE  2   /* an |e_k| > max_e */
#define PEAQ_TRACK_MAX_SEGMENTS_PER_CALL (1u << 20)   /* summed over the pairs of one peaq_batch_cut_track: 16 MiB of staging */
typedef struct {               /* 48 bytes */
  int32_t  lag0;               /* as given */
  uint32_t flags;
  uint32_t n_windows, n_valid;
  uint32_t n_filled, n_segments;
  double   d_min, d_max;       /* over the knots, samples */
  double   max_abs_e;          /* the steepest segment, also where it is out of range */
} peaq_track;
size_t peaq_track_size (void);
/* Host only.  The fit above: d, valid (NULL: all valid) of n_windows <= PEAQ_DRIFT_MAX_WINDOWS entries, knots of
 * n_windows, a and e of max (n_windows - 1, 1).  out->lag0 is set to 0.  PEAQ_ERR_ARG: a NULL array, a window out of
 * 4096 .. 2^20 (odd ones are taken), too many windows, a max_e outside (0, 1 / 64]. */
int peaq_track_fit (const double *d, const uint8_t *valid, uint32_t n_windows, uint32_t window, double max_e,
                    peaq_track *out, double *knots, double *a, double *e);
/* Host only.  k (i) of item 4 for n_seg >= 1 segments (0 for n_seg == 0 or window == 0). */
uint32_t peaq_track_segment (int64_t i, uint32_t window, uint32_t n_seg);
/* Host only.  Item 6: peaq_drift_index along the segment of i. */
void peaq_track_index (uint32_t window, uint32_t n_seg, const double *a, const double *e, int64_t i, int64_t *m,
                       int32_t *phi);
/* Host only.  peaq_drift_lengths with the track in the line's place: *n_keep is the largest count <= n_common with
 * skip_test + i + m_i < n_test for every i below it.  i + m_i does not decrease with i where every |e_k| <= 1 / 64 and
 * neighbouring segments meet within PEAQ_TRACK_MAX_STEP, as the fit's do (gstpeaq_amd/csrc/peaq_track_math.h has the
 * argument); for other segments the count is that of a binary search over i. */
void peaq_track_lengths (int32_t lag0, uint32_t window, uint32_t n_seg, const double *a, const double *e,
                         uint32_t n_ref, uint32_t n_test, uint32_t *skip_ref, uint32_t *skip_test, uint32_t *n_keep);
/* peaq_batch_estimate_drift (same arguments up to d_win_sub; its max_e is PEAQ_DRIFT_MAX_E whatever max_e is here),
 * then the two record arrays are read back and the fit above runs per pair: the window records are
 * peaq_batch_estimate_delay's and peaq_batch_refine_delay's on the slices bit for bit, and the line's record comes out
 * beside the track's (drift: host, [n_pairs], may be NULL).  out: host [n_pairs]; knots: host [n_pairs][w_max]; a, e:
 * host [n_pairs][seg_stride], row p holding out[p].n_segments entries (knots and segments behind a pair's own are 0).
 * The call BLOCKS, as the drift estimate does.
 * Refusals as peaq_batch_estimate_drift's, and: a seg_stride below w_max - 1 or below 1, a max_e outside (0, 1 / 64],
 * NULL out, knots, a or e. */
int peaq_batch_estimate_track (peaq_ctx *ctx, int channels, int n_pairs,
                               const float *d_ref, const float *d_test, size_t pair_stride,
                               const uint32_t *n_ref, const uint32_t *n_test, uint32_t n_uniform,
                               const int32_t *lag0 /* host */, uint32_t window, uint32_t R, double min_corr, double max_e,
                               uint32_t w_max, peaq_delay *d_win_delay /* device */, peaq_subdelay *d_win_sub /* device */,
                               peaq_drift *drift /* host, [n_pairs], may be NULL */, peaq_track *out /* host, [n_pairs] */,
                               double *knots /* host */, uint32_t seg_stride, double *a /* host */, double *e /* host */,
                               void *stream);
/* peaq_batch_cut of the test signal along each pair's track (n_seg[p] segments in row p of a and e, host arrays):
 * out[p][i][c] = (float) sum_{o = -32 .. 32} shift_tab[phi_i][o] (double) in[p][skip[p] + i + m_i + o][c] for
 * i < n_keep[p], (m_i, phi_i) = peaq_track_index (window, n_seg[p], a[p], e[p], i): fused multiply-adds in the order
 * o = -32 .. 32 in FP64, rounded once to FP32.  A tap whose index falls outside [0, n_in[p]) contributes nothing.
 * Samples of d_out past n_keep[p] are left as they were.  A pair whose segments all hold the same (a, e), |e| <=
 * PEAQ_DRIFT_MAX_E, is bit for bit peaq_batch_cut_drift's output (so with e = 0 and a = q / 256 peaq_batch_cut_shifted's);
 * a pair whose segments are all (0, 0) has its bits moved as they are (peaq_batch_cut's) and does not look at n_in[p].
 * All per-pair arrays and the segments travel through the pinned staging slots.
 * Refusals as peaq_batch_cut_drift's, and: an a or e that is not finite, |a| > PEAQ_DRIFT_MAX_A, |e| >
 * PEAQ_TRACK_MAX_E, an n_seg of 0 or above seg_stride, a window out of 4096 .. 2^20, more than
 * PEAQ_TRACK_MAX_SEGMENTS_PER_CALL segments in all, neighbouring segments more than PEAQ_TRACK_MAX_STEP apart where
 * they meet (the kernel's staged span is sized for lines that meet), NULL n_seg, a or e. */
int peaq_batch_cut_track (peaq_ctx *ctx, int channels, int n_pairs,
                          const float *d_in, size_t in_stride, const uint32_t *n_in /* host */,
                          const uint32_t *skip /* host */, const uint32_t *n_keep /* host */,
                          uint32_t window, const uint32_t *n_seg /* host */, uint32_t seg_stride,
                          const double *a /* host */, const double *e /* host */,
                          float *d_out, size_t out_stride, void *stream);
/* peaq_run_pair_drift with the track in the line's place: peaq_batch_estimate_track (window, R = min (window / 4, 1024),
 * min_corr 0.5, max_e 1 / 64); peaq_track_lengths; plain cut of the reference to n_keep; track cut of the test signal;
 * the gain, if any, measured AFTER the cut.  A flagged record (every segment 0) scores what peaq_run_pair_aligned
 * scores.  delay, track and gain (host) may be NULL. */
int peaq_run_pair_track (peaq_ctx *ctx, int advanced, int channels, double playback_level_db, uint32_t rate,
                         uint32_t max_lag, uint32_t window, int mode, double max_gain_db,
                         const float *ref, size_t n_ref, const float *test, size_t n_test,
                         peaq_delay *delay /* host */, peaq_track *track /* host */, peaq_gain *gain /* host */,
                         peaq_result *out);

/* ---- delay steps on the device ------------------------------------------------
 * A player or a link that drops or repeats a block, a concealed packet loss, an edit that removes a few hundred samples:
 * from such a point to the item's end the delay differs by a fixed amount.  The track above spreads a small step over a
 * whole window and is flagged PEAQ_TRACK_F_RANGE by a larger one (more than window / 64 samples).  This stage finds, for
 * every segment of a track that looks like a step, the POSITION of the step inside the two windows around it
 * (peaq_batch_locate_steps), rebuilds the track as PIECES -- lines that need not meet, with breakpoints anywhere
 * (peaq_steps_fit) -- and cuts the test signal along them (peaq_batch_cut_pieces).  Only the test signal is changed; a
 * positive step drops samples of it and a negative one repeats some, which is what the material did.  Not done, here or
 * anywhere: the apex of a bend, two steps in neighbouring segments (each masks the other's ratio test), cross-fading at
 * a step, steps= on trajectories and traces, and the host-fed pipelines (peaq_batch_run_host*, the CLI's --list), which
 * align to whole samples only.
 *
 *   Coordinates are those of "constant drift on the device": lag0, skip_ref, skip_test, n_common = peaq_aligned_lengths
 *   (lag0, ...); A_ref[i] = ref[skip_ref + i], A_test[j] = test[skip_test + j]; r and t their FP64 mono sums (the two
 *   channels added in double, left first); a sample outside its signal counts as 0.
 *   Locate.  A candidate is { pair, lo, hi, LA, LB } with lo < hi <= n_common of its pair and integer delays LA != LB:
 *   the hypothesis that the delay is LA before some c in [lo, hi] and LB from c on.  With d[i] = t[i + LA] - t[i + LB]
 *   and h[i] = r[i] d[i] (each rounded once), H[c] = sum over lo <= i < c of h[i], H[lo] = 0:
 *     s     = the sign of P = sum over lo <= i < hi of r[i] (t[i + LA] + t[i + LB]), + for 0: the polarity;
 *     c*    = the c in [lo, hi] with the largest s H[c];
 *     gain_left = s H[c*], gain_right = s (H[c*] - H[hi]), norm = sqrt (R2 D2), R2 = sum r[i]^2, D2 = sum d[i]^2 over
 *     the interval.  Both gains are >= 0; for a true step each is about the cross-energy the step moves on its side.
 *   The order of every sum is fixed by the index within the interval alone, in chunks of 4096 positions from lo on:
 *     in chunk j, lane l (0 .. 255) owns positions 16 l .. 16 l + 15 of the chunk; run_u = h_0 + ... + h_u over its own,
 *     added one after the other from 0 (a position at or behind hi adds 0); S_l = run_15;
 *     before_l = the S of the lanes 64 (l / 64) .. l - 1, added one after the other from 0; wave total w_v = before_l +
 *     S_l at l = 64 v + 63; waves_l = the w of the waves in front of l's, one after the other from 0;
 *     Hloc = waves_l + (before_l + run_u) is the sum from the chunk's start up to and including that position; the
 *     chunk's total T_j = ((w_0 + w_1) + w_2) + w_3, which is Hloc at its last position to the bit;
 *     C_0 = 0, C_{j+1} = C_j + T_j; H[c] = C_j + Hloc for c in chunk j (c - lo in 4096 j + 1 .. 4096 j + 4096), H[hi] =
 *     C behind the last chunk.  Every H is within (16 + 64 + 4 + 1024) 2^-53 sum |h| < 1.3e-13 sum |h| of the exact sum.
 *     P, R2 and D2: a lane's terms as fused multiply-adds in the order of u, then the wave (a butterfly), the four waves
 *     (0 + 1) + (2 + 3), then the chunks one after the other.
 *   Comparisons are exact, on these values: inside a chunk the largest (s > 0) or smallest (s < 0) Hloc, the smallest c
 *   among equals; between chunks and against c = lo (value 0) the largest s (C_j + that Hloc), the smallest c among
 *   equals.  No floating-point atomics.  A candidate's record does not depend on the other candidates of the call or on
 *   where the buffers lie, and repeats bit for bit. */
#define PEAQ_STEP_MAX_SPAN  (1u << 22)  /* hi - lo of a candidate that is searched */
#define PEAQ_STEP_MAX_L     1064960     /* 2^20 + 16384: |LA|, |LB| */
#define PEAQ_STEP_F_NONE    1   /* norm is 0 or not finite: c = lo, both gains 0 */
#define PEAQ_STEP_F_SPAN    2   /* hi - lo > PEAQ_STEP_MAX_SPAN: nothing was searched; c = lo, gains and norm 0 */
#define PEAQ_STEP_F_WEAK    4   /* set by peaq_steps_fit: located, but not accepted */
#define PEAQ_STEP_MIN_STEP  0.75       /* defaults of min_step, ratio and min_gain (DESIGN.md 19 has the measurements) */
#define PEAQ_STEP_RATIO     3.
#define PEAQ_STEP_MIN_GAIN  0.0021
#define PEAQ_PIECES_MAX_PER_PAIR  (2u * PEAQ_DRIFT_MAX_WINDOWS)
#define PEAQ_PIECES_MAX_PER_CALL  (1u << 20)   /* summed over the pairs of one peaq_batch_cut_pieces: 20 MiB of staging */
#define PEAQ_PIECES_F_RANGE 2   /* an |e_j| > max_e among the pieces: every a_j and e_j is 0 */
typedef struct {               /* 20 bytes */
  uint32_t pair, lo, hi;
  int32_t  LA, LB;
} peaq_step_candidate;
typedef struct {               /* 48 bytes */
  uint32_t pair;               /* as given */
  uint32_t c;                  /* c*, in lo .. hi */
  int32_t  LA, LB;             /* as given */
  uint32_t flags;
  uint32_t reserved;
  double   gain_left, gain_right, norm;
} peaq_step;
typedef struct {               /* 24 bytes */
  uint32_t flags;              /* PEAQ_PIECES_F_RANGE */
  uint32_t n_candidates, n_accepted, n_pieces;
  double   max_abs_e;          /* the steepest piece, also where it is out of range */
} peaq_pieces;
size_t peaq_step_candidate_size (void);
size_t peaq_step_size (void);
size_t peaq_pieces_size (void);
/* Batch layout and lengths as for peaq_batch_refine_delay; lag0: host array of n_pairs lags, which fix each pair's
 * coordinates.  cand: HOST array of n_cand candidates, resolved on the host and sent through the pinned staging slots,
 * copied on `stream`.  d_out: device array of n_cand peaq_step, in the order of cand.  Enqueues on `stream` and returns,
 * synchronising nothing.  The chunks' rows (peaq_steps_workspace_bytes) live in the context and are reused; a call on
 * another stream waits, on the device, for the previous call's kernels.
 * PEAQ_ERR_ARG, before any device is touched and with the offending value in the message: peaq_batch_refine_delay's
 * refusals (lag0 in the place of lag), and: a NULL cand with n_cand > 0, a pair index >= n_pairs, lo >= hi, hi beyond
 * the pair's n_common, LA == LB, |LA| or |LB| above PEAQ_STEP_MAX_L, n_cand < 0 or more than 65535 candidates. */
int peaq_batch_locate_steps (peaq_ctx *ctx, int channels, int n_pairs,
                             const float *d_ref, const float *d_test, size_t pair_stride,
                             const uint32_t *n_ref, const uint32_t *n_test, uint32_t n_uniform,
                             const int32_t *lag0 /* host */, int n_cand, const peaq_step_candidate *cand /* host */,
                             peaq_step *d_out /* device, [n_cand] */, void *stream);
/* The rows of peaq_batch_locate_steps for n_cand candidates whose longest interval is span_max (above
 * PEAQ_STEP_MAX_SPAN: that), in bytes: 64 per chunk of 4096 positions and candidate.  Candidates are taken in groups,
 * so it stops growing with n_cand at 256 MiB.  0 for no candidates. */
size_t peaq_steps_workspace_bytes (int n_cand, uint32_t span_max);
/* Host only, FP64, every operation rounded on its own.  The candidates of one pair's track, from its knots s_w (peaq_track_fit's or
 * peaq_batch_estimate_track's: they stay readable under PEAQ_TRACK_F_RANGE), in the order of k.  D_k = s_{k+1} - s_k
 * for the S = n_windows - 1 segments (fewer than 2 windows: none).  Segment k is a candidate when |D_k| >= min_step and
 * |D_k| >= ratio max (|D_{k-1}|, |D_{k+1}|), a neighbour that does not exist counting as 0 (a constant drift has equal
 * D and gives none); lo = k window, hi = min ((k + 2) window, n_common), LA = (int) rint (s_k), LB = (int) rint
 * (s_{k+1}), to nearest even; a candidate with LA == LB (or with lo >= hi) is dropped.  out: room for max (n_windows -
 * 1, 1) entries, their `pair` set to the argument; *n: how many.  PEAQ_ERR_ARG: NULL knots, out or n, a window out of
 * 4096 .. 2^20, more than PEAQ_DRIFT_MAX_WINDOWS windows, n_windows x window beyond n_common, a min_step or ratio that
 * is negative or not finite. */
int peaq_steps_candidates (const double *knots, uint32_t n_windows, uint32_t window, uint32_t n_common, uint32_t pair,
                           double min_step, double ratio, peaq_step_candidate *out, uint32_t *n);
/* Host only, FP64, every operation rounded on its own.  One pair's track rebuilt as pieces.  steps: the n_steps records
 * peaq_batch_locate_steps wrote for peaq_steps_candidates (same knots, window, n_common, min_step, ratio), in that
 * order; the call derives the candidates again and refuses records that are not theirs.
 *   Segments: (a_k, e_k) of segment k are item 4 of "delay track on the device" taken from the knots -- the track's own
 *   bits where it kept them.  Segment k's own outputs are [start_k, start_{k+1}), start_0 = 0, start_k = window / 2 + k
 *   window, the last one running to the pair's end.
 *   Accept: a record with flags == 0 and min (gain_left, gain_right) >= min_gain norm is a step at c; any other gets
 *   PEAQ_STEP_F_WEAK added to its flags (in steps) and its segment stays the track's.
 *   Pieces (b_j, a_j, e_j), b_0 = 0, b strictly increasing, piece j covering outputs [b_j, b_{j+1}) and the last one
 *   running to the pair's end, in the order of the segments; a piece that would be empty is left out; neighbours with
 *   identical (a, e) are not merged.  A segment without a step is one piece with its own line, from start_k -- or from
 *   the c of a step in segment k - 1 that lies behind start_k -- to start_{k+1} -- or to the c of a step in segment k + 1
 *   that lies before it.  A step in segment k replaces it by two pieces: the line of segment k - 1 up to c and the line
 *   of segment k + 1 from c on, where (s_k, 0) stands for the left line if segment k - 1 does not exist or is a step
 *   itself, and (s_{k+1}, 0) for the right line likewise.  A c outside the segment's own outputs reaches into the
 *   neighbour as said, unless that neighbour is a step itself: then c is taken as the border between the two.
 *   Range: any |e_j| > max_e (0 < max_e <= 1 / 64) sets PEAQ_PIECES_F_RANGE and every a_j and e_j to 0; b stays.  A
 *   pair whose track is PEAQ_TRACK_F_RANGE through a step alone comes out unflagged once the step is accepted.
 * b, a, e: room for max (n_windows - 1, 1) + n_steps entries; out->n_pieces of them are written.
 * PEAQ_ERR_ARG: NULL arrays, a window, window count, n_common, min_step, ratio as above, a min_gain that is negative
 * or not finite, a max_e outside (0, 1 / 64], an n_steps or a record's LA, LB that are not the candidates'. */
int peaq_steps_fit (const double *knots, uint32_t n_windows, uint32_t window, uint32_t n_common,
                    double min_step, double ratio, double min_gain, double max_e,
                    peaq_step *steps, uint32_t n_steps, peaq_pieces *out, uint32_t *b, double *a, double *e);
/* Host only.  Where output i >= 0 reads: peaq_drift_index (a_j, e_j, i) along the piece j of i, the largest j with
 * b_j <= i.  The device evaluates the same operations. */
void peaq_pieces_index (uint32_t n_pieces, const uint32_t *b, const double *a, const double *e, int64_t i, int64_t *m,
                        int32_t *phi);
/* Host only.  peaq_track_lengths with pieces in the track's place: *n_keep is the largest count <= n_common with
 * skip_test + i + m_i < n_test for EVERY i below it.  i + m_i does not decrease inside a piece (|e| <= 1 / 64) but may
 * fall by any amount across a breakpoint, so the pieces are searched one by one in their order
 * (gstpeaq_amd/csrc/peaq_steps_math.h has the argument). */
void peaq_pieces_lengths (int32_t lag0, uint32_t n_pieces, const uint32_t *b, const double *a, const double *e,
                          uint32_t n_ref, uint32_t n_test, uint32_t *skip_ref, uint32_t *skip_test, uint32_t *n_keep);
/* peaq_batch_estimate_track (same arguments up to knots; the track's own segments are not handed out), then per pair
 * peaq_steps_candidates, ONE peaq_batch_locate_steps over all pairs' candidates, a read-back, and peaq_steps_fit.  The
 * window, delay and sub-delay records, the line's and the track's records are the earlier stages' bit for bit.  steps:
 * host [n_pairs][steps_stride], row p holding pieces[p].n_candidates records (`pair` = p; the rest 0); pieces: host
 * [n_pairs]; b, a, e: host [n_pairs][piece_stride], row p holding pieces[p].n_pieces entries (the rest 0).  The call
 * BLOCKS, as the track estimate does.
 * Refusals as peaq_batch_estimate_track's and peaq_steps_fit's, and: a steps_stride below max (w_max - 1, 1), a
 * piece_stride below 2 max (w_max - 1, 1), NULL steps, pieces, b, a or e, more than 65535 candidates in all. */
int peaq_batch_estimate_steps (peaq_ctx *ctx, int channels, int n_pairs,
                               const float *d_ref, const float *d_test, size_t pair_stride,
                               const uint32_t *n_ref, const uint32_t *n_test, uint32_t n_uniform,
                               const int32_t *lag0 /* host */, uint32_t window, uint32_t R, double min_corr, double max_e,
                               double min_step, double ratio, double min_gain,
                               uint32_t w_max, peaq_delay *d_win_delay /* device */, peaq_subdelay *d_win_sub /* device */,
                               peaq_drift *drift /* host, [n_pairs], may be NULL */, peaq_track *track /* host, [n_pairs] */,
                               double *knots /* host */, uint32_t steps_stride, peaq_step *steps /* host */,
                               peaq_pieces *pieces /* host, [n_pairs] */, uint32_t piece_stride,
                               uint32_t *b /* host */, double *a /* host */, double *e /* host */, void *stream);
/* peaq_batch_cut_track's definition with peaq_pieces_index in the place of peaq_track_index (n_pieces[p] pieces in row
 * p of b, a and e, host arrays):
 * out[p][i][c] = (float) sum_{o = -32 .. 32} shift_tab[phi_i][o] (double) in[p][skip[p] + i + m_i + o][c] for
 * i < n_keep[p]: fused multiply-adds in the order o = -32 .. 32 in FP64, rounded once to FP32.  A tap whose index falls
 * outside [0, n_in[p]) contributes nothing.  Samples of d_out past n_keep[p] are left as they were.  Lines need not
 * meet, breakpoints may sit anywhere, a piece may be one output long, a jump may be thousands of samples either way.
 * Pieces equal to a track's segments (b_j = the segments' starts) give peaq_batch_cut_track's output bit for bit; one
 * piece with |e| <= PEAQ_DRIFT_MAX_E gives peaq_batch_cut_drift's; a pair whose pieces are all (0, 0) has its bits
 * moved as they are (peaq_batch_cut's) and does not look at n_in[p].  All per-pair arrays and the pieces travel through
 * the pinned staging slots.
 * Refusals as peaq_batch_cut_drift's, and: an a or e that is not finite, |a| > PEAQ_DRIFT_MAX_A, |e| > PEAQ_TRACK_MAX_E,
 * an n_pieces of 0, above piece_stride or above PEAQ_PIECES_MAX_PER_PAIR, more than PEAQ_PIECES_MAX_PER_CALL pieces in
 * all, a b_0 that is not 0, a b_j that is not above b_{j-1}, NULL n_pieces, b, a or e. */
int peaq_batch_cut_pieces (peaq_ctx *ctx, int channels, int n_pairs,
                           const float *d_in, size_t in_stride, const uint32_t *n_in /* host */,
                           const uint32_t *skip /* host */, const uint32_t *n_keep /* host */,
                           const uint32_t *n_pieces /* host */, uint32_t piece_stride,
                           const uint32_t *b /* host */, const double *a /* host */, const double *e /* host */,
                           float *d_out, size_t out_stride, void *stream);
/* peaq_run_pair_track with this stage in the track's place: peaq_batch_estimate_steps (window, R = min (window / 4,
 * 1024), min_corr 0.5, max_e 1 / 64, the PEAQ_STEP_* defaults); peaq_pieces_lengths; plain cut of the reference to
 * n_keep; pieces cut of the test signal; the gain, if any, measured AFTER the cut.  A flagged record (every piece 0)
 * scores what peaq_run_pair_aligned scores.  steps: host, room for max_steps records, of which min (max_steps,
 * pieces->n_candidates) are written.  delay, track, pieces, steps and gain (host) may be NULL. */
int peaq_run_pair_steps (peaq_ctx *ctx, int advanced, int channels, double playback_level_db, uint32_t rate,
                         uint32_t max_lag, uint32_t window, int mode, double max_gain_db,
                         const float *ref, size_t n_ref, const float *test, size_t n_test,
                         peaq_delay *delay /* host */, peaq_track *track /* host */, peaq_pieces *pieces /* host */,
                         peaq_step *steps /* host */, uint32_t max_steps, peaq_gain *gain /* host */,
                         peaq_result *out);

/* ---- device calibration (measurement support, bench.py) -----------------------
 * Runs a fixed FP64 multiply-add kernel (ONE wave per SIMD, sixteen independent chains; `iterations` x 512
 * multiply-adds per wave, <= 0: about 70 ms) on the context's device -- alone: it waits for everything this PROCESS has
 * in flight on the device first (hipDeviceSynchronize) and runs on a stream of its own; work of other processes on the
 * same device is the caller's to exclude -- and reports the shader clock the device held under that load and the FP64
 * rate it gave.  MI355X clocks to its power budget, and this path's kernels are FP64-dense: the same library differs
 * by several per cent from box to box.  bench.py calls this before and after its timed region so that a throughput
 * line carries the clock it was measured at.  The kernel starts from the idle device's clock: its FIRST half is
 * reported as the ramp (ramp_*), its SECOND half as the steady state (the unprefixed fields). */
typedef struct {
  double elapsed_ms;          /* HIP events around the whole kernel (both halves) */
  double shader_clock_mhz;    /* steady state: s_memtime ticks / constant-rate wall-clock ticks, mean over all waves */
  double fp64_tflops;         /* steady state: 2 x the half's multiply-adds / mean duration of a wave's second half */
  double cycles_per_fma;      /* steady state: shader cycles per v_fma_f64 of a wave that has its SIMD to itself (4 = the pipe) */
  double max_clock_mhz;       /* hipDeviceProp_t::clockRate */
  int    compute_units;
  double ramp_clock_mhz;      /* the same over the first half: from the idle clock upwards, waves still being dispatched */
  double ramp_cycles_per_fma;
  double event_fp64_tflops;   /* 2 x all multiply-adds / elapsed_ms: includes launch, ramp and tail */
  /* where the kernel's waves (one per SIMD of the device as the runtime reports it) actually ran: distinct SIMDs
   * (HW_ID / XCC_ID of every wave), the most waves any one of them got (2 = that SIMD ran them one after the other:
   * the kernel then lasts twice a wave's lifetime and event_fp64_tflops halves), and the time between the first and
   * the last wave's start */
  int    simds_used;
  int    max_waves_on_a_simd;
  double dispatch_spread_ms;
} peaq_calibration;
int peaq_calibrate (peaq_ctx *ctx, int iterations, peaq_calibration *out);

/* ---- synthetic workload (include/peaq_synth.h on the device) -------------
 * Fills d_ref/d_test [n_pairs][pair_stride][channels] with the seeded pairs
 * seed0 .. seed0+n_pairs-1, n_samples each.  Benchmark / test utility. */
int peaq_synth_fill (peaq_ctx *ctx, uint32_t seed0, int n_pairs, int channels,
                     uint32_t n_samples, size_t pair_stride,
                     float *d_ref, float *d_test, void *stream);

/* ---- stage-level access for parity tests ----------------------------------
 * Runs only the stateless front end (window, FFT, power spectra, band
 * grouping, spreading, per-frame MOV ingredients) on ONE pair resident in
 * device memory and copies the per-frame records to host memory:
 *   out[frame][channel][PEAQ_DEBUG_RECORD_DOUBLES]
 * see DESIGN.md "frame record" for the layout. */
#define PEAQ_DEBUG_RECORD_DOUBLES 576
int peaq_debug_frontend (peaq_ctx *ctx, int bands, int channels, double playback_level_db,
                         const float *d_ref, const float *d_test, uint32_t n_ref, uint32_t n_test,
                         int n_frames, double *host_out);

/* Development switch of the basic version's front end, for A/B runs and comparison tests within one process:
 * 0 = one wave per (pair, frame, channel) that carries reference and test together (the default), 1 = the two-wave
 * kernel the advanced version's FFT path is built on, -1 = what the environment variable PEAQ_AMD_FE says ("two_waves"; read once).
 * Applies to every launch of the basic version's front end: batch runs, sessions, brokers and the stage entries (one
 * kernel for all of them, so that a session's reading and a batch over the same samples agree bit for bit).  Returns
 * the previous value. */
int peaq_debug_select_frontend (int two_waves);

/* The basic version's front end over n_pairs pairs resident in device memory ([pair][pair_stride][channels]), launched
 * the way the batch path launches it, frames_per_launch frames of every pair per grid.  Returns the records as the
 * kernels exchange them, out[pair][frame][channel][PEAQ_DEBUG_RAW_RECORD_DOUBLES] for frame < n_frames (at least the
 * longest pair's frame count; records of frames a pair does not have are zero):
 *   { root ref[112], root test[112], noise in bands[112], bandwidth ref, bandwidth test, EHS, flags ref, flags test,
 *     hop energy ref, hop energy of ref - test, pad[9] },  root = (spread band energy)^(1/4). */
#define PEAQ_DEBUG_RAW_RECORD_DOUBLES 352
int peaq_debug_frontend_pairs (peaq_ctx *ctx, int channels, double playback_level_db,
                               const float *d_ref, const float *d_test, int n_pairs, size_t pair_stride,
                               const uint32_t *n_ref, const uint32_t *n_test, int frames_per_launch,
                               int n_frames, double *host_out);

/* The same for the filter-bank ear model (advanced): per-block records
 *   out[block][channel][PEAQ_DEBUG_FB_RECORD_DOUBLES] =
 *   { unsmeared ref[40], unsmeared test[40], excitation ref[40], excitation test[40],
 *     above-threshold flag, pad[7] } */
#define PEAQ_DEBUG_FB_RECORD_DOUBLES 168
int peaq_debug_filterbank (peaq_ctx *ctx, int channels, double playback_level_db,
                           const float *d_ref, const float *d_test, uint32_t n_ref, uint32_t n_test,
                           int n_blocks, int blocks_per_launch, double *host_out);

/* The stateful back end of the basic version on its own: feeds n_frames front-end
 * records of ONE pair (host memory, [frame][channel][PEAQ_DEBUG_RECORD_DOUBLES],
 * e.g. from peaq_debug_frontend or hand-built) through time smearing, level and
 * pattern adaptation, modulation processing and the MOV layer starting from a
 * fresh state, and returns per (frame, channel) PEAQ_DEBUG_BACKEND_DOUBLES doubles:
 *   8 band vectors of 112 -- excitation ref/test (fftearmodel.c:496-504), spectrally
 *   adapted ref/test (leveladapter.c:243-340), modulation ref/test and average
 *   loudness ref/test (modpatt.c:223-251) -- then total loudness ref, test
 *   (earmodel.c:891-907; only written while the loudness gate is still closed), six unused, and then the MOV
 *   layer's values of this frame BEFORE accumulation, computed for every frame whether or not the gates of
 *   gstpeaq.c:871,880-881 let the accumulators see them: ModDiff1, ModDiff2, TempWt (movs.c:205-254), noise
 *   loudness (:354-371), mean and maximum of the band noise-to-mask ratios (:971-1023) and, with channel 0
 *   only, detection probability and steps above threshold of the frame (:1224-1276).
 * `result` (may be NULL) receives the MOVs/DI/ODG after the last frame.
 * Pins the HIP pattern layer against the reference's own known-answer vectors
 * (testpeaq.c:433-599,748-810). */
#define PEAQ_DEBUG_BACKEND_DOUBLES 912
int peaq_debug_backend (peaq_ctx *ctx, int channels, int n_frames, const double *host_records,
                        double *host_out, peaq_result *result);

/* Host only, no device: self-check of the constant tables of the FP64 filter-bank engine.  Its long filters run
 * in a "block-sum" form (three rectangular windows per Hann window, running sums over 32-sample blocks: DESIGN.md 3);
 * the function evaluates that form and the direct tile of the short filters FROM THE TABLES on a pseudo-random
 * window and returns the largest deviation from the plain sums of fbearmodel.c:399-435, relative to each band's
 * largest output (about 4e-15).  tests/test_capi_host.py runs it on the CPU. */
double peaq_debug_fb_tables_selfcheck (void);

/* The advanced version's MOV layer on its own (fresh state): the filter-bank back end over
 *   fb_records  [n_blocks][channels][PEAQ_DEBUG_FB_RECORD_DOUBLES]   (as peaq_debug_filterbank returns them)
 * and the 55-band FFT back end over
 *   fft_records [n_frames][channels][PEAQ_DEBUG_RECORD_DOUBLES]      (as peaq_debug_frontend returns them for 55 bands),
 * every block's / frame's MOV values BEFORE accumulation -- also those the gates of gstpeaq.c:988,996-997 keep from
 * the accumulators:
 *   out_blocks [n_blocks][channels][PEAQ_DEBUG_ADV_BLOCK_DOUBLES] = { RmsModDiff (movs.c:205-254, RMS normalisation
 *              :243-244), its weight, the noise loudness of RmsNoiseLoudAsym and its missing-components term
 *              (movs.c:551-577), AvgLinDist (movs.c:679-706), total loudness of ref and test while the loudness
 *              gate is closed (earmodel.c:891-907; 0 afterwards), pad }
 *   out_frames [n_frames][channels][2] = { SegmentalNMR's 10 log10 of the mean band NMR (movs.c:1010-1020), that mean }
 * and the pair's result after the last block and frame. */
#define PEAQ_DEBUG_ADV_BLOCK_DOUBLES 8
int peaq_debug_backend_advanced (peaq_ctx *ctx, int channels, int n_blocks, const double *fb_records,
                                 int n_frames, const double *fft_records, double *out_blocks,
                                 double *out_frames, peaq_result *result);

/* The SHIPPED instantiations of the back ends on records, cut into launches (tests/test_gpu_backend_gates.py).
 * peaq_debug_backend and peaq_debug_backend_advanced run the debug instantiations, in one launch.  This entry runs
 * the kernels every product path runs -- no per-frame dump, no reading points, no trace -- from a fresh state:
 *   advanced == 0: fft_records [n_frames][channels][PEAQ_DEBUG_RECORD_DOUBLES] with 109 bands; n_blocks, fb_records
 *                  and blocks_per_launch are ignored (fb_records may be NULL)
 *   advanced != 0: fft_records with 55 bands and fb_records [n_blocks][channels][PEAQ_DEBUG_FB_RECORD_DOUBLES]
 * in launches of frames_per_launch frames (blocks_per_launch blocks; the last launch takes what is left).  Between
 * two launches everything the back end carries -- the accumulators' status and fields, the frame on which the
 * loudness gate opened, the filters' state -- goes through the pair's state in device memory, as it does between the
 * chunks of a batch and the windows of a session.  Then the read-out: only `result` (required) comes back.  A result
 * that depends on where the launches are cut is a bug in that hand-over. */
int peaq_debug_backend_plain (peaq_ctx *ctx, int advanced, int channels, int n_frames, const double *fft_records,
                              int frames_per_launch, int n_blocks, const double *fb_records, int blocks_per_launch,
                              peaq_result *result);

/* The primitives of csrc/peaq_wave.h on their own (tests/test_gpu_wave_primitives.py): the inline functions every
 * kernel is made of -- logarithm, exponential, quotient and roots, the wave reductions and scans, the lane moves,
 * the register DFTs -- called by one small kernel on host arrays.
 *   in  [planes_in][n]   host memory, plane p at in + p n
 *   out [planes_out][n]  likewise
 * The arrays are padded with 0. to whole workgroups of four waves, so every wave runs with all 64 lanes active.
 * Element-wise ops: out[i] = f(in[0][i] (, in[1][i])).  Cross-lane ops: every 64 consecutive elements are one wave
 * (lane = i & 63) and out[i] is what lane i holds afterwards -- 64 values per wave also where all lanes agree.
 * op (planes in -> out):
 *   "log_pos" "log_pos_sk" "log_nonneg" "log_nonneg_sk" "log_tab" "log_tab_nonneg" "exp_fast" "exp_fast_sk" "exp_tab"
 *   "sqrt_pos" "rsqrt_pos" (1 -> 1; _sk: the instantiation with its constants in scalar registers),
 *   "div_fast" (a, b), "pow_pos" (x, y), "pow_tab" = exp_tab(y log_tab(x)) and "pow_logtab" = exp_fast(y log_tab(x)),
 *   the two forms the back ends raise to a power with (2 -> 1),
 *   "log_nonneg_n5" "exp_fast_n5" (5 -> 5: plane k is element k of each lane's array of five),
 *   "wave_sum" "wave_max" "wave_prefix_sum" "lane_below" "lane_above" "read_lane_0" "read_lane_63" (1 -> 1),
 *   "wave_sum2" (2 -> 2), "wave_sum4" "rows_transpose4" (4 -> 4),
 *   "wave_suffix_geometric" "wave_prefix_geometric" "wave_prefix_geometric_f32" (1 -> 1, params[0] = m),
 *   "wave_prefix_geometric_z" (3 -> 3, params[0] = m: three scans in a row through the same pair of zero registers).
 *   The prefix forms get m, m^2 .. m^16 by repeated squaring and the row weight m^((lane & 15) + 1) by squaring and
 *   multiplying, as the filter bank's slope filter forms them (csrc/peaq_fb.hip); the FP32 form does the same in
 *   FP32 from (float)m and rounds its data to FP32.
 *   "dft4" "dft8" "dft16" (8, 16, 32 planes in and out: planes 2 k, 2 k + 1 are the real and imaginary part of x[k]).
 * PEAQ_ERR_ARG (before any device is touched) for an unknown op, a plane or parameter count other than the op's, and
 * NULL arguments. */
int peaq_debug_wave (peaq_ctx *ctx, const char *op, size_t n, int planes_in, const double *in,
                     int n_params, const double *params, int planes_out, double *out);

/* Host only, no device: the tables log_tab ([130][2]: 2 / C, ln C [- ln 2] per bin) and exp_tab ([64]: 2^(j/64)) that
 * every context uploads (csrc/peaq_device.h, CommonTables). */
int peaq_debug_common_tables (double *log_tab /* [260] */, double *exp_tab /* [64] */);

/* Host only, no device, no samples: the code that cuts a session's two streams into launches (csrc/peaq_host.h,
 * StreamFramer), run the way a session runs it -- push k adds n_samples[k] samples to pad[k] (0 = ref, 1 = test), and
 * after every push windows of at most max_frames FFT frames, then (advanced) of at most max_blocks filter-bank blocks,
 * are taken until nothing comes back; after the last push the stream is flushed.  pad[k] = -1 flushes in mid-stream
 * as well (n_samples[k] is ignored).  drain_every_push = 0 takes windows at the flushes only, with everything pushed
 * before still waiting -- a broker's session whose flush is requested before the ticks have caught up.  Every window
 * is one launch:
 *   windows[w] = { kind (0 = FFT frames, 1 = filter-bank blocks), first unit, units, valid samples on ref, on test }
 * where the valid samples fall short of whole units only in the zero-padded unit of the flush.  *n_windows is the
 * number of windows the stream has; the first max_windows of them are written (windows may be NULL if that is 0).
 * A session runs this with 64 / 120 units per launch, the broker with 8 / 48. */
#define PEAQ_DEBUG_STREAM_WINDOW_FIELDS 5
int peaq_debug_stream_plan (int advanced, unsigned max_frames, unsigned max_blocks, int drain_every_push,
                            size_t n_pushes, const int *pad, const uint64_t *n_samples, size_t max_windows,
                            uint64_t *windows, size_t *n_windows);

/* Host only, no device, no samples: what ONE slot of a broker contributes to its ticks -- the per-slot policy of the
 * tick (csrc/peaq_host.h, take_slot_windows) on a stream of one channel, under the broker's caps of 8 FFT frames and 48
 * filter-bank blocks a tick.  Event k: pad[k] = 0 or 1 pushes n_samples[k] samples to that pad (counted, not stored),
 * -1 requests a flush (peaq_broker_flush), -2 is one tick (n_samples[k] is ignored for both).  After the last event a
 * flush is requested if none is pending, and ticks run until one takes nothing and no flush is pending.  metered: the
 * slot's meter is on, which holds the blocks back behind the frames and, in the advanced version, adds a closing entry
 * when the blocks end without a flush block.
 *   rows[r] = { tick (from 0; every tick counts, also one that takes nothing), kind, first unit, units,
 *               valid samples on ref, on test }
 * kind 0 = FFT frames, 1 = filter-bank blocks, 2 = the meter's closing entry (first = the stream's block count, the
 * rest 0).  *n_rows is the number of rows; the first max_rows of them are written (rows may be NULL if that is 0). */
#define PEAQ_DEBUG_BROKER_PLAN_FIELDS 6
int peaq_debug_broker_plan (int advanced, int metered, size_t n_events, const int *pad, const uint64_t *n_samples,
                            size_t max_rows, uint64_t *rows, size_t *n_rows);

#ifdef __cplusplus
}
#endif
#endif /* PEAQ_AMD_H */

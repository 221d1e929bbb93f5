// peaq_kernels.h -- launch interfaces of the HIP kernels (host side sees plain
// functions; the kernels themselves live in the .hip files).
#pragma once
#include <hip/hip_runtime.h>

#include "peaq_device.h"

namespace peaq {

// ---- FFT ear-model front end -------------------------------------------------
struct FrontendArgs {
  const float* ref;             // [pair][pair_stride][channels] interleaved F32
  const float* test;
  size_t pair_stride;           // samples (per channel) between consecutive pairs
  const uint32_t* n_ref;        // per-pair lengths in samples per channel (device), or nullptr
  const uint32_t* n_test;
  uint32_t n_uniform_ref;       // lengths used when n_ref/n_test are null
  uint32_t n_uniform_test;
  const uint32_t* n_frames;     // per-pair total frame count (device), or nullptr
  uint32_t n_frames_uniform;
  // frame f starts at buffer sample (f - frame_origin) * 1024 + off_{ref,test}
  // (batch: all zero; sessions: the staging buffer holds a window of the stream)
  unsigned frame_origin;
  long long off_ref, off_test;
  int channels;
  unsigned frame0;              // first frame of this launch
  unsigned frames_per_launch;
  unsigned fpl_magic;           // ceil(2^32 / frames_per_launch): x / frames_per_launch = mulhi(x, magic), exact while
                                // x (magic d - 2^32) < 2^32 -- launch_frontend fills it in and refuses launches beyond that
  double level_factor;          // fftearmodel.c:312-313
  const CommonTables* common;
  const BandTables* bands;      // FFT model, 109 or 55 bands
  double* records;              // [pair][frame - frame0][channel][kRecDoubles]
  // Broker launches (many live sessions in one grid): every "pair" of the launch is a session
  // at its own position in its stream.  When set, pair p processes frames
  // [pair_frame0[p], pair_frame0[p] + pair_nframes[p]) and its buffer starts at that frame.
  const uint32_t* pair_frame0;
  const uint32_t* pair_nframes;
  // -DPEAQ_FE_PROFILE builds only (tools/fe_profile.py): [2 waves][16 phases] cycle sums + [32] wave count
  unsigned long long* prof;
  Settings cfg;                 // centre_ehs_window, ehs_dc_before_window
};
hipError_t launch_frontend(int bands, const FrontendArgs& a, unsigned n_pairs, hipStream_t stream);
// (109 bands: the one-wave kernel frontend_pair_kernel -- both signals of a frame in one wave --, unless
// PEAQ_AMD_FE=two_waves (read once) or select_frontend(1) asks for frontend_kernel<109>; select_frontend returns the
// previous override, -1: the environment decides)
int select_frontend(int two_waves);
// Most frames per launch for which the kernel's reciprocal multiplication is exact whatever the divisor:
// the error term magic d - 2^32 is below d and the dividend below n_pairs d, so n_pairs d^2 <= 2^32 is enough.
inline unsigned max_frames_per_launch(unsigned n_pairs) {
  unsigned long long d = 65535;
  while (d > 1 && (unsigned long long)(n_pairs ? n_pairs : 1) * d * d > (1ull << 32)) d >>= 1;
  return (unsigned)d;
}

// ---- reading points of a trajectory (peaq_batch_run_trajectory) ----------------
// Point k of pair p reads the state after F(a_k) FFT frames and B(a_k) filter-bank blocks,
// a_k = min((k + 1) interval, n_ref[p], n_test[p]).  A kernel argument of the points instantiations only: the
// argument blocks of the other launches keep their size and layout.
struct PointArgs {
  PointSnap* snap;              // [pair][n_points]
  const uint32_t* n_ref;        // per-pair lengths (device), or nullptr: n_uniform
  const uint32_t* n_test;
  uint32_t n_uniform;
  uint32_t interval;
  int n_points;
};

// ---- per-frame and per-block MOV traces (peaq_batch_run_trace) -------------------
// The records mirror peaq_frame_trace / peaq_block_trace in include/peaq_amd.h (peaq_batch.hip asserts the sizes and
// the flag values).  A kernel argument of the trace instantiations only, like PointArgs.
constexpr uint32_t kTraceAbove = 1u, kTraceModOpen = 2u, kTraceLoudOpen = 4u, kTraceFlush = 8u;
struct FrameTrace {             // 128 bytes = eight 16-byte stores
  double ch[2][6];
  double p_detect, steps;
  uint32_t flags, frame;
  double reserved;
};
struct BlockTrace {             // 96 bytes; ch[1] starts on an odd double
  double ch[2][5];
  uint32_t flags, block;
  double reserved;
};
struct TraceArgs {
  FrameTrace* frames;           // [pair][frame_stride], 16-byte aligned; record f of a pair at its ABSOLUTE frame index
                                // (as RunOutputs::live, the live instantiations: at its index within the LAUNCH, and
                                // the strides are the most units of a launch; the same holds for blocks)
  size_t frame_stride;
  BlockTrace* blocks;           // [pair][block_stride] (filter-bank back end)
  size_t block_stride;
  const uint32_t* n_ref;        // per-pair lengths (device), or nullptr: n_uniform -- the flush frame / block is the one
  const uint32_t* n_test;       // after the full ones of min(n_ref, n_test)
  uint32_t n_uniform;
};

// ---- per-band traces (peaq_batch_run_bands) ------------------------------------------
// The values the FFT back end has per (frame, channel, band) before it reduces them, stored where they come up.  The
// bits mirror PEAQ_BAND_* in include/peaq_amd.h (peaq_batch.hip asserts them).  A kernel argument of the bands
// instantiation only, like PointArgs and TraceArgs.
constexpr uint32_t kBandNmr = 1u, kBandExcRef = 2u, kBandExcTest = 4u, kBandDetect = 8u, kBandSteps = 16u;
constexpr uint32_t kBandAll = 31u, kBandAdvanced = kBandNmr | kBandExcRef;   // (the 55-band path has the first two)
constexpr int band_row(int bands) { return (bands + 1) & ~1; }                // doubles per row: 110 / 56
struct BandArgs {
  double* bands;                // [pair][frame_stride][channel][plane slot][band_row], 16-byte aligned; a pair's rows at
  size_t frame_stride;          // its ABSOLUTE frame index
  uint32_t planes;              // kBand* bits; the slot of a plane is the rank of its bit among the set ones
};

// ---- per-band traces of the pattern layer (peaq_batch_run_pattern_bands, basic version) --------
// The per-band terms of the modulation differences, their weight and the noise loudness, and the patterns they are made
// of, stored where they come up.  The bits mirror PEAQ_PAT_BAND_* in include/peaq_amd.h (peaq_batch.hip asserts them).
// A kernel argument of the pattern-bands instantiation only; rows and slots as BandArgs'.
constexpr uint32_t kPatBandModDiff1 = 0x1u, kPatBandModDiff2 = 0x2u, kPatBandModWt = 0x4u, kPatBandNoiseLoud = 0x8u,
                   kPatBandUnsmRef = 0x10u, kPatBandUnsmTest = 0x20u, kPatBandExcRef = 0x40u, kPatBandExcTest = 0x80u,
                   kPatBandAdaptRef = 0x100u, kPatBandAdaptTest = 0x200u, kPatBandModRef = 0x400u,
                   kPatBandModTest = 0x800u, kPatBandAvgLoudRef = 0x1000u, kPatBandAll = 0x1FFFu;
struct PatternBandArgs {
  double* bands;                // [pair][frame_stride][channel][plane slot][band_row (109)], 16-byte aligned
  size_t frame_stride;
  uint32_t planes;              // kPatBand* bits; the slot of a plane is the rank of its bit among the set ones
};

// ---- per-band summary (peaq_batch_run_band_summary) ---------------------------------------------
// The band values of the two traces above reduced over the pair's COUNTED frames (first .. last frame above the data
// boundary) where they come up: one row per quantity, band_row doubles, the row's denominator in its last entry.  The
// rows mirror PEAQ_BAND_SUMMARY_* in include/peaq_amd.h (peaq_batch.hip asserts them).  A kernel argument of the
// summary instantiation only, like BandArgs.
enum { kSumNmrSum, kSumNmrMax, kSumNmrDisturbed, kSumExcRef, kSumExcTest, kSumModDiff1, kSumModDiff2, kSumNoiseLoud };
constexpr int band_summary_rows(bool advanced) { return advanced ? 4 : 8; }   // (the 55-band path has the first four)
struct SummaryArgs {
  double* rows;                 // [pair][channel][rows][band_row], 16-byte aligned: the caller's array, and between the
                                // launches of a run the pair's running rows (loaded at entry, stored at exit)
  double* saved;                // the same shape (scratch): the rows as they were when the pair last turned tentative
};
// after a run's last back-end launch: a pair that ends tentative gets its saved rows back
hipError_t launch_summary_restore(const PairState* state, int advanced, const SummaryArgs& sum, unsigned n_pairs,
                                  unsigned pair_doubles, hipStream_t stream);

// ---- pattern back end (time smearing .. MOV accumulation) -------------------
struct BackendArgs {
  const double* records;        // as written by the front end
  unsigned frame0, frames_per_launch;
  const uint32_t* n_frames;
  uint32_t n_frames_uniform;
  int channels;
  int advanced;                 // 0: basic (109 bands, 11 MOVs); 1: FFT part of advanced (55 bands)
  const CommonTables* common;   // log_tab
  const BandTables* bands;
  PairState* state;             // [pair]
  // broker launches: per-pair frame window and state slot (see FrontendArgs)
  const uint32_t* pair_frame0;
  const uint32_t* pair_nframes;
  const uint32_t* pair_slot;    // state index of pair p (nullptr: p)
  double* debug;                // basic version only: [pair][frame - frame0][channel][kDbgDoubles], or nullptr
  Settings cfg;                 // floor_steps
  // batch launches only (nullptr otherwise): workgroup 0 adds the shader-clock ticks and the constant-rate ticks of
  // its own lifetime to clk[0], clk[1] -- the clock the device held while the step ran (peaq_batch_last_clock)
  unsigned long long* clk;
};
// (launch_backend: below, after RunOutputs)

// ---- read-out: accumulators -> MOVs -> DI -> ODG --------------------------------
struct ResultRecord {           // mirrors peaq_result in include/peaq_amd.h
  double movs[11];
  double di, odg, totalsnr, frames, fb_blocks;
};
hipError_t launch_finalize(const PairState* state, int advanced, int channels, unsigned n_pairs,
                           ResultRecord* out, hipStream_t stream, const Settings& cfg = Settings());   // clamp_movs
hipError_t launch_state_init(PairState* state, int advanced, unsigned n_pairs, hipStream_t stream);
// trajectories: every snapshot as state_init_kernel leaves a pair, and the read-out of n_pairs x n_points snapshots
hipError_t launch_points_init(PointSnap* snap, size_t n_snaps, hipStream_t stream);
hipError_t launch_finalize_points(const PointSnap* snap, int advanced, int channels, unsigned n_pairs, int n_points,
                                  ResultRecord* out, hipStream_t stream, const Settings& cfg);

// ---- advanced mode: filter-bank ear model ------------------------------------------
// Broker launches: "pair" p of the launch is a live session at its own position in its stream.
struct FbPairWindow {
  uint32_t block0;              // index of the session's first block of this launch (0 = its very first block)
  uint32_t n_blocks;            // blocks of this session in this launch
  uint32_t prev_blocks;         // n_blocks of the session's previous launch (where its history tail sits)
  uint32_t slot;                // index of the session's filter state, rows and PairState
};

struct FbFrontArgs {
  const float* ref;
  const float* test;
  size_t pair_stride;
  const uint32_t* n_ref;        // per-pair lengths (device) or nullptr
  const uint32_t* n_test;
  uint32_t n_uniform_ref, n_uniform_test;
  const uint32_t* n_blocks;     // per-pair total block count (device) or nullptr
  uint32_t n_blocks_uniform;
  // block b starts at buffer sample (b - block_origin) * 192 + off_{ref,test}
  unsigned block_origin;
  long long off_ref, off_test;
  int channels;
  unsigned block0, blocks_per_launch;
  unsigned launch_idx;          // running index of this launch (selects the peak slot, FbSignalState::peak_slot)
  unsigned prev_blocks;         // blocks_per_launch of the previous launch on these rows
  int first_launch;             // no history yet: the filter-bank delay line starts at zero
  double level_factor;          // fbearmodel.c:252-253
  const BandTables* bands;      // 40 bands
  const FbTables* fb;
  FbSignalState* fbstate;       // [pair][channel][2]
  double* hp_scratch;           // rows [signal][hp_row_stride]: 1456 history + filtered samples of the launch
  const double* hp_prev;        // rows of the previous launch (history source); nullptr: hp_scratch itself
  size_t hp_row_stride;
  double* records;              // [pair][block - block0][channel][kFbRecDoubles]
  const FbPairWindow* windows;  // broker launches (see above); nullptr: the uniform fields apply, slot = pair
  Settings cfg;                 // swap_slope
  int fir_fp64;                 // arithmetic of the FIR bank (peaq_fb.hip): 0 = v_mfma_f32, 1 = v_mfma_f64 (exact to the oracle's
                                // 1e-9), 2 = v_mfma_f32_16x16x32_f16 on operands split in two FP16 parts (three products per term)
  double hf_xscale, hf_xunscale;   // mode 2: power of two that puts the filtered signal's full scale at 2^10..2^11, and its inverse
};
hipError_t launch_fb_frontend(const FbFrontArgs& a, unsigned n_pairs, hipStream_t stream);   // high-pass + filter bank
hipError_t launch_fb_hp(const FbFrontArgs& a, unsigned n_pairs, hipStream_t stream);
hipError_t launch_fb_bank(const FbFrontArgs& a, unsigned n_pairs, hipStream_t stream);

struct FbBackendArgs {
  const double* records;
  unsigned block0, blocks_per_launch;
  const uint32_t* n_blocks;
  uint32_t n_blocks_uniform;
  int channels;
  const CommonTables* common;   // log_tab
  const BandTables* bands;
  PairState* state;
  const FbPairWindow* windows;  // broker launches
  Settings cfg;                 // swap_mod_patts
  // stage tests only (peaq_debug_backend_advanced): [pair][block - block0][channel][kDbgFbDoubles] -- the block's MOV
  // values before accumulation, computed for EVERY block in the debug instantiation -- or nullptr
  double* debug;
};
// ---- per-band traces of the filter-bank path (peaq_batch_run_fb_bands) ----------------------
// The values the filter-bank back end has per (block, channel, band) before it reduces them, stored where they come up.
// The bits mirror PEAQ_FB_BAND_* in include/peaq_amd.h (peaq_batch.hip asserts them).  A kernel argument of the
// filter-bank bands instantiation only, like PointArgs and TraceArgs.
constexpr uint32_t kFbBandModDiff = 0x1u, kFbBandModWt = 0x2u, kFbBandNoiseLoud = 0x4u, kFbBandMissing = 0x8u,
                   kFbBandLinDist = 0x10u, kFbBandUnsmRef = 0x20u, kFbBandUnsmTest = 0x40u, kFbBandExcRef = 0x80u,
                   kFbBandExcTest = 0x100u, kFbBandAdaptRef = 0x200u, kFbBandAdaptTest = 0x400u, kFbBandModRef = 0x800u,
                   kFbBandModTest = 0x1000u, kFbBandAll = 0x1FFFu;
struct FbBandArgs {
  double* bands;                // [pair][block_stride][channel][plane slot][kFbBands], 16-byte aligned; a pair's rows at
  size_t block_stride;          // its ABSOLUTE block index
  uint32_t planes;              // kFbBand* bits; the slot of a plane is the rank of its bit among the set ones
};

// ---- per-band summary of the filter-bank path (peaq_batch_run_fb_band_summary) --------------
// The term planes above reduced over the pair's COUNTED blocks (first .. last block above the data boundary) where they
// come up: one row per quantity, kFbSumRow doubles -- the 40 bands, the row's denominator, a zero.  The rows mirror
// PEAQ_FB_BAND_SUMMARY_* in include/peaq_amd.h (peaq_batch.hip asserts them).  A kernel argument of the filter-bank
// summary instantiation only, like FbBandArgs; the arrays work as SummaryArgs'.
enum { kFbSumExcRef, kFbSumExcTest, kFbSumModDiffW, kFbSumModDiffSq, kFbSumNoiseLoudSq, kFbSumMissingSq, kFbSumLinDist,
       kFbSumRows };
constexpr int kFbSumRow = 42;
struct FbSummaryArgs {
  double* rows;                 // [pair][channel][kFbSumRows][kFbSumRow], 16-byte aligned: the caller's array, and between
                                // the launches of a run the pair's running rows (loaded at entry, stored at exit)
  double* saved;                // the same shape (scratch): the rows as they were when the pair last turned tentative
};
// after a run's last filter-bank launch: a pair that ends tentative gets its saved rows back (summary_restore_kernel)
hipError_t launch_fb_summary_restore(const PairState* state, const FbSummaryArgs& fsum, unsigned n_pairs,
                                     unsigned pair_doubles, hipStream_t stream);

// ---- scores of time spans inside each pair (peaq_batch_run_windows, peaq_batch_run_adv_spans) ------------------------
// Span s of a pair -- a window of the basic version, a span of the advanced version -- covers FFT frames [first, end)
// (window_frames below: the device and peaq_window_frames use the one rule) and, in the advanced version, filter-bank
// blocks [first_b, end_b) (span_blocks below: the device and peaq_span_blocks use the one rule).  It is the read-out of
// the version's accumulators that start fresh before frame `first` / block `first_b` and are fed what the pair's own
// were fed in those units.  The feed is what the trace instantiations of the same run leave (scratch of the context) and
// the FFT front end's scalars; a span's accumulators sit in a PointSnap between the launches of a run.  A kernel
// argument of window_replay_kernel, span_replay_fft_kernel and span_replay_fb_kernel only (peaq_replay.hip).
struct WindowSpan { uint32_t start, length; };       // mirrors peaq_window in include/peaq_amd.h
struct SpanArgs {
  ResultRecord* out;            // [pair][n_spans]: where the read-out of the snapshots goes (the caller's d_windows / d_spans)
  PointSnap* snap;              // [pair][n_spans] (scratch)
  const WindowSpan* spans;      // [n_spans] (device), shared by all pairs
  int n_spans;
  const FrameTrace* frames;     // [pair][frame_stride] (scratch): record f of a pair at its absolute frame index
  size_t frame_stride;
  const BlockTrace* blocks;     // [pair][block_stride] (scratch): record b of a pair at its absolute block index;
  size_t block_stride;          // nullptr, 0 in the basic version
  const uint32_t* n_ref;        // per-pair lengths (device), or nullptr: n_uniform
  const uint32_t* n_test;
  uint32_t n_uniform;
};
// frames [first, end) of the span {start, length} of a pair with these lengths; T = count_frames of the pair
#if defined(__HIPCC__)
__host__ __device__
#endif
inline void window_frames(uint32_t n_ref, uint32_t n_test, uint32_t start, uint32_t length, uint32_t& first,
                          uint32_t& end) {
  const uint32_t n = n_ref < n_test ? n_ref : n_test, m = n_ref < n_test ? n_test : n_ref;
  const uint32_t full = n >= (uint32_t)kFrame ? (n - kFrame) / kHop + 1 : 0u;
  const uint32_t total = full + (m > (uint64_t)full * kHop ? 1u : 0u);
  const uint64_t e = (uint64_t)start + length;
  const uint32_t a0 = start < n ? start : n, a1 = e < n ? (uint32_t)e : n;
  first = start >= m ? total : a0 >= (uint32_t)kFrame ? (a0 - kFrame) / kHop + 1 : 0u;
  end = e >= m ? total : a1 >= (uint32_t)kFrame ? (a1 - kFrame) / kHop + 1 : 0u;
}
// blocks [first, end) of the span {start, length} of a pair with these lengths; B (a) = a / 192 is the trajectory's
// (PointWalk<true>::count), TB = count_frames (.., 192, 192) of the pair
#if defined(__HIPCC__)
__host__ __device__
#endif
inline void span_blocks(uint32_t n_ref, uint32_t n_test, uint32_t start, uint32_t length, uint32_t& first,
                        uint32_t& end) {
  const uint32_t n = n_ref < n_test ? n_ref : n_test, m = n_ref < n_test ? n_test : n_ref;
  const uint32_t full = n / (uint32_t)kFbFrame;
  const uint32_t total = full + (m > (uint64_t)full * kFbFrame ? 1u : 0u);
  const uint64_t e = (uint64_t)start + length;
  const uint32_t a0 = start < n ? start : n, a1 = e < n ? (uint32_t)e : n;
  first = start >= m ? total : a0 / (uint32_t)kFbFrame;
  end = e >= m ? total : a1 / (uint32_t)kFbFrame;
}
// after launch_backend (its trace instantiation) of the same chunk, on the same stream: frames [frame0, frame0 +
// frames_per_launch) of every pair replayed into the spans that meet them -- all eleven accumulators of the basic
// version; SegmentalNMR, EHS and the energies of the advanced version
hipError_t launch_span_replay_fft(const SpanArgs& spn, bool advanced, const double* records, unsigned frame0,
                                  unsigned frames_per_launch, int channels, unsigned n_pairs, hipStream_t stream);
// after launch_fb_backend (its trace instantiation) of the same chunk, on the same stream: blocks [block0, block0 +
// blocks_per_launch) of every pair replayed into RmsModDiff, RmsNoiseLoudAsym and AvgLinDist of the spans that meet them
hipError_t launch_span_replay_fb(const SpanArgs& spn, unsigned block0, unsigned blocks_per_launch, int channels,
                                 unsigned n_pairs, hipStream_t stream);

// ---- sliding-window scores of a live stream (peaq_session_set_meter, peaq_session_meter_read) ------------------------
// Window k of a stream covers FFT frames [k hop, k hop + window) and, in the advanced version, the filter-bank blocks
// [start_k / 192, e_k / 192) with start_k = k ? 1024 (k hop + 1) : 0 and e_k = 1024 (k hop + window + 1); a window that
// takes the stream's last frame takes the blocks to the last.  K = ceil (window / hop) windows are open at once, window
// k in slot k % K; a finished window's fields go to the delivered ring at k % ring_depth.  Each path (FFT frames,
// filter-bank blocks) writes the words of the snapshots that it owns, as the replays of peaq_replay.hip do.  The feed is
// what the live instantiations of the back ends leave: record u of a launch at [stream][u - first_unit].  A kernel
// argument of the three kernels of peaq_meter.hip only.
struct MeterArgs {
  PointSnap* open;              // [stream][k_open]: the open windows' fields between launches
  PointSnap* ring;              // [stream][ring_depth]: the delivered windows' fields
  uint32_t window, hop;         // W, H in frames
  uint32_t k_open, ring_depth;  // K = ceil (W / H) <= kMeterMaxOpen; the ring's slots
  const FrameTrace* frames;     // [stream][frame_stride], launch-relative (FFT kernels)
  size_t frame_stride;
  const BlockTrace* blocks;     // [stream][block_stride], launch-relative (filter-bank kernel)
  size_t block_stride;
  uint32_t unit0, n_units;      // the launch's units of the kernel's own path: [unit0, unit0 + n_units); n_units may be 0
  uint32_t total_frames;        // T, the stream's frames, once its flush is known; UINT_MAX before
  uint32_t total_units;         // the stream's units of the kernel's own path, once its flush is known; UINT_MAX before
  uint32_t rec_stride;          // FFT kernels: frames between the front end's records of consecutive streams of the launch
  // Broker launches (nullptr otherwise: the uniform fields above apply and stream p's snapshots are at index p): stream
  // p of the launch is a session at its own position, its snapshots at its slot.  The FFT kernels take the rows the
  // broker uploads for its back end, the filter-bank kernel its windows; n_units is clamped to the trace stride.
  const uint32_t* s_unit0;      // [stream] (pair_frame0)
  const uint32_t* s_nunits;     // [stream] (pair_nframes); may be 0
  const uint32_t* s_slot;       // [stream] (pair_slot)
  const FbPairWindow* s_win;    // [stream]: block0, n_blocks (may be 0), slot
  const uint32_t* s_total_frames;   // [stream]: total_frames of each stream
  const uint32_t* s_total_units;    // [stream]: total_units of each stream
};
constexpr uint32_t kMeterMaxOpen = 64, kMeterMaxDepth = 4096;
// after launch_backend (its live instantiation) of the same units, on the same stream: frames [unit0, unit0 + n_units)
// of every stream replayed into the windows that are open in them -- all eleven accumulators of the basic version;
// SegmentalNMR, EHS and the energies of the advanced version.  records: the FFT front end's of the launch.
hipError_t launch_meter_fft(const MeterArgs& m, bool advanced, const double* records, int channels, unsigned n_streams,
                            hipStream_t stream);
// after launch_fb_backend (its live instantiation): blocks [unit0, unit0 + n_units) into RmsModDiff, RmsNoiseLoudAsym
// and AvgLinDist of the windows that are open in them
hipError_t launch_meter_fb(const MeterArgs& m, int channels, unsigned n_streams, hipStream_t stream);

// ---- band rows of the meter's readings (peaq_session_set_meter_bands, peaq_session_meter_read_bands) -----------------
// Rows 0 .. 3 of the band summary (kSumNmrSum .. kSumExcRef) of every window of the meter, reduced over the window's
// COUNTED frames: the first .. the last of its frames above the data boundary, what accumulators that start fresh at
// the window's first frame count.  The feed is what the live-band instantiations of the FFT back end leave
// (RunOutputs::live_bnd): the planes NMR and EXC_REF of frame u of a launch at [stream][u - first unit], and the frame's
// flags in its trace record (MeterArgs::frames).  A kernel argument of meter_bands_kernel only (peaq_meter_bands.hip),
// beside the launch's MeterArgs, whose windows, units and per-stream rows it walks.
constexpr int kMeterBandRows = 4;
constexpr uint32_t kMeterBandsMaxOpen = 16, kMeterBandsMaxDepth = 256;
// doubles of one (open window, channel): the running rows, the saved rows, then the status word and its padding
constexpr int meter_band_snap(int bands) { return 2 * kMeterBandRows * band_row(bands) + 2; }
struct MeterBandArgs {
  const double* planes;         // [stream][MeterArgs::frame_stride][channel][2][band_row]: NMR, EXC_REF, launch-relative
  double* open;                 // [stream][k_open][channel][meter_band_snap]: the open windows between launches
  double* ring;                 // [stream][ring_depth][channel][kMeterBandRows][band_row]: the delivered windows' rows
};
// after launch_meter_fft of the same units, on the same stream, with the same MeterArgs
hipError_t launch_meter_bands(const MeterArgs& m, const MeterBandArgs& mb, bool advanced, int channels, unsigned n_streams,
                              hipStream_t stream);

// ---- delay watch of a live stream (peaq_session_set_align, peaq_session_watch_read; peaq_watch.hip) ----------------
// Watch window k of a stream covers the whole FFT frames [k W, (k + 1) W).  A frame's row: c[d + 31] for d = -31 .. 31,
// the sum of r[n] t[n + d] over the frame's own n = 512 .. 1535 (r, t: the mono sums in double), then e_ref and e_test,
// the sums of r[n]^2 and t[n]^2 over the same n.  A window's record is the sum of its frames' rows in frame order.
constexpr int kWatchLags = 31, kWatchCols = 2 * kWatchLags + 3;   // 63 lags and the two energies
constexpr int kWatchRow = 66;                    // doubles between rows (16-byte rows)
constexpr uint32_t kWatchMaxFrames = 65536;
struct WatchState {                              // per stream, on the device
  double acc[kWatchRow];                         // the window that is filling
  double latest[kWatchRow];                      // the newest complete window
  uint64_t index;                                // k of the window that is filling
  uint64_t latest_index;
  uint32_t count;                                // frames in acc, < W
  uint32_t latest_first, latest_frames;          // k W, W of `latest`; latest_frames 0: no window is complete yet
  uint32_t pad_;
};
struct WatchArgs {
  const float* ref;             // [stream][pair_stride][channels]: the staged samples the front end of the launch read,
  const float* test;            // frame f of the launch at sample 1024 f
  size_t pair_stride;
  int channels;
  uint32_t n_frames;            // whole frames of the launch (never the flush frame): of every stream, or with s_frames
                                // the most any stream has
  uint32_t window;              // W
  double* rows;                 // [stream][row_stride][kWatchRow]: scratch between the two kernels
  uint32_t row_stride;          // >= n_frames
  WatchState* state;            // [stream], or with s_slot [slot]
  // Broker launches (nullptr otherwise): stream p of the launch has its own count of whole frames, which may be 0 (its
  // unit of this tick is the flush frame), and its state at its slot -- rows the tick uploads
  const uint32_t* s_frames;     // [stream]
  const uint32_t* s_slot;       // [stream] (pair_slot)
};
// after launch_frontend of the same whole frames, on the same stream: delay_watch_frames_kernel, delay_watch_fold_kernel
// (a stream's state before its first frame is all zero bytes)
hipError_t launch_delay_watch(const WatchArgs& a, unsigned n_streams, hipStream_t stream);

// ---- the optional outputs of a run -------------------------------------------------------------
// What a run writes besides its results, host side: the kernel argument of each output by value, absent while its
// array is null.  The public entries of peaq_batch.hip fill in what the caller gave; batch_run_locked adds what only it
// knows (the device length arrays of `pts`, `trc` and `spn`, the snapshots, `sum.saved`).  A launch takes the whole aggregate
// and picks the instantiation; a metered session passes `live` alone, other sessions, the broker and the stage entries
// pass none.
struct RunOutputs {
  PointArgs pts{};              // trajectory (peaq_batch_run_trajectory): interval, n_points; snap from batch_run_locked
  ResultRecord* d_points = nullptr;   // [n_pairs][n_points]: where the read-out of the snapshots goes
  TraceArgs trc{};              // peaq_batch_run_trace
  BandArgs bnd{};               // peaq_batch_run_bands
  FbBandArgs fbnd{};            // peaq_batch_run_fb_bands
  PatternBandArgs pbd{};        // peaq_batch_run_pattern_bands
  SummaryArgs sum{};            // peaq_batch_run_band_summary
  FbSummaryArgs fsum{};         // peaq_batch_run_fb_band_summary
  SpanArgs spn{};               // peaq_batch_run_windows, peaq_batch_run_adv_spans: spans, n_spans, out; the rest from
                                // batch_run_locked, which points `trc` at the context's frame (and, in the advanced
                                // version, block) scratch: the replays' feed
  TraceArgs live{};             // a metered session's launches: the trace records, but record u of the launch at [launch
                                // index][u - first unit of the launch] -- the feed of peaq_meter.hip.  Stands alone.
  BandArgs live_bnd{};          // with `live` only (the band meter): the planes of a frame at the same launch-relative
                                // index, frame_stride the most frames of a launch -- the feed of peaq_meter_bands.hip
  bool has_live() const { return live.frames != nullptr || live.blocks != nullptr; }
  bool has_live_bnd() const { return live_bnd.bands != nullptr; }
  bool has_pts() const { return d_points != nullptr; }
  bool has_trc() const { return trc.frames != nullptr; }
  bool has_bnd() const { return bnd.bands != nullptr; }
  bool has_fbnd() const { return fbnd.bands != nullptr; }
  bool has_pbd() const { return pbd.bands != nullptr; }
  bool has_sum() const { return sum.rows != nullptr; }
  bool has_fsum() const { return fsum.rows != nullptr; }
  bool has_spn() const { return spn.out != nullptr; }
  bool any() const {
    return has_pts() || has_trc() || has_bnd() || has_fbnd() || has_pbd() || has_sum() || has_fsum() || has_spn() ||
           has_live() || has_live_bnd();
  }
};
// The instantiation of the FFT back end: summary, pattern bands, bands, trace, points, a.debug, plain -- the first
// that is present (out.fbnd and out.fsum are the other path's).  launch_backend in peaq_backend.hip has the table of what it refuses.
hipError_t launch_backend(const BackendArgs& a, unsigned n_pairs, hipStream_t stream, const RunOutputs& out = RunOutputs());
// The instantiation of the filter-bank back end: summary (out.fsum), bands (out.fbnd), trace, points, a.debug, plain --
// the first that is present (out.bnd, out.pbd and out.sum are the other path's: this one runs its plain kernels beside
// them).
hipError_t launch_fb_backend(const FbBackendArgs& a, unsigned n_pairs, hipStream_t stream,
                             const RunOutputs& out = RunOutputs());

// ---- synthetic workload --------------------------------------------------------------
hipError_t launch_synth(uint32_t seed0, unsigned n_pairs, int channels, uint32_t n_samples, size_t pair_stride,
                        float* ref, float* test, hipStream_t stream);

}  // namespace peaq

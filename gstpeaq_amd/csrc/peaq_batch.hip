// peaq_batch.hip -- the batch driver: N whole (ref, test) pairs resident in device memory (BASELINE.json configs
// 2-4), one pair from host memory, the timing of the last batch, the synthetic workload.
//
// Framing follows the reference element: FFT frames of 2048 samples every 1024
// (do_processing, gstpeaq.c:596-611), filter-bank blocks of 192 every 192, and
// at the end ONE zero-padded frame/block built from whatever is left on either
// side (do_flush, gstpeaq.c:716-745).  Frame f of a pair reads samples
// [1024 f, 1024 f + 2048) of each signal, zero beyond the signal's length.
#include "peaq_host.h"

using namespace peaq;

// ---------------------------------------------------------------------------
// batch
// ---------------------------------------------------------------------------
static const size_t kRecordBudget = (size_t)1536 << 20;   // HBM for per-frame records of one chunk
// Filter-bank blocks per launch (a multiple of the tile of 10) and the HBM one buffer of high-passed rows
// may take.  Long launches pay: per block the bank kernel costs 0.150 ms in launches of 320 blocks, 0.142 at
// 840 (fewer drained-CU tails, fewer pipeline hand-overs) -- 4096 stereo pairs x 10 s: 4.57 -> 4.74 M
// frame-pairs/s for 2 x 21 GB of rows + 18 GB of block records, small change on a 288 GB device.  Round 4, FP64
// engine, same job: 420 / 630 / 840 / 1250 blocks per launch = 5.14 / 5.19 / 5.20 / 5.26 M -- but 1250 means
// 2 x 32 GB of rows + 27 GB of records per context that has run such a batch, and a process with three contexts
// (the parity suite has) no longer leaves room for another process on the device: 840 stays.
#ifndef PEAQ_FB_CHUNK
#define PEAQ_FB_CHUNK 840
#endif
#ifndef PEAQ_FB_ROWGB
#define PEAQ_FB_ROWGB 24
#endif
static const unsigned kFbBlocksPerChunk = PEAQ_FB_CHUNK;
static const size_t kFbRowBudget = (size_t)PEAQ_FB_ROWGB << 30;

// blocks per launch of the filter-bank path: kFbBlocksPerChunk unless the batch is so large that the
// rows of that many blocks would not fit the budget; always a multiple of the tile (10 blocks)
unsigned fb_blocks_per_chunk(int n_pairs, int channels, uint32_t max_blocks) {
  const size_t n_signals = (size_t)n_pairs * channels * 2;
  const size_t per_signal = kFbRowBudget / std::max<size_t>(n_signals, 1) / sizeof(double);
  size_t bc = per_signal > (size_t)kFbRing ? (per_signal - kFbRing) / kFbFrame : 0;
  bc = std::min<size_t>(bc, kFbBlocksPerChunk) / 10 * 10;
  bc = std::max<size_t>(bc, 10);
  return static_cast<unsigned>(std::min<size_t>(bc, (max_blocks + 9) / 10 * 10));
}

unsigned frames_per_chunk(int n_pairs, int channels, uint32_t max_frames) {
  const size_t per_frame = (size_t)n_pairs * channels * kRecDoubles * sizeof(double);
  size_t fc = kRecordBudget / std::max<size_t>(per_frame, 1);
  fc = std::max<size_t>(fc, 4);
  fc = std::min<size_t>(fc, 64);
  // few pairs: take long chunks so that the launch count stays small
  if ((size_t)max_frames * per_frame <= ((size_t)256 << 20)) fc = max_frames;
  // the front end takes a work item apart with a 32-bit reciprocal of the frames per launch, exact up to
  // max_frames_per_launch (launch_frontend refuses more): a 30-minute mono file is two chunks, not one
  fc = std::min<size_t>(fc, max_frames_per_launch((unsigned)n_pairs));
  return static_cast<unsigned>(std::min<size_t>(fc, std::max<uint32_t>(max_frames, 1)));
}

extern "C" size_t peaq_batch_workspace_bytes(int advanced, int channels, int n_pairs, uint32_t n_max) {
  const uint32_t frames = count_frames(n_max, n_max, kFrame, kHop);
  const unsigned fc = frames_per_chunk(n_pairs, channels, frames);
  size_t b = 2 * (size_t)n_pairs * fc * channels * kRecDoubles * sizeof(double) + (size_t)n_pairs * sizeof(PairState) +
             (size_t)n_pairs * 4 * sizeof(uint32_t);
  if (advanced) {
    const unsigned bc = fb_blocks_per_chunk(n_pairs, channels, count_frames(n_max, n_max, kFbFrame, kFbFrame));
    const size_t nbuf = count_frames(n_max, n_max, kFbFrame, kFbFrame) > bc ? 2 : 1;   // pipelined: double buffers
    b += nbuf * (size_t)n_pairs * bc * channels * kFbRecDoubles * sizeof(double);
    b += (size_t)n_pairs * channels * 2 *
         (sizeof(FbSignalState) + nbuf * ((size_t)bc * kFbFrame + kFbRing) * sizeof(double));
  }
  return b;
}

static int run_filterbank_path(peaq_ctx* c, int channels, double level_db, int n_pairs, const float* d_ref,
                               const float* d_test, size_t pair_stride, const uint32_t* d_nref,
                               const uint32_t* d_ntest, uint32_t n_uniform, const uint32_t* d_nblocks,
                               uint32_t max_blocks, hipStream_t stream, hipEvent_t bank_gate, const RunOutputs& out) {
    // ---- filter-bank path: blocks of 192 samples (gstpeaq.c:648-652) ------------------
    const unsigned n_signals = (unsigned)n_pairs * channels * 2;
    const unsigned bc = fb_blocks_per_chunk(n_pairs, channels, max_blocks);
    const size_t row_stride = (size_t)kFbRing + (size_t)bc * kFbFrame;
    const bool piped = !PEAQ_DEV_SERIAL_KERNELS && max_blocks > bc;   // more than one chunk: 3-stage pipeline, double buffers
    HIP_TRY(c->hp_scratch.reserve((size_t)n_signals * row_stride * sizeof(double)));
    HIP_TRY(c->fb_records.reserve((size_t)n_pairs * bc * channels * kFbRecDoubles * sizeof(double)));
    if (piped) {
      HIP_TRY(c->hp_scratch2.reserve((size_t)n_signals * row_stride * sizeof(double)));
      HIP_TRY(c->fb_records2.reserve((size_t)n_pairs * bc * channels * kFbRecDoubles * sizeof(double)));
    }
    HIP_TRY(c->fbstate.reserve((size_t)n_signals * sizeof(FbSignalState)));
    HIP_TRY(hipMemsetAsync(c->fbstate.p, 0, (size_t)n_signals * sizeof(FbSignalState), stream));
    const ModelSetup m{c, c->settings, 1, channels, level_db};
    FbFrontArgs ff = m.fb_frontend();
    ff.ref = d_ref;
    ff.test = d_test;
    ff.pair_stride = pair_stride;
    ff.n_ref = d_nref;
    ff.n_test = d_ntest;
    ff.n_uniform_ref = ff.n_uniform_test = n_uniform;
    ff.n_blocks = d_nblocks;
    ff.n_blocks_uniform = max_blocks;
    ff.block_origin = 0;
    ff.fbstate = c->fbstate.as<FbSignalState>();
    ff.hp_row_stride = row_stride;
    FbBackendArgs fbk = m.fb_backend(ff);
    fbk.n_blocks = d_nblocks;
    fbk.n_blocks_uniform = max_blocks;
    fbk.state = c->state.as<PairState>();
    // Three stages per chunk of blocks, each on its own stream: the high-pass filter (a few hundred
    // waves, latency bound), the filter bank (the bulk), the back end (one workgroup per pair).
    // Stage s of chunk i runs beside stage s+1 of chunk i-1; rows and records are double buffered.
    hipStream_t s_hp = piped ? c->aux3 : stream, s_bank = stream, s_be = piped ? c->aux4 : stream;
    if (piped) {
      hipEvent_t ready = c->next_event();
      if (!ready) return fail(PEAQ_ERR_DEVICE, "hipEventCreate failed");
      HIP_TRY(hipEventRecord(ready, stream));          // state initialised, filter state cleared
      HIP_TRY(hipStreamWaitEvent(s_hp, ready, 0));
      HIP_TRY(hipStreamWaitEvent(s_be, ready, 0));
    }
    double* rows[2] = {c->hp_scratch.as<double>(), piped ? c->hp_scratch2.as<double>() : c->hp_scratch.as<double>()};
    double* recs[2] = {c->fb_records.as<double>(), piped ? c->fb_records2.as<double>() : c->fb_records.as<double>()};
    hipEvent_t bank_done[2] = {nullptr, nullptr}, be_done[2] = {nullptr, nullptr};
    unsigned prev = 0, chunk = 0;
    for (uint32_t b0 = 0; b0 < max_blocks; b0 += bc, ++chunk) {
      const unsigned nb = std::min<uint32_t>(bc, max_blocks - b0);
      const int b = chunk & 1;
      ff.block0 = b0;
      ff.blocks_per_launch = nb;
      ff.launch_idx = chunk;                             // (sessions, broker, stage entry points: one stream, always slot 0)
      ff.prev_blocks = prev;
      ff.first_launch = b0 == 0;
      ff.hp_scratch = rows[b];
      ff.hp_prev = chunk ? rows[b ^ 1] : nullptr;
      ff.records = recs[b];
      fbk.records = recs[b];
      fbk.block0 = b0;
      fbk.blocks_per_launch = nb;
      hipEvent_t e0 = c->next_event(), e1 = c->next_event(), e_hp = c->next_event(), e_be = c->next_event();
      if (!e0 || !e1 || !e_hp || !e_be) return fail(PEAQ_ERR_DEVICE, "hipEventCreate failed");
      if (piped) {
        if (bank_done[b]) HIP_TRY(hipStreamWaitEvent(s_hp, bank_done[b], 0));   // rows[b] no longer read
        if (be_done[b]) HIP_TRY(hipStreamWaitEvent(s_hp, be_done[b], 0));       // recs[b] no longer read
      }
      HIP_TRY(launch_fb_hp(ff, n_pairs, s_hp));
      if (piped) {
        HIP_TRY(hipEventRecord(e_hp, s_hp));
        HIP_TRY(hipStreamWaitEvent(s_bank, e_hp, 0));
      }
      if (chunk == 0 && bank_gate) HIP_TRY(hipStreamWaitEvent(s_bank, bank_gate, 0));   // (batch_run_locked: the FFT path's head)
      HIP_TRY(hipEventRecord(e0, s_bank));
      HIP_TRY(launch_fb_bank(ff, n_pairs, s_bank));
      HIP_TRY(hipEventRecord(e1, s_bank));
      bank_done[b] = e1;
      if (piped) HIP_TRY(hipStreamWaitEvent(s_be, e1, 0));
      HIP_TRY(launch_fb_backend(fbk, n_pairs, s_be, out));
      // (spans: this chunk's blocks into the spans that meet them, from the block records just written)
      if (out.has_spn()) HIP_TRY(launch_span_replay_fb(out.spn, b0, nb, channels, n_pairs, s_be));
      if (piped) {
        HIP_TRY(hipEventRecord(e_be, s_be));
        be_done[b] = e_be;
      }
      c->spans.push_back({e0, e1, 2});
      c->fb_last_bank_begin = e0;
      c->fb_last_bank_end = e1;
      prev = nb;
    }
    if (piped)
      for (int i = 0; i < 2; ++i)
        if (be_done[i]) HIP_TRY(hipStreamWaitEvent(stream, be_done[i], 0));    // join: `stream` ends the path
  return PEAQ_OK;
}

// The records and bits of include/peaq_amd.h are those of peaq_kernels.h: the public entries below hand the caller's
// arrays and masks to the kernels as they are.
static_assert(sizeof(peaq_result) == sizeof(ResultRecord), "peaq_result of include/peaq_amd.h and ResultRecord");
static_assert(sizeof(peaq_frame_trace) == 128 && sizeof(FrameTrace) == 128 && sizeof(peaq_block_trace) == 96 &&
                  sizeof(BlockTrace) == 96,
              "the trace records of include/peaq_amd.h and peaq_kernels.h");
static_assert(offsetof(peaq_frame_trace, flags) == offsetof(FrameTrace, flags) && offsetof(FrameTrace, flags) == 112 &&
                  offsetof(peaq_block_trace, flags) == offsetof(BlockTrace, flags) && offsetof(BlockTrace, flags) == 80,
              "the kernels store the records as eight / six 16-byte words");
static_assert(PEAQ_TRACE_ABOVE == kTraceAbove && PEAQ_TRACE_MOD_OPEN == kTraceModOpen &&
                  PEAQ_TRACE_LOUD_OPEN == kTraceLoudOpen && PEAQ_TRACE_FLUSH == kTraceFlush,
              "the flags of include/peaq_amd.h and peaq_kernels.h");
static_assert(PEAQ_BAND_NMR == kBandNmr && PEAQ_BAND_EXC_REF == kBandExcRef && PEAQ_BAND_EXC_TEST == kBandExcTest &&
                  PEAQ_BAND_DETECT == kBandDetect && PEAQ_BAND_STEPS == kBandSteps,
              "the planes of include/peaq_amd.h and peaq_kernels.h");
static_assert(PEAQ_FB_BAND_MODDIFF == kFbBandModDiff && PEAQ_FB_BAND_MODWT == kFbBandModWt &&
                  PEAQ_FB_BAND_NOISELOUD == kFbBandNoiseLoud && PEAQ_FB_BAND_MISSING == kFbBandMissing &&
                  PEAQ_FB_BAND_LINDIST == kFbBandLinDist && PEAQ_FB_BAND_UNSM_REF == kFbBandUnsmRef &&
                  PEAQ_FB_BAND_UNSM_TEST == kFbBandUnsmTest && PEAQ_FB_BAND_EXC_REF == kFbBandExcRef &&
                  PEAQ_FB_BAND_EXC_TEST == kFbBandExcTest && PEAQ_FB_BAND_ADAPT_REF == kFbBandAdaptRef &&
                  PEAQ_FB_BAND_ADAPT_TEST == kFbBandAdaptTest && PEAQ_FB_BAND_MOD_REF == kFbBandModRef &&
                  PEAQ_FB_BAND_MOD_TEST == kFbBandModTest,
              "the filter-bank planes of include/peaq_amd.h and peaq_kernels.h");
static_assert(PEAQ_PAT_BAND_MODDIFF1 == kPatBandModDiff1 && PEAQ_PAT_BAND_MODDIFF2 == kPatBandModDiff2 &&
                  PEAQ_PAT_BAND_MODWT == kPatBandModWt && PEAQ_PAT_BAND_NOISELOUD == kPatBandNoiseLoud &&
                  PEAQ_PAT_BAND_UNSM_REF == kPatBandUnsmRef && PEAQ_PAT_BAND_UNSM_TEST == kPatBandUnsmTest &&
                  PEAQ_PAT_BAND_EXC_REF == kPatBandExcRef && PEAQ_PAT_BAND_EXC_TEST == kPatBandExcTest &&
                  PEAQ_PAT_BAND_ADAPT_REF == kPatBandAdaptRef && PEAQ_PAT_BAND_ADAPT_TEST == kPatBandAdaptTest &&
                  PEAQ_PAT_BAND_MOD_REF == kPatBandModRef && PEAQ_PAT_BAND_MOD_TEST == kPatBandModTest &&
                  PEAQ_PAT_BAND_AVGLOUD_REF == kPatBandAvgLoudRef,
              "the pattern-band planes of include/peaq_amd.h and peaq_kernels.h");
static_assert(PEAQ_BAND_SUMMARY_NMR_SUM == kSumNmrSum && PEAQ_BAND_SUMMARY_NMR_MAX == kSumNmrMax &&
                  PEAQ_BAND_SUMMARY_NMR_DISTURBED == kSumNmrDisturbed && PEAQ_BAND_SUMMARY_EXC_REF_SUM == kSumExcRef &&
                  PEAQ_BAND_SUMMARY_EXC_TEST_SUM == kSumExcTest && PEAQ_BAND_SUMMARY_MODDIFF1_WSUM == kSumModDiff1 &&
                  PEAQ_BAND_SUMMARY_MODDIFF2_WSUM == kSumModDiff2 && PEAQ_BAND_SUMMARY_NOISELOUD_SUM == kSumNoiseLoud,
              "the summary rows of include/peaq_amd.h and peaq_kernels.h");
static_assert(PEAQ_FB_BAND_SUMMARY_EXC_REF_SUM == kFbSumExcRef && PEAQ_FB_BAND_SUMMARY_EXC_TEST_SUM == kFbSumExcTest &&
                  PEAQ_FB_BAND_SUMMARY_MODDIFF_WSUM == kFbSumModDiffW && PEAQ_FB_BAND_SUMMARY_MODDIFF_SQ == kFbSumModDiffSq &&
                  PEAQ_FB_BAND_SUMMARY_NOISELOUD_SQ == kFbSumNoiseLoudSq &&
                  PEAQ_FB_BAND_SUMMARY_MISSING_SQ == kFbSumMissingSq && PEAQ_FB_BAND_SUMMARY_LINDIST_SUM == kFbSumLinDist &&
                  kFbSumRows == 7 && kFbSumRow == kFbBands + 2,
              "the filter-bank summary rows of include/peaq_amd.h and peaq_kernels.h");

static_assert(sizeof(peaq_window) == sizeof(WindowSpan) && offsetof(peaq_window, length) == offsetof(WindowSpan, length),
              "peaq_window of include/peaq_amd.h and WindowSpan");

static int batch_run_locked(const char* who, peaq_ctx* c, int advanced, int channels, double level_db, int n_pairs,
                            const float* d_ref, const float* d_test, size_t pair_stride, const uint32_t* n_ref,
                            const uint32_t* n_test, uint32_t n_uniform, peaq_result* d_results, hipStream_t stream,
                            RunOutputs out);

// peaq_batch_run, peaq_batch_run_trajectory, peaq_batch_run_trace, peaq_batch_run_bands, peaq_batch_run_fb_bands,
// peaq_batch_run_pattern_bands, peaq_batch_run_band_summary, peaq_batch_run_fb_band_summary, peaq_batch_run_windows and
// peaq_batch_run_adv_spans: one driver, the points, the trace records, the band rows, the summary, the windows and the spans optional -- what `out` holds (`who` names the entry in messages)
static int batch_run_entry(const char* who, peaq_ctx* c, int advanced, int channels, double level_db, int n_pairs,
                           const float* d_ref, const float* d_test, size_t pair_stride, const uint32_t* n_ref,
                           const uint32_t* n_test, uint32_t n_uniform, peaq_result* d_results, void* stream_,
                           const RunOutputs& out) {
  const std::string w(who);
  if (!c) return fail(PEAQ_ERR_ARG, w + ": ctx is NULL");
  if (int rc = check_channels(w, channels)) return rc;
  if (n_pairs < 0) return fail(PEAQ_ERR_ARG, w + ": n_pairs < 0");
  if (n_pairs == 0) return PEAQ_OK;
  if (!d_ref || !d_test || (!d_results && !out.any())) return fail(PEAQ_ERR_ARG, w + ": NULL buffer");
  if ((n_ref == nullptr) != (n_test == nullptr))
    return fail(PEAQ_ERR_ARG, w + ": give both n_ref and n_test or neither");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  std::lock_guard<std::mutex> lock(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  if (c->batch_pending) {            // the workspace is still owned by the previous call
    HIP_TRY(hipEventSynchronize(c->batch_end));
    c->batch_pending = false;
  }
  c->spans.clear();
  c->events_used = 0;
  const int rc = batch_run_locked(who, c, advanced, channels, level_db, n_pairs, d_ref, d_test, pair_stride, n_ref,
                                  n_test, n_uniform, d_results, stream, out);
  if (rc != PEAQ_OK) {
    // part of the pipeline may already run on the context's own streams: nothing may touch the
    // workspace (or free it) before that work has drained
    const std::string msg = peaq_err_string();
    (void)hipDeviceSynchronize();
    c->batch_pending = false;
    return fail(rc, msg);
  }
  return PEAQ_OK;
}

extern "C" int peaq_batch_run(peaq_ctx* c, int advanced, int channels, double level_db, int n_pairs,
                              const float* d_ref, const float* d_test, size_t pair_stride, const uint32_t* n_ref,
                              const uint32_t* n_test, uint32_t n_uniform, peaq_result* d_results, void* stream_) {
  return batch_run_entry("peaq_batch_run", c, advanced, channels, level_db, n_pairs, d_ref, d_test, pair_stride, n_ref,
                         n_test, n_uniform, d_results, stream_, RunOutputs());
}

// ---- what the output entries check of their own arguments: no context, no device ----------------------------------
static int check_not_null(const std::string& w, const char* name, const void* p) {
  return p ? PEAQ_OK : fail(PEAQ_ERR_ARG, w + ": " + name + " is NULL");
}
// (with_address: the summary entry's message prints the pointer)
static int check_aligned(const std::string& w, const char* name, const void* p, bool with_address = false) {
  if (reinterpret_cast<uintptr_t>(p) % 16 == 0) return PEAQ_OK;
  char addr[32] = "";
  if (with_address) std::snprintf(addr, sizeof addr, " %p", const_cast<void*>(p));
  return fail(PEAQ_ERR_ARG, w + ": " + name + addr + " is not 16-byte aligned");
}
static int check_output(const std::string& w, const char* name, const void* p, bool with_address = false) {
  if (int rc = check_not_null(w, name, p)) return rc;
  return check_aligned(w, name, p, with_address);
}

// A stride of the caller's array held against the longest pair's count of FFT frames or of filter-bank blocks, made
// from the host's lengths.  (Lengths the common driver is going to refuse are left to it.)
static int check_stride(const std::string& w, const char* name, size_t stride, bool blocks, int n_pairs,
                        const uint32_t* n_ref, const uint32_t* n_test, uint32_t n_uniform) {
  if (n_pairs <= 0 || (n_ref == nullptr) != (n_test == nullptr)) return PEAQ_OK;
  const unsigned frame = blocks ? kFbFrame : kFrame, hop = blocks ? kFbFrame : kHop;
  uint32_t longest = 0;
  for (int p = 0; p < n_pairs; ++p) {
    longest = std::max(longest, count_frames(n_ref ? n_ref[p] : n_uniform, n_test ? n_test[p] : n_uniform, frame, hop));
    if (!n_ref) break;
  }
  if (stride < longest)
    return fail(PEAQ_ERR_ARG, w + ": " + name + " " + std::to_string(stride) + " is below the longest pair's " +
                                  std::to_string(longest) + (blocks ? " blocks" : " frames"));
  return PEAQ_OK;
}

// `planes` as a band entry takes it: bits of `all`, whose top bit `top` names; of these the advanced version of the
// FFT planes has `advanced_has` only.  0 or an error with the value in the message.
static int check_planes(const std::string& w, uint32_t planes, uint32_t all, const char* top,
                        uint32_t advanced_has = ~0u) {
  if (planes == 0) return fail(PEAQ_ERR_ARG, w + ": planes is 0 (no plane requested)");
  if (planes & ~all) return fail(PEAQ_ERR_ARG, w + ": planes " + std::to_string(planes) + " has a bit above " + top);
  if (planes & ~advanced_has)
    return fail(PEAQ_ERR_ARG, w + ": planes " + std::to_string(planes) +
                                  " asks for a plane the advanced version does not have (" +
                                  std::to_string(planes & ~advanced_has) +
                                  ": its 55-band path has PEAQ_BAND_NMR and PEAQ_BAND_EXC_REF only)");
  return PEAQ_OK;
}
int check_band_planes(const std::string& w, int advanced, uint32_t planes) {
  return check_planes(w, planes, kBandAll, "16 (PEAQ_BAND_STEPS)", advanced ? kBandAdvanced : ~0u);
}
int check_fb_band_planes(const std::string& w, uint32_t planes) {
  return check_planes(w, planes, kFbBandAll, "4096 (PEAQ_FB_BAND_MOD_TEST)");
}
int check_pattern_band_planes(const std::string& w, uint32_t planes) {
  return check_planes(w, planes, kPatBandAll, "4096 (PEAQ_PAT_BAND_AVGLOUD_REF)");
}

// What build_fft_band_tables and build_fb_band_tables build (host only: no context, no device), each once per process
// on its first use; `second` is the row the entry gives beside the centre frequencies.
enum BandSet { kBands109, kBands55, kBandsFb };
static int copy_band_tables(const char* who, BandSet set, double* fc, double* second,
                            const double (BandTables::*second_row)[kBandStride]) {
  if (!fc && !second) return fail(PEAQ_ERR_ARG, std::string(who) + ": NULL argument");
  static std::once_flag once[3];
  static std::unique_ptr<BandTables> tabs[3];
  std::call_once(once[set], [set] {
    tabs[set] = std::make_unique<BandTables>();
    if (set == kBandsFb) {
      auto fb = std::make_unique<FbTables>();          // (the bank's coefficients come with the bands; not kept)
      build_fb_band_tables(*tabs[set], *fb);
    } else {
      build_fft_band_tables(set == kBands109 ? 109 : 55, *tabs[set]);
    }
  });
  const BandTables& t = *tabs[set];
  for (int b = 0; b < t.bands; ++b) {
    if (fc) fc[b] = t.fc[b];
    if (second) second[b] = (t.*second_row)[b];
  }
  return PEAQ_OK;
}

// snapshot scratch of a trajectory; 0 when it does not fit size_t
static size_t trajectory_snap_bytes(int n_pairs, int n_points) {
  const size_t n = (size_t)std::max(n_pairs, 0) * (size_t)std::max(n_points, 0);
  return n > SIZE_MAX / sizeof(PointSnap) ? 0 : n * sizeof(PointSnap);
}

extern "C" int peaq_batch_run_trajectory(peaq_ctx* c, int advanced, int channels, double level_db, int n_pairs,
                                         const float* d_ref, const float* d_test, size_t pair_stride,
                                         const uint32_t* n_ref, const uint32_t* n_test, uint32_t n_uniform,
                                         uint32_t interval, int n_points, peaq_result* d_points,
                                         peaq_result* d_results, void* stream_) {
  // (the points' own arguments first: they need no context)
  if (interval == 0) return fail(PEAQ_ERR_ARG, "peaq_batch_run_trajectory: interval is 0");
  if (n_points < 1) return fail(PEAQ_ERR_ARG, "peaq_batch_run_trajectory: n_points < 1");
  if (!d_points) return fail(PEAQ_ERR_ARG, "peaq_batch_run_trajectory: d_points is NULL");
  if (n_pairs > 0 && trajectory_snap_bytes(n_pairs, n_points) == 0)
    return fail(PEAQ_ERR_NOMEM, "peaq_batch_run_trajectory: n_pairs x n_points snapshots exceed the address space");
  RunOutputs out;
  out.pts.interval = interval;
  out.pts.n_points = n_points;
  out.d_points = reinterpret_cast<ResultRecord*>(d_points);
  return batch_run_entry("peaq_batch_run_trajectory", c, advanced, channels, level_db, n_pairs, d_ref, d_test,
                         pair_stride, n_ref, n_test, n_uniform, d_results, stream_, out);
}

// The trace's own arguments first: they need no context (and no device: the strides are held against counts made
// from the host's lengths).
extern "C" int peaq_batch_run_trace(peaq_ctx* c, int advanced, int channels, double level_db, int n_pairs,
                                    const float* d_ref, const float* d_test, size_t pair_stride, const uint32_t* n_ref,
                                    const uint32_t* n_test, uint32_t n_uniform, peaq_frame_trace* d_frames,
                                    size_t frame_stride, peaq_block_trace* d_blocks, size_t block_stride,
                                    peaq_result* d_results, void* stream_) {
  const std::string w("peaq_batch_run_trace");
  if (int rc = check_not_null(w, "d_frames", d_frames)) return rc;
  if (advanced && !d_blocks) return fail(PEAQ_ERR_ARG, w + ": d_blocks is NULL (the advanced version writes block records)");
  if (!advanced && d_blocks) return fail(PEAQ_ERR_ARG, w + ": d_blocks must be NULL in the basic version (it has no filter-bank blocks)");
  if (int rc = check_aligned(w, "d_frames", d_frames)) return rc;
  if (int rc = check_aligned(w, "d_blocks", d_blocks)) return rc;
  if (int rc = check_stride(w, "frame_stride", frame_stride, false, n_pairs, n_ref, n_test, n_uniform)) return rc;
  if (advanced)
    if (int rc = check_stride(w, "block_stride", block_stride, true, n_pairs, n_ref, n_test, n_uniform)) return rc;
  RunOutputs out;
  out.trc.frames = reinterpret_cast<FrameTrace*>(d_frames);
  out.trc.frame_stride = frame_stride;
  out.trc.blocks = reinterpret_cast<BlockTrace*>(d_blocks);
  out.trc.block_stride = block_stride;
  return batch_run_entry("peaq_batch_run_trace", c, advanced, channels, level_db, n_pairs, d_ref, d_test, pair_stride,
                         n_ref, n_test, n_uniform, d_results, stream_, out);
}

// ---- band traces ----------------------------------------------------------------------------------------------
extern "C" int peaq_band_count(int advanced) { return advanced ? 55 : 109; }
extern "C" int peaq_band_row(int advanced) { return band_row(peaq_band_count(advanced)); }

extern "C" int peaq_band_tables(int advanced, double* fc, double* mask_diff) {
  return copy_band_tables("peaq_band_tables", advanced ? kBands55 : kBands109, fc, mask_diff, &BandTables::mask_diff);
}

// The band trace's own arguments first, as the trace's: they need no context and no device.
extern "C" int peaq_batch_run_bands(peaq_ctx* c, int advanced, int channels, double level_db, int n_pairs,
                                    const float* d_ref, const float* d_test, size_t pair_stride, const uint32_t* n_ref,
                                    const uint32_t* n_test, uint32_t n_uniform, uint32_t planes, double* d_bands,
                                    size_t frame_stride, peaq_result* d_results, void* stream_) {
  const std::string w("peaq_batch_run_bands");
  if (int rc = check_band_planes(w, advanced, planes)) return rc;
  if (int rc = check_output(w, "d_bands", d_bands)) return rc;
  if (int rc = check_stride(w, "frame_stride", frame_stride, false, n_pairs, n_ref, n_test, n_uniform)) return rc;
  RunOutputs out;
  out.bnd = {d_bands, frame_stride, planes};
  return batch_run_entry("peaq_batch_run_bands", c, advanced, channels, level_db, n_pairs, d_ref, d_test, pair_stride,
                         n_ref, n_test, n_uniform, d_results, stream_, out);
}

// ---- band traces of the filter-bank path ------------------------------------------------------------------------
extern "C" int peaq_fb_band_count(void) { return kFbBands; }

extern "C" int peaq_fb_band_tables(double* fc, double* internal_noise) {
  return copy_band_tables("peaq_fb_band_tables", kBandsFb, fc, internal_noise, &BandTables::internal_noise);
}

// The band trace's own arguments first, as peaq_batch_run_bands': they need no context and no device.
extern "C" int peaq_batch_run_fb_bands(peaq_ctx* c, int channels, double level_db, int n_pairs, const float* d_ref,
                                       const float* d_test, size_t pair_stride, const uint32_t* n_ref,
                                       const uint32_t* n_test, uint32_t n_uniform, uint32_t planes, double* d_bands,
                                       size_t block_stride, peaq_result* d_results, void* stream_) {
  const std::string w("peaq_batch_run_fb_bands");
  if (int rc = check_fb_band_planes(w, planes)) return rc;
  if (int rc = check_output(w, "d_bands", d_bands)) return rc;
  if (int rc = check_stride(w, "block_stride", block_stride, true, n_pairs, n_ref, n_test, n_uniform)) return rc;
  RunOutputs out;
  out.fbnd = {d_bands, block_stride, planes};
  return batch_run_entry("peaq_batch_run_fb_bands", c, 1, channels, level_db, n_pairs, d_ref, d_test, pair_stride, n_ref,
                         n_test, n_uniform, d_results, stream_, out);
}

// ---- band traces of the pattern layer (basic version) ----------------------------------------------------------
// (the 109 bands of peaq_band_tables(0, ...), with the internal noise beside the centre frequencies)
extern "C" int peaq_pattern_band_tables(double* fc, double* internal_noise) {
  return copy_band_tables("peaq_pattern_band_tables", kBands109, fc, internal_noise, &BandTables::internal_noise);
}

// The band trace's own arguments first, as peaq_batch_run_bands': they need no context and no device.
extern "C" int peaq_batch_run_pattern_bands(peaq_ctx* c, int channels, double level_db, int n_pairs, const float* d_ref,
                                            const float* d_test, size_t pair_stride, const uint32_t* n_ref,
                                            const uint32_t* n_test, uint32_t n_uniform, uint32_t planes,
                                            double* d_bands, size_t frame_stride, peaq_result* d_results,
                                            void* stream_) {
  const std::string w("peaq_batch_run_pattern_bands");
  if (int rc = check_pattern_band_planes(w, planes)) return rc;
  if (int rc = check_output(w, "d_bands", d_bands)) return rc;
  if (int rc = check_stride(w, "frame_stride", frame_stride, false, n_pairs, n_ref, n_test, n_uniform)) return rc;
  RunOutputs out;
  out.pbd = {d_bands, frame_stride, planes};
  return batch_run_entry("peaq_batch_run_pattern_bands", c, 0, channels, level_db, n_pairs, d_ref, d_test, pair_stride,
                         n_ref, n_test, n_uniform, d_results, stream_, out);
}

// ---- band summary ------------------------------------------------------------------------------------------------
extern "C" int peaq_band_summary_rows(int advanced) { return band_summary_rows(advanced != 0); }

// The summary's own argument first, as the band traces': it needs no context and no device.
extern "C" int peaq_batch_run_band_summary(peaq_ctx* c, int advanced, int channels, double level_db, int n_pairs,
                                           const float* d_ref, const float* d_test, size_t pair_stride,
                                           const uint32_t* n_ref, const uint32_t* n_test, uint32_t n_uniform,
                                           double* d_summary, peaq_result* d_results, void* stream_) {
  if (int rc = check_output("peaq_batch_run_band_summary", "d_summary", d_summary, true)) return rc;
  RunOutputs out;
  out.sum.rows = d_summary;
  return batch_run_entry("peaq_batch_run_band_summary", c, advanced ? 1 : 0, channels, level_db, n_pairs, d_ref, d_test,
                         pair_stride, n_ref, n_test, n_uniform, d_results, stream_, out);
}

// ---- band summary of the filter-bank path ---------------------------------------------------------------------
extern "C" int peaq_fb_band_summary_rows(void) { return kFbSumRows; }
extern "C" int peaq_fb_band_summary_row(void) { return kFbSumRow; }

// The summary's own argument first, as peaq_batch_run_band_summary's: it needs no context and no device.
extern "C" int peaq_batch_run_fb_band_summary(peaq_ctx* c, int channels, double level_db, int n_pairs,
                                              const float* d_ref, const float* d_test, size_t pair_stride,
                                              const uint32_t* n_ref, const uint32_t* n_test, uint32_t n_uniform,
                                              double* d_summary, peaq_result* d_results, void* stream_) {
  if (int rc = check_output("peaq_batch_run_fb_band_summary", "d_summary", d_summary, true)) return rc;
  RunOutputs out;
  out.fsum.rows = d_summary;
  return batch_run_entry("peaq_batch_run_fb_band_summary", c, 1, channels, level_db, n_pairs, d_ref, d_test, pair_stride,
                         n_ref, n_test, n_uniform, d_results, stream_, out);
}

extern "C" size_t peaq_trace_sizes(size_t* frame_bytes, size_t* block_bytes) {
  if (frame_bytes) *frame_bytes = sizeof(peaq_frame_trace);
  if (block_bytes) *block_bytes = sizeof(peaq_block_trace);
  return sizeof(peaq_frame_trace);
}

extern "C" size_t peaq_batch_trajectory_workspace_bytes(int advanced, int channels, int n_pairs, uint32_t n_max,
                                                        int n_points) {
  return peaq_batch_workspace_bytes(advanced, channels, n_pairs, n_max) + trajectory_snap_bytes(n_pairs, n_points);
}

// ---- scores of time windows inside each pair (basic version) -------------------------------------------------------
extern "C" int peaq_window_frames(uint32_t n_ref, uint32_t n_test, uint32_t start, uint32_t length, uint32_t* first,
                                  uint32_t* count) {
  if (!first && !count) return fail(PEAQ_ERR_ARG, "peaq_window_frames: NULL argument");
  uint32_t f = 0, e = 0;
  window_frames(n_ref, n_test, start, length, f, e);
  if (first) *first = f;
  if (count) *count = e - f;
  return PEAQ_OK;
}

// the scratch a windows or spans run adds to the plain run's: the frame records and (max_blocks: the advanced version's;
// 0 in the basic) the block records the replays read, the spans' snapshots, the spans themselves; 0 when it does not fit
// size_t
static size_t spans_scratch_bytes(bool advanced, int n_pairs, uint32_t max_frames, uint32_t max_blocks, int n_spans) {
  const size_t np = (size_t)std::max(n_pairs, 0), ns = (size_t)std::max(n_spans, 0);
  const size_t per_pair = (size_t)std::max<uint32_t>(max_frames, 1) * sizeof(FrameTrace) +
                          (advanced ? (size_t)std::max<uint32_t>(max_blocks, 1) * sizeof(BlockTrace) : 0) +
                          ns * sizeof(PointSnap);
  if (np && per_pair > (SIZE_MAX - ns * sizeof(WindowSpan)) / np) return 0;
  return np * per_pair + ns * sizeof(WindowSpan);
}

// The windows' own arguments first, as the traces': they need no context and no device.
extern "C" int peaq_batch_run_windows(peaq_ctx* c, int channels, double level_db, int n_pairs, const float* d_ref,
                                      const float* d_test, size_t pair_stride, const uint32_t* n_ref,
                                      const uint32_t* n_test, uint32_t n_uniform, const peaq_window* windows,
                                      int n_windows, peaq_result* d_windows, peaq_result* d_results, void* stream_) {
  const std::string w("peaq_batch_run_windows");
  if (int rc = check_span_list(w, "windows", "window", windows, n_windows, "d_windows", d_windows)) return rc;
  if (int rc = check_aligned(w, "d_windows", d_windows)) return rc;
  RunOutputs out;
  out.spn.out = reinterpret_cast<ResultRecord*>(d_windows);
  out.spn.spans = reinterpret_cast<const WindowSpan*>(windows);     // (host: batch_run_locked puts them on the device)
  out.spn.n_spans = n_windows;
  return batch_run_entry("peaq_batch_run_windows", c, 0, channels, level_db, n_pairs, d_ref, d_test, pair_stride, n_ref,
                         n_test, n_uniform, d_results, stream_, out);
}

extern "C" size_t peaq_batch_windows_workspace_bytes(int channels, int n_pairs, uint32_t n_max, int n_windows) {
  return peaq_batch_workspace_bytes(0, channels, n_pairs, n_max) +
         spans_scratch_bytes(false, n_pairs, count_frames(n_max, n_max, kFrame, kHop), 0, n_windows);
}

// ---- scores of time spans inside each pair (advanced version) ----------------------------------------------------
extern "C" int peaq_span_blocks(uint32_t n_ref, uint32_t n_test, uint32_t start, uint32_t length, uint32_t* first,
                                uint32_t* count) {
  if (!first && !count) return fail(PEAQ_ERR_ARG, "peaq_span_blocks: NULL argument");
  uint32_t f = 0, e = 0;
  span_blocks(n_ref, n_test, start, length, f, e);
  if (first) *first = f;
  if (count) *count = e - f;
  return PEAQ_OK;
}

// The spans' own arguments first, as the windows': they need no context and no device.
extern "C" int peaq_batch_run_adv_spans(peaq_ctx* c, int channels, double level_db, int n_pairs, const float* d_ref,
                                        const float* d_test, size_t pair_stride, const uint32_t* n_ref,
                                        const uint32_t* n_test, uint32_t n_uniform, const peaq_window* spans,
                                        int n_spans, peaq_result* d_spans, peaq_result* d_results, void* stream_) {
  const std::string w("peaq_batch_run_adv_spans");
  if (int rc = check_span_list(w, "spans", "span", spans, n_spans, "d_spans", d_spans)) return rc;
  if (int rc = check_aligned(w, "d_spans", d_spans)) return rc;
  RunOutputs out;
  out.spn.out = reinterpret_cast<ResultRecord*>(d_spans);
  out.spn.spans = reinterpret_cast<const WindowSpan*>(spans);       // (host: batch_run_locked puts them on the device)
  out.spn.n_spans = n_spans;
  return batch_run_entry("peaq_batch_run_adv_spans", c, 1, channels, level_db, n_pairs, d_ref, d_test, pair_stride, n_ref,
                         n_test, n_uniform, d_results, stream_, out);
}

extern "C" size_t peaq_batch_adv_spans_workspace_bytes(int channels, int n_pairs, uint32_t n_max, int n_spans) {
  return peaq_batch_workspace_bytes(1, channels, n_pairs, n_max) +
         spans_scratch_bytes(true, n_pairs, count_frames(n_max, n_max, kFrame, kHop),
                             count_frames(n_max, n_max, kFbFrame, kFbFrame), n_spans);
}

// One whole (ref, test) pair from host memory: the batch path with n_pairs = 1 -- for a caller that holds both
// files (the CLI).  The same frames and blocks as a session fed with the same samples (count_frames), but every
// kernel sees the whole stream: one front-end launch, the filter-bank path pipelined over its three streams.
// points != nullptr: peaq_run_pair_trajectory, n_points readings into host memory as well.
static int run_pair_host(const char* who, peaq_ctx* c, int advanced, int channels, double level_db, const float* ref,
                         size_t n_ref, const float* test, size_t n_test, uint32_t interval, int n_points,
                         peaq_result* points, peaq_result* out) {
  const std::string w(who);
  if (!c || (!out && !points)) return fail(PEAQ_ERR_ARG, w + ": NULL argument");
  if (int rc = check_channels(w, channels)) return rc;
  if ((n_ref && !ref) || (n_test && !test)) return fail(PEAQ_ERR_ARG, w + ": NULL samples");
  if (n_ref > 0xFFFFFFFFu || n_test > 0xFFFFFFFFu) return fail(PEAQ_ERR_ARG, w + ": more than 2^32 samples");
  HIP_TRY(hipSetDevice(c->device));
  size_t stride = std::max<size_t>(std::max(n_ref, n_test), 2);
  stride += stride & 1;                              // 8-byte rows: the frame loads are dword pairs
  DevBuf d_ref, d_test, d_res, d_pts;
  const size_t bytes = stride * channels * sizeof(float);
  HIP_TRY(d_ref.reserve(bytes));
  HIP_TRY(d_test.reserve(bytes));
  HIP_TRY(d_res.reserve(sizeof(peaq_result)));
  if (points) HIP_TRY(d_pts.reserve((size_t)n_points * sizeof(peaq_result)));
  HIP_TRY(hipMemset(d_ref.p, 0, bytes));
  HIP_TRY(hipMemset(d_test.p, 0, bytes));
  if (n_ref) HIP_TRY(hipMemcpy(d_ref.p, ref, n_ref * channels * sizeof(float), hipMemcpyHostToDevice));
  if (n_test) HIP_TRY(hipMemcpy(d_test.p, test, n_test * channels * sizeof(float), hipMemcpyHostToDevice));
  const uint32_t h_n[2] = {(uint32_t)n_ref, (uint32_t)n_test};    // peaq_batch_run takes the lengths as HOST arrays
  const int rc =
      points ? peaq_batch_run_trajectory(c, advanced, channels, level_db, 1, d_ref.as<float>(), d_test.as<float>(),
                                         stride, h_n, h_n + 1, 0, interval, n_points, d_pts.as<peaq_result>(),
                                         d_res.as<peaq_result>(), nullptr)
             : peaq_batch_run(c, advanced, channels, level_db, 1, d_ref.as<float>(), d_test.as<float>(), stride, h_n,
                              h_n + 1, 0, d_res.as<peaq_result>(), nullptr);
  if (rc != PEAQ_OK) return rc;
  HIP_TRY(hipDeviceSynchronize());
  if (out) HIP_TRY(hipMemcpy(out, d_res.p, sizeof(peaq_result), hipMemcpyDeviceToHost));
  if (points) HIP_TRY(hipMemcpy(points, d_pts.p, (size_t)n_points * sizeof(peaq_result), hipMemcpyDeviceToHost));
  return PEAQ_OK;
}

extern "C" int peaq_run_pair(peaq_ctx* c, int advanced, int channels, double level_db, const float* ref, size_t n_ref,
                             const float* test, size_t n_test, peaq_result* out) {
  if (!out) return fail(PEAQ_ERR_ARG, "peaq_run_pair: NULL argument");
  return run_pair_host("peaq_run_pair", c, advanced, channels, level_db, ref, n_ref, test, n_test, 0, 0, nullptr, out);
}

extern "C" int peaq_run_pair_trajectory(peaq_ctx* c, int advanced, int channels, double level_db, const float* ref,
                                        size_t n_ref, const float* test, size_t n_test, uint32_t interval,
                                        int n_points, peaq_result* points, peaq_result* out) {
  if (interval == 0) return fail(PEAQ_ERR_ARG, "peaq_run_pair_trajectory: interval is 0");
  if (n_points < 1) return fail(PEAQ_ERR_ARG, "peaq_run_pair_trajectory: n_points < 1");
  if (!points) return fail(PEAQ_ERR_ARG, "peaq_run_pair_trajectory: points is NULL");
  return run_pair_host("peaq_run_pair_trajectory", c, advanced, channels, level_db, ref, n_ref, test, n_test, interval,
                       n_points, points, out);
}

static int batch_run_locked(const char* who, peaq_ctx* c, int advanced, int channels, double level_db, int n_pairs,
                            const float* d_ref, const float* d_test, size_t pair_stride, const uint32_t* n_ref,
                            const uint32_t* n_test, uint32_t n_uniform, peaq_result* d_results, hipStream_t stream,
                            RunOutputs out) {

  // ---- frame counts -------------------------------------------------------------------
  uint32_t max_frames = 0, max_blocks = 0;
  const uint32_t* d_nref = nullptr;
  const uint32_t* d_ntest = nullptr;
  const uint32_t* d_nframes = nullptr;
  const uint32_t* d_nblocks = nullptr;
  if (n_ref) {
    std::vector<uint32_t> h(4 * (size_t)n_pairs);
    for (int p = 0; p < n_pairs; ++p) {
      if (n_ref[p] > pair_stride || n_test[p] > pair_stride)
        return fail(PEAQ_ERR_ARG, std::string(who) + ": a pair is longer than pair_stride");
      h[p] = n_ref[p];
      h[n_pairs + p] = n_test[p];
      h[2 * (size_t)n_pairs + p] = count_frames(n_ref[p], n_test[p], kFrame, kHop);
      h[3 * (size_t)n_pairs + p] = count_frames(n_ref[p], n_test[p], kFbFrame, kFbFrame);
      max_frames = std::max(max_frames, h[2 * (size_t)n_pairs + p]);
      max_blocks = std::max(max_blocks, h[3 * (size_t)n_pairs + p]);
    }
    HIP_TRY(c->counts.reserve(h.size() * sizeof(uint32_t)));
    HIP_TRY(hipMemcpyAsync(c->counts.p, h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));      // h goes out of scope
    d_nref = c->counts.as<uint32_t>();
    d_ntest = d_nref + n_pairs;
    d_nframes = d_nref + 2 * (size_t)n_pairs;
    d_nblocks = d_nref + 3 * (size_t)n_pairs;
  } else {
    if (n_uniform > pair_stride)
      return fail(PEAQ_ERR_ARG, std::string(who) + ": n_uniform > pair_stride");
    max_frames = count_frames(n_uniform, n_uniform, kFrame, kHop);
    max_blocks = count_frames(n_uniform, n_uniform, kFbFrame, kFbFrame);
  }

  const unsigned fc = frames_per_chunk(n_pairs, channels, max_frames);
  const size_t rec_bytes = (size_t)n_pairs * fc * channels * kRecDoubles * sizeof(double);
  HIP_TRY(c->records.reserve(rec_bytes));
  HIP_TRY(c->records2.reserve(rec_bytes));
  HIP_TRY(c->state.reserve((size_t)n_pairs * sizeof(PairState)));
  // The band rows (FFT, filter bank, pattern layer) arrive complete: the back end that has them writes the caller's rows
  // directly and the other path runs its plain kernels.  What only this function knows of the other outputs:
  // trajectory: the snapshots of the reading points, [pair][point] (the back ends write them, finalize_points reads them)
  const size_t n_snaps = out.has_pts() ? (size_t)n_pairs * out.pts.n_points : 0;
  if (out.has_pts()) {
    HIP_TRY(c->snaps.reserve(n_snaps * sizeof(PointSnap)));
    out.pts.snap = c->snaps.as<PointSnap>();
    out.pts.n_ref = d_nref;
    out.pts.n_test = d_ntest;
    out.pts.n_uniform = n_uniform;
  }
  // trace: the back ends write the caller's record arrays directly -- no scratch of its own
  if (out.has_trc()) {
    out.trc.n_ref = d_nref;
    out.trc.n_test = d_ntest;
    out.trc.n_uniform = n_uniform;
  }
  // windows (basic version) and spans (advanced version): every launch of the back end(s) is the trace instantiation,
  // writing frame records -- and the filter-bank back end block records -- into scratch of the context, and is followed
  // on its own stream by the replay of its units into the spans' snapshots (peaq_replay.hip).  All of it is reserved
  // here, so that running out of memory is reported before anything is enqueued.
  const size_t n_ssnaps = out.has_spn() ? (size_t)n_pairs * out.spn.n_spans : 0;
  if (out.has_spn()) {
    if (out.has_trc() || out.has_pts() || out.has_bnd() || out.has_fbnd() || out.has_pbd() || out.has_sum() ||
        out.has_fsum())
      return fail(PEAQ_ERR_ARG, std::string(who) + (advanced ? ": spans are a run of their own, of the advanced version"
                                                             : ": windows are a run of their own, of the basic version"));
    if (spans_scratch_bytes(advanced, n_pairs, max_frames, max_blocks, out.spn.n_spans) == 0)
      return fail(PEAQ_ERR_NOMEM, std::string(who) + (advanced ? ": the spans' scratch exceeds the address space"
                                                               : ": the windows' scratch exceeds the address space"));
    const size_t frame_stride = std::max<uint32_t>(max_frames, 1);
    const size_t block_stride = advanced ? std::max<uint32_t>(max_blocks, 1) : 0;
    HIP_TRY(c->spn_frames.reserve((size_t)n_pairs * frame_stride * sizeof(FrameTrace)));
    if (advanced) HIP_TRY(c->spn_blocks.reserve((size_t)n_pairs * block_stride * sizeof(BlockTrace)));
    HIP_TRY(c->snaps.reserve(n_ssnaps * sizeof(PointSnap)));
    HIP_TRY(c->spn_list.reserve((size_t)out.spn.n_spans * sizeof(WindowSpan)));
    HIP_TRY(hipMemcpyAsync(c->spn_list.p, out.spn.spans, (size_t)out.spn.n_spans * sizeof(WindowSpan),
                           hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));           // the caller's array is read by now
    out.trc = TraceArgs{c->spn_frames.as<FrameTrace>(), frame_stride, advanced ? c->spn_blocks.as<BlockTrace>() : nullptr,
                        block_stride, d_nref, d_ntest, n_uniform};
    out.spn.spans = c->spn_list.as<WindowSpan>();
    out.spn.snap = c->snaps.as<PointSnap>();
    out.spn.frames = out.trc.frames;
    out.spn.frame_stride = frame_stride;
    out.spn.blocks = out.trc.blocks;
    out.spn.block_stride = block_stride;
    out.spn.n_ref = d_nref;
    out.spn.n_test = d_ntest;
    out.spn.n_uniform = n_uniform;
  }
  // band summary: every FFT back-end launch of the run is the summary instantiation.  The caller's rows start from zero
  // and carry the running sums from launch to launch; the copy a pair takes when it turns tentative goes to scratch of
  // the same shape (reserved here, so that running out of memory is reported before anything is enqueued).
  const size_t sum_pair_doubles = (size_t)channels * band_summary_rows(advanced != 0) * band_row(advanced ? 55 : 109);
  if (out.has_sum()) {
    HIP_TRY(c->sum_saved.reserve((size_t)n_pairs * sum_pair_doubles * sizeof(double)));
    out.sum.saved = c->sum_saved.as<double>();
  }
  // ... and the filter-bank summary likewise with the filter-bank back end's launches; a run has one of the two
  // summaries (launch_fb_backend refuses both), so the saved copy is the same buffer
  const size_t fsum_pair_doubles = (size_t)channels * kFbSumRows * kFbSumRow;
  if (out.has_fsum()) {
    HIP_TRY(c->sum_saved.reserve((size_t)n_pairs * fsum_pair_doubles * sizeof(double)));
    out.fsum.saved = c->sum_saved.as<double>();
  }

  HIP_TRY(hipEventRecord(c->batch_begin, stream));
  HIP_TRY(launch_state_init(c->state.as<PairState>(), advanced, n_pairs, stream));
  if (out.has_sum()) HIP_TRY(hipMemsetAsync(out.sum.rows, 0, (size_t)n_pairs * sum_pair_doubles * sizeof(double), stream));
  if (out.has_fsum())                                // (before the fork below: the filter-bank path's stream waits for it)
    HIP_TRY(hipMemsetAsync(out.fsum.rows, 0, (size_t)n_pairs * fsum_pair_doubles * sizeof(double), stream));
  if (out.has_pts()) HIP_TRY(launch_points_init(out.pts.snap, n_snaps, stream));   // (before the fork: both paths write snapshots)
  if (out.has_spn()) HIP_TRY(launch_points_init(out.spn.snap, n_ssnaps, stream));   // every span starts fresh (before the fork: both replays write snapshots)
  hipEvent_t fb_done = nullptr, forked = nullptr;
  c->fb_last_bank_begin = c->fb_last_bank_end = nullptr;
  const bool with_fb = advanced && max_blocks > 0;
  if (with_fb) {
    // the filter-bank path (its own ear model, accumulators 0, 1, 4) is independent of the FFT
    // path (accumulators 2, 3): it runs on a third stream from here on and joins at the end
    forked = c->next_event();
    if (!forked) return fail(PEAQ_ERR_DEVICE, "hipEventCreate failed");
    HIP_TRY(hipEventRecord(forked, stream));
    HIP_TRY(hipStreamWaitEvent(c->aux2, forked, 0));
  }
  // (its launches are issued further down, between the FFT path's head and the rest of its chunks)
  auto issue_filterbank_path = [&](hipEvent_t bank_gate) -> int {
    hipStream_t s_fb = PEAQ_DEV_SERIAL_KERNELS ? stream : c->aux2;
    const int rc = run_filterbank_path(c, channels, level_db, n_pairs, d_ref, d_test, pair_stride, d_nref, d_ntest,
                                       n_uniform, d_nblocks, max_blocks, s_fb, bank_gate, out);
    if (rc != PEAQ_OK) return rc;
    fb_done = c->next_event();
    if (!fb_done) return fail(PEAQ_ERR_DEVICE, "hipEventCreate failed");
    HIP_TRY(hipEventRecord(fb_done, s_fb));
    return PEAQ_OK;
  };

  const ModelSetup m{c, c->settings, advanced ? 1 : 0, channels, level_db};
  FrontendArgs fa = m.frontend();
  fa.ref = d_ref;
  fa.test = d_test;
  fa.pair_stride = pair_stride;
  fa.n_ref = d_nref;
  fa.n_test = d_ntest;
  fa.n_uniform_ref = n_uniform;
  fa.n_uniform_test = n_uniform;
  fa.n_frames = d_nframes;
  fa.n_frames_uniform = max_frames;
  fa.frame_origin = 0;
  fa.off_ref = 0;
  fa.off_test = 0;
  BackendArgs ba = m.backend(fa);
  ba.n_frames = d_nframes;
  ba.n_frames_uniform = max_frames;
  ba.state = c->state.as<PairState>();
  HIP_TRY(c->clk.reserve(2 * sizeof(unsigned long long)));
  HIP_TRY(hipMemsetAsync(c->clk.p, 0, 2 * sizeof(unsigned long long), stream));   // (the first back-end launch waits for this stream)
  ba.clk = c->clk.as<unsigned long long>();

  // Software pipeline over chunks of frames: the front end of chunk i+1 (throughput bound,
  // millions of workgroups) runs on the caller's stream while the back end of chunk i
  // (one workgroup per pair, latency bound) runs on the context's second stream; the
  // per-frame records are double buffered.
  hipEvent_t back_done[2] = {nullptr, nullptr}, head_done = nullptr;
  unsigned chunk = 0;
  // Advanced version: the last chunks of the FFT path are held back until the filter-bank path's last bank launch
  // is through.  An advanced pass ends with that launch's back end alone on the device (one workgroup per pair walking
  // 840 blocks: 12 ms at a fraction of the machine) while all FFT chunks, ready from the start, have long run beside
  // the FIRST bank launch and slowed it by their own time; two chunks of frontend_kernel<55> are about what the tail
  // has room for (profiles/r05_timeline_adv.txt).  PEAQ_AMD_ADV_DEFER=<chunks>[b] (development): other counts; "b" =
  // wait for the last bank launch's begin instead of its end.
  const unsigned n_chunks = fc ? (max_frames + fc - 1) / fc : 0u;   // (a pair of two empty signals has no frames at all)
  static const int defer_env = [] { const char* e = std::getenv("PEAQ_AMD_ADV_DEFER"); return e && *e ? std::atoi(e) : -1; }();
  static const bool defer_begin = [] { const char* e = std::getenv("PEAQ_AMD_ADV_DEFER"); return e && std::strchr(e, 'b'); }();
  const bool fb_piped = with_fb && !PEAQ_DEV_SERIAL_KERNELS;
  const unsigned defer = !fb_piped ? 0u : std::min<unsigned>(defer_env >= 0 ? (unsigned)defer_env : 2u, n_chunks > 4 ? n_chunks - 4 : 0u);
  // ... and with the FP64 bank the FIRST bank launch waits for the front end of all chunks before those (the head).
  // Two workgroups of fb_bank_kernel<MfmaF64> fill a CU's registers and LDS: whatever runs beside it does so in place
  // of one of them, and then neither kernel has the waves to cover its latencies -- beside the first bank launch a chunk
  // of frontend_kernel<55> took 33 .. 39 ms, alone it takes 6.6 (profiles/r05_timeline_adv.txt: before / after).  The
  // first two walks of the high-pass filter, which the bank has to wait for anyway, run beside the head.  Measured:
  // 5.38 M -> 5.47 M; the reduced-precision engine, whose bank kernel leaves room beside it, loses 0.6 % and keeps
  // the old order.  PEAQ_AMD_ADV_HEAD=<chunks> (development): other counts.
  static const int head_env = [] { const char* e = std::getenv("PEAQ_AMD_ADV_HEAD"); return e && *e ? std::atoi(e) : -1; }();
  const unsigned head = !fb_piped ? 0u : std::min<unsigned>(head_env >= 0 ? (unsigned)head_env : (c->fir_fp64 == PEAQ_FIR_F64 ? n_chunks : 0u), n_chunks - defer);
  auto issue_chunk = [&](uint32_t f0) -> int {
    const unsigned nf = std::min<uint32_t>(fc, max_frames - f0);
    if (defer && chunk == n_chunks - defer)
      HIP_TRY(hipStreamWaitEvent(stream, defer_begin ? c->fb_last_bank_begin : c->fb_last_bank_end, 0));
    double* recs = (chunk & 1) ? c->records2.as<double>() : c->records.as<double>();
    fa.frame0 = f0;
    fa.frames_per_launch = nf;
    fa.records = recs;
    ba.frame0 = f0;
    ba.frames_per_launch = nf;
    ba.records = recs;
    hipEvent_t e0 = c->next_event(), e1 = c->next_event(), e2 = c->next_event(), e3 = c->next_event();
    if (!e0 || !e1 || !e2 || !e3) return fail(PEAQ_ERR_DEVICE, "hipEventCreate failed");
    if (back_done[chunk & 1]) HIP_TRY(hipStreamWaitEvent(stream, back_done[chunk & 1], 0));   // buffer free again
    HIP_TRY(hipEventRecord(e0, stream));
    HIP_TRY(launch_frontend(m.fft_bands(), fa, n_pairs, stream));
    HIP_TRY(hipEventRecord(e1, stream));
    HIP_TRY(hipStreamWaitEvent(c->aux, e1, 0));
    HIP_TRY(hipEventRecord(e2, c->aux));
    if (!PEAQ_DEV_SKIP_BACKEND) HIP_TRY(launch_backend(ba, n_pairs, c->aux, out));
    // (windows and spans: this chunk's frames into the spans that meet them, from the trace records just written and
    // from `recs` -- which e3 below keeps from being reused before the replay has read it)
    if (!PEAQ_DEV_SKIP_BACKEND && out.has_spn())
      HIP_TRY(launch_span_replay_fft(out.spn, advanced != 0, recs, f0, nf, channels, n_pairs, c->aux));
    HIP_TRY(hipEventRecord(e3, c->aux));
    back_done[chunk & 1] = e3;
    head_done = e1;
    c->spans.push_back({e0, e1, 0});
    c->spans.push_back({e2, e3, 1});
    return PEAQ_OK;
  };
  uint32_t f0 = 0;
  for (; chunk < head; f0 += fc, ++chunk) {
    const int rc = issue_chunk(f0);
    if (rc != PEAQ_OK) return rc;
  }
  if (with_fb) {
    const int rc = issue_filterbank_path(head ? head_done : nullptr);
    if (rc != PEAQ_OK) return rc;
  }
  for (; f0 < max_frames; f0 += fc, ++chunk) {
    const int rc = issue_chunk(f0);
    if (rc != PEAQ_OK) return rc;
  }
  for (int i = 0; i < 2; ++i)
    if (back_done[i]) HIP_TRY(hipStreamWaitEvent(stream, back_done[i], 0));
  if (fb_done) HIP_TRY(hipStreamWaitEvent(stream, fb_done, 0));
  if (out.has_sum())
    HIP_TRY(launch_summary_restore(c->state.as<PairState>(), advanced, out.sum, n_pairs, (unsigned)sum_pair_doubles, stream));
  if (out.has_fsum())
    HIP_TRY(launch_fb_summary_restore(c->state.as<PairState>(), out.fsum, n_pairs, (unsigned)fsum_pair_doubles, stream));
  if (d_results)
    HIP_TRY(launch_finalize(c->state.as<PairState>(), advanced, channels, n_pairs,
                            reinterpret_cast<ResultRecord*>(d_results), stream, c->settings));
  if (out.has_pts())
    HIP_TRY(launch_finalize_points(out.pts.snap, advanced, channels, n_pairs, out.pts.n_points, out.d_points, stream,
                                   c->settings));
  if (out.has_spn())                                 // (the replays have joined `stream` above)
    HIP_TRY(launch_finalize_points(out.spn.snap, advanced, channels, n_pairs, out.spn.n_spans, out.spn.out, stream,
                                   c->settings));
  HIP_TRY(hipEventRecord(c->batch_end, stream));
  c->batch_pending = true;
  return PEAQ_OK;
}

extern "C" int peaq_batch_last_timing(peaq_ctx* c, peaq_batch_timing* out) {
  if (!c || !out) return fail(PEAQ_ERR_ARG, "peaq_batch_last_timing: NULL argument");
  std::lock_guard<std::mutex> lock(c->mu);
  std::memset(out, 0, sizeof *out);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipEventSynchronize(c->batch_end));
  c->batch_pending = false;
  HIP_TRY(hipEventElapsedTime(&out->total_ms, c->batch_begin, c->batch_end));
  for (const TimedSpan& s : c->spans) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s.a, s.b));
    if (s.kind == 0) {
      out->frontend_ms += ms;
      out->frontend_launches++;
    } else if (s.kind == 1) {
      out->backend_ms += ms;
      out->backend_launches++;
    } else {
      out->fb_ms += ms;
      out->fb_launches++;
    }
  }
  return PEAQ_OK;
}

extern "C" int peaq_batch_last_clock(peaq_ctx* c, double* shader_clock_mhz) {
  if (!c || !shader_clock_mhz) return fail(PEAQ_ERR_ARG, "peaq_batch_last_clock: NULL argument");
  std::lock_guard<std::mutex> lock(c->mu);
  *shader_clock_mhz = 0.;
  if (!c->clk.p) return PEAQ_OK;                     // no batch yet
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipEventSynchronize(c->batch_end));
  unsigned long long h[2] = {0, 0};
  HIP_TRY(hipMemcpy(h, c->clk.p, sizeof h, hipMemcpyDeviceToHost));
  int wall_khz = 100000;
  (void)hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, c->device);
  if (h[1]) *shader_clock_mhz = (double)h[0] / (double)h[1] * (wall_khz * 1e-3);
  return PEAQ_OK;
}

// ---------------------------------------------------------------------------
// synthetic workload
// ---------------------------------------------------------------------------
extern "C" int peaq_synth_fill(peaq_ctx* c, uint32_t seed0, int n_pairs, int channels, uint32_t n_samples,
                               size_t pair_stride, float* d_ref, float* d_test, void* stream) {
  if (!c || !d_ref || !d_test) return fail(PEAQ_ERR_ARG, "peaq_synth_fill: NULL argument");
  if (int rc = check_channels("peaq_synth_fill", channels)) return rc;
  if (n_samples > pair_stride) return fail(PEAQ_ERR_ARG, "peaq_synth_fill: n_samples > pair_stride");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(launch_synth(seed0, n_pairs, channels, n_samples, pair_stride, d_ref, d_test,
                       static_cast<hipStream_t>(stream)));
  return PEAQ_OK;
}

// peaq_host.h -- what the host-side translation units behind include/peaq_amd.h share: the error convention and the
// argument checks every entry point repeats, the framing arithmetic, device buffers, the context, the model half of
// the kernels' argument blocks (ModelSetup), and the stream framer (StreamFramer: the element's do_processing /
// do_flush on the host-side stand-ins for its two GstAdapters) that sessions, the broker and peaq_debug_stream_plan
// run; and what the stages in front of the batch driver share: their scratch owner, their argument checks, the steps
// of the one-pair conveniences.  Host code, but for one marked section of device-side pieces of those stages (a copy
// body and a workgroup sum: no kernel is defined here); the model's kernels are in peaq_frontend.hip /
// peaq_backend.hip / peaq_fb.hip / peaq_synth.hip.
//   peaq_ctx.hip      errors, version, framing, context, settings, calibration
//   peaq_batch.hip    batch driver (peaq_batch_run, peaq_run_pair), timing, synthetic workload
//   peaq_resample.hip sample-rate conversion to 48 kHz in front of the batch driver (kernels and host side)
//   peaq_align.hip    delay estimation and cutting in front of the batch driver (kernels and host side); the steps of
//                     the one-pair conveniences (upload and conversion, delay estimate, scoring)
//   peaq_pcm.hip      PCM decoder in front of them (kernels and host side) and the host-fed batches (peaq_batch_run_host,
//                     peaq_batch_run_host_refs)
//   peaq_gather.hip   copy by source index, what shares one uploaded reference among its tests (kernel and host side)
//   peaq_gain.hip     level and polarity matching between delay estimation and the cut (kernels and host side)
//   peaq_frac.hip     sub-sample delay estimate and fractional-delay cut behind the integer aligner (kernels and host side)
//   peaq_drift.hip    constant drift: per-window delays through the two stages above, the robust line fit (host), the
//                     test signal's cut along the line (kernel and host side)
//   peaq_track.hip    delay track: the drift stage's per-window delays kept as knots and segments (host), the test
//                     signal's cut along them (kernel and host side)
//   peaq_steps.hip    delay steps: where inside two windows the delay jumps (kernels), the track rebuilt as pieces that
//                     jump there (host), the test signal's cut along pieces (kernel and host side)
//   peaq_wide.hip     wide delay search: the decimator in front of the aligner (kernels and host side), the coarse-to-fine
//                     estimate through the aligner and the cut
//   peaq_debug.hip    stage-level entry points for the parity tests, and the framer on its own (no device)
//   peaq_debug_wave.hip  the primitives of peaq_wave.h on their own, for their unit tests
//   peaq_watch.hip    the delay watch of a live stream (kernels; the host side is in the session and the broker)
//   peaq_live_rate.hip  rate conversion of live streams: the range converter over segments (kernel and host side), the
//                     host arithmetic from raw to converted counts that the stream framer counts with
//   peaq_session.hip  streaming sessions (one per `peaq` element): one StreamFramer, one launch per window
//   peaq_broker.hip   live-pipeline broker (a StreamFramer per session, one launch per tick), one or several devices
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <optional>
#include <string>
#include <thread>
#include <vector>

#include "../../include/peaq_amd.h"
#include "peaq_device.h"
#include "peaq_kernels.h"
#include "peaq_tables.h"
#include "peaq_wave.h"

#ifdef PEAQ_DEV_PROBES                               // VARIANT builds only (csrc/Makefile): never in the product library
#define PEAQ_DEV_TU_CAPI
#include "dev_probes.inc"
#endif
#ifndef PEAQ_DEV_SERIAL_KERNELS
#define PEAQ_DEV_SERIAL_KERNELS false
#endif
#ifndef PEAQ_DEV_SKIP_BACKEND
#define PEAQ_DEV_SKIP_BACKEND false
#endif
#ifndef PEAQ_DEV_BE_STREAM_PRIO
#define PEAQ_DEV_BE_STREAM_PRIO(prio, lo, hi)
#endif

// ---------------------------------------------------------------------------
// errors: every entry point returns PEAQ_OK or a negative code; the message of the calling thread's last failure
// is what peaq_last_error() hands out
// ---------------------------------------------------------------------------
std::string& peaq_err_string();
inline int fail(int code, const std::string& msg) {
  peaq_err_string() = msg;
  return code;
}
#define HIP_TRY(expr)                                                                                     \
  do {                                                                                                    \
    hipError_t e_ = (expr);                                                                               \
    if (e_ != hipSuccess)                                                                                 \
      return fail(e_ == hipErrorOutOfMemory ? PEAQ_ERR_NOMEM : PEAQ_ERR_DEVICE,                           \
                  std::string(#expr) + ": " + hipGetErrorString(e_));                                     \
  } while (0)

// the two argument checks most entry points share (`who` names the entry point in the message)
inline int check_channels(const std::string& who, int channels) {
  return channels == 1 || channels == 2
             ? PEAQ_OK
             : fail(PEAQ_ERR_ARG, who + ": channels must be 1 or 2, not " + std::to_string(channels));
}
inline int check_level(const std::string& who, double level_db) {
  return level_db >= 0. && level_db <= 130.
             ? PEAQ_OK
             : fail(PEAQ_ERR_ARG, who + ": playback level outside 0..130 dB (gstpeaq.c:275-281)");
}
// a caller's list of windows ("windows", "window") or spans and the array their readings go to, as the entries that
// take one check them: the list, its count, the lengths, the output, in this order
inline int check_span_list(const std::string& who, const char* plural, const char* singular, const peaq_window* list,
                           int n, const char* out_name, const void* out) {
  if (!list) return fail(PEAQ_ERR_ARG, who + ": " + plural + " is NULL");
  if (n < 1 || n > PEAQ_WINDOWS_MAX)
    return fail(PEAQ_ERR_ARG, who + ": n_" + plural + " " + std::to_string(n) + " is outside 1 .. " +
                                  std::to_string(PEAQ_WINDOWS_MAX));
  for (int i = 0; i < n; ++i)
    if (list[i].length == 0)
      return fail(PEAQ_ERR_ARG, who + ": " + singular + " " + std::to_string(i) + " has length 0");
  return out ? PEAQ_OK : fail(PEAQ_ERR_ARG, who + ": " + out_name + " is NULL");
}

// ---------------------------------------------------------------------------
// framing arithmetic
// ---------------------------------------------------------------------------
// number of frames the element processes for signals of n_ref / n_test samples:
// full frames while BOTH adapters hold `frame` samples, then one flush frame if
// anything is left on either side.
inline uint32_t count_frames(uint64_t n_ref, uint64_t n_test, uint32_t frame, uint32_t hop) {
  const uint64_t n = std::min(n_ref, n_test);
  const uint64_t full = n >= frame ? (n - frame) / hop + 1 : 0;
  const bool left = n_ref > full * hop || n_test > full * hop;
  return static_cast<uint32_t>(full + (left ? 1 : 0));
}

// ---------------------------------------------------------------------------
// growable device buffer; frees itself (its owner selects the device and drains its streams first)
// ---------------------------------------------------------------------------
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) cap = bytes;
    // PEAQ_AMD_POISON=1 (tests/test_gpu_poison.py): every workspace starts as NaNs (all bits set) instead of whatever
    // the allocator hands out -- fresh memory is zero, recycled memory is not; nothing may depend on either.  State
    // that has to start from zero is set to zero explicitly where it is created.
    static const bool poison = [] { const char* v = std::getenv("PEAQ_AMD_POISON"); return v && *v && *v != '0'; }();
    if (e == hipSuccess && poison) {
      e = hipMemset(p, 0xFF, bytes);
      if (e == hipSuccess) e = hipDeviceSynchronize();   // (the owners' own streams do not wait for the null stream)
    }
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <typename T>
  T* as() const { return static_cast<T*>(p); }
};

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
struct TimedSpan {
  hipEvent_t a, b;
  int kind;   // 0 front end, 1 back end, 2 filter bank
};

struct peaq_ctx {
  int device = 0;
  peaq::CommonTables* d_common = nullptr;
  peaq::BandTables* d_bands109 = nullptr;
  peaq::BandTables* d_bands55 = nullptr;
  peaq::BandTables* d_bands40 = nullptr;
  peaq::FbTables* d_fb = nullptr;
  std::mutex mu;            // serialises batch calls / workspace use
  // batch workspace
  DevBuf records, records2, fb_records, fb_records2, state, fbstate, hp_scratch, hp_scratch2, counts, clk;
  DevBuf snaps;             // trajectories: the reading points' snapshots [pair][point] (peaq_batch_run_trajectory)
  DevBuf spn_frames, spn_list;   // windows and spans: the frame records the FFT replay reads [pair][frame], the caller's list on the device (peaq_batch_run_windows, peaq_batch_run_adv_spans; the snapshots are `snaps`)
  DevBuf spn_blocks;        // spans: the block records the filter-bank replay reads [pair][block] (peaq_batch_run_adv_spans)
  DevBuf sum_saved;         // band summaries: the rows as they were when a pair last turned tentative (peaq_batch_run_band_summary, peaq_batch_run_fb_band_summary)
  hipStream_t aux = nullptr;   // the back end runs here, overlapped with the next chunk's front end
  hipStream_t aux2 = nullptr;  // advanced: the filter-bank path runs here, beside the FFT path
  hipStream_t aux3 = nullptr, aux4 = nullptr;   // ... its high-pass stage and its back end (3-stage pipeline)
  hipEvent_t batch_begin = nullptr, batch_end = nullptr;
  hipEvent_t fb_last_bank_begin = nullptr, fb_last_bank_end = nullptr;   // of the running batch's filter-bank path (pool events)
  bool batch_pending = false;
  std::vector<TimedSpan> spans;
  std::vector<hipEvent_t> event_pool;
  size_t events_used = 0;
  unsigned long long* d_prof = nullptr;   // -DPEAQ_FE_PROFILE builds only
  int fir_fp64 = 1;                       // advanced version: arithmetic of the FIR bank (PEAQ_FIR_*; default the reference's FP64)
  peaq::Settings settings;                      // the reference's settings.h switches (peaq_ctx_set_settings)
  struct RsState* rs = nullptr;           // rate converter: tap tables per rate, length scratch (peaq_resample.hip)
  struct AlignState* al = nullptr;        // aligner: spectra scratch, length scratch (peaq_align.hip)
  struct FeedState* feed = nullptr;       // PCM decoder and host feed: length scratch, staging sets, streams (peaq_pcm.hip)
  struct GatherState* ga = nullptr;       // gather: index and length scratch (peaq_gather.hip)
  struct GainState* gn = nullptr;         // gain matching: partial sums, length scratch (peaq_gain.hip)
  struct FracState* fr = nullptr;         // sub-sample stage: the two tables, partial sums, length scratch (peaq_frac.hip)
  struct StepsState* sp = nullptr;        // steps stage: the chunks' rows (peaq_steps.hip)
  struct WideState* wd = nullptr;         // wide search: the decimator's taps, its FP64 outputs, length scratch (peaq_wide.hip)

  hipEvent_t next_event() {
    if (events_used == event_pool.size()) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) return nullptr;
      event_pool.push_back(e);
    }
    return event_pool[events_used++];
  }
};

// free what a stage has cached in the context; the device is idle.  peaq_resample.hip, peaq_align.hip, peaq_pcm.hip,
// peaq_gather.hip, peaq_gain.hip, peaq_frac.hip, peaq_steps.hip, peaq_wide.hip
void resample_release(peaq_ctx* c);
void align_release(peaq_ctx* c);
void feed_release(peaq_ctx* c);
void gather_release(peaq_ctx* c);
void gain_release(peaq_ctx* c);
void frac_release(peaq_ctx* c);
void steps_release(peaq_ctx* c);
void wide_release(peaq_ctx* c);
// The rate converter for the range converter of live streams (peaq_resample.hip -> peaq_live_rate.hip): L, M and K of a
// rate, with the refusal every entry gives for a rate it does not take (host only); the converted length without the
// 32-bit limit; and the plain [L][2K] tap table on the device -- for a tiled rate uploaded at the first call -- with
// the converter's length slots (the caller holds the context's lock).
struct RateGeometry {
  uint32_t L, M, K;
};
int resample_geometry(const char* who, uint32_t rate, RateGeometry* out);
uint64_t resampled_length_u64(uint64_t n, uint32_t rate);
int resample_plain_table(peaq_ctx* c, uint32_t rate, const double** taps, RateGeometry* geo, struct LenStage** lens);
// Live rate conversion on the host (peaq_live_rate.hip; include/peaq_amd.h, "live rate conversion"), for a geometry
// that resample_geometry gave: the converted samples n_have raw ones deliver, the raw span of a run of outputs, and
// the longest raw span any run of `count` outputs has.
uint64_t live_rate_ready(const RateGeometry& g, uint32_t rate, uint64_t n_have, bool ended);
void live_rate_span(const RateGeometry& g, uint64_t out_first, uint32_t out_count, uint64_t* in_first, uint64_t* in_end);
// one launch of the range converter over segments that stage_window made (no checks but the strides; enqueues on `stream`)
int live_rate_convert(peaq_ctx* c, int channels, uint32_t rate, int n_segments, const peaq_rate_segment* seg,
                      const float* d_in, size_t in_stride, float* d_out, size_t out_stride, hipStream_t stream);
inline size_t live_rate_span_max(const RateGeometry& g, size_t count) {
  return (count * g.M + g.L - 1) / g.L + 2 * (size_t)g.K + 1;
}
// the sub-sample stage's shift table on the device and its length slots, for the drift cut (peaq_frac.hip; the caller
// holds the context's lock)
int frac_shift_table(peaq_ctx* c, const double** shift, struct LenStage** lens);
// peaq_batch_estimate_drift with `who` naming the entry point in its refusals, for the track stage (peaq_drift.hip)
int drift_estimate(const std::string& who, peaq_ctx* c, int channels, int n_pairs, const float* d_ref, const float* d_test,
                   size_t pair_stride, const uint32_t* n_ref, const uint32_t* n_test, uint32_t n_uniform, const int32_t* lag0,
                   uint32_t window, uint32_t R, double min_corr, double max_e, uint32_t w_max, peaq_delay* d_win_delay,
                   peaq_subdelay* d_win_sub, peaq_drift* out, void* stream);
// mode (PEAQ_GAIN_* with or without PEAQ_GAIN_PER_CHANNEL) and max_gain_db as every entry point of the stage takes them
int check_gain_mode(const std::string& who, int mode, double max_gain_db);
// max_lag of the aligner, 1 .. 16384 (peaq_align.hip)
int check_max_lag(const std::string& who, uint32_t max_lag);
// planes of a band trace, PEAQ_BAND_* bits the version has (peaq_batch.hip)
int check_band_planes(const std::string& who, int advanced, uint32_t planes);
int check_fb_band_planes(const std::string& who, uint32_t planes);
int check_pattern_band_planes(const std::string& who, uint32_t planes);

// ---------------------------------------------------------------------------
// Per-pair host arrays of one call (lengths, skips): staged in pinned host memory and copied on the caller's stream,
// so the call enqueues and returns.  A slot is reused kLenSlots calls later, after the event recorded behind the
// kernel that read it.  The owner holds the context's lock around upload() and sent().
// ---------------------------------------------------------------------------
constexpr int kLenSlots = 4;
struct LenSlot {
  uint32_t* host = nullptr;     // pinned
  size_t host_cap = 0;          // entries
  DevBuf dev;
  hipEvent_t done = nullptr;
  bool pending = false;
};
struct LenStage {
  LenSlot slots[kLenSlots];
  unsigned next_slot = 0;

  // `count` entries from h into the next slot, copied to its device buffer on `stream`; *out: the slot
  int upload(const uint32_t* h, size_t count, hipStream_t stream, LenSlot** out) {
    LenSlot* slot = &slots[next_slot++ % kLenSlots];
    if (slot->pending) {                               // the call kLenSlots calls ago still reads this slot
      HIP_TRY(hipEventSynchronize(slot->done));
      slot->pending = false;
    }
    if (!slot->done) HIP_TRY(hipEventCreateWithFlags(&slot->done, hipEventDisableTiming));
    if (count > slot->host_cap) {
      if (slot->host) (void)hipHostFree(slot->host);
      slot->host = nullptr;
      slot->host_cap = 0;
      HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&slot->host), count * sizeof(uint32_t), hipHostMallocDefault));
      slot->host_cap = count;
    }
    HIP_TRY(slot->dev.reserve(count * sizeof(uint32_t)));
    std::memcpy(slot->host, h, count * sizeof(uint32_t));
    HIP_TRY(hipMemcpyAsync(slot->dev.p, slot->host, count * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    *out = slot;
    return PEAQ_OK;
  }
  // behind the last kernel that reads the slot
  int sent(LenSlot* slot, hipStream_t stream) {
    HIP_TRY(hipEventRecord(slot->done, stream));
    slot->pending = true;
    return PEAQ_OK;
  }
  void release() {                                     // (the device is idle; the device buffers free themselves)
    for (LenSlot& sl : slots) {
      if (sl.host) (void)hipHostFree(sl.host);
      if (sl.done) (void)hipEventDestroy(sl.done);
      sl.host = nullptr;
      sl.done = nullptr;
    }
  }
};

// ---------------------------------------------------------------------------
// Scratch of a stage, shared between its calls and their streams: grown only when its last user is done, waited for
// by a call on another stream, marked behind the last launch of every call.  The owner holds the context's lock.
// Nothing here reads the buffer: a stage's kernels write what they read (PEAQ_AMD_POISON).
// ---------------------------------------------------------------------------
struct StageScratch {
  DevBuf buf;
  hipEvent_t free_ev = nullptr;   // behind the last kernel that used the buffer
  bool busy = false;

  int acquire(size_t bytes, hipStream_t stream) {
    if (!free_ev) HIP_TRY(hipEventCreateWithFlags(&free_ev, hipEventDisableTiming));
    if (bytes > buf.cap && busy) {                     // growing frees the old buffer: its last user has to be done
      HIP_TRY(hipEventSynchronize(free_ev));
      busy = false;
    }
    HIP_TRY(buf.reserve(bytes));
    if (busy) HIP_TRY(hipStreamWaitEvent(stream, free_ev, 0));   // (a call on another stream)
    return PEAQ_OK;
  }
  // behind a call's last launch -- also after a failed one: what was enqueued before it still uses the buffer
  hipError_t mark(hipStream_t stream) {
    const hipError_t e = hipEventRecord(free_ev, stream);
    busy = e == hipSuccess;
    return e;
  }
  void release() {                                     // (the device is idle)
    if (free_ev) (void)hipEventDestroy(free_ev);
    free_ev = nullptr;
    busy = false;
    buf.release();
  }
};

// a stage's state in the context: `lens` and `scratch`, whatever else it holds frees itself
template <typename S>
void release_stage(S*& st) {
  if (!st) return;
  st->lens.release();
  st->scratch.release();
  delete st;
  st = nullptr;
}

// Pairs are taken in groups whose scratch stays below `budget` (or is one pair's, if that is more): the scratch of a
// call of n_pairs pairs of per_pair bytes each, and the pairs of a group.
struct PairGroups {
  size_t bytes;
  int group;
};
inline PairGroups pair_groups(size_t per_pair, int n_pairs, size_t budget) {
  if (n_pairs <= 0) return {0, 0};
  const size_t bytes = std::min((size_t)n_pairs * per_pair, std::max(budget, per_pair));
  return {bytes, (int)std::min<size_t>((size_t)n_pairs, std::max<size_t>(1, bytes / per_pair))};
}

// ---------------------------------------------------------------------------
// argument checks of the batch stages (`who` names the entry point); the context is the caller's to look at, last
// ---------------------------------------------------------------------------
// the call's shape: channels, and a count of `noun` in 0 .. 65535 (a grid's y extent)
inline int check_count(const std::string& who, int n, const char* name = "n_pairs", const char* noun = "pairs") {
  if (n < 0) return fail(PEAQ_ERR_ARG, who + ": " + name + " " + std::to_string(n) + " < 0");
  if (n > 65535) return fail(PEAQ_ERR_ARG, who + ": " + std::to_string(n) + " " + noun + " are more than 65535 in one call");
  return PEAQ_OK;
}
inline int check_shape(const std::string& who, int channels, int n_pairs) {
  if (int rc = check_channels(who, channels)) return rc;
  return check_count(who, n_pairs);
}

// The cut geometry: n_out runs, run p being n_keep[p] samples from skip[p] on of some row of d_in [n_rows][in_stride],
// to row p of d_out [n_out][out_stride] (`noun`: what a run is called, "pair" or "output").  skip and n_keep are
// not NULL where n_out > 0: the caller has looked, it knows their names.  *keep_max: the longest run.
inline int check_cut_geometry(const std::string& who, const char* noun, int channels, int n_rows, int n_out,
                              const float* d_in, size_t in_stride, const uint32_t* skip, const uint32_t* n_keep,
                              const float* d_out, size_t out_stride, uint32_t* keep_max) {
  *keep_max = 0;
  if (n_out <= 0) return PEAQ_OK;
  if (!d_in || !d_out) return fail(PEAQ_ERR_ARG, who + ": NULL buffer");
  for (int p = 0; p < n_out; ++p) {
    if ((uint64_t)skip[p] + n_keep[p] > in_stride)
      return fail(PEAQ_ERR_ARG, who + ": " + noun + " " + std::to_string(p) + ": skip " + std::to_string(skip[p]) +
                                    " + n_keep " + std::to_string(n_keep[p]) + " passes in_stride " + std::to_string(in_stride));
    *keep_max = std::max(*keep_max, n_keep[p]);
  }
  if (*keep_max > out_stride)
    return fail(PEAQ_ERR_ARG, who + ": out_stride " + std::to_string(out_stride) + " is smaller than the longest n_keep (" +
                                  std::to_string(*keep_max) + " samples)");
  const char* i0 = reinterpret_cast<const char*>(d_in);
  const char* o0 = reinterpret_cast<const char*>(d_out);
  const size_t ib = (size_t)n_rows * in_stride * channels * sizeof(float);
  const size_t ob = (size_t)n_out * out_stride * channels * sizeof(float);
  if (i0 < o0 + ob && o0 < i0 + ib) return fail(PEAQ_ERR_ARG, who + ": d_out overlaps d_in");
  return PEAQ_OK;
}

// per-pair lengths n[p] -- or, n being NULL, n_uniform -- against the stride of their buffer; *n_max: the longest
inline int check_lengths(const std::string& who, int n_pairs, const uint32_t* n, uint32_t n_uniform, const char* name,
                         size_t stride, const char* stride_name, uint32_t* n_max = nullptr) {
  uint32_t longest = 0;
  if (!n_max) n_max = &longest;
  *n_max = 0;
  if (n_pairs <= 0) return PEAQ_OK;
  if (!n) {
    *n_max = n_uniform;
    if (n_uniform > stride)
      return fail(PEAQ_ERR_ARG, who + ": n_uniform " + std::to_string(n_uniform) + " passes " + stride_name + " " +
                                    std::to_string(stride));
    return PEAQ_OK;
  }
  for (int p = 0; p < n_pairs; ++p) {
    if (n[p] > stride)
      return fail(PEAQ_ERR_ARG, who + ": pair " + std::to_string(p) + ": " + name + " " + std::to_string(n[p]) + " passes " +
                                    stride_name + " " + std::to_string(stride));
    *n_max = std::max(*n_max, n[p]);
  }
  return PEAQ_OK;
}

// ---------------------------------------------------------------------------
// The steps of the one-pair conveniences (peaq_run_pair_rate, _aligned, _matched, _trace, _subsample, _drift, _track, _steps), defined in
// peaq_align.hip.  Each of them blocks; the stage calls between them are the entry point's own.
// ---------------------------------------------------------------------------
// (a) what every peaq_run_pair_* call checks, beside check_level where it looks at the level: channels, rate, ctx and
//     (need_out) out, samples, their counts
int check_pair_args(const std::string& who, const peaq_ctx* c, int channels, uint32_t rate, const float* ref,
                    size_t n_ref, const float* test, size_t n_test, const void* out, bool need_out);
// (b) a host pair on the device at 48 kHz: s48[0], s48[1] of `stride` samples per channel, zeros behind len[i]
struct PairBuffers {
  DevBuf raw[2], s48[2];
  uint32_t len[2] = {0, 0};
  size_t stride = 0;
  const float* d(int i) const { return s48[i].as<float>(); }
};
int upload_pair_48k(peaq_ctx* c, int channels, uint32_t rate, const float* ref, size_t n_ref, const float* test,
                    size_t n_test, PairBuffers& pb);
// (c) the delay of the pair, estimated and fetched
int estimate_one_delay(peaq_ctx* c, int channels, const PairBuffers& pb, uint32_t max_lag, peaq_delay* rec);
// (d) one prepared pair scored with peaq_batch_run, the result fetched
int score_one_pair(peaq_ctx* c, int advanced, int channels, double level_db, const float* d_ref, const float* d_test,
                   size_t stride, uint32_t len_ref, uint32_t len_test, peaq_result* out);
// (e) the head of peaq_run_pair_subsample, _drift, _track and _steps, behind the checks of their own parameters: the
//     gain mode, max_lag, the level and (a); *gain cleared; (b) into `in`; (c) into *rec and, where asked for, *delay.
//     With a window (0: the entry has none), *W: the whole windows of the common part, at most PEAQ_DRIFT_MAX_WINDOWS.
int begin_delay_pair(const std::string& who, peaq_ctx* c, int channels, double level_db, uint32_t rate, uint32_t max_lag,
                     uint32_t window, int mode, double max_gain_db, const float* ref, size_t n_ref, const float* test,
                     size_t n_test, peaq_delay* delay, peaq_gain* gain, const void* out, PairBuffers& in, peaq_delay* rec,
                     uint32_t* W);
// (f) their tail: `keep` samples of the reference from skip[0] on cut plainly, those of the test signal by
//     cut_test(d_out, out_stride) -- the stage's cut of in.d(1) from skip[1] on --, the gain that `mode` asks for measured
//     on the two CUT buffers and applied into a third one, fetched into *gain; (d)
int score_cut_pair(peaq_ctx* c, int advanced, int channels, double level_db, const PairBuffers& in, const uint32_t skip[2],
                   uint32_t keep, int mode, double max_gain_db, peaq_gain* gain,
                   const std::function<int(float* d_out, size_t out_stride)>& cut_test, peaq_result* out);

// ---------------------------------------------------------------------------
// DEVICE SIDE.  The pieces the kernels of peaq_align.hip, peaq_gain.hip, peaq_frac.hip, peaq_drift.hip, peaq_track.hip, peaq_steps.hip and peaq_gather.hip share
// (256 threads per workgroup).  No kernel is defined in this header.  (What only the cuts along a delay share is in
// peaq_delay_cut.h.)
// ---------------------------------------------------------------------------
// A workgroup's share of the copy of `count` consecutive floats from src to dst: the 16-byte units v0 .. v0 + 255,
// counted from the first 16-byte aligned float of dst, and with `ends` the unaligned head and the tail, at most 3
// floats each.  Stores are 16 bytes; loads are too where src + head is aligned alike (the whole run is, or is
// not), else four dwords.  f(x, i) is what is stored for x, a float4 or a float whose (first) float is float i of
// the run.
struct CopyBits {
  __device__ __forceinline__ float4 operator()(float4 x, size_t) const { return x; }
  __device__ __forceinline__ float operator()(float x, size_t) const { return x; }
};
template <typename F>
__device__ __forceinline__ void copy_run(const float* __restrict__ src, float* __restrict__ dst, size_t count, size_t v0,
                                         bool ends, F f) {
  const size_t head = min(count, (size_t)((16 - ((uintptr_t)dst & 15)) & 15) / sizeof(float));
  const size_t vecs = (count - head) / 4;
  const bool same_phase = ((uintptr_t)(src + head) & 15) == 0;   // of the whole run: units are 16 bytes apart
  const size_t v = v0 + threadIdx.x;
  if (v < vecs) {
    const float* s = src + head + 4 * v;
    float4 x;
    if (same_phase)
      x = *reinterpret_cast<const float4*>(s);
    else
      x = {s[0], s[1], s[2], s[3]};
    *reinterpret_cast<float4*>(dst + head + 4 * v) = f(x, head + 4 * v);
  }
  if (ends) {
    if (threadIdx.x < head) dst[threadIdx.x] = f(src[threadIdx.x], (size_t)threadIdx.x);
    const size_t tail0 = head + 4 * vecs;
    if (tail0 + threadIdx.x < count) dst[tail0 + threadIdx.x] = f(src[tail0 + threadIdx.x], tail0 + threadIdx.x);
  }
}

// N sums of one workgroup: the wave (peaq::wave_sum), then the four waves (0 + 1) + (2 + 3); valid in every thread.
// sh: [4][N] of LDS, declared in the kernel.
template <int N>
__device__ __forceinline__ void block_sum4(double (&s)[N], double (*sh)[N]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < N; ++k) s[k] = peaq::wave_sum(s[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) sh[wave][k] = s[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) s[k] = (sh[0][k] + sh[1][k]) + (sh[2][k] + sh[3][k]);
}

// ---- batch driver pieces used elsewhere (peaq_batch.hip) --------------------------------------------------
unsigned fb_blocks_per_chunk(int n_pairs, int channels, uint32_t max_blocks);
unsigned frames_per_chunk(int n_pairs, int channels, uint32_t max_frames);

// ---------------------------------------------------------------------------
// The model half of the four kernel argument blocks: what follows from the context, the settings, the version, the
// channel count and the playback level, whoever launches.  Geometry -- buffers, strides, counts, origins, windows,
// launch index, state, debug and clock pointers -- is the caller's.
// ---------------------------------------------------------------------------
struct ModelSetup {
  const peaq_ctx* ctx;
  peaq::Settings cfg;
  int advanced, channels;
  double level_db;

  int fft_bands() const { return advanced ? 55 : 109; }   // gstpeaq.c:521-526
  peaq::FrontendArgs frontend() const {
    peaq::FrontendArgs fa{};
    fa.cfg = cfg;
    fa.channels = channels;
    fa.level_factor = peaq::fft_level_factor(level_db);
    fa.common = ctx->d_common;
    fa.bands = advanced ? ctx->d_bands55 : ctx->d_bands109;
    fa.prof = ctx->d_prof;
    return fa;
  }
  // the back end of the front end `fa`: its records, its bands and (broker launches) its per-pair frame windows
  peaq::BackendArgs backend(const peaq::FrontendArgs& fa) const {
    peaq::BackendArgs ba{};
    ba.cfg = fa.cfg;
    ba.channels = fa.channels;
    ba.advanced = advanced;
    ba.common = fa.common;
    ba.bands = fa.bands;
    ba.records = fa.records;
    ba.pair_frame0 = fa.pair_frame0;
    ba.pair_nframes = fa.pair_nframes;
    return ba;
  }
  peaq::FbFrontArgs fb_frontend() const {
    peaq::FbFrontArgs ff{};
    ff.cfg = cfg;
    ff.fir_fp64 = ctx->fir_fp64;
    ff.channels = channels;
    ff.level_factor = peaq::fb_level_factor(level_db);
    // split-FP16 FIR (fir_fp64 == 2): the power of two that puts the filtered signal's full scale -- |x| = 1 times
    // the playback-level factor -- between 2^10 and 2^11 of FP16's 65504 (30 dB of headroom for samples beyond full
    // scale and for the high-pass filter's overshoot)
    const int e = 10 - std::ilogb(ff.level_factor);
    ff.hf_xscale = std::ldexp(1., e);
    ff.hf_xunscale = std::ldexp(1., -e);
    ff.bands = ctx->d_bands40;
    ff.fb = ctx->d_fb;
    return ff;
  }
  peaq::FbBackendArgs fb_backend(const peaq::FbFrontArgs& ff) const {
    peaq::FbBackendArgs fbk{};
    fbk.cfg = ff.cfg;
    fbk.channels = ff.channels;
    fbk.common = ctx->d_common;
    fbk.bands = ff.bands;
    fbk.records = ff.records;
    fbk.windows = ff.windows;
    return fbk;
  }
};

constexpr unsigned kSessionMaxFrames = 64;   // FFT frames per launch of a session
constexpr unsigned kSessionMaxBlocks = 120;  // filter-bank blocks per launch of a session
constexpr unsigned kBrokerMaxFrames = 8;     // FFT frames one session contributes to one tick of the broker
constexpr unsigned kBrokerMaxBlocks = 48;    // filter-bank blocks one session contributes to one tick
// a broker slot's flush: asked for by peaq_broker_flush, carried out by the ticks, one path at a time
struct SlotFlush {
  bool requested = false, fft_done = false, fb_done = false;
  void request() { *this = SlotFlush{true, false, false}; }
  void clear() { *this = SlotFlush{}; }
};

// host-side stand-in for a GstAdapter: the not yet consumed tail of one pad's stream.
// Consumed samples are skipped with a read offset and the storage is compacted only once more
// than half of it is dead, so a pad that runs far ahead of the other one (a whole file pushed on
// `ref` before `test` starts) costs O(n) in total, like gst_adapter_flush, not O(n^2).
struct PadFifo {
  std::vector<float> buf;   // interleaved; live data starts at buf[head]
  size_t head = 0;
  uint64_t base = 0;        // stream sample index (per channel) of buf[head]
  uint64_t total = 0;       // samples (per channel) pushed so far
  const float* at(uint64_t pos, int channels) const { return buf.data() + head + (size_t)(pos - base) * channels; }
  size_t live_floats() const { return buf.size() - head; }
  void append(const float* data, size_t n_floats) { buf.insert(buf.end(), data, data + n_floats); }
  void drop_until(uint64_t keep_from, int channels) {
    if (keep_from <= base) return;
    const size_t drop = std::min((size_t)(keep_from - base) * channels, live_floats());
    head += drop;
    base = keep_from;
    if (head == buf.size()) {
      buf.clear();
      head = 0;
    } else if (head >= 65536 && head > buf.size() / 2) {
      buf.erase(buf.begin(), buf.begin() + head);
      head = 0;
    }
  }
};

// ---------------------------------------------------------------------------
// The element's framing policy, do_processing / do_flush (gstpeaq.c:596-611, 716-745, 769-771), for one (ref, test)
// stream: whole FFT frames of 2048 every 1024 while BOTH pads hold one, whole filter-bank blocks of 192 (advanced
// version), and at a flush ONE zero-padded unit per kind from whatever is left on either pad.  Host only, no lock
// and no device work: the owner (a session, a broker slot) holds its own lock around every call.
// ---------------------------------------------------------------------------
enum StreamUnit { kUnitFrame = 0, kUnitBlock = 1 };

// one launch's worth of one kind of unit
struct StreamWindow {
  uint32_t first = 0, count = 0;    // index of the first unit and how many (0: nothing to launch)
  uint32_t prev_blocks = 0;         // blocks: the count of the previous window (where the kernel's history tail sits)
  bool flush = false;               // the zero-padded unit of the flush: nothing of this kind follows it
  uint64_t pos[2] = {0, 0};         // stream sample the window starts at, per pad
  uint64_t valid[2] = {0, 0};       // samples present from there, per pad (short of whole units only in the flush unit)
};

struct StreamFramer {
  bool advanced = false;
  int channels = 1;
  PadFifo pad[2];
  uint64_t pos[2][2] = {{0, 0}, {0, 0}};   // [kind][pad]: stream sample where the next unit starts
  uint32_t done[2] = {0, 0};               // [kind]: units handed out so far
  uint32_t prev_blocks = 0;
  // Live alignment (include/peaq_amd.h, "live alignment"): a held stream hands out nothing; release() ends the hold
  // with the samples each pad drops from its head, before any unit exists.  Units, done[] and left() then count the
  // stream as scored, pad p from its sample skip[p] on.  Never held and nothing skipped unless the owner asks.
  bool held = false;
  uint64_t skip[2] = {0, 0};
  // Live rate conversion (include/peaq_amd.h, "live rate conversion"): the FIFO of a pad whose rate is not 48000 holds
  // RAW samples, and pad[p].total counts them; everything else here -- have(), left(), scored(), pos, skip, the
  // windows' pos / valid -- counts CONVERTED samples.  `ended`: the flush has been asked for, so that the converted
  // length is the stream's own.  The rates outlive reset().
  uint32_t rate[2] = {48000, 48000};
  RateGeometry geo[2] = {{1, 1, 0}, {1, 1, 0}};
  bool ended = false;

  void reset(bool advanced_, int channels_) {
    StreamFramer fresh;
    for (int p = 0; p < 2; ++p) {
      fresh.rate[p] = rate[p];
      fresh.geo[p] = geo[p];
    }
    *this = std::move(fresh);
    advanced = advanced_;
    channels = channels_;
  }
  void set_rate(int p, uint32_t r, const RateGeometry& g) {
    rate[p] = r;
    geo[p] = g;
  }
  bool rated(int p) const { return rate[p] != 48000; }
  // n samples (per channel) more on pad p; data == nullptr: counted but not stored (peaq_debug_stream_plan)
  void append(int p, const float* data, size_t n) {
    if (data) pad[p].append(data, n * channels);
    pad[p].total += n;
  }
  // samples of pad p that can be framed: what was pushed, or what of it converts
  uint64_t have(int p) const {
    return rated(p) ? live_rate_ready(geo[p], rate[p], pad[p].total, ended) : pad[p].total;
  }
  // the raw samples [*lo, *hi) of a rated pad behind `count` converted ones from `first` on, inside what the pad holds
  void raw_span(int p, uint64_t first, uint64_t count, uint64_t* lo, uint64_t* hi) const {
    live_rate_span(geo[p], first, static_cast<uint32_t>(count), lo, hi);
    *hi = std::min(*hi, pad[p].total);
    *lo = std::min(*lo, *hi);
  }
  uint64_t left(StreamUnit kind, int p) const { return have(p) - pos[kind][p]; }
  void hold() { held = true; }
  void release(uint64_t skip_ref, uint64_t skip_test) {   // (a skip stops at what the pad holds: the caller's plan)
    skip[0] = skip_ref;
    skip[1] = skip_test;
    for (int kind = 0; kind < 2; ++kind)
      for (int p = 0; p < 2; ++p) pos[kind][p] = skip[p];
    held = false;
  }
  uint64_t scored(int p) const { return have(p) - skip[p]; }   // samples of pad p in the stream as scored
  // samples present on both pads and not yet framed: of one kind, and the larger of the kinds in use (what the
  // broker's back-pressure counts)
  uint64_t backlog(StreamUnit kind) const { return std::min(left(kind, 0), left(kind, 1)); }
  uint64_t backlog() const {
    return advanced ? std::max(backlog(kUnitFrame), backlog(kUnitBlock)) : backlog(kUnitFrame);
  }
  // a whole frame, or (advanced) a whole block, is waiting
  bool ready(StreamUnit kind) const {
    return backlog(kind) >= (uint64_t)(kind == kUnitBlock ? peaq::kFbFrame : peaq::kFrame);
  }
  bool ready() const { return ready(kUnitFrame) || (advanced && ready(kUnitBlock)); }

  // The next window of `kind`, at most `cap` units, and the stream moves on past it.  Whole units first; with
  // `flushing`, once no whole unit is left and something remains on either pad, the one zero-padded unit: each pad
  // contributes, and moves on by, min(left, unit).
  StreamWindow take(StreamUnit kind, unsigned cap, bool flushing) {
    const uint64_t unit = kind == kUnitBlock ? peaq::kFbFrame : peaq::kFrame;
    const uint64_t hop = kind == kUnitBlock ? peaq::kFbFrame : peaq::kHop;
    const uint64_t l[2] = {left(kind, 0), left(kind, 1)}, av = std::min(l[0], l[1]);
    StreamWindow w;
    if (held) return w;
    uint64_t adv[2];
    if (av >= unit) {
      w.count = static_cast<uint32_t>(std::min<uint64_t>((av - unit) / hop + 1, cap));
      w.valid[0] = w.valid[1] = (uint64_t)(w.count - 1) * hop + unit;
      adv[0] = adv[1] = (uint64_t)w.count * hop;
    } else if (flushing && (l[0] || l[1])) {
      w.count = 1;
      w.flush = true;
      for (int p = 0; p < 2; ++p) w.valid[p] = adv[p] = std::min(l[p], unit);
    } else {
      return w;
    }
    w.first = done[kind];
    done[kind] += w.count;
    for (int p = 0; p < 2; ++p) {
      w.pos[p] = pos[kind][p];
      pos[kind][p] += adv[p];
    }
    if (kind == kUnitBlock) {
      w.prev_blocks = prev_blocks;
      prev_blocks = w.count;
    }
    return w;
  }
  // drops what both consumers are done with (windows taken before are no longer readable: copy first)
  void trim() {
    for (int p = 0; p < 2; ++p) {
      uint64_t keep = advanced ? std::min(pos[kUnitFrame][p], pos[kUnitBlock][p]) : pos[kUnitFrame][p], end;
      if (rated(p)) raw_span(p, keep, 1, &keep, &end);   // (the first raw sample the next unit reads)
      pad[p].drop_until(keep, channels);
    }
  }
};

// the samples of window w, from the framer's FIFOs into dst[pad] (pinned staging); a rated pad: the raw samples behind
// the window into raw[pad], and seg[pad] the segment that converts them into the window
inline void stage_window(const StreamFramer& fr, const StreamWindow& w, float* const dst[2], float* const raw[2] = nullptr,
                         peaq_rate_segment* const seg[2] = nullptr) {
  for (int p = 0; p < 2; ++p) {
    if (!fr.rated(p)) {
      if (w.valid[p])
        std::memcpy(dst[p], fr.pad[p].at(w.pos[p], fr.channels), (size_t)w.valid[p] * fr.channels * sizeof(float));
      continue;
    }
    uint64_t lo, hi;
    fr.raw_span(p, w.pos[p], w.valid[p], &lo, &hi);
    if (hi > lo) std::memcpy(raw[p], fr.pad[p].at(lo, fr.channels), (size_t)(hi - lo) * fr.channels * sizeof(float));
    *seg[p] = peaq_rate_segment{w.pos[p], lo, fr.ended ? fr.pad[p].total : UINT64_MAX, static_cast<uint32_t>(w.valid[p]),
                                static_cast<uint32_t>(hi - lo)};
  }
}

// What a session does after every push and, with `flushing`, at its flush: frames, then (advanced) blocks, in
// windows of at most max_frames / max_blocks until nothing comes back or the flush unit has, then trim.
// run(kind, window) launches a window; a result other than PEAQ_OK ends the walk.
template <typename Run>
int drain_stream(StreamFramer& fr, unsigned max_frames, unsigned max_blocks, bool flushing, Run&& run) {
  for (StreamUnit kind : {kUnitFrame, kUnitBlock}) {
    if (kind == kUnitBlock && !fr.advanced) break;
    const unsigned cap = kind == kUnitBlock ? max_blocks : max_frames;
    for (;;) {
      const StreamWindow w = fr.take(kind, cap, flushing);
      if (!w.count) break;
      const int rc = run(kind, w);
      if (rc != PEAQ_OK) return rc;
      if (w.flush) break;
    }
  }
  fr.trim();
  return PEAQ_OK;
}

// ---------------------------------------------------------------------------
// The meter's arithmetic (include/peaq_amd.h, "meter"): W, H in FFT frames, window k covers frames [k H, k H + W).
// Host only; the device walks the same windows in peaq_meter.hip.
// ---------------------------------------------------------------------------
inline int check_meter_config(const std::string& who, const peaq_meter_config& c) {
  if (c.window_frames < 1 || c.hop_frames < 1)
    return fail(PEAQ_ERR_ARG, who + ": window_frames " + std::to_string(c.window_frames) + " and hop_frames " +
                                  std::to_string(c.hop_frames) + " must both be at least 1");
  const uint64_t k_open = ((uint64_t)c.window_frames + c.hop_frames - 1) / c.hop_frames;
  if (k_open > peaq::kMeterMaxOpen)
    return fail(PEAQ_ERR_ARG, who + ": window_frames " + std::to_string(c.window_frames) + " over hop_frames " +
                                  std::to_string(c.hop_frames) + " keeps " + std::to_string(k_open) +
                                  " windows open at once, more than " + std::to_string(peaq::kMeterMaxOpen));
  if (c.depth < 1 || c.depth > peaq::kMeterMaxDepth)
    return fail(PEAQ_ERR_ARG, who + ": depth " + std::to_string(c.depth) + " is outside 1 .. " +
                                  std::to_string(peaq::kMeterMaxDepth));
  return PEAQ_OK;
}
// The band meter (include/peaq_amd.h, "meter: band rows") on a geometry that check_meter_config has passed: every open
// window keeps its rows twice, hence the narrower limits.
inline int check_meter_bands_config(const std::string& who, const peaq_meter_config& c) {
  const uint64_t k_open = ((uint64_t)c.window_frames + c.hop_frames - 1) / c.hop_frames;
  if (k_open > peaq::kMeterBandsMaxOpen)
    return fail(PEAQ_ERR_ARG, who + ": window_frames " + std::to_string(c.window_frames) + " over hop_frames " +
                                  std::to_string(c.hop_frames) + " keeps " + std::to_string(k_open) +
                                  " windows open at once, more than the band meter's " +
                                  std::to_string(peaq::kMeterBandsMaxOpen));
  if (c.depth > peaq::kMeterBandsMaxDepth)
    return fail(PEAQ_ERR_ARG, who + ": depth " + std::to_string(c.depth) + " is outside the band meter's 1 .. " +
                                  std::to_string(peaq::kMeterBandsMaxDepth));
  return PEAQ_OK;
}
// doubles of the band meter's three device arrays per stream: the launch's planes, the open windows, the delivered ring
struct MeterBandSizes {
  size_t planes, open, ring, set;   // set: one reading's rows [channel][4][row]
  MeterBandSizes(uint32_t k_open, uint32_t ring_slots, unsigned max_frames, bool advanced, int channels) {
    const size_t row = (size_t)peaq::band_row(advanced ? 55 : 109);
    set = (size_t)channels * peaq::kMeterBandRows * row;
    planes = (size_t)max_frames * channels * 2 * row;
    open = (size_t)k_open * channels * (size_t)peaq::meter_band_snap(advanced ? 55 : 109);
    ring = (size_t)ring_slots * set;
  }
  size_t bytes() const { return (planes + open + ring) * sizeof(double); }
};
// windows that are complete once `units` frames have run: b_k = k H + W <= units
inline uint64_t meter_complete(uint64_t units, uint32_t W, uint32_t H) { return units >= W ? (units - W) / H + 1 : 0; }
// readings of a finished stream of T frames: the complete windows and, if the end cuts one short, the oldest such
inline uint64_t meter_rows(uint64_t T, uint32_t W, uint32_t H) {
  const uint64_t c = meter_complete(T, W, H);
  return c + (c * H < T ? 1 : 0);
}
// Row k without its result.  `ended`: the stream's lengths are known (its flush has been asked for); before that only
// complete windows are asked for, and none of them reaches the end.
inline void meter_row(uint64_t k, uint32_t W, uint32_t H, bool ended, uint64_t n_ref, uint64_t n_test,
                      peaq_meter_reading* row) {
  const uint64_t a = k * H, b = a + W;
  const uint64_t start = a ? 1024 * (a + 1) : 0, e = 1024 * (b + 1);
  row->index = k;
  row->start = start;
  row->first_frame = static_cast<uint32_t>(a);
  row->first_block = static_cast<uint32_t>(start / peaq::kFbFrame);
  row->n_frames = W;
  row->n_blocks = static_cast<uint32_t>(e / peaq::kFbFrame) - row->first_block;
  row->length = e - start;
  if (!ended) return;
  const uint64_t m = std::max(n_ref, n_test);
  const uint64_t T = count_frames(n_ref, n_test, peaq::kFrame, peaq::kHop);
  const uint64_t TB = count_frames(n_ref, n_test, peaq::kFbFrame, peaq::kFbFrame);
  if (b >= T) {                                      // takes the stream's last frame: blocks to the last
    row->n_frames = static_cast<uint32_t>(T - a);
    row->n_blocks = static_cast<uint32_t>(TB) - row->first_block;
    row->length = start >= m ? 0 : m - start;        // (only the flush frame: no sample window has exactly that)
  } else if (e == m) {
    row->length = 0;                                 // (the batch rule would add the flush frame)
  }
}

// ---------------------------------------------------------------------------
// Live alignment (include/peaq_amd.h, "live alignment"): the configuration as every entry that takes one checks it,
// rules A and B on the host, and a watch record from the device's state.  Host only.
// ---------------------------------------------------------------------------
constexpr uint32_t kLiveProbeMax = 1u << 20, kLiveProbeMargin = 2048;
// *probe: the probe with the default filled in
inline int check_live_align(const std::string& who, const peaq_live_align_config& c, uint32_t* probe) {
  if (c.reserved != 0) return fail(PEAQ_ERR_ARG, who + ": reserved " + std::to_string(c.reserved) + " must be 0");
  if (c.max_lag > 16384)
    return fail(PEAQ_ERR_ARG, who + ": max_lag " + std::to_string(c.max_lag) + " is outside 0 .. 16384");
  const uint32_t p = c.probe ? c.probe : 48000 + 2 * c.max_lag;
  if (p < c.max_lag + kLiveProbeMargin || p > kLiveProbeMax)
    return fail(PEAQ_ERR_ARG, who + ": probe " + std::to_string(p) + " is outside max_lag + 2048 = " +
                                  std::to_string(c.max_lag + kLiveProbeMargin) + " .. " + std::to_string(kLiveProbeMax));
  if (c.watch_frames > peaq::kWatchMaxFrames)
    return fail(PEAQ_ERR_ARG, who + ": watch_frames " + std::to_string(c.watch_frames) + " is outside 0 .. " +
                                  std::to_string(peaq::kWatchMaxFrames));
  *probe = p;
  return PEAQ_OK;
}
struct LiveAlignGeometry {
  uint32_t max_lag = 0, probe = 0, window = 0;       // max_lag 0: no acquisition; window 0: no watch
  bool on() const { return max_lag || window; }
};
// rule A for what the pads hold and the lag the aligner found
inline void live_align_plan(uint32_t probe, uint64_t have_ref, uint64_t have_test, int32_t lag, peaq_live_delay* out) {
  out->probe_ref = static_cast<uint32_t>(std::min<uint64_t>(have_ref, probe));
  out->probe_test = static_cast<uint32_t>(std::min<uint64_t>(have_test, probe));
  const uint64_t late = lag > 0 ? (uint64_t)lag : 0, early = lag < 0 ? (uint64_t)(-(int64_t)lag) : 0;
  out->skip_ref = static_cast<uint32_t>(std::min(early, have_ref));
  out->skip_test = static_cast<uint32_t>(std::min(late, have_test));
}
// the record of an acquisition: rule A for what the pads held, and the aligner's record (nullptr: no estimate ran
// because a pad was empty -- lag 0 and the all-zero record the aligner documents for an empty signal)
inline peaq_live_delay live_delay_acquired(uint32_t probe, const uint64_t have[2], const peaq_delay* rec) {
  peaq_live_delay d{};
  live_align_plan(probe, have[0], have[1], rec ? rec->lag : 0, &d);
  static_assert(sizeof d.d == sizeof(peaq_delay), "peaq_live_delay::d mirrors peaq_delay");
  if (rec) std::memcpy(&d.d, rec, sizeof(peaq_delay));
  d.acquired = 1;
  return d;
}
// The device workspace of live alignment, a session's or a broker's: `probes` probes a launch of the aligner, `streams`
// streams of at most max_frames whole frames a launch of the watch.
struct LiveAlignBuffers {
  DevBuf probe[2], rec;             // acquisition: the probes [probes][probe][channels], peaq_delay [probes]
  DevBuf rows, state;               // watch: one launch's rows [streams][max_frames][kWatchRow]; WatchState [streams]
  int reserve(const peaq_live_align_config& cfg, uint32_t probe_len, int channels, size_t probes, size_t streams,
              unsigned max_frames) {
    if (cfg.max_lag) {
      for (int p = 0; p < 2; ++p) HIP_TRY(probe[p].reserve(probes * probe_len * channels * sizeof(float)));
      HIP_TRY(rec.reserve(probes * sizeof(peaq_delay)));
    }
    if (cfg.watch_frames) {
      HIP_TRY(rows.reserve(streams * max_frames * peaq::kWatchRow * sizeof(double)));
      HIP_TRY(state.reserve(streams * sizeof(peaq::WatchState)));
    }
    return PEAQ_OK;
  }
  // the watch behind the front end `fa`, over n_frames whole frames of every stream (a broker adds s_frames, s_slot)
  peaq::WatchArgs watch(const peaq::FrontendArgs& fa, uint32_t window, uint32_t n_frames, uint32_t stride) const {
    peaq::WatchArgs wa{};
    wa.ref = fa.ref;
    wa.test = fa.test;
    wa.pair_stride = fa.pair_stride;
    wa.channels = fa.channels;
    wa.n_frames = n_frames;
    wa.window = window;
    wa.rows = rows.as<double>();
    wa.row_stride = stride;
    wa.state = state.as<peaq::WatchState>();
    return wa;
  }
};
// rule B's read-out of a window's sums: norm, the arg-max with the aligner's tie rule, the runner-up
inline void delay_watch_pick(const double* c, double e_ref, double e_test, int32_t* offset, double* peak,
                             double* runner_up, double* norm) {
  constexpr int D = peaq::kWatchLags;
  *offset = 0;
  *peak = *runner_up = *norm = 0.;
  const double e2 = e_ref * e_test;
  bool finite = std::isfinite(e2);
  for (int i = 0; i <= 2 * D; ++i) finite = finite && std::isfinite(c[i]);
  if (!finite) {
    *norm = std::nan("");
    return;
  }
  if (!(e2 > 0.)) return;
  const double nrm = std::sqrt(e2);
  double best = 0.;
  for (int i = 0; i <= 2 * D; ++i) best = std::max(best, std::fabs(c[i]));
  const double floor_ = best - 1e-12 * nrm;
  unsigned key = 0xFFFFFFFFu;                        // 2 |d| + (d < 0), as align_pick_kernel
  for (int d = -D; d <= D; ++d)
    if (std::fabs(c[d + D]) >= floor_) key = std::min(key, 2u * (unsigned)std::abs(d) + (d < 0 ? 1u : 0u));
  const int lag = (key & 1u) ? -(int)(key >> 1) : (int)(key >> 1);
  double second = 0.;
  for (int d = -D; d <= D; ++d)
    if (d != lag) second = std::max(second, std::fabs(c[d + D]));
  *offset = lag;
  *peak = c[lag + D];
  *runner_up = second;
  *norm = nrm;
}
// the public record of a stream's watch state as the device left it
inline void delay_watch_record(const peaq::WatchState& st, peaq_delay_watch* out) {
  std::memset(out, 0, sizeof *out);
  if (!st.latest_frames) return;
  out->index = st.latest_index;
  out->first_frame = st.latest_first;
  out->n_frames = st.latest_frames;
  std::memcpy(out->c, st.latest, sizeof out->c);
  out->e_ref = st.latest[peaq::kWatchCols - 2];
  out->e_test = st.latest[peaq::kWatchCols - 1];
  delay_watch_pick(out->c, out->e_ref, out->e_test, &out->offset, &out->peak, &out->runner_up, &out->norm);
}

// One geometry, and what the host keeps per metered stream (a session, a broker slot): guarded by the owner's lock.
struct MeterGeometry {
  bool on = false;
  bool bands = false;               // the band meter (set_meter_bands): only with `on`, off again with every set_meter
  uint32_t window = 0, hop = 0, depth = 0, k_open = 0;
  uint32_t ring = 0;                // depth + 2 slots: at a read the filter-bank path may have finished one window more
                                    // than the FFT path, and during a flush the FFT path two more than the other
  void set(const peaq_meter_config& c) {
    window = c.window_frames;
    hop = c.hop_frames;
    depth = c.depth;
    k_open = (c.window_frames + c.hop_frames - 1) / c.hop_frames;
    ring = c.depth + 2;
  }
};
// The meter's device workspace, a session's or a broker's: `streams` streams, each at most max_frames / max_blocks
// units a launch.  What depends on the launch (unit0, n_units, rec_stride, the totals, the s_* rows) is the caller's.
struct MeterBuffers {
  DevBuf open, ring;                // PointSnap [stream][k_open], [stream][ring]
  DevBuf frame_trc, block_trc;      // one launch's trace records [launch index][max_frames / max_blocks]: the live back
                                    // ends' output, the meter kernels' feed
  DevBuf readout;                   // ResultRecord [ring]
  std::vector<peaq::ResultRecord> host;
  size_t frame_stride = 0, block_stride = 0;
  // the band meter (reserve_bands): one launch's planes [launch index][max_frames][channel][2][row] -- the live-band back
  // ends' output, meter_bands_kernel's feed --, the open windows' rows and the delivered rows (peaq::MeterBandArgs)
  DevBuf band_planes, band_open, band_ring;
  size_t band_open_doubles = 0, band_ring_doubles = 0;   // per stream
  int reserve_bands(const MeterGeometry& g, size_t streams, unsigned max_frames, bool advanced, int channels) {
    const MeterBandSizes z(g.k_open, g.ring, max_frames, advanced, channels);
    HIP_TRY(band_planes.reserve(streams * z.planes * sizeof(double)));
    HIP_TRY(band_open.reserve(streams * z.open * sizeof(double)));
    HIP_TRY(band_ring.reserve(streams * z.ring * sizeof(double)));
    band_open_doubles = z.open;
    band_ring_doubles = z.ring;
    return PEAQ_OK;
  }
  // fresh rows for streams [first, first + count): no counted frame, status initial (kInit is 0), zeros delivered
  int restart_bands(size_t first, size_t count, hipStream_t stream) {
    static_assert(peaq::kInit == 0, "a fresh band snapshot is all zero bytes");
    HIP_TRY(hipMemsetAsync(band_open.as<double>() + first * band_open_doubles, 0,
                           count * band_open_doubles * sizeof(double), stream));
    HIP_TRY(hipMemsetAsync(band_ring.as<double>() + first * band_ring_doubles, 0,
                           count * band_ring_doubles * sizeof(double), stream));
    return PEAQ_OK;
  }
  peaq::MeterBandArgs band_args() const {
    return peaq::MeterBandArgs{band_planes.as<double>(), band_open.as<double>(), band_ring.as<double>()};
  }
  int reserve(const MeterGeometry& g, size_t streams, unsigned max_frames, unsigned max_blocks, bool advanced) {
    HIP_TRY(open.reserve(streams * g.k_open * sizeof(peaq::PointSnap)));
    HIP_TRY(ring.reserve(streams * g.ring * sizeof(peaq::PointSnap)));
    HIP_TRY(readout.reserve((size_t)g.ring * sizeof(peaq::ResultRecord)));
    HIP_TRY(frame_trc.reserve(streams * max_frames * sizeof(peaq::FrameTrace)));
    if (advanced) HIP_TRY(block_trc.reserve(streams * max_blocks * sizeof(peaq::BlockTrace)));
    try {
      host.resize(g.ring);
    } catch (const std::bad_alloc&) {
      return fail(PEAQ_ERR_NOMEM, "out of host memory");
    }
    frame_stride = max_frames;
    block_stride = max_blocks;
    return PEAQ_OK;
  }
  peaq::MeterArgs args(const MeterGeometry& g) const {
    peaq::MeterArgs m{};
    m.open = open.as<peaq::PointSnap>();
    m.ring = ring.as<peaq::PointSnap>();
    m.window = g.window;
    m.hop = g.hop;
    m.k_open = g.k_open;
    m.ring_depth = g.ring;
    m.frames = frame_trc.as<peaq::FrameTrace>();
    m.frame_stride = frame_stride;
    m.blocks = block_trc.as<peaq::BlockTrace>();
    m.block_stride = block_stride;
    return m;
  }
  // the live back ends' output: the launch's records at their index within the launch (no flush flag: n_uniform);
  // nothing with the meter off
  peaq::RunOutputs outputs(const MeterGeometry& g) const {
    peaq::RunOutputs out;
    if (g.on) {
      out.live.frames = frame_trc.as<peaq::FrameTrace>();
      out.live.frame_stride = frame_stride;
      out.live.blocks = block_trc.as<peaq::BlockTrace>();
      out.live.block_stride = block_stride;
      out.live.n_uniform = UINT_MAX;
      if (g.bands) {
        out.live_bnd.bands = band_planes.as<double>();
        out.live_bnd.frame_stride = frame_stride;
        out.live_bnd.planes = peaq::kBandNmr | peaq::kBandExcRef;
      }
    }
    return out;
  }
};
struct MeterStream {
  uint64_t n_taken = 0;             // readings handed out or counted as dropped so far
  bool ended = false;               // the flush has been asked for: the lengths, T and TB below are the stream's
  uint64_t n_ref = 0, n_test = 0;
  uint32_t total[2] = {0, 0};       // [kind]: T, TB
  void end(const StreamFramer& fr) {
    ended = true;
    n_ref = fr.scored(0);
    n_test = fr.scored(1);
    total[kUnitFrame] = count_frames(n_ref, n_test, peaq::kFrame, peaq::kHop);
    total[kUnitBlock] = count_frames(n_ref, n_test, peaq::kFbFrame, peaq::kFbFrame);
  }
  // what both paths have finished of the units handed out so far, by arithmetic alone
  uint64_t delivered(const StreamFramer& fr, const MeterGeometry& g) const {
    if (ended && fr.done[kUnitFrame] == total[kUnitFrame] && (!fr.advanced || fr.done[kUnitBlock] == total[kUnitBlock]))
      return meter_rows(total[kUnitFrame], g.window, g.hop);
    uint64_t d = meter_complete(fr.done[kUnitFrame], g.window, g.hop);
    if (fr.advanced) {
      // block e_k / 192 - 1 has run: e_k = 1024 (b_k + 1) < 192 (blocks + 1)
      const uint64_t f = (192ull * fr.done[kUnitBlock] + 191u) / 1024u;
      d = std::min(d, meter_complete(f >= 1 ? f - 1 : 0, g.window, g.hop));
    }
    // (a flush under way: the windows that take the last frame count only once both paths are at the end)
    return ended ? std::min(d, meter_complete(total[kUnitFrame] ? total[kUnitFrame] - 1 : 0, g.window, g.hop)) : d;
  }
  // The delivered, not yet read readings of the stream whose ring is `snaps`, oldest first, at most cap: the read-out
  // of their slots alone (at most two runs of the ring), then the rows' own fields.  Waits for `stream`.  With
  // band_rows, the band meter's rows of the same readings from the stream's ring of them, `band_ring`.
  int read(const StreamFramer& fr, const MeterGeometry& g, const peaq::PointSnap* snaps, DevBuf& readout,
           std::vector<peaq::ResultRecord>& host, int channels, hipStream_t stream, const peaq::Settings& cfg,
           peaq_meter_reading* out, int cap, int* n_read, uint64_t* dropped, const double* band_ring = nullptr,
           double* band_rows = nullptr, size_t band_set = 0) {
    const uint64_t have = delivered(fr, g);
    uint64_t from = n_taken;
    if (have > g.depth && from < have - g.depth) from = have - g.depth;
    if (dropped) *dropped = from - n_taken;
    n_taken = from;
    const uint64_t n = std::min<uint64_t>(have - from, (uint64_t)cap);
    if (n == 0) return PEAQ_OK;
    for (uint64_t done = 0; done < n;) {
      const uint32_t s0 = static_cast<uint32_t>((from + done) % g.ring);
      const uint32_t run = static_cast<uint32_t>(std::min<uint64_t>(n - done, g.ring - s0));
      HIP_TRY(peaq::launch_finalize_points(snaps + s0, fr.advanced, channels, 1, (int)run,
                                           readout.as<peaq::ResultRecord>() + s0, stream, cfg));
      HIP_TRY(hipMemcpyAsync(host.data() + s0, readout.as<peaq::ResultRecord>() + s0, run * sizeof(peaq::ResultRecord),
                             hipMemcpyDeviceToHost, stream));
      // (band_rows: the rows of the same slots, `band_set` doubles a reading, straight into the caller's array)
      if (band_rows)
        HIP_TRY(hipMemcpyAsync(band_rows + done * band_set, band_ring + s0 * band_set, run * band_set * sizeof(double),
                               hipMemcpyDeviceToHost, stream));
      done += run;
    }
    HIP_TRY(hipStreamSynchronize(stream));
    static_assert(sizeof(peaq::ResultRecord) == sizeof(peaq_result), "ResultRecord mirrors peaq_result");
    for (uint64_t i = 0; i < n; ++i) {
      meter_row(from + i, g.window, g.hop, ended, n_ref, n_test, out + i);
      std::memcpy(&out[i].r, &host[(from + i) % g.ring], sizeof(peaq_result));
    }
    n_taken = from + n;
    *n_read = static_cast<int>(n);
    return PEAQ_OK;
  }
};

// ---------------------------------------------------------------------------
// What one slot of the broker contributes to one tick (peaq_broker.hip, peaq_debug_broker_plan): at most one window
// per kind -- whole units (do_processing), else, once per flush, the zero-padded unit of do_flush.  Host only; the
// owner holds the slot's lock, and the stream is not held.  Only positions are taken: the samples are copied later,
// and trim() is the caller's, behind that copy.
// ---------------------------------------------------------------------------
struct SlotTake {
  StreamWindow fft, fb;             // count 0: none of that kind
  bool closing = false;             // meter: the blocks ended in this tick without a flush block -- the windows that run to
                                    // the last block are delivered by an entry without units (block0 = the stream's blocks)
};
inline SlotTake take_slot_windows(StreamFramer& fr, SlotFlush& fl, MeterStream& ms, bool metered, bool advanced,
                                  unsigned max_frames, unsigned max_blocks) {
  SlotTake t;
  const bool flush_fft = fl.requested && !fl.fft_done;
  if (metered && fl.requested && !ms.ended) ms.end(fr);   // the stream's end is known from here on
  t.fft = fr.take(kUnitFrame, max_frames, flush_fft);
  if (flush_fft && (t.fft.flush || !t.fft.count)) fl.fft_done = true;   // (no whole frame was left)
  if (advanced) {
    // With the meter on the two paths of a stream stay at a common sample horizon, so that a window's two halves
    // meet in the delivered ring: the blocks go no further than the frame after the last one taken, 1024 (frames + 2)
    // samples.  Whatever blocks are whole while no frame is lie below that, so nothing waits that a tick without the
    // meter would take unless a frame waits too; and 48 blocks a tick outrun 8 frames.  The cap holds through a
    // flush's backlog as well, until the stream's last frame has been taken (above, in this tick at the latest):
    // only the tail of the blocks, and the flush block, run free.
    const bool capped = metered && (!ms.ended || fr.done[kUnitFrame] < ms.total[kUnitFrame]);
    const bool flush_fb = fl.requested && !fl.fb_done && !capped;
    unsigned fb_cap = max_blocks;
    if (capped) {
      const uint64_t reach = 1024ull * ((uint64_t)fr.done[kUnitFrame] + 2) / peaq::kFbFrame;
      const uint64_t room = reach > fr.done[kUnitBlock] ? reach - fr.done[kUnitBlock] : 0;
      fb_cap = (unsigned)std::min<uint64_t>(room, max_blocks);
    }
    if (fb_cap) t.fb = fr.take(kUnitBlock, fb_cap, flush_fb);
    if (flush_fb && (t.fb.flush || !t.fb.count)) {
      fl.fb_done = true;
      // (a window whose streaming end fell on the last block was stored then already: the closing entry stores the
      // same fields again)
      t.closing = metered && !t.fb.count && ms.total[kUnitFrame];
    }
  }
  if (fl.requested && fl.fft_done && (!advanced || fl.fb_done)) fl.clear();
  return t;
}

// peaq_session.hip -- streaming sessions: one per `peaq` element instance / (ref, test) stream.
#include "peaq_host.h"

using namespace peaq;

struct peaq_session {
  peaq_ctx* ctx = nullptr;
  int advanced = 0, channels = 1;
  double level_db = 92.;
  Settings cfg;                     // the context's settings when the session was created
  std::mutex mu;
  StreamFramer framer;            // the two pads' FIFOs and where the next frame / block starts (guarded by mu)
  DevBuf fb_records, fbstate, hp_rows;
  hipStream_t stream = nullptr;
  hipEvent_t staged = nullptr;    // the pinned staging buffers may be rewritten after this
  bool staged_pending = false;
  float* h_stage[2] = {nullptr, nullptr};   // pinned
  DevBuf d_sig[2], records, state, result;
  size_t stage_samples = 0;

  ModelSetup model() const { return ModelSetup{ctx, cfg, advanced, channels, level_db}; }
};

static int session_alloc(peaq_session* s) {
  s->stage_samples = (size_t)(kSessionMaxFrames - 1) * kHop + kFrame;   // >= kSessionMaxBlocks * 192
  const size_t bytes = s->stage_samples * s->channels * sizeof(float);
  for (int p = 0; p < 2; ++p) {
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&s->h_stage[p]), bytes, hipHostMallocDefault));
    HIP_TRY(s->d_sig[p].reserve(bytes));
  }
  HIP_TRY(s->records.reserve((size_t)kSessionMaxFrames * s->channels * kRecDoubles * sizeof(double)));
  HIP_TRY(s->state.reserve(sizeof(PairState)));
  HIP_TRY(s->result.reserve(sizeof(ResultRecord)));
  HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&s->staged, hipEventDisableTiming));
  HIP_TRY(launch_state_init(s->state.as<PairState>(), s->advanced, 1, s->stream));
  if (s->advanced) {
    const unsigned n_signals = 2 * s->channels;
    HIP_TRY(s->fb_records.reserve((size_t)kSessionMaxBlocks * s->channels * kFbRecDoubles * sizeof(double)));
    HIP_TRY(s->fbstate.reserve(n_signals * sizeof(FbSignalState)));
    HIP_TRY(hipMemsetAsync(s->fbstate.p, 0, n_signals * sizeof(FbSignalState), s->stream));
    HIP_TRY(s->hp_rows.reserve((size_t)n_signals * (kFbRing + (size_t)kSessionMaxBlocks * kFbFrame) * sizeof(double)));
  }
  return PEAQ_OK;
}

extern "C" int peaq_session_create(peaq_ctx* c, int advanced, int channels, double level_db, peaq_session** out) {
  if (!c || !out) return fail(PEAQ_ERR_ARG, "peaq_session_create: NULL argument");
  *out = nullptr;
  if (int rc = check_channels("peaq_session_create", channels)) return rc;
  if (int rc = check_level("peaq_session_create", level_db)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  peaq_session* s = new (std::nothrow) peaq_session;
  if (!s) return fail(PEAQ_ERR_NOMEM, "out of host memory");
  s->ctx = c;
  s->cfg = c->settings;
  s->advanced = advanced ? 1 : 0;
  s->channels = channels;
  s->level_db = level_db;
  s->framer.reset(s->advanced, channels);
  const int rc = session_alloc(s);
  if (rc != PEAQ_OK) {
    peaq_session_destroy(s);
    return rc;
  }
  *out = s;
  return PEAQ_OK;
}

extern "C" void peaq_session_destroy(peaq_session* s) {
  if (!s) return;
  (void)hipSetDevice(s->ctx->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  for (int p = 0; p < 2; ++p)
    if (s->h_stage[p]) (void)hipHostFree(s->h_stage[p]);
  if (s->staged) (void)hipEventDestroy(s->staged);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;                         // (the device buffers go with it)
}

// the samples of window w: FIFOs -> pinned staging -> device
static int session_stage(peaq_session* s, const StreamWindow& w) {
  if (s->staged_pending) {
    HIP_TRY(hipEventSynchronize(s->staged));
    s->staged_pending = false;
  }
  stage_window(s->framer, w, s->h_stage);
  for (int p = 0; p < 2; ++p)
    if (w.valid[p])
      HIP_TRY(hipMemcpyAsync(s->d_sig[p].p, s->h_stage[p], (size_t)w.valid[p] * s->channels * sizeof(float),
                             hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipEventRecord(s->staged, s->stream));
  s->staged_pending = true;
  return PEAQ_OK;
}

// run the FFT frames of window w (valid[] is shorter than whole frames only for the flush frame)
static int session_run_frames(peaq_session* s, const StreamWindow& w) {
  {
    const int rc = session_stage(s, w);
    if (rc != PEAQ_OK) return rc;
  }
  const ModelSetup m = s->model();
  FrontendArgs fa = m.frontend();
  fa.ref = s->d_sig[0].as<float>();
  fa.test = s->d_sig[1].as<float>();
  fa.pair_stride = s->stage_samples;
  fa.n_uniform_ref = static_cast<uint32_t>(w.valid[0]);
  fa.n_uniform_test = static_cast<uint32_t>(w.valid[1]);
  fa.n_frames_uniform = w.first + w.count;
  fa.frame_origin = w.first;
  fa.frame0 = w.first;
  fa.frames_per_launch = w.count;
  fa.records = s->records.as<double>();
  HIP_TRY(launch_frontend(m.fft_bands(), fa, 1, s->stream));
  BackendArgs ba = m.backend(fa);
  ba.frame0 = w.first;
  ba.frames_per_launch = w.count;
  ba.n_frames_uniform = w.first + w.count;
  ba.state = s->state.as<PairState>();
  HIP_TRY(launch_backend(ba, 1, s->stream));
  return PEAQ_OK;
}

// run the filter-bank blocks of window w (advanced mode)
static int session_run_blocks(peaq_session* s, const StreamWindow& w) {
  {
    const int rc = session_stage(s, w);
    if (rc != PEAQ_OK) return rc;
  }
  const ModelSetup m = s->model();
  FbFrontArgs ff = m.fb_frontend();
  ff.ref = s->d_sig[0].as<float>();
  ff.test = s->d_sig[1].as<float>();
  ff.pair_stride = s->stage_samples;
  ff.n_uniform_ref = static_cast<uint32_t>(w.valid[0]);
  ff.n_uniform_test = static_cast<uint32_t>(w.valid[1]);
  ff.n_blocks_uniform = w.first + w.count;
  ff.block_origin = w.first;
  ff.block0 = w.first;
  ff.blocks_per_launch = w.count;
  ff.prev_blocks = w.prev_blocks;
  ff.first_launch = w.first == 0;
  ff.fbstate = s->fbstate.as<FbSignalState>();
  ff.hp_scratch = s->hp_rows.as<double>();
  ff.hp_row_stride = kFbRing + (size_t)kSessionMaxBlocks * kFbFrame;
  ff.records = s->fb_records.as<double>();
  HIP_TRY(launch_fb_frontend(ff, 1, s->stream));
  FbBackendArgs fbk = m.fb_backend(ff);
  fbk.block0 = w.first;
  fbk.blocks_per_launch = w.count;
  fbk.n_blocks_uniform = w.first + w.count;
  fbk.state = s->state.as<PairState>();
  HIP_TRY(launch_fb_backend(fbk, 1, s->stream));
  return PEAQ_OK;
}

// do_processing (gstpeaq.c:596-611), and with `flushing` do_flush (gstpeaq.c:716-745, 769-771)
static int session_drain(peaq_session* s, bool flushing) {
  return drain_stream(s->framer, kSessionMaxFrames, kSessionMaxBlocks, flushing,
                      [s](StreamUnit kind, const StreamWindow& w) {
                        return kind == kUnitBlock ? session_run_blocks(s, w) : session_run_frames(s, w);
                      });
}

extern "C" int peaq_session_push(peaq_session* s, int pad, const float* data, size_t n) {
  if (!s) return fail(PEAQ_ERR_ARG, "peaq_session_push: session is NULL");
  if (pad != 0 && pad != 1) return fail(PEAQ_ERR_ARG, "peaq_session_push: pad must be 0 (ref) or 1 (test)");
  if (n == 0) return PEAQ_OK;
  if (!data) return fail(PEAQ_ERR_ARG, "peaq_session_push: data is NULL");
  std::lock_guard<std::mutex> lock(s->mu);          // GST_OBJECT_LOCK in pad_chain (gstpeaq.c:619)
  HIP_TRY(hipSetDevice(s->ctx->device));
  try {
    s->framer.append(pad, data, n);
  } catch (const std::bad_alloc&) {
    return fail(PEAQ_ERR_NOMEM, "out of host memory");
  }
  return session_drain(s, false);
}

extern "C" int peaq_session_flush(peaq_session* s) {
  if (!s) return fail(PEAQ_ERR_ARG, "peaq_session_flush: session is NULL");
  std::lock_guard<std::mutex> lock(s->mu);
  HIP_TRY(hipSetDevice(s->ctx->device));
  return session_drain(s, true);
}

extern "C" int peaq_session_results(peaq_session* s, peaq_result* out) {
  if (!s || !out) return fail(PEAQ_ERR_ARG, "peaq_session_results: NULL argument");
  std::lock_guard<std::mutex> lock(s->mu);
  HIP_TRY(hipSetDevice(s->ctx->device));
  HIP_TRY(launch_finalize(s->state.as<PairState>(), s->advanced, s->channels, 1, s->result.as<ResultRecord>(),
                          s->stream, s->cfg));
  HIP_TRY(hipMemcpyAsync(out, s->result.p, sizeof(peaq_result), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return PEAQ_OK;
}

extern "C" int peaq_session_set_level(peaq_session* s, double level_db) {
  if (!s) return fail(PEAQ_ERR_ARG, "peaq_session_set_level: session is NULL");
  if (int rc = check_level("peaq_session_set_level", level_db)) return rc;
  std::lock_guard<std::mutex> lock(s->mu);
  s->level_db = level_db;            // the level factors are per-launch kernel arguments
  return PEAQ_OK;
}

extern "C" int peaq_session_reset(peaq_session* s) {
  if (!s) return fail(PEAQ_ERR_ARG, "peaq_session_reset: session is NULL");
  std::lock_guard<std::mutex> lock(s->mu);
  HIP_TRY(hipSetDevice(s->ctx->device));
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->framer.reset(s->advanced, s->channels);
  if (s->advanced)
    HIP_TRY(hipMemsetAsync(s->fbstate.p, 0, 2 * s->channels * sizeof(FbSignalState), s->stream));
  HIP_TRY(launch_state_init(s->state.as<PairState>(), s->advanced, 1, s->stream));
  return PEAQ_OK;
}

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
  DevBuf d_sig, records, state, result;     // d_sig: the two pads' windows, [pad][stage_samples][channels]
  size_t stage_samples = 0;
  float* sig(int p) const { return d_sig.as<float>() + (size_t)p * stage_samples * channels; }

  // live rate conversion (peaq_session_set_rates; peaq_live_rate.hip), guarded by mu like the rest: the raw samples
  // behind a window of a rated pad, [pad][h_raw_samples] pinned and [pad][d_raw_samples] on the device (the device
  // rows take a probe's raw samples as well)
  float* h_raw = nullptr;
  DevBuf d_raw;
  size_t h_raw_samples = 0, d_raw_samples = 0;
  float* raw_host(int p) const { return h_raw + (size_t)p * h_raw_samples * channels; }
  float* raw_dev(int p) const { return d_raw.as<float>() + (size_t)p * d_raw_samples * channels; }

  // the meter (peaq_session_set_meter; peaq_meter.hip), guarded by mu like the rest
  struct Meter : MeterGeometry, MeterStream {
    MeterBuffers buf;               // one stream, kSessionMaxFrames / kSessionMaxBlocks units a launch
    bool closed[2] = {false, false};   // [kind]: a launch that ends this path's units has gone out
  } meter;

  // live alignment (peaq_session_set_align; peaq_watch.hip), guarded by mu like the rest
  struct Align : LiveAlignGeometry {
    LiveAlignBuffers buf;           // one probe a launch of the aligner, one stream of the watch
    peaq_live_delay delay{};        // all zero while the stream holds
  } align;

  ModelSetup model() const { return ModelSetup{ctx, cfg, advanced, channels, level_db}; }
};

// behind a back-end launch of a metered session: the launch's units into the open windows; a launch that ends the
// path's units (count may be 0) delivers the windows that run to the stream's end
static int session_meter_step(peaq_session* s, StreamUnit kind, uint32_t first, uint32_t count) {
  const peaq_session::Meter& mt = s->meter;
  MeterArgs m = mt.buf.args(mt);
  m.unit0 = first;
  m.n_units = count;
  m.rec_stride = count;
  m.total_frames = mt.ended ? mt.total[kUnitFrame] : UINT_MAX;
  m.total_units = mt.ended ? mt.total[kind] : UINT_MAX;
  if (kind == kUnitFrame) {
    HIP_TRY(launch_meter_fft(m, s->advanced != 0, s->records.as<double>(), s->channels, 1, s->stream));
    if (mt.bands) HIP_TRY(launch_meter_bands(m, mt.buf.band_args(), s->advanced != 0, s->channels, 1, s->stream));
  } else
    HIP_TRY(launch_meter_fb(m, s->channels, 1, s->stream));
  if (s->meter.ended && first + count == s->meter.total[kind]) s->meter.closed[kind] = true;
  return PEAQ_OK;
}

// a fresh meter of the geometry that is set: every snapshot as launch_points_init leaves it, the index at 0
static int session_meter_restart(peaq_session* s) {
  peaq_session::Meter& mt = s->meter;
  HIP_TRY(launch_points_init(mt.buf.open.as<PointSnap>(), mt.k_open, s->stream));
  HIP_TRY(launch_points_init(mt.buf.ring.as<PointSnap>(), mt.ring, s->stream));
  if (mt.bands)
    if (int rc = mt.buf.restart_bands(0, 1, s->stream)) return rc;
  static_cast<MeterStream&>(mt) = MeterStream();
  mt.closed[0] = mt.closed[1] = false;
  return PEAQ_OK;
}

// a fresh stream for the alignment that is set: held until the delay is acquired, the watch at index 0
static int session_align_restart(peaq_session* s) {
  peaq_session::Align& al = s->align;
  al.delay = peaq_live_delay{};
  if (al.max_lag) s->framer.hold();
  if (al.window) HIP_TRY(hipMemsetAsync(al.buf.state.p, 0, sizeof(WatchState), s->stream));
  return PEAQ_OK;
}

// Rule A: the delay of the probes the two pads hold, by the batch aligner on the session's stream; the one wait of the
// stream; the framer released with the skips.  Within the push or the flush that completes the probe.
static int session_acquire(peaq_session* s) {
  peaq_session::Align& al = s->align;
  StreamFramer& fr = s->framer;
  const uint64_t have[2] = {fr.have(0), fr.have(1)};   // (a rated pad: converted samples, as the probe and the skips)
  const uint32_t n[2] = {static_cast<uint32_t>(std::min<uint64_t>(have[0], al.probe)),
                         static_cast<uint32_t>(std::min<uint64_t>(have[1], al.probe))};
  peaq_delay rec{};                                  // (an empty pad: the record the aligner documents for it)
  if (n[0] && n[1]) {
    for (int p = 0; p < 2; ++p) {
      if (!fr.rated(p)) {
        HIP_TRY(hipMemcpyAsync(al.buf.probe[p].p, fr.pad[p].at(0, s->channels), (size_t)n[p] * s->channels * sizeof(float),
                               hipMemcpyHostToDevice, s->stream));
        continue;
      }
      // the probe's raw samples up, converted into the probe buffer
      uint64_t lo, hi;
      fr.raw_span(p, 0, n[p], &lo, &hi);
      HIP_TRY(hipMemcpyAsync(s->raw_dev(p), fr.pad[p].at(lo, s->channels), (size_t)(hi - lo) * s->channels * sizeof(float),
                             hipMemcpyHostToDevice, s->stream));
      const peaq_rate_segment seg{0, lo, fr.ended ? fr.pad[p].total : UINT64_MAX, n[p], static_cast<uint32_t>(hi - lo)};
      if (int rc = live_rate_convert(s->ctx, s->channels, fr.rate[p], 1, &seg, s->raw_dev(p), s->d_raw_samples,
                                             al.buf.probe[p].as<float>(), al.probe, s->stream))
        return rc;
    }
    if (int rc = peaq_batch_estimate_delay(s->ctx, s->channels, 1, al.buf.probe[0].as<float>(), al.buf.probe[1].as<float>(),
                                           al.probe, n, n + 1, 0, al.max_lag, al.buf.rec.as<peaq_delay>(), s->stream))
      return rc;
    HIP_TRY(hipMemcpyAsync(&rec, al.buf.rec.p, sizeof rec, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
  al.delay = live_delay_acquired(al.probe, have, &rec);
  fr.release(al.delay.skip_ref, al.delay.skip_test);
  return PEAQ_OK;
}

static int session_alloc(peaq_session* s) {
  s->stage_samples = (size_t)(kSessionMaxFrames - 1) * kHop + kFrame;   // >= kSessionMaxBlocks * 192
  const size_t bytes = s->stage_samples * s->channels * sizeof(float);
  for (int p = 0; p < 2; ++p)
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&s->h_stage[p]), bytes, hipHostMallocDefault));
  HIP_TRY(s->d_sig.reserve(2 * bytes));
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
  if (s->h_raw) (void)hipHostFree(s->h_raw);
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
  const StreamFramer& fr = s->framer;
  peaq_rate_segment seg[2];
  float* const raw[2] = {s->h_raw ? s->raw_host(0) : nullptr, s->h_raw ? s->raw_host(1) : nullptr};
  peaq_rate_segment* const segp[2] = {&seg[0], &seg[1]};
  stage_window(fr, w, s->h_stage, raw, segp);
  for (int p = 0; p < 2; ++p) {
    const size_t n = fr.rated(p) ? seg[p].in_have : w.valid[p];
    if (n)
      HIP_TRY(hipMemcpyAsync(fr.rated(p) ? s->raw_dev(p) : s->sig(p), fr.rated(p) ? raw[p] : s->h_stage[p],
                             n * s->channels * sizeof(float), hipMemcpyHostToDevice, s->stream));
  }
  HIP_TRY(hipEventRecord(s->staged, s->stream));
  s->staged_pending = true;
  // rated pads: the range converter writes the window in place of the copy -- both pads in one launch where they share
  // a rate, the rows of d_raw and d_sig being the pads
  const bool both = fr.rated(0) && fr.rate[0] == fr.rate[1];
  for (int p = 0; p < 2; ++p) {
    if (!fr.rated(p) || (both && p)) continue;
    if (int rc = live_rate_convert(s->ctx, s->channels, fr.rate[p], both ? 2 : 1, seg + p, s->raw_dev(p),
                                           s->d_raw_samples, s->sig(p), s->stage_samples, s->stream))
      return rc;
  }
  return PEAQ_OK;
}

// the raw staging of the rated pads, for the largest window and (device side) the probe of an acquisition
static int session_raw_reserve(peaq_session* s) {
  const StreamFramer& fr = s->framer;
  size_t h_need = 0, d_need = 0;
  for (int p = 0; p < 2; ++p) {
    if (!fr.rated(p)) continue;
    h_need = std::max(h_need, live_rate_span_max(fr.geo[p], s->stage_samples));
    d_need = std::max(d_need, live_rate_span_max(fr.geo[p], std::max<size_t>(s->stage_samples, s->align.probe)));
  }
  if (h_need > s->h_raw_samples) {
    if (s->h_raw) (void)hipHostFree(s->h_raw);
    s->h_raw = nullptr;
    s->h_raw_samples = 0;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&s->h_raw), 2 * h_need * s->channels * sizeof(float), hipHostMallocDefault));
    s->h_raw_samples = h_need;
  }
  if (d_need > s->d_raw_samples) {
    HIP_TRY(s->d_raw.reserve(2 * d_need * s->channels * sizeof(float)));
    s->d_raw_samples = d_need;
  }
  return PEAQ_OK;
}

// run the FFT frames of window w (valid[] is shorter than whole frames only for the flush frame)
static int session_run_frames(peaq_session* s, const StreamWindow& w) {
  if (int rc = session_stage(s, w)) return rc;
  const ModelSetup m = s->model();
  FrontendArgs fa = m.frontend();
  fa.ref = s->sig(0);
  fa.test = s->sig(1);
  fa.pair_stride = s->stage_samples;
  fa.n_uniform_ref = static_cast<uint32_t>(w.valid[0]);
  fa.n_uniform_test = static_cast<uint32_t>(w.valid[1]);
  fa.n_frames_uniform = w.first + w.count;
  fa.frame_origin = w.first;
  fa.frame0 = w.first;
  fa.frames_per_launch = w.count;
  fa.records = s->records.as<double>();
  HIP_TRY(launch_frontend(m.fft_bands(), fa, 1, s->stream));
  if (s->align.window && !w.flush) {
    const WatchArgs wa = s->align.buf.watch(fa, s->align.window, w.count, w.count);
    HIP_TRY(launch_delay_watch(wa, 1, s->stream));
  }
  BackendArgs ba = m.backend(fa);
  ba.frame0 = w.first;
  ba.frames_per_launch = w.count;
  ba.n_frames_uniform = w.first + w.count;
  ba.state = s->state.as<PairState>();
  HIP_TRY(launch_backend(ba, 1, s->stream, s->meter.buf.outputs(s->meter)));
  return s->meter.on ? session_meter_step(s, kUnitFrame, w.first, w.count) : PEAQ_OK;
}

// run the filter-bank blocks of window w (advanced mode)
static int session_run_blocks(peaq_session* s, const StreamWindow& w) {
  if (int rc = session_stage(s, w)) return rc;
  const ModelSetup m = s->model();
  FbFrontArgs ff = m.fb_frontend();
  ff.ref = s->sig(0);
  ff.test = s->sig(1);
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
  HIP_TRY(launch_fb_backend(fbk, 1, s->stream, s->meter.buf.outputs(s->meter)));
  return s->meter.on ? session_meter_step(s, kUnitBlock, w.first, w.count) : PEAQ_OK;
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
  if (s->framer.ended && s->framer.rated(pad))
    return fail(PEAQ_ERR_STATE, "peaq_session_push: the stream of a pad at " + std::to_string(s->framer.rate[pad]) +
                                    " Hz ended at its flush; peaq_session_reset starts the next one");
  HIP_TRY(hipSetDevice(s->ctx->device));
  try {
    s->framer.append(pad, data, n);
  } catch (const std::bad_alloc&) {
    return fail(PEAQ_ERR_NOMEM, "out of host memory");
  }
  if (s->framer.held && std::min(s->framer.have(0), s->framer.have(1)) >= s->align.probe)
    if (int rc = session_acquire(s)) return rc;
  return session_drain(s, false);
}

extern "C" int peaq_session_flush(peaq_session* s) {
  if (!s) return fail(PEAQ_ERR_ARG, "peaq_session_flush: session is NULL");
  std::lock_guard<std::mutex> lock(s->mu);
  HIP_TRY(hipSetDevice(s->ctx->device));
  s->framer.ended = true;                            // (rated pads: what is there converts to the end)
  if (s->framer.held)                                // the probe is what is there
    if (int rc = session_acquire(s)) return rc;
  peaq_session::Meter& mt = s->meter;
  const bool ends_now = mt.on && !mt.ended;
  if (ends_now) mt.end(s->framer);                   // the stream's end is known from here on: the launches below carry it
  if (int rc = session_drain(s, true)) {
    // (a device error: the stream is lost as after any failed call; the meter at least does not report an end)
    if (ends_now) {
      mt.ended = false;
      mt.closed[0] = mt.closed[1] = false;
    }
    return rc;
  }
  if (mt.on && mt.total[kUnitFrame]) {
    // a path whose units were all whole ones has no flush unit: its windows that run to the end are delivered by a
    // launch without units
    for (StreamUnit kind : {kUnitFrame, kUnitBlock}) {
      if (kind == kUnitBlock && !s->advanced) break;
      if (!mt.closed[kind] && s->framer.done[kind] == mt.total[kind])
        if (int rc = session_meter_step(s, kind, mt.total[kind], 0)) return rc;
    }
  }
  return PEAQ_OK;
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
  if (s->align.on())
    if (int rc = session_align_restart(s)) return rc;
  return s->meter.on ? session_meter_restart(s) : PEAQ_OK;
}

// the meter and the alignment are set on a stream that has not begun (the caller holds the session's lock)
static int session_not_begun(const peaq_session* s, const std::string& who, const char* what) {
  const uint64_t pushed = s->framer.pad[0].total + s->framer.pad[1].total;
  if (!pushed) return PEAQ_OK;
  return fail(PEAQ_ERR_ARG, who + ": the stream has begun (" + std::to_string(pushed) + " samples pushed); set " + what +
                                " before the first push or right after peaq_session_reset");
}

extern "C" size_t peaq_meter_reading_size(void) { return sizeof(peaq_meter_reading); }

extern "C" int peaq_meter_frames(double seconds, uint32_t* frames) {
  if (!frames) return fail(PEAQ_ERR_ARG, "peaq_meter_frames: frames is NULL");
  if (!(seconds >= 0.) || !(seconds <= 1e6))
    return fail(PEAQ_ERR_ARG, "peaq_meter_frames: seconds " + std::to_string(seconds) + " is outside 0 .. 1e6");
  const long long f = std::llround(seconds * 48000. / 1024.);
  *frames = static_cast<uint32_t>(f < 1 ? 1 : f);
  return PEAQ_OK;
}

extern "C" int peaq_meter_readings(uint64_t n_ref, uint64_t n_test, const peaq_meter_config* cfg, peaq_meter_reading* rows,
                                  int cap, int* n) {
  if (!cfg || !n) return fail(PEAQ_ERR_ARG, "peaq_meter_readings: NULL argument");
  if (cfg->window_frames < 1 || cfg->hop_frames < 1)
    return fail(PEAQ_ERR_ARG, "peaq_meter_readings: window_frames " + std::to_string(cfg->window_frames) +
                                  " and hop_frames " + std::to_string(cfg->hop_frames) + " must both be at least 1");
  if (cap < 0 || (cap > 0 && !rows))
    return fail(PEAQ_ERR_ARG, "peaq_meter_readings: cap " + std::to_string(cap) + " with rows " + (rows ? "set" : "NULL"));
  const uint64_t total = meter_rows(count_frames(n_ref, n_test, kFrame, kHop), cfg->window_frames, cfg->hop_frames);
  if (total > (uint64_t)INT_MAX) return fail(PEAQ_ERR_ARG, "peaq_meter_readings: more than INT_MAX rows");
  for (uint64_t k = 0; k < total && k < (uint64_t)cap; ++k)
    meter_row(k, cfg->window_frames, cfg->hop_frames, true, n_ref, n_test, rows + k);
  *n = static_cast<int>(total);
  return PEAQ_OK;
}

extern "C" int peaq_session_set_meter(peaq_session* s, const peaq_meter_config* cfg) {
  if (!s) return fail(PEAQ_ERR_ARG, "peaq_session_set_meter: session is NULL");
  const bool off = !cfg || cfg->window_frames == 0;
  if (!off)
    if (int rc = check_meter_config("peaq_session_set_meter", *cfg)) return rc;
  std::lock_guard<std::mutex> lock(s->mu);
  if (int rc = session_not_begun(s, "peaq_session_set_meter", "the meter")) return rc;
  peaq_session::Meter& mt = s->meter;
  mt.bands = false;                                  // (the band meter goes with the geometry: meter first, then bands)
  if (off) {
    mt.on = false;
    return PEAQ_OK;
  }
  HIP_TRY(hipSetDevice(s->ctx->device));
  mt.on = false;                                     // (stays off if the workspace cannot be reserved)
  MeterGeometry g;
  g.set(*cfg);
  HIP_TRY(hipStreamSynchronize(s->stream));          // (the buffers may be replaced)
  if (int rc = mt.buf.reserve(g, 1, kSessionMaxFrames, kSessionMaxBlocks, s->advanced != 0)) return rc;
  mt.set(*cfg);
  if (int rc = session_meter_restart(s)) return rc;
  mt.on = true;
  return PEAQ_OK;
}

// peaq_session_meter_read and (with_rows) peaq_session_meter_read_bands: one cursor
static int session_meter_read(peaq_session* s, const std::string& who, peaq_meter_reading* out, bool with_rows, double* rows,
                              int cap, int* n_read, uint64_t* dropped) {
  if (!s || !n_read) return fail(PEAQ_ERR_ARG, who + ": NULL argument");
  *n_read = 0;
  if (dropped) *dropped = 0;
  if (cap < 0 || (cap > 0 && !out))
    return fail(PEAQ_ERR_ARG, who + ": cap " + std::to_string(cap) + " with out " + (out ? "set" : "NULL"));
  if (with_rows && cap > 0 && !rows) return fail(PEAQ_ERR_ARG, who + ": cap " + std::to_string(cap) + " with rows NULL");
  std::lock_guard<std::mutex> lock(s->mu);
  peaq_session::Meter& mt = s->meter;
  if (!mt.on) return fail(PEAQ_ERR_ARG, who + ": the meter is off (peaq_session_set_meter)");
  if (with_rows && !mt.bands) return fail(PEAQ_ERR_ARG, who + ": the band meter is off (peaq_session_set_meter_bands)");
  HIP_TRY(hipSetDevice(s->ctx->device));
  const size_t set = with_rows ? MeterBandSizes(mt.k_open, mt.ring, 0, s->advanced != 0, s->channels).set : 0;
  return mt.read(s->framer, mt, mt.buf.ring.as<PointSnap>(), mt.buf.readout, mt.buf.host, s->channels, s->stream, s->cfg,
                 out, cap, n_read, dropped, mt.buf.band_ring.as<double>(), with_rows ? rows : nullptr, set);
}

extern "C" int peaq_session_meter_read(peaq_session* s, peaq_meter_reading* out, int cap, int* n_read, uint64_t* dropped) {
  return session_meter_read(s, "peaq_session_meter_read", out, false, nullptr, cap, n_read, dropped);
}

extern "C" int peaq_session_meter_read_bands(peaq_session* s, peaq_meter_reading* out, double* rows, int cap, int* n_read,
                                             uint64_t* dropped) {
  return session_meter_read(s, "peaq_session_meter_read_bands", out, true, rows, cap, n_read, dropped);
}

extern "C" int peaq_meter_band_rows(void) { return kMeterBandRows; }

extern "C" int peaq_meter_bands_workspace(const peaq_meter_config* cfg, int advanced, int channels, size_t* bytes) {
  const std::string who("peaq_meter_bands_workspace");
  if (!cfg || !bytes) return fail(PEAQ_ERR_ARG, who + ": NULL argument");
  *bytes = 0;
  if (int rc = check_meter_config(who, *cfg)) return rc;
  if (int rc = check_meter_bands_config(who, *cfg)) return rc;
  if (int rc = check_channels(who, channels)) return rc;
  MeterGeometry g;
  g.set(*cfg);
  *bytes = MeterBandSizes(g.k_open, g.ring, kSessionMaxFrames, advanced != 0, channels).bytes();
  return PEAQ_OK;
}

extern "C" int peaq_session_set_meter_bands(peaq_session* s, int on) {
  const std::string who("peaq_session_set_meter_bands");
  if (!s) return fail(PEAQ_ERR_ARG, who + ": session is NULL");
  std::lock_guard<std::mutex> lock(s->mu);
  if (int rc = session_not_begun(s, who, "the band meter")) return rc;
  peaq_session::Meter& mt = s->meter;
  if (!mt.on) return fail(PEAQ_ERR_ARG, who + ": the meter is off; set it first (peaq_session_set_meter)");
  mt.bands = false;                                  // (stays off if the workspace cannot be reserved)
  if (!on) return PEAQ_OK;
  if (int rc = check_meter_bands_config(who, peaq_meter_config{mt.window, mt.hop, mt.depth})) return rc;
  HIP_TRY(hipSetDevice(s->ctx->device));
  HIP_TRY(hipStreamSynchronize(s->stream));          // (the buffers may be replaced)
  if (int rc = mt.buf.reserve_bands(mt, 1, kSessionMaxFrames, s->advanced != 0, s->channels)) return rc;
  if (int rc = mt.buf.restart_bands(0, 1, s->stream)) return rc;
  mt.bands = true;
  return PEAQ_OK;
}

extern "C" size_t peaq_live_delay_size(void) { return sizeof(peaq_live_delay); }
extern "C" size_t peaq_delay_watch_size(void) { return sizeof(peaq_delay_watch); }

extern "C" int peaq_live_align_plan(const peaq_live_align_config* cfg, uint64_t have_ref, uint64_t have_test, int32_t lag,
                                    uint32_t* probe_ref, uint32_t* probe_test, uint32_t* skip_ref, uint32_t* skip_test) {
  const std::string who("peaq_live_align_plan");
  if (!cfg) return fail(PEAQ_ERR_ARG, who + ": cfg is NULL");
  uint32_t probe = 0;
  if (int rc = check_live_align(who, *cfg, &probe)) return rc;
  if (cfg->max_lag == 0) return fail(PEAQ_ERR_ARG, who + ": max_lag 0 sets no acquisition");
  if (lag < -(int64_t)cfg->max_lag || lag > (int64_t)cfg->max_lag)
    return fail(PEAQ_ERR_ARG, who + ": lag " + std::to_string(lag) + " is outside -max_lag .. max_lag = " +
                                  std::to_string(cfg->max_lag));
  peaq_live_delay d{};
  live_align_plan(probe, have_ref, have_test, lag, &d);
  if (probe_ref) *probe_ref = d.probe_ref;
  if (probe_test) *probe_test = d.probe_test;
  if (skip_ref) *skip_ref = d.skip_ref;
  if (skip_test) *skip_test = d.skip_test;
  return PEAQ_OK;
}

extern "C" int peaq_delay_watch_pick(const double* c, double e_ref, double e_test, int32_t* offset, double* peak,
                                     double* runner_up, double* norm) {
  if (!c) return fail(PEAQ_ERR_ARG, "peaq_delay_watch_pick: c is NULL");
  int32_t o;
  double p, r, n;
  delay_watch_pick(c, e_ref, e_test, &o, &p, &r, &n);
  if (offset) *offset = o;
  if (peak) *peak = p;
  if (runner_up) *runner_up = r;
  if (norm) *norm = n;
  return PEAQ_OK;
}

extern "C" int peaq_session_set_align(peaq_session* s, const peaq_live_align_config* cfg) {
  const std::string who("peaq_session_set_align");
  if (!s) return fail(PEAQ_ERR_ARG, who + ": session is NULL");
  const bool off = !cfg || (cfg->max_lag == 0 && cfg->watch_frames == 0);
  uint32_t probe = 0;
  if (cfg)
    if (int rc = check_live_align(who, *cfg, &probe)) return rc;
  std::lock_guard<std::mutex> lock(s->mu);
  if (int rc = session_not_begun(s, who, "the alignment")) return rc;
  peaq_session::Align& al = s->align;
  al.max_lag = al.probe = al.window = 0;             // (stays off if the workspace cannot be reserved)
  al.delay = peaq_live_delay{};
  s->framer.held = false;
  if (off) return PEAQ_OK;
  HIP_TRY(hipSetDevice(s->ctx->device));
  HIP_TRY(hipStreamSynchronize(s->stream));          // (the buffers may be replaced)
  if (int rc = al.buf.reserve(*cfg, probe, s->channels, 1, 1, kSessionMaxFrames)) return rc;
  al.max_lag = cfg->max_lag;
  al.probe = probe;
  al.window = cfg->watch_frames;
  if (int rc = session_raw_reserve(s)) return rc;
  return session_align_restart(s);
}

// Live rate conversion (include/peaq_amd.h): the pads' rates, on a stream that has not begun.
extern "C" int peaq_session_set_rates(peaq_session* s, uint32_t rate_ref, uint32_t rate_test) {
  const std::string who("peaq_session_set_rates");
  if (!s) return fail(PEAQ_ERR_ARG, who + ": session is NULL");
  const uint32_t rate[2] = {rate_ref, rate_test};
  RateGeometry geo[2] = {{1, 1, 0}, {1, 1, 0}};
  for (int p = 0; p < 2; ++p)
    if (rate[p] != 48000)
      if (int rc = resample_geometry(who.c_str(), rate[p], &geo[p])) return rc;
  std::lock_guard<std::mutex> lock(s->mu);
  if (int rc = session_not_begun(s, who, "the rates")) return rc;
  HIP_TRY(hipSetDevice(s->ctx->device));
  HIP_TRY(hipStreamSynchronize(s->stream));          // (the buffers may be replaced)
  for (int p = 0; p < 2; ++p) s->framer.set_rate(p, rate[p], geo[p]);
  if (int rc = session_raw_reserve(s)) {             // (stays off if the staging cannot be reserved)
    for (int p = 0; p < 2; ++p) s->framer.set_rate(p, 48000, RateGeometry{1, 1, 0});
    return rc;
  }
  return PEAQ_OK;
}

extern "C" int peaq_session_align_read(peaq_session* s, peaq_live_delay* out) {
  if (!s || !out) return fail(PEAQ_ERR_ARG, "peaq_session_align_read: NULL argument");
  std::lock_guard<std::mutex> lock(s->mu);
  if (!s->align.max_lag)
    return fail(PEAQ_ERR_ARG, "peaq_session_align_read: no acquisition is set (peaq_session_set_align, max_lag)");
  HIP_TRY(hipSetDevice(s->ctx->device));
  HIP_TRY(hipStreamSynchronize(s->stream));
  *out = s->align.delay;
  return PEAQ_OK;
}

extern "C" int peaq_session_watch_read(peaq_session* s, peaq_delay_watch* out) {
  if (!s || !out) return fail(PEAQ_ERR_ARG, "peaq_session_watch_read: NULL argument");
  std::lock_guard<std::mutex> lock(s->mu);
  if (!s->align.window)
    return fail(PEAQ_ERR_ARG, "peaq_session_watch_read: the watch is off (peaq_session_set_align, watch_frames)");
  HIP_TRY(hipSetDevice(s->ctx->device));
  WatchState st;
  HIP_TRY(hipMemcpyAsync(&st, s->align.buf.state.p, sizeof st, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  delay_watch_record(st, out);
  return PEAQ_OK;
}

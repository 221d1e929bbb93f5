// peaq_debug.hip -- stage-level entry points for the parity tests: the front end, the filter bank and the pattern
// back end each on their own (include/peaq_amd.h, "stage-level access").
#include "peaq_host.h"

using namespace peaq;

// ---------------------------------------------------------------------------
// stage-level access for parity tests
// ---------------------------------------------------------------------------
extern "C" int peaq_debug_frontend(peaq_ctx* c, int bands, int channels, double level_db, const float* d_ref,
                                   const float* d_test, uint32_t n_ref, uint32_t n_test, int n_frames,
                                   double* host_out) {
  if (!c || !d_ref || !d_test || !host_out) return fail(PEAQ_ERR_ARG, "peaq_debug_frontend: NULL argument");
  if (bands != 109 && bands != 55) return fail(PEAQ_ERR_ARG, "peaq_debug_frontend: bands must be 109 or 55");
  if (int rc = check_channels("peaq_debug_frontend", channels)) return rc;
  const uint32_t total = count_frames(n_ref, n_test, kFrame, kHop);
  if (n_frames < 0 || (uint32_t)n_frames > total) return fail(PEAQ_ERR_ARG, "peaq_debug_frontend: too many frames");
  if (n_frames == 0) return PEAQ_OK;
  HIP_TRY(hipSetDevice(c->device));
  const size_t bytes = (size_t)n_frames * channels * kRecDoubles * sizeof(double);
  DevBuf rec_buf, n_buf;
  HIP_TRY(rec_buf.reserve(bytes));
  double* d_rec = rec_buf.as<double>();
  HIP_TRY(hipMemset(d_rec, 0, bytes));
  uint32_t h_n[2] = {n_ref, n_test};
  HIP_TRY(n_buf.reserve(sizeof h_n));
  uint32_t* d_n = n_buf.as<uint32_t>();
  HIP_TRY(hipMemcpy(d_n, h_n, sizeof h_n, hipMemcpyHostToDevice));
  FrontendArgs fa = ModelSetup{c, c->settings, bands == 55, channels, level_db}.frontend();
  fa.ref = d_ref;
  fa.test = d_test;
  fa.pair_stride = std::max(n_ref, n_test);
  fa.n_ref = d_n;
  fa.n_test = d_n + 1;
  fa.n_frames = nullptr;
  fa.n_frames_uniform = total;
  fa.frame0 = 0;
  fa.frames_per_launch = n_frames;
  fa.records = d_rec;
  std::vector<double> h_rec((size_t)n_frames * channels * kRecDoubles);
  // one pair: launches of at most max_frames_per_launch(1) frames, the records of a launch follow the previous one's
  hipError_t e = hipSuccess;
  for (uint32_t f0 = 0; f0 < (uint32_t)n_frames && e == hipSuccess; f0 += max_frames_per_launch(1)) {
    fa.frame0 = f0;
    fa.frames_per_launch = std::min<uint32_t>(max_frames_per_launch(1), (uint32_t)n_frames - f0);
    fa.records = d_rec + (size_t)f0 * channels * kRecDoubles;
    e = launch_frontend(bands, fa, 1, nullptr);
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(h_rec.data(), d_rec, bytes, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(PEAQ_ERR_DEVICE, std::string("peaq_debug_frontend: ") + hipGetErrorString(e));
  // the test-facing layout spells the two derived vectors out (the back end's own arithmetic, on the host)
  BandTables t;
  build_fft_band_tables(bands, t);
  for (size_t r = 0; r < (size_t)n_frames * channels; ++r) {
    const double* in = h_rec.data() + r * kRecDoubles;
    double* out = host_out + r * kPubDoubles;
    for (int b = 0; b < kBandStride; ++b) {
      excitation_from_root(in[kRecRootRef + b], t.inv_spread_norm[b], t.inv_spread_norm_pow03[b], out[kPubUnsmRef + b],
                           out[kPubLoudRef + b]);
      excitation_from_root(in[kRecRootTest + b], t.inv_spread_norm[b], t.inv_spread_norm_pow03[b],
                           out[kPubUnsmTest + b], out[kPubLoudTest + b]);
      out[kPubNoise + b] = in[kRecNoise + b];
    }
    for (int i = 0; i < kPubDoubles - kPubScalars; ++i) out[kPubScalars + i] = in[kRecScalars + i];
  }
  return PEAQ_OK;
}

// Which kernel the basic version's front end is (launch_frontend), whoever launches:
// 0 = the one-wave kernel, 1 = frontend_kernel<109>, -1 = what PEAQ_AMD_FE says.  Returns the previous selection.
extern "C" int peaq_debug_select_frontend(int two_waves) { return select_frontend(two_waves); }

// The basic version's front end over SEVERAL pairs the way the batch path launches it -- one grid per launch of
// frames_per_launch frames over all pairs, per-pair lengths and frame counts -- with the records as the kernels
// exchange them: out[pair][frame][channel][PEAQ_DEBUG_RAW_RECORD_DOUBLES], frame < n_frames; the records of frames a
// pair does not have stay zero.
static_assert(kRecDoubles == PEAQ_DEBUG_RAW_RECORD_DOUBLES, "record layouts must match");
extern "C" int peaq_debug_frontend_pairs(peaq_ctx* c, int channels, double level_db, const float* d_ref,
                                         const float* d_test, int n_pairs, size_t pair_stride, const uint32_t* n_ref,
                                         const uint32_t* n_test, int frames_per_launch, int n_frames, double* host_out) {
  if (!c || !d_ref || !d_test || !n_ref || !n_test || !host_out)
    return fail(PEAQ_ERR_ARG, "peaq_debug_frontend_pairs: NULL argument");
  if (int rc = check_channels("peaq_debug_frontend_pairs", channels)) return rc;
  if (n_pairs < 1 || n_frames < 1 || frames_per_launch < 1 ||
      (uint32_t)frames_per_launch > max_frames_per_launch((unsigned)n_pairs))
    return fail(PEAQ_ERR_ARG, "peaq_debug_frontend_pairs: bad counts");
  std::vector<uint32_t> h_n(3 * (size_t)n_pairs);
  for (int p = 0; p < n_pairs; ++p) {
    if (n_ref[p] > pair_stride || n_test[p] > pair_stride)
      return fail(PEAQ_ERR_ARG, "peaq_debug_frontend_pairs: a signal is longer than the pair stride");
    h_n[p] = n_ref[p];
    h_n[n_pairs + p] = n_test[p];
    h_n[2 * (size_t)n_pairs + p] = count_frames(n_ref[p], n_test[p], kFrame, kHop);
    if (h_n[2 * (size_t)n_pairs + p] > (uint32_t)n_frames) return fail(PEAQ_ERR_ARG, "peaq_debug_frontend_pairs: n_frames too small");
  }
  HIP_TRY(hipSetDevice(c->device));
  const size_t per_frame = (size_t)channels * kRecDoubles;
  const size_t launch_bytes = (size_t)n_pairs * frames_per_launch * per_frame * sizeof(double);
  DevBuf rec_buf, n_buf;
  HIP_TRY(rec_buf.reserve(launch_bytes));
  HIP_TRY(n_buf.reserve(h_n.size() * sizeof(uint32_t)));
  uint32_t* d_n = n_buf.as<uint32_t>();
  HIP_TRY(hipMemcpy(d_n, h_n.data(), h_n.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  FrontendArgs fa = ModelSetup{c, c->settings, 0, channels, level_db}.frontend();
  fa.ref = d_ref;
  fa.test = d_test;
  fa.pair_stride = pair_stride;
  fa.n_ref = d_n;
  fa.n_test = d_n + n_pairs;
  fa.n_frames = d_n + 2 * (size_t)n_pairs;
  fa.records = rec_buf.as<double>();
  std::vector<double> h_rec(launch_bytes / sizeof(double));
  for (int f0 = 0; f0 < n_frames; f0 += frames_per_launch) {
    const int nf = std::min(frames_per_launch, n_frames - f0);
    fa.frame0 = f0;
    fa.frames_per_launch = nf;
    const size_t bytes = (size_t)n_pairs * nf * per_frame * sizeof(double);
    HIP_TRY(hipMemset(fa.records, 0, bytes));
    HIP_TRY(launch_frontend(109, fa, n_pairs, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h_rec.data(), fa.records, bytes, hipMemcpyDeviceToHost));
    for (int p = 0; p < n_pairs; ++p)
      std::copy(h_rec.begin() + (size_t)p * nf * per_frame, h_rec.begin() + (size_t)(p + 1) * nf * per_frame,
                host_out + ((size_t)p * n_frames + f0) * per_frame);
  }
  return PEAQ_OK;
}

extern "C" int peaq_debug_filterbank(peaq_ctx* c, int channels, double level_db, const float* d_ref,
                                     const float* d_test, uint32_t n_ref, uint32_t n_test, int n_blocks,
                                     int blocks_per_launch, double* host_out) {
  if (!c || !d_ref || !d_test || !host_out) return fail(PEAQ_ERR_ARG, "peaq_debug_filterbank: NULL argument");
  if (int rc = check_channels("peaq_debug_filterbank", channels)) return rc;
  const uint32_t total = count_frames(n_ref, n_test, kFbFrame, kFbFrame);
  if (n_blocks < 0 || (uint32_t)n_blocks > total || blocks_per_launch < 1)
    return fail(PEAQ_ERR_ARG, "peaq_debug_filterbank: bad block counts");
  if (n_blocks == 0) return PEAQ_OK;
  HIP_TRY(hipSetDevice(c->device));
  const unsigned n_signals = 2 * channels;
  const size_t row_stride = (size_t)kFbRing + (size_t)blocks_per_launch * kFbFrame;
  DevBuf rows, recs, st;
  HIP_TRY(rows.reserve(n_signals * row_stride * sizeof(double)));
  HIP_TRY(recs.reserve((size_t)blocks_per_launch * channels * kFbRecDoubles * sizeof(double)));
  HIP_TRY(st.reserve(n_signals * sizeof(FbSignalState)));
  HIP_TRY(hipMemset(st.p, 0, n_signals * sizeof(FbSignalState)));
  FbFrontArgs ff = ModelSetup{c, c->settings, 1, channels, level_db}.fb_frontend();
  ff.ref = d_ref;
  ff.test = d_test;
  ff.pair_stride = std::max(n_ref, n_test);
  ff.n_uniform_ref = n_ref;
  ff.n_uniform_test = n_test;
  ff.n_blocks_uniform = n_blocks;
  ff.fbstate = st.as<FbSignalState>();
  ff.hp_scratch = rows.as<double>();
  ff.hp_row_stride = row_stride;
  ff.records = recs.as<double>();
  hipError_t e = hipSuccess;
  unsigned prev = 0;
  for (int b0 = 0; b0 < n_blocks && e == hipSuccess; b0 += blocks_per_launch) {
    const unsigned nb = std::min(blocks_per_launch, n_blocks - b0);
    ff.block0 = b0;
    ff.blocks_per_launch = nb;
    ff.prev_blocks = prev;
    ff.first_launch = b0 == 0;
    e = hipMemset(recs.p, 0, recs.cap);
    if (e == hipSuccess) e = launch_fb_frontend(ff, 1, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess)
      e = hipMemcpy(host_out + (size_t)b0 * channels * kFbRecDoubles, recs.p,
                    (size_t)nb * channels * kFbRecDoubles * sizeof(double), hipMemcpyDeviceToHost);
    prev = nb;
  }
  if (e != hipSuccess) return fail(PEAQ_ERR_DEVICE, std::string("peaq_debug_filterbank: ") + hipGetErrorString(e));
  return PEAQ_OK;
}

// the back ends on their own take records, not samples: the playback level has gone into those already
constexpr double kNoLevel = 92.;

// test-facing layout (kPub*) -> the record the kernels exchange: root = (E norm)^(1/10); the E^0.3 vector of the
// input is implied by E (the back end derives both from the root)
static hipError_t upload_public_records(int bands, int channels, int n_frames, const double* host_records, void* d_recs) {
  BandTables t;
  build_fft_band_tables(bands, t);
  std::vector<double> h_rec((size_t)n_frames * channels * kRecDoubles, 0.);
  for (size_t r = 0; r < (size_t)n_frames * channels; ++r) {
    const double* in = host_records + r * kPubDoubles;
    double* out = h_rec.data() + r * kRecDoubles;
    for (int b = 0; b < bands; ++b) {
      out[kRecRootRef + b] = std::pow(in[kPubUnsmRef + b] / t.inv_spread_norm[b], 0.1);
      out[kRecRootTest + b] = std::pow(in[kPubUnsmTest + b] / t.inv_spread_norm[b], 0.1);
    }
    for (int b = 0; b < kBandStride; ++b) out[kRecNoise + b] = in[kPubNoise + b];
    for (int i = 0; i < kRecDoubles - kRecScalars; ++i) out[kRecScalars + i] = in[kPubScalars + i];
  }
  return hipMemcpy(d_recs, h_rec.data(), h_rec.size() * sizeof(double), hipMemcpyHostToDevice);
}

extern "C" int peaq_debug_backend(peaq_ctx* c, int channels, int n_frames, const double* host_records,
                                  double* host_out, peaq_result* result) {
  if (!c || !host_records || !host_out) return fail(PEAQ_ERR_ARG, "peaq_debug_backend: NULL argument");
  if (int rc = check_channels("peaq_debug_backend", channels)) return rc;
  if (n_frames < 1) return fail(PEAQ_ERR_ARG, "peaq_debug_backend: n_frames < 1");
  HIP_TRY(hipSetDevice(c->device));
  const size_t rec_bytes = (size_t)n_frames * channels * kRecDoubles * sizeof(double);
  const size_t dbg_bytes = (size_t)n_frames * channels * kDbgDoubles * sizeof(double);
  DevBuf recs, dbg, st, res;
  HIP_TRY(recs.reserve(rec_bytes));
  HIP_TRY(dbg.reserve(dbg_bytes));
  HIP_TRY(st.reserve(sizeof(PairState)));
  HIP_TRY(res.reserve(sizeof(ResultRecord)));
  HIP_TRY(upload_public_records(109, channels, n_frames, host_records, recs.p));
  HIP_TRY(hipMemset(dbg.p, 0, dbg_bytes));
  HIP_TRY(launch_state_init(st.as<PairState>(), 0, 1, nullptr));
  const ModelSetup m{c, c->settings, 0, channels, kNoLevel};
  BackendArgs ba = m.backend(m.frontend());
  ba.records = recs.as<double>();
  ba.frame0 = 0;
  ba.frames_per_launch = n_frames;
  ba.n_frames_uniform = n_frames;
  ba.state = st.as<PairState>();
  ba.debug = dbg.as<double>();
  HIP_TRY(launch_backend(ba, 1, nullptr));
  HIP_TRY(launch_finalize(st.as<PairState>(), 0, channels, 1, res.as<ResultRecord>(), nullptr, c->settings));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(host_out, dbg.p, dbg_bytes, hipMemcpyDeviceToHost));
  if (result) HIP_TRY(hipMemcpy(result, res.p, sizeof(peaq_result), hipMemcpyDeviceToHost));
  return PEAQ_OK;
}

// The advanced version's two back ends on their own (fresh state): the filter-bank back end over n_blocks block
// records (from peaq_debug_filterbank) and the 55-band FFT back end over n_frames front-end records (from
// peaq_debug_frontend with 55 bands), each in its debug instantiation -- the MOV values of EVERY block / frame
// before accumulation -- followed by the read-out of the pair's result.
extern "C" int peaq_debug_backend_advanced(peaq_ctx* c, int channels, int n_blocks, const double* host_fb_records,
                                           int n_frames, const double* host_fft_records, double* out_blocks,
                                           double* out_frames, peaq_result* result) {
  if (!c || !host_fb_records || !host_fft_records || !out_blocks || !out_frames)
    return fail(PEAQ_ERR_ARG, "peaq_debug_backend_advanced: NULL argument");
  if (int rc = check_channels("peaq_debug_backend_advanced", channels)) return rc;
  if (n_blocks < 1 || n_frames < 1) return fail(PEAQ_ERR_ARG, "peaq_debug_backend_advanced: n_blocks, n_frames must be >= 1");
  HIP_TRY(hipSetDevice(c->device));
  const size_t fbrec_bytes = (size_t)n_blocks * channels * kFbRecDoubles * sizeof(double);
  const size_t fbdbg_bytes = (size_t)n_blocks * channels * kDbgFbDoubles * sizeof(double);
  const size_t rec_bytes = (size_t)n_frames * channels * kRecDoubles * sizeof(double);
  const size_t dbg_bytes = (size_t)n_frames * channels * kDbgDoubles * sizeof(double);
  DevBuf fbrecs, fbdbg, recs, dbg, st, res;
  HIP_TRY(fbrecs.reserve(fbrec_bytes));
  HIP_TRY(fbdbg.reserve(fbdbg_bytes));
  HIP_TRY(recs.reserve(rec_bytes));
  HIP_TRY(dbg.reserve(dbg_bytes));
  HIP_TRY(st.reserve(sizeof(PairState)));
  HIP_TRY(res.reserve(sizeof(ResultRecord)));
  HIP_TRY(hipMemcpy(fbrecs.p, host_fb_records, fbrec_bytes, hipMemcpyHostToDevice));
  HIP_TRY(upload_public_records(55, channels, n_frames, host_fft_records, recs.p));
  HIP_TRY(hipMemset(fbdbg.p, 0, fbdbg_bytes));
  HIP_TRY(hipMemset(dbg.p, 0, dbg_bytes));
  HIP_TRY(launch_state_init(st.as<PairState>(), 1, 1, nullptr));
  const ModelSetup m{c, c->settings, 1, channels, kNoLevel};
  BackendArgs ba = m.backend(m.frontend());
  ba.records = recs.as<double>();
  ba.frame0 = 0;
  ba.frames_per_launch = n_frames;
  ba.n_frames_uniform = n_frames;
  ba.state = st.as<PairState>();
  ba.debug = dbg.as<double>();
  HIP_TRY(launch_backend(ba, 1, nullptr));
  FbBackendArgs fbk = m.fb_backend(m.fb_frontend());
  fbk.records = fbrecs.as<double>();
  fbk.block0 = 0;
  fbk.blocks_per_launch = n_blocks;
  fbk.n_blocks_uniform = n_blocks;
  fbk.state = st.as<PairState>();
  fbk.debug = fbdbg.as<double>();
  HIP_TRY(launch_fb_backend(fbk, 1, nullptr));
  HIP_TRY(launch_finalize(st.as<PairState>(), 1, channels, 1, res.as<ResultRecord>(), nullptr, c->settings));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out_blocks, fbdbg.p, fbdbg_bytes, hipMemcpyDeviceToHost));
  {
    std::vector<double> h((size_t)n_frames * channels * kDbgDoubles);
    HIP_TRY(hipMemcpy(h.data(), dbg.p, dbg_bytes, hipMemcpyDeviceToHost));
    for (size_t r = 0; r < (size_t)n_frames * channels; ++r) {
      out_frames[2 * r] = h[r * kDbgDoubles + kDbgMov + 3];       // SegmentalNMR's value (dB)
      out_frames[2 * r + 1] = h[r * kDbgDoubles + kDbgMov + 4];   // the mean band NMR it is the logarithm of
    }
  }
  if (result) HIP_TRY(hipMemcpy(result, res.p, sizeof(peaq_result), hipMemcpyDeviceToHost));
  return PEAQ_OK;
}

// The SHIPPED instantiations of the back ends (no debug dump, no points, no trace) on records, from a fresh state, cut
// into launches of the given sizes: launch k takes frames [k frames_per_launch, (k + 1) frames_per_launch) with frame0
// advancing, and everything a launch leaves to the next goes through the PairState (the accumulators' status and
// fields, loudness_reached, the filters).  Then the read-out; only the result comes back.
extern "C" int peaq_debug_backend_plain(peaq_ctx* c, int advanced, int channels, int n_frames,
                                        const double* host_fft_records, int frames_per_launch, int n_blocks,
                                        const double* host_fb_records, int blocks_per_launch, peaq_result* result) {
  if (!c || !host_fft_records || !result || (advanced && !host_fb_records))
    return fail(PEAQ_ERR_ARG, "peaq_debug_backend_plain: NULL argument");
  if (int rc = check_channels("peaq_debug_backend_plain", channels)) return rc;
  if (n_frames < 1 || frames_per_launch < 1)
    return fail(PEAQ_ERR_ARG, "peaq_debug_backend_plain: n_frames, frames_per_launch must be >= 1");
  if (advanced && (n_blocks < 1 || blocks_per_launch < 1))
    return fail(PEAQ_ERR_ARG, "peaq_debug_backend_plain: n_blocks, blocks_per_launch must be >= 1");
  HIP_TRY(hipSetDevice(c->device));
  const int adv = advanced ? 1 : 0;
  const size_t rec_bytes = (size_t)n_frames * channels * kRecDoubles * sizeof(double);
  const size_t fbrec_bytes = adv ? (size_t)n_blocks * channels * kFbRecDoubles * sizeof(double) : 0;
  DevBuf recs, fbrecs, st, res;
  HIP_TRY(recs.reserve(rec_bytes));
  if (adv) HIP_TRY(fbrecs.reserve(fbrec_bytes));
  HIP_TRY(st.reserve(sizeof(PairState)));
  HIP_TRY(res.reserve(sizeof(ResultRecord)));
  HIP_TRY(upload_public_records(adv ? 55 : 109, channels, n_frames, host_fft_records, recs.p));
  if (adv) HIP_TRY(hipMemcpy(fbrecs.p, host_fb_records, fbrec_bytes, hipMemcpyHostToDevice));
  HIP_TRY(launch_state_init(st.as<PairState>(), adv, 1, nullptr));
  const ModelSetup m{c, c->settings, adv, channels, kNoLevel};
  BackendArgs ba = m.backend(m.frontend());
  ba.n_frames_uniform = n_frames;
  ba.state = st.as<PairState>();
  ba.debug = nullptr;
  for (int f0 = 0; f0 < n_frames; f0 += frames_per_launch) {
    ba.frame0 = f0;
    ba.frames_per_launch = std::min(frames_per_launch, n_frames - f0);
    ba.records = recs.as<double>() + (size_t)f0 * channels * kRecDoubles;   // a launch indexes its records from its own frame0
    HIP_TRY(launch_backend(ba, 1, nullptr));
  }
  if (adv) {
    FbBackendArgs fbk = m.fb_backend(m.fb_frontend());
    fbk.n_blocks_uniform = n_blocks;
    fbk.state = st.as<PairState>();
    fbk.debug = nullptr;
    for (int b0 = 0; b0 < n_blocks; b0 += blocks_per_launch) {
      fbk.block0 = b0;
      fbk.blocks_per_launch = std::min(blocks_per_launch, n_blocks - b0);
      fbk.records = fbrecs.as<double>() + (size_t)b0 * channels * kFbRecDoubles;
      HIP_TRY(launch_fb_backend(fbk, 1, nullptr));
    }
  }
  HIP_TRY(launch_finalize(st.as<PairState>(), adv, channels, 1, res.as<ResultRecord>(), nullptr, c->settings));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(result, res.p, sizeof(peaq_result), hipMemcpyDeviceToHost));
  return PEAQ_OK;
}

// Host only: a StreamFramer fed with sample counts alone, drained the way peaq_session_push / _flush drain theirs.
extern "C" int peaq_debug_stream_plan(int advanced, unsigned max_frames, unsigned max_blocks, int drain_every_push,
                                      size_t n_pushes, const int* pad, const uint64_t* n_samples, size_t max_windows,
                                      uint64_t* windows, size_t* n_windows) {
  if (!n_windows || (n_pushes && (!pad || !n_samples)) || (max_windows && !windows))
    return fail(PEAQ_ERR_ARG, "peaq_debug_stream_plan: NULL argument");
  if (max_frames < 1 || max_blocks < 1) return fail(PEAQ_ERR_ARG, "peaq_debug_stream_plan: a cap is 0");
  for (size_t k = 0; k < n_pushes; ++k)
    if (pad[k] < -1 || pad[k] > 1) return fail(PEAQ_ERR_ARG, "peaq_debug_stream_plan: pad must be 0 (ref), 1 (test) or -1 (flush)");
  StreamFramer fr;
  fr.reset(advanced != 0, 1);
  size_t n = 0;
  auto note = [&](StreamUnit kind, const StreamWindow& w) {
    if (n < max_windows) {
      uint64_t* o = windows + n * PEAQ_DEBUG_STREAM_WINDOW_FIELDS;
      o[0] = kind;
      o[1] = w.first;
      o[2] = w.count;
      o[3] = w.valid[0];
      o[4] = w.valid[1];
    }
    ++n;
    return (int)PEAQ_OK;
  };
  for (size_t k = 0; k < n_pushes; ++k) {
    if (pad[k] >= 0) fr.append(pad[k], nullptr, n_samples[k]);
    if (pad[k] < 0 || drain_every_push) (void)drain_stream(fr, max_frames, max_blocks, pad[k] < 0, note);
  }
  (void)drain_stream(fr, max_frames, max_blocks, true, note);
  *n_windows = n;
  return PEAQ_OK;
}

// Host only: one slot of the broker fed with sample counts alone, ticked the way broker_tick_locked ticks it.
extern "C" int peaq_debug_broker_plan(int advanced, int metered, size_t n_events, const int* pad, const uint64_t* n_samples,
                                      size_t max_rows, uint64_t* rows, size_t* n_rows) {
  if (!n_rows || (n_events && (!pad || !n_samples)) || (max_rows && !rows))
    return fail(PEAQ_ERR_ARG, "peaq_debug_broker_plan: NULL argument");
  for (size_t k = 0; k < n_events; ++k)
    if (pad[k] < -2 || pad[k] > 1)
      return fail(PEAQ_ERR_ARG, "peaq_debug_broker_plan: pad must be 0 (ref), 1 (test), -1 (flush) or -2 (tick)");
  StreamFramer fr;
  fr.reset(advanced != 0, 1);
  SlotFlush flush;
  MeterStream meter;
  size_t n = 0;
  uint64_t n_ticks = 0;
  auto note = [&](uint64_t kind, uint64_t first, uint64_t count, uint64_t v_ref, uint64_t v_test) {
    if (n < max_rows) {
      uint64_t* o = rows + n * PEAQ_DEBUG_BROKER_PLAN_FIELDS;
      o[0] = n_ticks;
      o[1] = kind;
      o[2] = first;
      o[3] = count;
      o[4] = v_ref;
      o[5] = v_test;
    }
    ++n;
  };
  auto tick = [&]() {                                // -> the tick took something
    const SlotTake t = take_slot_windows(fr, flush, meter, metered != 0, advanced != 0, kBrokerMaxFrames, kBrokerMaxBlocks);
    fr.trim();
    if (t.fft.count) note(kUnitFrame, t.fft.first, t.fft.count, t.fft.valid[0], t.fft.valid[1]);
    if (t.fb.count) note(kUnitBlock, t.fb.first, t.fb.count, t.fb.valid[0], t.fb.valid[1]);
    if (t.closing) note(2, meter.total[kUnitBlock], 0, 0, 0);
    ++n_ticks;
    return t.fft.count || t.fb.count || t.closing;
  };
  for (size_t k = 0; k < n_events; ++k) {
    if (pad[k] >= 0) fr.append(pad[k], nullptr, n_samples[k]);
    if (pad[k] == -1) flush.request();
    if (pad[k] == -2) (void)tick();
  }
  if (!flush.requested) flush.request();
  while (tick() || flush.requested) {
  }
  *n_rows = n;
  return PEAQ_OK;
}

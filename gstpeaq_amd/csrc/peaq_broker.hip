// peaq_broker.hip -- the live-pipeline broker: many sessions, one launch per kernel and tick; one or several devices.
#include "peaq_host.h"

using namespace peaq;

// ---------------------------------------------------------------------------
// broker: many live sessions, one launch per tick
// ---------------------------------------------------------------------------
// A process that hosts many `peaq` elements (BASELINE.json configs[5]: 1024
// concurrent live pipelines) would otherwise issue one 1-workgroup launch pair
// per element and buffer.  The broker keeps the FIFOs of all its sessions on
// the host and, on every tick, gathers whatever frames (and, in the advanced
// version, filter-bank blocks) became ready in ANY session into ONE launch per
// kernel: workgroup (pair p, frame fl) of the front-end grid is frame
// pair_frame0[p] + fl of session pair_slot[p]; the filter-bank kernels get a
// FbPairWindow per session.  The recurrent state of a session stays in its slot
// in HBM between ticks, so the result of a session is the same whether its
// frames were run alone, in a batch, or interleaved with other sessions'.
// The framing per session is that of do_processing / do_flush
// (gstpeaq.c:596-611, 716-745, 769-771).
namespace {
constexpr size_t kBrokerStageSamples = (size_t)(kBrokerMaxFrames - 1) * kHop + kFrame;   // (kBrokerMax*: peaq_host.h)
constexpr size_t kBrokerFbStageSamples = (size_t)kBrokerMaxBlocks * kFbFrame;
constexpr size_t kBrokerRowStride = (size_t)kFbRing + kBrokerFbStageSamples;
constexpr unsigned kBrokerAcquirePerTick = 8;   // live alignment: slots whose delay estimate one tick enqueues
// back-pressure: a push returns only once its session has no more than this many samples that are
// READY to be framed (present on both pads) and not yet launched -- four ticks' worth.  Samples one
// pad holds ahead of the other are never counted: like the reference's adapters they may pile up
// without bound while the other pad is silent (gstpeaq.c:626-636).
constexpr uint64_t kBrokerBacklog = (uint64_t)4 * kBrokerMaxFrames * kHop;

struct BrokerSlot {
  std::mutex mu;
  bool open = false;
  SlotFlush flush;
  StreamFramer framer;              // the two pads' FIFOs and where the next frame / block starts
  double t_ready_us = -1.;          // when the oldest not yet launched frame / block became whole (-1: none waiting)
  MeterStream meter;                // the slot's meter (peaq_broker_set_meter), fresh at every open
  // live alignment (peaq_broker_set_align): the framer is held until the delay is acquired
  peaq_live_delay delay{};          // all zero while the stream holds
  bool acquiring = false;           // the estimate over this slot's probes is enqueued: the next tick reads it
  uint64_t epoch = 0;               // counts opens and closes: an estimate enqueued for an earlier stream is dropped
};

// an estimate a tick has enqueued: read by the next tick
struct BrokerAcquire {
  int sid = 0;
  uint64_t epoch = 0;
  uint64_t have[2] = {0, 0};        // what the pads held when the probes were taken
};

// microseconds on a monotonic clock (latency bookkeeping of the broker)
static double now_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// running maximum + histogram with eight buckets per octave (1 us .. 2^26 us)
struct UsHistogram {
  uint64_t n = 0, bucket[8 * 27] = {};
  double max = 0., sum = 0.;
  void add(double us) {
    ++n;
    sum += us;
    max = std::max(max, us);
    const int i = us <= 1. ? 0 : std::min<int>(8 * 27 - 1, (int)(8. * std::log2(us)));
    ++bucket[i];
  }
  double quantile(double q) const {                  // upper edge of the bucket that holds it
    if (!n) return 0.;
    uint64_t need = (uint64_t)std::ceil(q * (double)n), seen = 0;
    for (int i = 0; i < 8 * 27; ++i) {
      seen += bucket[i];
      if (seen >= need) return std::min(max, std::exp2((i + 1) / 8.));
    }
    return max;
  }
};

// staging of one kind of unit (FFT frames or filter-bank blocks): pinned host + device buffers
struct BrokerStage {
  float* h[2] = {nullptr, nullptr};         // [launch pair][stage samples][channels]
  DevBuf d[2];
  size_t samples = 0;
  int alloc(size_t n_sessions, size_t stage_samples, int channels, bool pad0 = true, bool pad1 = true) {
    release();
    samples = stage_samples;
    const size_t bytes = n_sessions * stage_samples * channels * sizeof(float);
    for (int p = 0; p < 2; ++p) {
      if (!(p ? pad1 : pad0) || !bytes) continue;
      HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h[p]), bytes, hipHostMallocDefault));
      HIP_TRY(d[p].reserve(bytes));
    }
    return PEAQ_OK;
  }
  void release() {
    for (int p = 0; p < 2; ++p) {
      if (h[p]) (void)hipHostFree(h[p]);
      h[p] = nullptr;
    }
  }
  ~BrokerStage() { release(); }
};

// live rate conversion: the raw samples behind one kind of unit (or behind the probes) of the rated pads, an entry per
// launch pair as in the BrokerStage they convert into, and the segments of one tick
struct BrokerRawStage : BrokerStage {
  std::vector<peaq_rate_segment> seg[2];
};

// The per-pair scalars of a tick's launches: rows of max_sessions entries each, pinned on the host and uploaded as one
// prefix of the table.  Entry i of a row belongs to launch pair i of the FFT path or of the filter-bank path.
struct BrokerMeta {
  enum Row {
    kNRef,            // FFT pair: valid samples of the reference in its staging entry      (front end)
    kNTest,           //           ... of the test signal
    kFrame0,          //           the session's first frame of this tick                    (front end, back end, meter)
    kNFrames,         //           its frames of this tick
    kSlot,            //           the session's slot: PairState, meter snapshots, watch state (back end, meter, watch)
    kFbNRef,          // filter-bank pair: valid samples of the reference                    (filter-bank front end)
    kFbNTest,         //           ... of the test signal
    // uploaded with the meter or the watch on only; UINT_MAX until the session's flush is known:
    kTotalFrames,     // FFT pair: the stream's frame count                                  (meter, FFT path)
    kFbTotalFrames,   // filter-bank pair: the stream's frame count                          (meter, filter-bank path)
    kFbTotalBlocks,   //           the stream's block count
    // uploaded with the watch on only:
    kWatchFrames,     // FFT pair: its whole frames of this tick, 0 for a flush frame        (watch)
    kRows
  };
  int alloc(size_t n_sessions) {
    S = n_sessions;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h), kRows * S * sizeof(uint32_t), hipHostMallocDefault));
    HIP_TRY(d.reserve(kRows * S * sizeof(uint32_t)));
    return PEAQ_OK;
  }
  ~BrokerMeta() {
    if (h) (void)hipHostFree(h);
  }
  uint32_t* host(Row r) const { return h + r * S; }
  const uint32_t* dev(Row r) const { return d.as<uint32_t>() + r * S; }
  // the leading rows a tick uploads
  static size_t rows_uploaded(bool metered, bool watched) {
    return watched ? kRows : metered ? kFbTotalBlocks + 1 : kFbNTest + 1;
  }
  hipError_t upload(bool metered, bool watched, hipStream_t stream) const {
    return hipMemcpyAsync(d.p, h, rows_uploaded(metered, watched) * S * sizeof(uint32_t), hipMemcpyHostToDevice, stream);
  }
  size_t S = 0;
  uint32_t* h = nullptr;            // pinned
  DevBuf d;
};

// what one session contributes to a tick: decided under the slot lock in the tick's serial scan,
// copied into the staging buffers afterwards (by the staging threads, several sessions at a time)
struct BrokerJob {
  int sid = 0;
  unsigned fft_idx = 0, fb_idx = 0;   // staging entries (launch pairs) of the two windows
  StreamWindow fft, fb;               // count 0: none of that kind
};

// What the scan of the slots decided for one tick; the per-pair rows are in BrokerMeta and h_win.
struct TickPlan {
  double t_tick = 0.;                 // when the scan began
  unsigned active = 0, max_nf = 0;    // FFT path: launch pairs, the most frames any has
  unsigned fb_active = 0, max_nb = 0; // filter-bank path: launch pairs, the most blocks any has
  unsigned fb_closing = 0;            // meter: sessions whose blocks ended without a flush block (entries without units)
  uint64_t frames = 0;
  std::vector<BrokerJob>& jobs;       // this tick's staging work (the broker keeps the storage)
  unsigned n_acq = 0;                 // live alignment: this tick's estimates (peaq_broker::a_pending) ...
  uint32_t acq_n[2][kBrokerAcquirePerTick];   // ... and their probe lengths per pad
  explicit TickPlan(std::vector<BrokerJob>& storage) : jobs(storage) { jobs.clear(); }
  bool idle() const { return !active && !fb_active && !fb_closing && !n_acq; }
};

// A few helper threads for the tick's one heavy host-side step, the copy of every session's new samples
// into the pinned staging buffers (147 KB per stereo session and tick: with 1024 sessions one thread
// spends 12 ms per tick on it).  run(n, fn) calls fn(i) for i in [0, n) on the helpers and the caller.
class StagePool {
 public:
  explicit StagePool(unsigned helpers) {
    for (unsigned i = 0; i < helpers; ++i) threads_.emplace_back([this] { loop(); });
  }
  ~StagePool() {
    {
      std::lock_guard<std::mutex> l(mu_);
      stop_ = true;
    }
    cv_start_.notify_all();
    for (auto& t : threads_) t.join();
  }
  template <typename F>
  void run(size_t n, F&& fn) {
    if (threads_.empty() || n < 32) {
      for (size_t i = 0; i < n; ++i) fn(i);
      return;
    }
    std::function<void(size_t)> f = fn;
    {
      std::lock_guard<std::mutex> l(mu_);
      fn_ = &f;
      n_ = n;
      next_.store(0);
      busy_ = (unsigned)threads_.size();
      ++epoch_;
    }
    cv_start_.notify_all();
    work();
    std::unique_lock<std::mutex> l(mu_);
    cv_done_.wait(l, [this] { return busy_ == 0; });
    fn_ = nullptr;
  }

 private:
  void work() {
    for (;;) {
      const size_t i0 = next_.fetch_add(8);
      if (i0 >= n_) return;
      for (size_t i = i0; i < std::min(n_, i0 + 8); ++i) (*fn_)(i);
    }
  }
  void loop() {
    uint64_t seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> l(mu_);
        cv_start_.wait(l, [&] { return stop_ || epoch_ != seen; });
        if (stop_) return;
        seen = epoch_;
      }
      work();
      {
        std::lock_guard<std::mutex> l(mu_);
        if (--busy_ == 0) cv_done_.notify_one();
      }
    }
  }
  std::vector<std::thread> threads_;
  std::mutex mu_;
  std::condition_variable cv_start_, cv_done_;
  const std::function<void(size_t)>* fn_ = nullptr;
  size_t n_ = 0;
  std::atomic<size_t> next_{0};
  unsigned busy_ = 0;
  uint64_t epoch_ = 0;
  bool stop_ = false;
};
}  // namespace

struct peaq_broker {
  peaq_ctx* ctx = nullptr;
  int advanced = 0, channels = 1;
  double level_db = 92.;
  Settings cfg;                     // the context's settings when the broker was created
  int max_sessions = 0;
  std::vector<BrokerSlot*> slots;
  std::mutex tick_mu;               // one tick at a time; guards everything below
  hipStream_t stream = nullptr;
  hipEvent_t staged = nullptr;
  bool staged_pending = false;
  BrokerStage fft, fbs;
  BrokerMeta meta;                  // the per-pair scalars of a tick's launches
  FbPairWindow* h_win = nullptr;    // pinned: one per launch pair of the filter-bank launch
  DevBuf d_win, records, fb_records, state, fbstate, hp_rows, result;
  std::thread worker;
  std::atomic<bool> running{false};
  unsigned period_us = 0;
  std::atomic<bool> failed{false};  // a tick hit a device error: every later call reports it
  std::mutex err_mu;                // guards worker_error
  std::string worker_error;
  std::mutex cv_mu;                 // pushers blocked by the back-pressure wait here for the next tick
  std::condition_variable tick_cv;
  uint64_t n_ticks = 0, n_launches = 0, n_frames = 0;
  uint32_t max_active = 0;
  // timing (peaq_broker_stats_t): the device part of a tick is known when the next tick (or a read-out) has
  // waited for it, so the waits of its sessions are parked until then
  hipEvent_t t_begin = nullptr, t_end = nullptr;
  UsHistogram h_host, h_device, h_latency;
  std::vector<float> parked_wait_us;
  double parked_host_us = 0.;
  std::vector<BrokerJob> jobs;      // the storage of TickPlan::jobs
  std::unique_ptr<StagePool> stagers;
  // peaq_broker_create_multi: this broker owns no device; it deals its sessions out to one broker per device
  // (session id = shard + n_shards * the shard's own id) and forwards every call
  std::vector<peaq_broker*> shards;
  std::vector<peaq_ctx*> shard_ctx;
  std::vector<int> shard_open;      // open sessions per shard (guarded by tick_mu)
  // the meter (peaq_broker_set_meter; peaq_meter.hip): one geometry for all slots, because it shapes the launch
  MeterGeometry meter;
  MeterBuffers m_buf;               // a stream per slot, kBrokerMaxFrames / kBrokerMaxBlocks units a tick

  // live alignment (peaq_broker_set_align; peaq_watch.hip): one configuration for all slots
  LiveAlignGeometry align;
  LiveAlignBuffers a_buf;           // kBrokerAcquirePerTick probes a tick; the watch's rows per launch pair, state per slot
  float* a_hprobe[2] = {nullptr, nullptr};   // pinned: this tick's probes [kBrokerAcquirePerTick][probe][channels]
  peaq_delay* a_hrec = nullptr;     // pinned: the records of the last tick's estimates
  std::vector<BrokerAcquire> a_pending;      // the estimates the last tick enqueued

  // live rate conversion (peaq_broker_set_rates; peaq_live_rate.hip): one pair of rates for all slots, because they
  // size the staging; the raw side of the FFT windows, of the filter-bank windows and of the probes
  uint32_t rate[2] = {48000, 48000};
  RateGeometry geo[2] = {{1, 1, 0}, {1, 1, 0}};
  BrokerRawStage raw_fft, raw_fbs, raw_acq;
  bool rated(int p) const { return rate[p] != 48000; }

  ModelSetup model() const { return ModelSetup{ctx, cfg, advanced, channels, level_db}; }
};

// a held slot whose probe is there, or whose flush has been asked for: the next tick with room estimates its delay
static inline bool broker_probe_ready(const peaq_broker* b, const BrokerSlot& sl) {
  return sl.flush.requested || std::min(sl.framer.have(0), sl.framer.have(1)) >= b->align.probe;
}

static inline bool broker_is_multi(const peaq_broker* b) { return b && !b->shards.empty(); }
// An entry `who` that takes a session id, on a multi-device broker: call(shard, id there) of the device broker that
// owns session `sid` -> its result, or the refusal of a bad id.  Nothing: b owns its sessions itself.
template <typename F>
static std::optional<int> broker_forward(peaq_broker* b, int sid, const char* who, F&& call) {
  if (!broker_is_multi(b)) return std::nullopt;
  const int n = (int)b->shards.size();
  if (sid < 0 || sid >= b->max_sessions) return fail(PEAQ_ERR_ARG, std::string(who) + ": bad session id");
  return call(b->shards[sid % n], sid / n);
}

// window w of the slot's stream into staging entry `idx`
static void broker_stage_copy(peaq_broker* b, const BrokerSlot& sl, const BrokerStage& st, BrokerRawStage& rs, unsigned idx,
                              const StreamWindow& w) {
  const size_t off = idx * st.samples * b->channels, roff = idx * rs.samples * b->channels;
  float* const dst[2] = {st.h[0] + off, st.h[1] + off};
  float* const raw[2] = {rs.h[0] ? rs.h[0] + roff : nullptr, rs.h[1] ? rs.h[1] + roff : nullptr};
  peaq_rate_segment* const seg[2] = {rs.seg[0].empty() ? nullptr : &rs.seg[0][idx],      // (of a rated pad only)
                                     rs.seg[1].empty() ? nullptr : &rs.seg[1][idx]};
  stage_window(sl.framer, w, dst, raw, seg);
}

// the samples of `n` launch pairs up: a plain pad's windows as they are staged, a rated pad's raw samples and ONE
// launch of the range converter over the tick's segments, which writes the windows in place of the copy
static int broker_upload(peaq_broker* b, const BrokerStage& st, const BrokerRawStage& rs, unsigned n) {
  for (int p = 0; p < 2; ++p) {
    if (!b->rated(p)) {
      HIP_TRY(hipMemcpyAsync(st.d[p].p, st.h[p], n * st.samples * b->channels * sizeof(float), hipMemcpyHostToDevice, b->stream));
      continue;
    }
    HIP_TRY(hipMemcpyAsync(rs.d[p].p, rs.h[p], n * rs.samples * b->channels * sizeof(float), hipMemcpyHostToDevice, b->stream));
    if (int rc = live_rate_convert(b->ctx, b->channels, b->rate[p], (int)n, rs.seg[p].data(), rs.d[p].as<float>(),
                                           rs.samples, st.d[p].as<float>(), st.samples, b->stream))
      return rc;
  }
  return PEAQ_OK;
}

// ---- the phases of a tick, in the order broker_tick_locked runs them -----------------------------------------
// settle: the last tick's device work, if it is still out, is waited for.  Its device time is known now, and with it
// the latency of the sessions it served (wait for the tick + the tick's host part + its device part).
static int broker_settle(peaq_broker* b) {
  if (!b->staged_pending) return PEAQ_OK;
  HIP_TRY(hipEventSynchronize(b->staged));
  b->staged_pending = false;
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, b->t_begin, b->t_end) != hipSuccess) ms = 0.f;
  const double dev_us = 1e3 * ms;
  b->h_device.add(dev_us);
  b->h_host.add(b->parked_host_us);
  for (float w : b->parked_wait_us) b->h_latency.add((double)w + b->parked_host_us + dev_us);
  b->parked_wait_us.clear();
  return PEAQ_OK;
}

// release acquired (live alignment): the records of the estimates the last tick enqueued are in pinned memory now;
// their framers are released, and the streams' first units ride in this tick
static void broker_release_acquired(peaq_broker* b) {
  for (size_t i = 0; i < b->a_pending.size(); ++i) {
    const BrokerAcquire& q = b->a_pending[i];
    BrokerSlot& sl = *b->slots[q.sid];
    std::lock_guard<std::mutex> lock(sl.mu);
    if (!sl.open || sl.epoch != q.epoch || !sl.acquiring) continue;   // (closed, or closed and opened again, meanwhile)
    sl.delay = live_delay_acquired(b->align.probe, q.have, &b->a_hrec[i]);
    sl.acquiring = false;
    sl.framer.release(sl.delay.skip_ref, sl.delay.skip_test);
  }
  b->a_pending.clear();
}

// scan, a held slot (live alignment): nothing is taken from a held stream.  Once its probe is there (or its flush asked
// for) and no estimate of it is under way, its probes are staged, at most kBrokerAcquirePerTick slots a tick; the rest
// wait.  A flush with nothing on a pad releases the stream at once: no device work.
static void broker_scan_held(peaq_broker* b, TickPlan& pl, int sid, BrokerSlot& sl) {
  if (sl.acquiring || !broker_probe_ready(b, sl)) return;
  const StreamFramer& fr = sl.framer;
  const uint64_t have[2] = {fr.have(0), fr.have(1)};   // (a rated pad: converted samples, as the probe and the skips)
  if (!have[0] || !have[1]) {
    sl.delay = live_delay_acquired(b->align.probe, have, nullptr);
    sl.framer.release(sl.delay.skip_ref, sl.delay.skip_test);   // (0, 0)
    return;
  }
  if (pl.n_acq == kBrokerAcquirePerTick) return;
  const size_t i = pl.n_acq++;
  for (int p = 0; p < 2; ++p) {
    pl.acq_n[p][i] = static_cast<uint32_t>(std::min<uint64_t>(have[p], b->align.probe));
    if (!fr.rated(p)) {
      std::memcpy(b->a_hprobe[p] + i * (size_t)b->align.probe * b->channels, fr.pad[p].at(0, b->channels),
                  (size_t)pl.acq_n[p][i] * b->channels * sizeof(float));
      continue;
    }
    uint64_t lo, hi;                                 // the probe's raw samples; the launch converts them
    fr.raw_span(p, 0, pl.acq_n[p][i], &lo, &hi);
    std::memcpy(b->raw_acq.h[p] + i * b->raw_acq.samples * b->channels, fr.pad[p].at(lo, b->channels),
                (size_t)(hi - lo) * b->channels * sizeof(float));
    b->raw_acq.seg[p][i] = peaq_rate_segment{0, lo, fr.ended ? fr.pad[p].total : UINT64_MAX, pl.acq_n[p][i],
                                             static_cast<uint32_t>(hi - lo)};
  }
  b->a_pending.push_back(BrokerAcquire{sid, sl.epoch, {have[0], have[1]}});
  sl.acquiring = true;
}

// scan, a slot whose stream runs: its windows of this tick (take_slot_windows, peaq_host.h) into the plan, the rows of
// the meta table and h_win.  The samples are copied by the stage phase: only the positions are taken here.
static void broker_scan_slot(peaq_broker* b, TickPlan& pl, int sid, BrokerSlot& sl) {
  const SlotTake t = take_slot_windows(sl.framer, sl.flush, sl.meter, b->meter.on, b->advanced != 0, kBrokerMaxFrames,
                                       kBrokerMaxBlocks);
  const BrokerMeta& mt = b->meta;
  const uint32_t slot = static_cast<uint32_t>(sid);
  const uint32_t tot_f = sl.meter.ended ? sl.meter.total[kUnitFrame] : UINT_MAX;   // (UINT_MAX: the flush is not known yet)
  const uint32_t tot_b = sl.meter.ended ? sl.meter.total[kUnitBlock] : UINT_MAX;
  BrokerJob job{sid, 0, 0, t.fft, t.fb};
  if (t.fft.count) {
    const unsigned i = job.fft_idx = pl.active++;
    mt.host(BrokerMeta::kNRef)[i] = static_cast<uint32_t>(t.fft.valid[0]);
    mt.host(BrokerMeta::kNTest)[i] = static_cast<uint32_t>(t.fft.valid[1]);
    mt.host(BrokerMeta::kFrame0)[i] = t.fft.first;
    mt.host(BrokerMeta::kNFrames)[i] = t.fft.count;
    mt.host(BrokerMeta::kSlot)[i] = slot;
    mt.host(BrokerMeta::kTotalFrames)[i] = tot_f;
    mt.host(BrokerMeta::kWatchFrames)[i] = t.fft.flush ? 0 : t.fft.count;
    pl.frames += t.fft.count;
    pl.max_nf = std::max(pl.max_nf, t.fft.count);
  }
  if (t.closing) {                                   // (filled from the far end; the stage phase moves it up)
    const unsigned at = (unsigned)b->max_sessions - 1 - pl.fb_closing++;
    b->h_win[at] = FbPairWindow{tot_b, 0, 0, slot};
    mt.host(BrokerMeta::kFbTotalFrames)[at] = tot_f;
    mt.host(BrokerMeta::kFbTotalBlocks)[at] = tot_b;
  }
  if (t.fb.count) {
    const unsigned i = job.fb_idx = pl.fb_active++;
    mt.host(BrokerMeta::kFbNRef)[i] = static_cast<uint32_t>(t.fb.valid[0]);
    mt.host(BrokerMeta::kFbNTest)[i] = static_cast<uint32_t>(t.fb.valid[1]);
    mt.host(BrokerMeta::kFbTotalFrames)[i] = tot_f;
    mt.host(BrokerMeta::kFbTotalBlocks)[i] = tot_b;
    b->h_win[i] = FbPairWindow{t.fb.first, t.fb.count, t.fb.prev_blocks, slot};
    pl.max_nb = std::max(pl.max_nb, t.fb.count);
  }
  if (!t.fft.count && !t.fb.count) return;
  pl.jobs.push_back(job);
  if (sl.t_ready_us >= 0.) b->parked_wait_us.push_back((float)(pl.t_tick - sl.t_ready_us));
  // more whole units left behind (the per-tick cap)?  They have been waiting since now at the latest.
  sl.t_ready_us = (sl.framer.ready() || sl.flush.requested) ? pl.t_tick : -1.;
}

// scan: every open slot under its lock
static void broker_scan(peaq_broker* b, TickPlan& pl) {
  pl.t_tick = now_us();
  for (int sid = 0; sid < b->max_sessions; ++sid) {
    BrokerSlot& sl = *b->slots[sid];
    std::lock_guard<std::mutex> lock(sl.mu);
    if (!sl.open) continue;
    if (sl.framer.held) broker_scan_held(b, pl, sid, sl);
    if (!sl.framer.held) broker_scan_slot(b, pl, sid, sl);
  }
}

// stage: the meter's entries without units go behind the tick's own; the sessions' new samples into the pinned staging
// buffers; then drop what both consumers are done with.  (Only ticks consume, and ticks are serialised: the positions
// the scan recorded stay valid; a concurrent push may reallocate a FIFO, hence the slot lock around each copy.)
// Then the tick's device time begins, and the meta table's rows go up.
static int broker_stage(peaq_broker* b, const TickPlan& pl) {
  for (unsigned i = 0; i < pl.fb_closing; ++i) {
    const unsigned at = (unsigned)b->max_sessions - 1 - i, to = pl.fb_active + i;
    b->h_win[to] = b->h_win[at];
    for (BrokerMeta::Row r : {BrokerMeta::kFbTotalFrames, BrokerMeta::kFbTotalBlocks}) b->meta.host(r)[to] = b->meta.host(r)[at];
  }
  b->stagers->run(pl.jobs.size(), [b, &pl](size_t i) {
    const BrokerJob& j = pl.jobs[i];
    BrokerSlot& sl = *b->slots[j.sid];
    std::lock_guard<std::mutex> lock(sl.mu);
    if (j.fft.count) broker_stage_copy(b, sl, b->fft, b->raw_fft, j.fft_idx, j.fft);
    if (j.fb.count) broker_stage_copy(b, sl, b->fbs, b->raw_fbs, j.fb_idx, j.fb);
    sl.framer.trim();
  });
  HIP_TRY(hipEventRecord(b->t_begin, b->stream));
  HIP_TRY(b->meta.upload(b->meter.on, b->align.window != 0, b->stream));
  return PEAQ_OK;
}

// launch, FFT path: samples up; front end, watch, back end over the tick's `active` pairs.  With the meter on the live
// back end leaves this tick's records at [launch index][unit of the tick], and one small kernel behind it walks every
// session's units through its open windows (the filter-bank path below does the same).
static int broker_launch_fft(peaq_broker* b, const TickPlan& pl) {
  if (!pl.active) return PEAQ_OK;
  const BrokerMeta& mt = b->meta;
  const ModelSetup m = b->model();
  if (int rc = broker_upload(b, b->fft, b->raw_fft, pl.active)) return rc;
  FrontendArgs fa = m.frontend();
  fa.ref = b->fft.d[0].as<float>();
  fa.test = b->fft.d[1].as<float>();
  fa.pair_stride = b->fft.samples;
  fa.n_ref = mt.dev(BrokerMeta::kNRef);
  fa.n_test = mt.dev(BrokerMeta::kNTest);
  fa.pair_frame0 = mt.dev(BrokerMeta::kFrame0);
  fa.pair_nframes = mt.dev(BrokerMeta::kNFrames);
  fa.frames_per_launch = pl.max_nf;
  fa.records = b->records.as<double>();
  HIP_TRY(launch_frontend(m.fft_bands(), fa, pl.active, b->stream));
  if (b->align.window) {
    WatchArgs wa = b->a_buf.watch(fa, b->align.window, pl.max_nf, kBrokerMaxFrames);
    wa.s_frames = mt.dev(BrokerMeta::kWatchFrames);
    wa.s_slot = mt.dev(BrokerMeta::kSlot);
    HIP_TRY(launch_delay_watch(wa, pl.active, b->stream));
  }
  BackendArgs ba = m.backend(fa);
  ba.frames_per_launch = pl.max_nf;
  ba.state = b->state.as<PairState>();
  ba.pair_slot = mt.dev(BrokerMeta::kSlot);
  HIP_TRY(launch_backend(ba, pl.active, b->stream, b->m_buf.outputs(b->meter)));
  if (!b->meter.on) return PEAQ_OK;
  MeterArgs mf = b->m_buf.args(b->meter);
  mf.rec_stride = pl.max_nf;
  mf.s_unit0 = mt.dev(BrokerMeta::kFrame0);
  mf.s_nunits = mt.dev(BrokerMeta::kNFrames);
  mf.s_slot = mt.dev(BrokerMeta::kSlot);
  mf.s_total_frames = mf.s_total_units = mt.dev(BrokerMeta::kTotalFrames);
  HIP_TRY(launch_meter_fft(mf, b->advanced != 0, b->records.as<double>(), b->channels, pl.active, b->stream));
  if (b->meter.bands)                                // the band rows of the same windows, by the same per-stream rows
    HIP_TRY(launch_meter_bands(mf, b->m_buf.band_args(), b->advanced != 0, b->channels, pl.active, b->stream));
  return PEAQ_OK;
}

// launch, filter-bank path: samples and windows up; front end, back end over the tick's `fb_active` pairs; the meter
// over them and the entries without units behind them (whose windows go up alone in a tick that has no pair)
static int broker_launch_fb(peaq_broker* b, const TickPlan& pl) {
  const unsigned n_win = pl.fb_active + pl.fb_closing;
  const size_t win_bytes = n_win * sizeof(FbPairWindow);
  if (!pl.fb_active && n_win) HIP_TRY(hipMemcpyAsync(b->d_win.p, b->h_win, win_bytes, hipMemcpyHostToDevice, b->stream));
  if (pl.fb_active) {
    const BrokerMeta& mt = b->meta;
    const ModelSetup m = b->model();
    if (int rc = broker_upload(b, b->fbs, b->raw_fbs, pl.fb_active)) return rc;
    HIP_TRY(hipMemcpyAsync(b->d_win.p, b->h_win, win_bytes, hipMemcpyHostToDevice, b->stream));
    FbFrontArgs ff = m.fb_frontend();
    ff.ref = b->fbs.d[0].as<float>();
    ff.test = b->fbs.d[1].as<float>();
    ff.pair_stride = b->fbs.samples;
    ff.n_ref = mt.dev(BrokerMeta::kFbNRef);
    ff.n_test = mt.dev(BrokerMeta::kFbNTest);
    ff.blocks_per_launch = pl.max_nb;
    ff.fbstate = b->fbstate.as<FbSignalState>();
    ff.hp_scratch = b->hp_rows.as<double>();
    ff.hp_row_stride = kBrokerRowStride;
    ff.records = b->fb_records.as<double>();
    ff.windows = b->d_win.as<FbPairWindow>();
    HIP_TRY(launch_fb_frontend(ff, pl.fb_active, b->stream));
    FbBackendArgs fbk = m.fb_backend(ff);
    fbk.blocks_per_launch = pl.max_nb;
    fbk.state = b->state.as<PairState>();
    HIP_TRY(launch_fb_backend(fbk, pl.fb_active, b->stream, b->m_buf.outputs(b->meter)));
  }
  if (!b->meter.on || !n_win) return PEAQ_OK;
  MeterArgs mb = b->m_buf.args(b->meter);
  mb.s_win = b->d_win.as<FbPairWindow>();
  mb.s_total_frames = b->meta.dev(BrokerMeta::kFbTotalFrames);
  mb.s_total_units = b->meta.dev(BrokerMeta::kFbTotalBlocks);
  HIP_TRY(launch_meter_fb(mb, b->channels, n_win, b->stream));
  return PEAQ_OK;
}

// launch, acquisition (live alignment): one estimate over this tick's probes, its records copied to pinned memory --
// enqueued, not waited for: the next tick reads them after its wait for `staged`
static int broker_launch_acquire(peaq_broker* b, const TickPlan& pl) {
  if (!pl.n_acq) return PEAQ_OK;
  const LiveAlignBuffers& a = b->a_buf;
  const size_t row = (size_t)b->align.probe * b->channels;
  for (int p = 0; p < 2; ++p) {
    if (!b->rated(p)) {
      HIP_TRY(hipMemcpyAsync(a.probe[p].p, b->a_hprobe[p], pl.n_acq * row * sizeof(float), hipMemcpyHostToDevice, b->stream));
      continue;
    }
    const BrokerRawStage& rs = b->raw_acq;           // the probes' raw samples up, converted into the probe buffer
    HIP_TRY(hipMemcpyAsync(rs.d[p].p, rs.h[p], pl.n_acq * rs.samples * b->channels * sizeof(float), hipMemcpyHostToDevice,
                           b->stream));
    if (int rc = live_rate_convert(b->ctx, b->channels, b->rate[p], (int)pl.n_acq, rs.seg[p].data(),
                                           rs.d[p].as<float>(), rs.samples, a.probe[p].as<float>(), b->align.probe, b->stream))
      return rc;
  }
  if (int rc = peaq_batch_estimate_delay(b->ctx, b->channels, (int)pl.n_acq, a.probe[0].as<float>(), a.probe[1].as<float>(),
                                         b->align.probe, pl.acq_n[0], pl.acq_n[1], 0, b->align.max_lag,
                                         a.rec.as<peaq_delay>(), b->stream))
    return rc;
  HIP_TRY(hipMemcpyAsync(b->a_hrec, a.rec.p, pl.n_acq * sizeof(peaq_delay), hipMemcpyDeviceToHost, b->stream));
  return PEAQ_OK;
}

// finish: the events the next tick waits for and times by, the counters, the host part of this tick
static int broker_finish(peaq_broker* b, const TickPlan& pl, unsigned* n_active_out) {
  HIP_TRY(hipEventRecord(b->t_end, b->stream));
  HIP_TRY(hipEventRecord(b->staged, b->stream));
  b->staged_pending = true;
  b->parked_host_us = now_us() - pl.t_tick;
  ++b->n_launches;
  b->n_frames += pl.frames;
  const unsigned n_active = std::max(pl.active, pl.fb_active);
  b->max_active = std::max(b->max_active, n_active);
  if (n_active_out) *n_active_out = n_active;
  return PEAQ_OK;
}

static int broker_tick_locked(peaq_broker* b, unsigned* n_active_out) {
  TickPlan pl(b->jobs);
  if (n_active_out) *n_active_out = 0;
  HIP_TRY(hipSetDevice(b->ctx->device));
  if (int rc = broker_settle(b)) return rc;
  broker_release_acquired(b);
  broker_scan(b, pl);
  ++b->n_ticks;
  if (pl.idle()) return PEAQ_OK;
  if (int rc = broker_stage(b, pl)) return rc;
  if (int rc = broker_launch_fft(b, pl)) return rc;
  if (int rc = broker_launch_fb(b, pl)) return rc;
  if (int rc = broker_launch_acquire(b, pl)) return rc;
  return broker_finish(b, pl, n_active_out);
}

// one tick under tick_mu; a failure is remembered and stops the broker for good
static int broker_tick_checked(peaq_broker* b, unsigned* n_active) {
  if (b->failed.load()) {
    std::lock_guard<std::mutex> e(b->err_mu);
    return fail(PEAQ_ERR_DEVICE, "broker stopped after a device error: " + b->worker_error);
  }
  const int rc = broker_tick_locked(b, n_active);
  if (rc != PEAQ_OK) {
    std::lock_guard<std::mutex> e(b->err_mu);
    b->worker_error = peaq_err_string();
    b->failed.store(true);
  }
  return rc;
}

static int broker_failed(peaq_broker* b, const char* who) {
  std::lock_guard<std::mutex> e(b->err_mu);
  return fail(PEAQ_ERR_DEVICE, std::string(who) + ": broker stopped after a device error: " + b->worker_error);
}

extern "C" int peaq_broker_create(peaq_ctx* c, int advanced, int channels, double level_db, int max_sessions,
                                  peaq_broker** out) {
  if (!c || !out) return fail(PEAQ_ERR_ARG, "peaq_broker_create: NULL argument");
  *out = nullptr;
  if (int rc = check_channels("peaq_broker_create", channels)) return rc;
  if (int rc = check_level("peaq_broker_create", level_db)) return rc;
  if (max_sessions < 1 || max_sessions > 65536) return fail(PEAQ_ERR_ARG, "peaq_broker_create: max_sessions 1..65536");
  HIP_TRY(hipSetDevice(c->device));
  peaq_broker* b = new (std::nothrow) peaq_broker;
  if (!b) return fail(PEAQ_ERR_NOMEM, "out of host memory");
  b->ctx = c;
  b->cfg = c->settings;
  b->advanced = advanced ? 1 : 0;
  b->channels = channels;
  b->level_db = level_db;
  b->max_sessions = max_sessions;
  {
    // staging helpers beside the ticking thread: PEAQ_AMD_BROKER_STAGERS (default 3, 0 = none); idle
    // unless a tick has at least 32 sessions' samples to copy
    const char* e = std::getenv("PEAQ_AMD_BROKER_STAGERS");
    const long want = e && *e ? std::strtol(e, nullptr, 10) : 3;
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    b->stagers.reset(new StagePool(max_sessions >= 32 ? (unsigned)std::min<long>(std::max<long>(want, 0), hw - 1) : 0));
  }
  b->slots.reserve(max_sessions);
  for (int i = 0; i < max_sessions; ++i) b->slots.push_back(new BrokerSlot);
  const size_t S = (size_t)max_sessions;
  int rc = [&]() -> int {
    if (int r = b->fft.alloc(S, kBrokerStageSamples, channels)) return r;
    if (int r = b->meta.alloc(S)) return r;
    HIP_TRY(b->records.reserve(S * kBrokerMaxFrames * channels * kRecDoubles * sizeof(double)));
    HIP_TRY(b->state.reserve(S * sizeof(PairState)));
    HIP_TRY(b->result.reserve(sizeof(ResultRecord)));
    HIP_TRY(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&b->staged, hipEventDisableTiming));
    HIP_TRY(hipEventCreate(&b->t_begin));
    HIP_TRY(hipEventCreate(&b->t_end));
    HIP_TRY(launch_state_init(b->state.as<PairState>(), b->advanced, max_sessions, b->stream));
    if (b->advanced) {
      if (int r = b->fbs.alloc(S, kBrokerFbStageSamples, channels)) return r;
      const size_t n_signals = S * channels * 2;
      HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&b->h_win), S * sizeof(FbPairWindow), hipHostMallocDefault));
      HIP_TRY(b->d_win.reserve(S * sizeof(FbPairWindow)));
      HIP_TRY(b->fb_records.reserve(S * kBrokerMaxBlocks * channels * kFbRecDoubles * sizeof(double)));
      HIP_TRY(b->fbstate.reserve(n_signals * sizeof(FbSignalState)));
      HIP_TRY(hipMemsetAsync(b->fbstate.p, 0, n_signals * sizeof(FbSignalState), b->stream));
      HIP_TRY(b->hp_rows.reserve(n_signals * kBrokerRowStride * sizeof(double)));
    }
    return PEAQ_OK;
  }();
  if (rc != PEAQ_OK) {
    peaq_broker_destroy(b);
    return rc;
  }
  *out = b;
  return PEAQ_OK;
}

extern "C" int peaq_broker_create_multi(const int* devices, int n_devices, int advanced, int channels, double level_db,
                                        int max_sessions, const peaq_settings* settings, int fir_mode, peaq_broker** out) {
  if (!devices || !out) return fail(PEAQ_ERR_ARG, "peaq_broker_create_multi: NULL argument");
  *out = nullptr;
  if (n_devices < 1 || n_devices > 64) return fail(PEAQ_ERR_ARG, "peaq_broker_create_multi: 1..64 devices");
  if (max_sessions < n_devices) return fail(PEAQ_ERR_ARG, "peaq_broker_create_multi: fewer sessions than devices");
  peaq_broker* b = new (std::nothrow) peaq_broker;
  if (!b) return fail(PEAQ_ERR_NOMEM, "out of host memory");
  b->advanced = advanced ? 1 : 0;
  b->channels = channels;
  b->level_db = level_db;
  const int per_shard = (max_sessions + n_devices - 1) / n_devices;
  b->max_sessions = per_shard * n_devices;
  for (int i = 0; i < n_devices; ++i) {
    peaq_ctx* c = nullptr;
    int rc = peaq_ctx_create(devices[i], &c);
    if (rc == PEAQ_OK && settings) rc = peaq_ctx_set_settings(c, settings);
    if (rc == PEAQ_OK && fir_mode >= 0) rc = peaq_ctx_set_fir_mode(c, fir_mode);
    peaq_broker* sh = nullptr;
    if (rc == PEAQ_OK) rc = peaq_broker_create(c, advanced, channels, level_db, per_shard, &sh);
    if (rc != PEAQ_OK) {
      const std::string msg = peaq_err_string();
      if (c) peaq_ctx_destroy(c);
      peaq_broker_destroy(b);
      return fail(rc, "peaq_broker_create_multi: device " + std::to_string(devices[i]) + ": " + msg);
    }
    b->shards.push_back(sh);
    b->shard_ctx.push_back(c);
    b->shard_open.push_back(0);
  }
  *out = b;
  return PEAQ_OK;
}

// Test hook (include/peaq_amd.h): shard `shard` of a multi-device broker (0 of a plain one) is put into the state a
// device error during one of its ticks leaves it in -- failed for good, with `message` as the error it keeps.
extern "C" int peaq_debug_broker_fail_shard(peaq_broker* b, int shard, const char* message) {
  if (!b) return fail(PEAQ_ERR_ARG, "peaq_debug_broker_fail_shard: broker is NULL");
  peaq_broker* sh = b;
  if (broker_is_multi(b)) {
    if (shard < 0 || shard >= (int)b->shards.size()) return fail(PEAQ_ERR_ARG, "peaq_debug_broker_fail_shard: no such shard");
    sh = b->shards[shard];
  } else if (shard != 0) {
    return fail(PEAQ_ERR_ARG, "peaq_debug_broker_fail_shard: no such shard");
  }
  std::lock_guard<std::mutex> tick(sh->tick_mu);
  std::lock_guard<std::mutex> e(sh->err_mu);
  sh->worker_error = message ? message : "injected fault";
  sh->failed.store(true);
  return PEAQ_OK;
}

extern "C" int peaq_broker_devices(const peaq_broker* b) { return !b ? 0 : broker_is_multi(b) ? (int)b->shards.size() : 1; }
extern "C" size_t peaq_broker_stats_size(void) { return sizeof(peaq_broker_stats_t); }

extern "C" int peaq_broker_stop(peaq_broker* b) {
  if (!b) return fail(PEAQ_ERR_ARG, "peaq_broker_stop: broker is NULL");
  if (broker_is_multi(b)) {
    int rc = PEAQ_OK;
    for (peaq_broker* sh : b->shards) {
      const int r = peaq_broker_stop(sh);
      if (r != PEAQ_OK) rc = r;
    }
    return rc;
  }
  if (b->running.exchange(false) && b->worker.joinable()) b->worker.join();
  b->tick_cv.notify_all();          // blocked pushers go on ticking inline
  return PEAQ_OK;
}

extern "C" void peaq_broker_destroy(peaq_broker* b) {
  if (!b) return;
  if (broker_is_multi(b) || !b->ctx) {               // (no context: a multi broker whose creation failed half way)
    for (peaq_broker* sh : b->shards) peaq_broker_destroy(sh);
    for (peaq_ctx* c : b->shard_ctx) peaq_ctx_destroy(c);
    delete b;
    return;
  }
  (void)peaq_broker_stop(b);
  (void)hipSetDevice(b->ctx->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  if (b->h_win) (void)hipHostFree(b->h_win);
  for (int p = 0; p < 2; ++p)
    if (b->a_hprobe[p]) (void)hipHostFree(b->a_hprobe[p]);
  if (b->a_hrec) (void)hipHostFree(b->a_hrec);
  if (b->staged) (void)hipEventDestroy(b->staged);
  if (b->t_begin) (void)hipEventDestroy(b->t_begin);
  if (b->t_end) (void)hipEventDestroy(b->t_end);
  if (b->stream) (void)hipStreamDestroy(b->stream);
  for (BrokerSlot* s : b->slots) delete s;
  delete b;                         // (the staging buffers, the meta table and the device buffers go with it)
}

extern "C" int peaq_broker_open(peaq_broker* b, int* session_id) {
  if (!b || !session_id) return fail(PEAQ_ERR_ARG, "peaq_broker_open: NULL argument");
  if (broker_is_multi(b)) {                            // the device with the fewest open sessions takes it
    std::lock_guard<std::mutex> place(b->tick_mu);
    const int n = (int)b->shards.size();
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return b->shard_open[x] < b->shard_open[y]; });
    int err_rc = PEAQ_OK;
    std::string err_msg;
    for (int i : order) {
      int local = -1;
      const int rc = peaq_broker_open(b->shards[i], &local);
      if (rc == PEAQ_OK) {
        ++b->shard_open[i];
        *session_id = i + n * local;
        return PEAQ_OK;
      }
      if (rc != PEAQ_ERR_STATE && err_rc == PEAQ_OK) {   // a device's own failure, not "its slots are in use": keep it
        err_rc = rc;
        err_msg = "device " + std::to_string(b->shards[i]->ctx->device) + ": " + peaq_err_string();
      }
    }
    if (err_rc != PEAQ_OK) return fail(err_rc, "peaq_broker_open: " + err_msg);
    return fail(PEAQ_ERR_STATE, "peaq_broker_open: all session slots are in use");
  }
  std::lock_guard<std::mutex> tick(b->tick_mu);
  for (int sid = 0; sid < b->max_sessions; ++sid) {
    BrokerSlot& sl = *b->slots[sid];
    std::lock_guard<std::mutex> lock(sl.mu);
    if (sl.open) continue;
    HIP_TRY(hipSetDevice(b->ctx->device));
    HIP_TRY(launch_state_init(b->state.as<PairState>() + sid, b->advanced, 1, b->stream));
    if (b->advanced)
      HIP_TRY(hipMemsetAsync(b->fbstate.as<FbSignalState>() + (size_t)sid * b->channels * 2, 0,
                             (size_t)b->channels * 2 * sizeof(FbSignalState), b->stream));
    if (b->meter.on) {                                 // a fresh meter: every snapshot as launch_points_init leaves it
      HIP_TRY(launch_points_init(b->m_buf.open.as<PointSnap>() + (size_t)sid * b->meter.k_open, b->meter.k_open, b->stream));
      HIP_TRY(launch_points_init(b->m_buf.ring.as<PointSnap>() + (size_t)sid * b->meter.ring, b->meter.ring, b->stream));
      if (b->meter.bands)
        if (int rc = b->m_buf.restart_bands((size_t)sid, 1, b->stream)) return rc;
    }
    if (b->align.window)                               // a fresh watch: index 0, nothing complete
      HIP_TRY(hipMemsetAsync(b->a_buf.state.as<WatchState>() + sid, 0, sizeof(WatchState), b->stream));
    sl.meter = MeterStream();
    sl.open = true;
    sl.flush.clear();
    sl.framer.reset(b->advanced, b->channels);
    sl.delay = peaq_live_delay{};
    sl.acquiring = false;
    ++sl.epoch;
    if (b->align.max_lag) sl.framer.hold();
    sl.t_ready_us = -1.;
    *session_id = sid;
    return PEAQ_OK;
  }
  return fail(PEAQ_ERR_STATE, "peaq_broker_open: all session slots are in use");
}

static BrokerSlot* broker_slot(peaq_broker* b, int sid) {
  if (!b || sid < 0 || sid >= b->max_sessions) return nullptr;
  return b->slots[sid];
}

extern "C" int peaq_broker_close(peaq_broker* b, int session_id) {
  if (const auto rc = broker_forward(b, session_id, "peaq_broker_close", peaq_broker_close)) {
    if (*rc == PEAQ_OK) {
      std::lock_guard<std::mutex> place(b->tick_mu);
      --b->shard_open[session_id % (int)b->shards.size()];
    }
    return *rc;
  }
  BrokerSlot* sl = broker_slot(b, session_id);
  if (!sl) return fail(PEAQ_ERR_ARG, "peaq_broker_close: bad broker or session id");
  std::lock_guard<std::mutex> tick(b->tick_mu);
  std::lock_guard<std::mutex> lock(sl->mu);
  if (!sl->open) return fail(PEAQ_ERR_STATE, "peaq_broker_close: session is not open");
  sl->open = false;
  sl->framer.reset(b->advanced, b->channels);
  sl->acquiring = false;
  ++sl->epoch;
  return PEAQ_OK;
}

// pad_chain (gstpeaq.c:613-640): only queues; the device work happens on the next tick
extern "C" int peaq_broker_push(peaq_broker* b, int session_id, int pad, const float* data, size_t n) {
  if (const auto fwd = broker_forward(b, session_id, "peaq_broker_push",
                       [&](peaq_broker* sh, int id) { return peaq_broker_push(sh, id, pad, data, n); }))
    return *fwd;
  BrokerSlot* sl = broker_slot(b, session_id);
  if (!sl) return fail(PEAQ_ERR_ARG, "peaq_broker_push: bad broker or session id");
  if (pad != 0 && pad != 1) return fail(PEAQ_ERR_ARG, "peaq_broker_push: pad must be 0 (ref) or 1 (test)");
  if (b->failed.load()) return broker_failed(b, "peaq_broker_push");
  if (n == 0) return PEAQ_OK;
  if (!data) return fail(PEAQ_ERR_ARG, "peaq_broker_push: data is NULL");
  // (a held stream's samples up to the probe do not count: they cannot go before the probe is there, and a push must
  // be able to bring it)
  auto backlog = [&]() {
    std::lock_guard<std::mutex> lock(sl->mu);
    const uint64_t waiting = sl->framer.backlog();
    if (!sl->framer.held) return waiting;
    return waiting > b->align.probe ? waiting - b->align.probe : 0;
  };
  {
    std::lock_guard<std::mutex> lock(sl->mu);
    if (!sl->open) return fail(PEAQ_ERR_STATE, "peaq_broker_push: session is not open");
    if (sl->framer.ended && sl->framer.rated(pad))
      return fail(PEAQ_ERR_STATE, "peaq_broker_push: the stream of a pad at " + std::to_string(sl->framer.rate[pad]) +
                                      " Hz ended at its flush; close the session and open it again");
    try {
      sl->framer.append(pad, data, n);
    } catch (const std::bad_alloc&) {
      return fail(PEAQ_ERR_NOMEM, "out of host memory");
    }
    if (sl->t_ready_us < 0. && sl->framer.ready()) sl->t_ready_us = now_us();
  }
  // back-pressure (the reference processes inside pad_chain, so its caller can never run ahead):
  // wait for the tick thread, or tick right here when there is none
  while (backlog() > kBrokerBacklog) {
    if (b->failed.load()) return broker_failed(b, "peaq_broker_push");
    if (b->running.load()) {
      std::unique_lock<std::mutex> w(b->cv_mu);
      b->tick_cv.wait_for(w, std::chrono::milliseconds(20));
    } else {
      std::lock_guard<std::mutex> tick(b->tick_mu);
      const int rc = broker_tick_checked(b, nullptr);
      if (rc != PEAQ_OK) return rc;
    }
  }
  return PEAQ_OK;
}

extern "C" int peaq_broker_flush(peaq_broker* b, int session_id) {
  if (const auto fwd = broker_forward(b, session_id, "peaq_broker_flush", peaq_broker_flush)) return *fwd;
  BrokerSlot* sl = broker_slot(b, session_id);
  if (!sl) return fail(PEAQ_ERR_ARG, "peaq_broker_flush: bad broker or session id");
  if (b->failed.load()) return broker_failed(b, "peaq_broker_flush");
  std::lock_guard<std::mutex> lock(sl->mu);
  if (!sl->open) return fail(PEAQ_ERR_STATE, "peaq_broker_flush: session is not open");
  sl->flush.request();
  sl->framer.ended = true;                           // (rated pads: what is there converts to the end)
  if (sl->t_ready_us < 0.) sl->t_ready_us = now_us();
  return PEAQ_OK;
}

extern "C" int peaq_broker_tick(peaq_broker* b, unsigned* n_active) {
  if (!b) return fail(PEAQ_ERR_ARG, "peaq_broker_tick: broker is NULL");
  if (broker_is_multi(b)) {                            // every device's launch of this tick (they run side by side)
    // EVERY device is ticked, whatever another one reports: a device that failed must not starve the sessions that
    // live on the others; the first error (with its message) is what the call returns afterwards
    unsigned total = 0;
    int first_rc = PEAQ_OK;
    std::string first_msg;
    for (peaq_broker* sh : b->shards) {
      unsigned n = 0;
      const int rc = peaq_broker_tick(sh, &n);
      if (rc != PEAQ_OK && first_rc == PEAQ_OK) {
        first_rc = rc;
        first_msg = peaq_err_string();
      }
      total += n;
    }
    if (n_active) *n_active = total;
    return first_rc == PEAQ_OK ? PEAQ_OK : fail(first_rc, first_msg);
  }
  std::lock_guard<std::mutex> tick(b->tick_mu);
  return broker_tick_checked(b, n_active);
}

// true while the session has whole frames / blocks (or a requested flush) not yet launched
// (a held stream: only once its probe is there -- ticks then acquire its delay, release it and go on)
static bool broker_slot_busy(const peaq_broker* b, BrokerSlot* sl) {
  std::lock_guard<std::mutex> lock(sl->mu);
  if (sl->framer.held) return sl->acquiring || broker_probe_ready(b, *sl);
  return sl->framer.ready() || sl->flush.requested;
}

extern "C" int peaq_broker_results(peaq_broker* b, int session_id, peaq_result* out) {
  if (const auto fwd = broker_forward(b, session_id, "peaq_broker_results",
                       [&](peaq_broker* sh, int id) { return peaq_broker_results(sh, id, out); }))
    return *fwd;
  BrokerSlot* sl = broker_slot(b, session_id);
  if (!sl || !out) return fail(PEAQ_ERR_ARG, "peaq_broker_results: bad broker, session id or out");
  std::lock_guard<std::mutex> tick(b->tick_mu);
  {
    std::lock_guard<std::mutex> lock(sl->mu);
    if (!sl->open) return fail(PEAQ_ERR_STATE, "peaq_broker_results: session is not open");
  }
  if (b->failed.load()) return broker_failed(b, "peaq_broker_results");
  while (broker_slot_busy(b, sl)) {
    const int rc = broker_tick_checked(b, nullptr);
    if (rc != PEAQ_OK) return rc;
  }
  HIP_TRY(hipSetDevice(b->ctx->device));
  HIP_TRY(launch_finalize(b->state.as<PairState>() + session_id, b->advanced, b->channels, 1,
                          b->result.as<ResultRecord>(), b->stream, b->cfg));
  HIP_TRY(hipMemcpyAsync(out, b->result.p, sizeof(peaq_result), hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return PEAQ_OK;
}

// `what` ("the meter", "the alignment") shapes the launch of every slot: entry `who` sets it while no tick thread runs
// and no session is open (the caller holds tick_mu)
static int broker_not_begun(peaq_broker* b, const std::string& who, const char* what) {
  if (b->running.load())
    return fail(PEAQ_ERR_ARG, who + ": the tick thread runs; set " + what + " before peaq_broker_start");
  for (int sid = 0; sid < b->max_sessions; ++sid) {
    std::lock_guard<std::mutex> lock(b->slots[sid]->mu);
    if (b->slots[sid]->open)
      return fail(PEAQ_ERR_ARG, who + ": session " + std::to_string(sid) + " is open; set " + what +
                                    " before the first peaq_broker_open");
  }
  return PEAQ_OK;
}

// One geometry for all sessions of the broker, because it shapes the launch: before the first open and before start.
extern "C" int peaq_broker_set_meter(peaq_broker* b, const peaq_meter_config* cfg) {
  if (!b) return fail(PEAQ_ERR_ARG, "peaq_broker_set_meter: broker is NULL");
  const bool off = !cfg || cfg->window_frames == 0;
  if (!off)
    if (int rc = check_meter_config("peaq_broker_set_meter", *cfg)) return rc;
  if (broker_is_multi(b)) {                            // every shard
    for (peaq_broker* sh : b->shards)
      if (int rc = peaq_broker_set_meter(sh, cfg)) return rc;
    return PEAQ_OK;
  }
  std::lock_guard<std::mutex> tick(b->tick_mu);
  if (int rc = broker_not_begun(b, "peaq_broker_set_meter", "the meter")) return rc;
  b->meter.on = false;
  b->meter.bands = false;                              // (the band meter goes with the geometry: meter first, then bands)
  if (off) return PEAQ_OK;
  MeterGeometry g;
  g.set(*cfg);
  HIP_TRY(hipSetDevice(b->ctx->device));
  HIP_TRY(hipStreamSynchronize(b->stream));            // (the buffers may be replaced)
  if (int rc = b->m_buf.reserve(g, (size_t)b->max_sessions, kBrokerMaxFrames, kBrokerMaxBlocks, b->advanced != 0)) return rc;
  b->meter = g;
  b->meter.on = true;
  return PEAQ_OK;
}

// The band rows of every slot's readings, where peaq_broker_set_meter is accepted and after it (which switches them off).
extern "C" int peaq_broker_set_meter_bands(peaq_broker* b, int on) {
  const std::string who("peaq_broker_set_meter_bands");
  if (!b) return fail(PEAQ_ERR_ARG, who + ": broker is NULL");
  if (broker_is_multi(b)) {                            // every shard
    for (peaq_broker* sh : b->shards)
      if (int rc = peaq_broker_set_meter_bands(sh, on)) return rc;
    return PEAQ_OK;
  }
  std::lock_guard<std::mutex> tick(b->tick_mu);
  if (int rc = broker_not_begun(b, who, "the band meter")) return rc;
  if (!b->meter.on) return fail(PEAQ_ERR_ARG, who + ": the meter is off; set it first (peaq_broker_set_meter)");
  b->meter.bands = false;                              // (stays off if the workspace cannot be reserved)
  if (!on) return PEAQ_OK;
  if (int rc = check_meter_bands_config(who, peaq_meter_config{b->meter.window, b->meter.hop, b->meter.depth})) return rc;
  HIP_TRY(hipSetDevice(b->ctx->device));
  HIP_TRY(hipStreamSynchronize(b->stream));            // (the buffers may be replaced)
  if (int rc = b->m_buf.reserve_bands(b->meter, (size_t)b->max_sessions, kBrokerMaxFrames, b->advanced != 0, b->channels))
    return rc;
  b->meter.bands = true;                               // (a slot's rows start fresh at its open)
  return PEAQ_OK;
}

// the raw staging of the rated pads: the windows of both kinds and, with an acquisition set, the probes; sized from
// the rates alone (the caller holds tick_mu; the device is idle)
static int broker_raw_reserve(peaq_broker* b) {
  const size_t S = (size_t)b->max_sessions;
  const bool r0 = b->rated(0), r1 = b->rated(1);
  auto span = [b](size_t count) {
    size_t n = 0;
    for (int p = 0; p < 2; ++p)
      if (b->rated(p)) n = std::max(n, live_rate_span_max(b->geo[p], count));
    return n;
  };
  struct Want {
    BrokerRawStage* rs;
    size_t entries, count;
  } const want[3] = {{&b->raw_fft, S, kBrokerStageSamples},
                     {&b->raw_fbs, b->advanced ? S : 0, kBrokerFbStageSamples},
                     {&b->raw_acq, b->align.max_lag ? kBrokerAcquirePerTick : 0, b->align.probe}};
  for (const Want& w : want) {
    if (int rc = w.rs->alloc(w.entries, span(w.count), b->channels, r0, r1)) return rc;
    try {
      for (int p = 0; p < 2; ++p) w.rs->seg[p].assign(b->rated(p) ? w.entries : 0, peaq_rate_segment{});
    } catch (const std::bad_alloc&) {
      return fail(PEAQ_ERR_NOMEM, "out of host memory");
    }
  }
  return PEAQ_OK;
}

// One configuration for all sessions of the broker, where peaq_broker_set_meter is accepted.
extern "C" int peaq_broker_set_align(peaq_broker* b, const peaq_live_align_config* cfg) {
  const std::string who("peaq_broker_set_align");
  if (!b) return fail(PEAQ_ERR_ARG, who + ": broker is NULL");
  const bool off = !cfg || (cfg->max_lag == 0 && cfg->watch_frames == 0);
  uint32_t probe = 0;
  if (cfg)
    if (int rc = check_live_align(who, *cfg, &probe)) return rc;
  if (broker_is_multi(b)) {                            // every shard
    for (peaq_broker* sh : b->shards)
      if (int rc = peaq_broker_set_align(sh, cfg)) return rc;
    return PEAQ_OK;
  }
  std::lock_guard<std::mutex> tick(b->tick_mu);
  if (int rc = broker_not_begun(b, who, "the alignment")) return rc;
  b->align = LiveAlignGeometry();
  if (off) return PEAQ_OK;
  HIP_TRY(hipSetDevice(b->ctx->device));
  HIP_TRY(hipStreamSynchronize(b->stream));            // (the buffers may be replaced)
  if (cfg->max_lag) {                                  // the pinned side of the probes and of their records
    const size_t bytes = (size_t)kBrokerAcquirePerTick * probe * b->channels * sizeof(float);
    for (int p = 0; p < 2; ++p) {
      if (b->a_hprobe[p]) (void)hipHostFree(b->a_hprobe[p]);
      b->a_hprobe[p] = nullptr;
      HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&b->a_hprobe[p]), bytes, hipHostMallocDefault));
    }
    if (!b->a_hrec)
      HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&b->a_hrec), kBrokerAcquirePerTick * sizeof(peaq_delay),
                            hipHostMallocDefault));
  }
  if (int rc = b->a_buf.reserve(*cfg, probe, b->channels, kBrokerAcquirePerTick, (size_t)b->max_sessions, kBrokerMaxFrames))
    return rc;
  b->align.max_lag = cfg->max_lag;
  b->align.probe = probe;
  b->align.window = cfg->watch_frames;
  return broker_raw_reserve(b);
}

// One pair of rates for all sessions of the broker, because they size the staging: where peaq_broker_set_meter is
// accepted.
extern "C" int peaq_broker_set_rates(peaq_broker* b, uint32_t rate_ref, uint32_t rate_test) {
  const std::string who("peaq_broker_set_rates");
  if (!b) return fail(PEAQ_ERR_ARG, who + ": broker is NULL");
  const uint32_t rate[2] = {rate_ref, rate_test};
  RateGeometry geo[2] = {{1, 1, 0}, {1, 1, 0}};
  for (int p = 0; p < 2; ++p)
    if (rate[p] != 48000)
      if (int rc = resample_geometry(who.c_str(), rate[p], &geo[p])) return rc;
  if (broker_is_multi(b)) {                            // every shard
    for (peaq_broker* sh : b->shards)
      if (int rc = peaq_broker_set_rates(sh, rate_ref, rate_test)) return rc;
    return PEAQ_OK;
  }
  if ((rate_ref != 48000 || rate_test != 48000) && b->max_sessions > 65535)
    return fail(PEAQ_ERR_ARG, who + ": more than 65535 sessions are more segments than one launch of the converter takes");
  std::lock_guard<std::mutex> tick(b->tick_mu);
  if (int rc = broker_not_begun(b, who, "the rates")) return rc;
  HIP_TRY(hipSetDevice(b->ctx->device));
  HIP_TRY(hipStreamSynchronize(b->stream));            // (the buffers may be replaced)
  auto set = [b](const uint32_t* r, const RateGeometry* g) {
    for (int p = 0; p < 2; ++p) {
      b->rate[p] = r[p];
      b->geo[p] = g[p];
      for (BrokerSlot* sl : b->slots) sl->framer.set_rate(p, r[p], g[p]);
    }
  };
  set(rate, geo);
  if (int rc = broker_raw_reserve(b)) {                // (stays off if the staging cannot be reserved)
    const uint32_t r48[2] = {48000, 48000};
    const RateGeometry g48[2] = {{1, 1, 0}, {1, 1, 0}};
    set(r48, g48);
    return rc;
  }
  return PEAQ_OK;
}

// The slot's delay as of the last tick enqueued.  A slot that still holds with its flush asked for is driven to its
// acquisition, as peaq_broker_results drives a session to its end.
extern "C" int peaq_broker_align_read(peaq_broker* b, int session_id, peaq_live_delay* out) {
  if (!b || !out) return fail(PEAQ_ERR_ARG, "peaq_broker_align_read: NULL argument");
  if (const auto fwd = broker_forward(b, session_id, "peaq_broker_align_read",
                       [&](peaq_broker* sh, int id) { return peaq_broker_align_read(sh, id, out); }))
    return *fwd;
  BrokerSlot* sl = broker_slot(b, session_id);
  if (!sl) return fail(PEAQ_ERR_ARG, "peaq_broker_align_read: bad session id " + std::to_string(session_id));
  std::lock_guard<std::mutex> tick(b->tick_mu);
  if (!b->align.max_lag)
    return fail(PEAQ_ERR_ARG, "peaq_broker_align_read: no acquisition is set (peaq_broker_set_align, max_lag)");
  if (b->failed.load()) return broker_failed(b, "peaq_broker_align_read");
  for (;;) {
    {
      std::lock_guard<std::mutex> lock(sl->mu);
      if (!sl->open) return fail(PEAQ_ERR_STATE, "peaq_broker_align_read: session is not open");
      if (!(sl->framer.held && sl->flush.requested)) break;
    }
    if (int rc = broker_tick_checked(b, nullptr)) return rc;
  }
  HIP_TRY(hipSetDevice(b->ctx->device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  std::lock_guard<std::mutex> lock(sl->mu);
  *out = sl->delay;
  return PEAQ_OK;
}

// The slot's newest complete watch window as of the last tick enqueued (the call waits for it); it does not tick.
extern "C" int peaq_broker_watch_read(peaq_broker* b, int session_id, peaq_delay_watch* out) {
  if (!b || !out) return fail(PEAQ_ERR_ARG, "peaq_broker_watch_read: NULL argument");
  if (const auto fwd = broker_forward(b, session_id, "peaq_broker_watch_read",
                       [&](peaq_broker* sh, int id) { return peaq_broker_watch_read(sh, id, out); }))
    return *fwd;
  BrokerSlot* sl = broker_slot(b, session_id);
  if (!sl) return fail(PEAQ_ERR_ARG, "peaq_broker_watch_read: bad session id " + std::to_string(session_id));
  std::lock_guard<std::mutex> tick(b->tick_mu);
  if (!b->align.window)
    return fail(PEAQ_ERR_ARG, "peaq_broker_watch_read: the watch is off (peaq_broker_set_align, watch_frames)");
  if (b->failed.load()) return broker_failed(b, "peaq_broker_watch_read");
  std::lock_guard<std::mutex> lock(sl->mu);
  if (!sl->open) return fail(PEAQ_ERR_STATE, "peaq_broker_watch_read: session is not open");
  HIP_TRY(hipSetDevice(b->ctx->device));
  WatchState st;
  HIP_TRY(hipMemcpyAsync(&st, b->a_buf.state.as<WatchState>() + session_id, sizeof st, hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  delay_watch_record(st, out);
  return PEAQ_OK;
}

// What was delivered up to the last tick that has been enqueued (the call waits for it); it does not tick.
// peaq_broker_meter_read and (with_rows) peaq_broker_meter_read_bands: one cursor per slot
static int broker_meter_read(peaq_broker* b, const char* who_c, int session_id, peaq_meter_reading* out, bool with_rows,
                             double* rows, int cap, int* n_read, uint64_t* dropped) {
  const std::string who(who_c);
  if (!b || !n_read) return fail(PEAQ_ERR_ARG, who + ": NULL argument");
  *n_read = 0;
  if (dropped) *dropped = 0;
  if (cap < 0 || (cap > 0 && !out))
    return fail(PEAQ_ERR_ARG, who + ": cap " + std::to_string(cap) + " with out " + (out ? "set" : "NULL"));
  if (with_rows && cap > 0 && !rows) return fail(PEAQ_ERR_ARG, who + ": cap " + std::to_string(cap) + " with rows NULL");
  if (const auto fwd = broker_forward(b, session_id, who_c, [&](peaq_broker* sh, int id) {
        return broker_meter_read(sh, who_c, id, out, with_rows, rows, cap, n_read, dropped);
      }))
    return *fwd;
  BrokerSlot* sl = broker_slot(b, session_id);
  if (!sl) return fail(PEAQ_ERR_ARG, who + ": bad session id " + std::to_string(session_id));
  std::lock_guard<std::mutex> tick(b->tick_mu);
  if (!b->meter.on) return fail(PEAQ_ERR_ARG, who + ": the meter is off (peaq_broker_set_meter)");
  if (with_rows && !b->meter.bands) return fail(PEAQ_ERR_ARG, who + ": the band meter is off (peaq_broker_set_meter_bands)");
  if (b->failed.load()) return broker_failed(b, who_c);
  std::lock_guard<std::mutex> lock(sl->mu);
  if (!sl->open) return fail(PEAQ_ERR_STATE, who + ": session is not open");
  HIP_TRY(hipSetDevice(b->ctx->device));
  const size_t set = with_rows ? MeterBandSizes(b->meter.k_open, b->meter.ring, 0, b->advanced != 0, b->channels).set : 0;
  return sl->meter.read(sl->framer, b->meter, b->m_buf.ring.as<PointSnap>() + (size_t)session_id * b->meter.ring,
                        b->m_buf.readout, b->m_buf.host, b->channels, b->stream, b->cfg, out, cap, n_read, dropped,
                        b->m_buf.band_ring.as<double>() + (size_t)session_id * b->m_buf.band_ring_doubles,
                        with_rows ? rows : nullptr, set);
}

extern "C" int peaq_broker_meter_read(peaq_broker* b, int session_id, peaq_meter_reading* out, int cap, int* n_read,
                                      uint64_t* dropped) {
  return broker_meter_read(b, "peaq_broker_meter_read", session_id, out, false, nullptr, cap, n_read, dropped);
}

extern "C" int peaq_broker_meter_read_bands(peaq_broker* b, int session_id, peaq_meter_reading* out, double* rows, int cap,
                                            int* n_read, uint64_t* dropped) {
  return broker_meter_read(b, "peaq_broker_meter_read_bands", session_id, out, true, rows, cap, n_read, dropped);
}

extern "C" int peaq_broker_start(peaq_broker* b, unsigned period_us) {
  if (!b) return fail(PEAQ_ERR_ARG, "peaq_broker_start: broker is NULL");
  if (broker_is_multi(b)) {                            // one tick thread per device
    for (peaq_broker* sh : b->shards) {
      const int rc = peaq_broker_start(sh, period_us);
      if (rc != PEAQ_OK) {
        (void)peaq_broker_stop(b);
        return rc;
      }
    }
    return PEAQ_OK;
  }
  if (b->running.exchange(true)) return fail(PEAQ_ERR_STATE, "peaq_broker_start: already running");
  b->period_us = period_us ? period_us : 2000;
  b->worker = std::thread([b]() {
    // fixed cadence: whatever arrived during one period shares one launch
    auto next = std::chrono::steady_clock::now();
    while (b->running.load()) {
      int rc;
      {
        std::lock_guard<std::mutex> tick(b->tick_mu);
        rc = broker_tick_checked(b, nullptr);
      }
      b->tick_cv.notify_all();
      if (rc != PEAQ_OK) break;
      next += std::chrono::microseconds(b->period_us);
      const auto now = std::chrono::steady_clock::now();
      if (next < now) next = now;
      std::this_thread::sleep_until(next);
    }
  });
  return PEAQ_OK;
}

extern "C" int peaq_broker_stats(peaq_broker* b, peaq_broker_stats_t* out) {
  if (!b || !out) return fail(PEAQ_ERR_ARG, "peaq_broker_stats: NULL argument");
  if (broker_is_multi(b)) {
    // counts add up over the devices (max_active: the most sessions the node served in one tick period, each
    // device's own maximum); times: the worst device's maximum and 99th percentile, means weighted by their samples
    peaq_broker_stats_t acc{};
    double tick_w = 0.;                                // (both tick means have a sample per launch)
    for (peaq_broker* sh : b->shards) {
      peaq_broker_stats_t s{};
      const int rc = peaq_broker_stats(sh, &s);
      if (rc != PEAQ_OK) return rc;
      acc.ticks += s.ticks;
      acc.launches += s.launches;
      acc.frames += s.frames;
      acc.max_active += s.max_active;
      acc.worker_failed |= s.worker_failed;
      acc.tick_host_us_max = std::max(acc.tick_host_us_max, s.tick_host_us_max);
      acc.tick_host_us_p99 = std::max(acc.tick_host_us_p99, s.tick_host_us_p99);
      acc.tick_device_us_max = std::max(acc.tick_device_us_max, s.tick_device_us_max);
      acc.tick_device_us_p99 = std::max(acc.tick_device_us_p99, s.tick_device_us_p99);
      acc.latency_us_max = std::max(acc.latency_us_max, s.latency_us_max);
      acc.latency_us_p99 = std::max(acc.latency_us_p99, s.latency_us_p99);
      acc.tick_host_us_mean += s.tick_host_us_mean * (double)s.launches;
      acc.tick_device_us_mean += s.tick_device_us_mean * (double)s.launches;
      tick_w += (double)s.launches;
      acc.latency_us_mean += s.latency_us_mean * (double)s.latency_samples;
      acc.latency_samples += s.latency_samples;
    }
    if (tick_w > 0.) {
      acc.tick_host_us_mean /= tick_w;
      acc.tick_device_us_mean /= tick_w;
    }
    if (acc.latency_samples) acc.latency_us_mean /= (double)acc.latency_samples;
    *out = acc;
    return PEAQ_OK;
  }
  std::lock_guard<std::mutex> tick(b->tick_mu);
  out->ticks = b->n_ticks;
  out->launches = b->n_launches;
  out->frames = b->n_frames;
  out->max_active = b->max_active;
  out->worker_failed = b->failed.load() ? 1 : 0;
  if (b->staged_pending && !b->failed.load()) {        // settle the last tick's timing
    HIP_TRY(hipSetDevice(b->ctx->device));
    if (int rc = broker_settle(b)) return rc;
  }
  out->tick_host_us_max = b->h_host.max;
  out->tick_host_us_p99 = b->h_host.quantile(0.99);
  out->tick_host_us_mean = b->h_host.n ? b->h_host.sum / (double)b->h_host.n : 0.;
  out->tick_device_us_mean = b->h_device.n ? b->h_device.sum / (double)b->h_device.n : 0.;
  out->tick_device_us_max = b->h_device.max;
  out->tick_device_us_p99 = b->h_device.quantile(0.99);
  out->latency_us_max = b->h_latency.max;
  out->latency_us_p99 = b->h_latency.quantile(0.99);
  out->latency_us_mean = b->h_latency.n ? b->h_latency.sum / (double)b->h_latency.n : 0.;
  out->latency_samples = b->h_latency.n;
  return PEAQ_OK;
}

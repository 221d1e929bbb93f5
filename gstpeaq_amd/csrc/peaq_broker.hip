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
constexpr unsigned kBrokerMaxFrames = 8;     // FFT frames one session contributes to one tick
constexpr unsigned kBrokerMaxBlocks = 48;    // filter-bank blocks one session contributes to one tick
constexpr size_t kBrokerStageSamples = (size_t)(kBrokerMaxFrames - 1) * kHop + kFrame;
constexpr size_t kBrokerFbStageSamples = (size_t)kBrokerMaxBlocks * kFbFrame;
constexpr size_t kBrokerRowStride = (size_t)kFbRing + kBrokerFbStageSamples;
constexpr size_t kMetaRows = 11;          // rows of h_meta; rows 7 .. 9 are uploaded with the meter or the watch on only,
                                          // row 10 with the watch on only
constexpr unsigned kBrokerAcquirePerTick = 8;   // live alignment: slots whose delay estimate one tick enqueues
// back-pressure: a push returns only once its session has no more than this many samples that are
// READY to be framed (present on both pads) and not yet launched -- four ticks' worth.  Samples one
// pad holds ahead of the other are never counted: like the reference's adapters they may pile up
// without bound while the other pad is silent (gstpeaq.c:626-636).
constexpr uint64_t kBrokerBacklog = (uint64_t)4 * kBrokerMaxFrames * kHop;

struct BrokerSlot {
  std::mutex mu;
  bool open = false;
  bool flush_requested = false, fft_flushed = false, fb_flushed = false;
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
  int alloc(size_t n_sessions, size_t stage_samples, int channels) {
    samples = stage_samples;
    const size_t bytes = n_sessions * stage_samples * channels * sizeof(float);
    for (int p = 0; p < 2; ++p) {
      HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h[p]), bytes, hipHostMallocDefault));
      HIP_TRY(d[p].reserve(bytes));
    }
    return PEAQ_OK;
  }
  ~BrokerStage() {
    for (int p = 0; p < 2; ++p)
      if (h[p]) (void)hipHostFree(h[p]);
  }
};

// what one session contributes to a tick: decided under the slot lock in the tick's serial scan,
// copied into the staging buffers afterwards (by the staging threads, several sessions at a time)
struct BrokerJob {
  int sid = 0;
  unsigned fft_idx = 0, fb_idx = 0;   // staging entries (launch pairs) of the two windows
  StreamWindow fft, fb;               // count 0: none of that kind
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
  uint32_t* h_meta = nullptr;       // pinned: 5 rows of max_sessions (n_ref, n_test, frame0, nframes, slot) + 2 rows (fb n_ref, n_test)
                                    // + 3 rows of the meter (total frames per FFT pair; total frames, total blocks per fb pair)
  FbPairWindow* h_win = nullptr;    // pinned: one per launch pair of the filter-bank launch
  DevBuf d_meta, d_win, records, fb_records, state, fbstate, hp_rows, result;
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
  std::vector<BrokerJob> jobs;      // this tick's staging work
  std::unique_ptr<StagePool> stagers;
  // peaq_broker_create_multi: this broker owns no device; it deals its sessions out to one broker per device
  // (session id = shard + n_shards * the shard's own id) and forwards every call
  std::vector<peaq_broker*> shards;
  std::vector<peaq_ctx*> shard_ctx;
  std::vector<int> shard_open;      // open sessions per shard (guarded by tick_mu)
  // the meter (peaq_broker_set_meter; peaq_meter.hip): one geometry for all slots, because it shapes the launch
  MeterGeometry meter;
  DevBuf m_open, m_ring;            // PointSnap [slot][k_open], [slot][ring]
  DevBuf m_ftrc, m_btrc;            // one tick's trace records [launch index][kBrokerMaxFrames / kBrokerMaxBlocks]
  DevBuf m_readout;                 // ResultRecord [ring]
  std::vector<ResultRecord> m_host;

  // live alignment (peaq_broker_set_align; peaq_watch.hip): one configuration for all slots
  LiveAlignGeometry align;
  float* a_hprobe[2] = {nullptr, nullptr};   // pinned: this tick's probes [kBrokerAcquirePerTick][probe][channels]
  DevBuf a_probe[2], a_rec;         // the same on the device; peaq_delay [kBrokerAcquirePerTick]
  peaq_delay* a_hrec = nullptr;     // pinned: the records of the last tick's estimates
  std::vector<BrokerAcquire> a_pending;      // the estimates the last tick enqueued
  DevBuf w_rows, w_state;           // watch: one tick's rows [launch pair][kBrokerMaxFrames][kWatchRow]; WatchState [slot]

  ModelSetup model() const { return ModelSetup{ctx, cfg, advanced, channels, level_db}; }
};

// a held slot whose probe is there, or whose flush has been asked for: the next tick with room estimates its delay
static inline bool broker_probe_ready(const peaq_broker* b, const BrokerSlot& sl) {
  return sl.flush_requested || std::min(sl.framer.pad[0].total, sl.framer.pad[1].total) >= b->align.probe;
}

static inline bool broker_is_multi(const peaq_broker* b) { return b && !b->shards.empty(); }
// -> the device broker that owns session `sid` of b, and the session's id there
static inline peaq_broker* broker_shard_of(peaq_broker* b, int sid, int* local) {
  const int n = (int)b->shards.size();
  if (sid < 0 || sid >= b->max_sessions) return nullptr;
  *local = sid / n;
  return b->shards[sid % n];
}

// window w of the slot's stream into staging entry `idx`
static void broker_stage_copy(const peaq_broker* b, const BrokerSlot& sl, const BrokerStage& st, unsigned idx,
                              const StreamWindow& w) {
  const size_t off = idx * st.samples * b->channels;
  float* const dst[2] = {st.h[0] + off, st.h[1] + off};
  stage_window(sl.framer, w, dst);
}

// the previous tick's device work is complete: its device time is known now, and with it the latency of the
// sessions it served (wait for the tick + the tick's host part + its device part)
static void broker_settle_timing(peaq_broker* b) {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, b->t_begin, b->t_end) != hipSuccess) ms = 0.f;
  const double dev_us = 1e3 * ms;
  b->h_device.add(dev_us);
  b->h_host.add(b->parked_host_us);
  for (float w : b->parked_wait_us) b->h_latency.add((double)w + b->parked_host_us + dev_us);
  b->parked_wait_us.clear();
}

static int broker_tick_locked(peaq_broker* b, unsigned* n_active_out) {
  peaq_ctx* c = b->ctx;
  if (n_active_out) *n_active_out = 0;
  HIP_TRY(hipSetDevice(c->device));
  if (b->staged_pending) {
    HIP_TRY(hipEventSynchronize(b->staged));
    b->staged_pending = false;
    broker_settle_timing(b);
  }
  // live alignment: the records of the estimates the last tick enqueued are in pinned memory now; their framers are
  // released, and the streams' first units ride in this tick
  for (size_t i = 0; i < b->a_pending.size(); ++i) {
    const BrokerAcquire& q = b->a_pending[i];
    BrokerSlot& sl = *b->slots[q.sid];
    std::lock_guard<std::mutex> lock(sl.mu);
    if (!sl.open || sl.epoch != q.epoch || !sl.acquiring) continue;   // (closed, or closed and opened again, meanwhile)
    peaq_live_delay d{};
    live_align_plan(b->align.probe, q.have[0], q.have[1], b->a_hrec[i].lag, &d);
    static_assert(sizeof d.d == sizeof(peaq_delay), "peaq_live_delay::d mirrors peaq_delay");
    std::memcpy(&d.d, &b->a_hrec[i], sizeof(peaq_delay));
    d.acquired = 1;
    sl.delay = d;
    sl.acquiring = false;
    sl.framer.release(d.skip_ref, d.skip_test);
  }
  b->a_pending.clear();
  const double t_tick = now_us();
  const size_t S = (size_t)b->max_sessions;
  uint32_t* m_nref = b->h_meta;
  uint32_t* m_ntest = b->h_meta + S;
  uint32_t* m_f0 = b->h_meta + 2 * S;
  uint32_t* m_nf = b->h_meta + 3 * S;
  uint32_t* m_slot = b->h_meta + 4 * S;
  uint32_t* m_fb_nref = b->h_meta + 5 * S;
  uint32_t* m_fb_ntest = b->h_meta + 6 * S;
  // the meter's rows (uploaded with the meter on only): the stream's frame count of each FFT pair, its frame and block
  // counts of each filter-bank pair -- UINT_MAX until the session's flush is known
  uint32_t* m_tot_f = b->h_meta + 7 * S;
  uint32_t* m_fb_tot_f = b->h_meta + 8 * S;
  uint32_t* m_fb_tot_b = b->h_meta + 9 * S;
  // the watch's row (uploaded with the watch on only): the whole frames of each FFT pair -- 0 for a flush frame
  uint32_t* m_wf = b->h_meta + 10 * S;
  const bool watched = b->align.window != 0;
  uint32_t acq_n[2][kBrokerAcquirePerTick];          // live alignment: the probe lengths of this tick's estimates
  const bool metered = b->meter.on;
  unsigned fb_closing = 0;                           // sessions whose blocks ended without a flush block (meter: see below)
  unsigned active = 0, max_nf = 0, fb_active = 0, max_nb = 0;
  uint64_t frames = 0;
  b->jobs.clear();
  for (int sid = 0; sid < b->max_sessions; ++sid) {
    BrokerSlot& sl = *b->slots[sid];
    std::lock_guard<std::mutex> lock(sl.mu);
    if (!sl.open) continue;
    if (sl.framer.held) {
      // live alignment: nothing is taken from a held stream.  Once its probe is there (or its flush asked for) and no
      // estimate of it is under way, its probes are staged, at most kBrokerAcquirePerTick slots a tick; the rest wait.
      const bool empty_pad = !sl.framer.pad[0].total || !sl.framer.pad[1].total;
      if (!sl.acquiring && empty_pad && broker_probe_ready(b, sl)) {
        // (a flush with nothing on a pad: the record the aligner documents for an empty signal, no device work)
        peaq_live_delay d{};
        live_align_plan(b->align.probe, sl.framer.pad[0].total, sl.framer.pad[1].total, 0, &d);
        d.acquired = 1;
        sl.delay = d;
        sl.framer.release(0, 0);
      } else if (!sl.acquiring && b->a_pending.size() < kBrokerAcquirePerTick && broker_probe_ready(b, sl)) {
        const size_t i = b->a_pending.size();
        BrokerAcquire q;
        q.sid = sid;
        q.epoch = sl.epoch;
        for (int p = 0; p < 2; ++p) {
          q.have[p] = sl.framer.pad[p].total;
          acq_n[p][i] = static_cast<uint32_t>(std::min<uint64_t>(q.have[p], b->align.probe));
          if (acq_n[p][i])
            std::memcpy(b->a_hprobe[p] + i * (size_t)b->align.probe * b->channels, sl.framer.pad[p].at(0, b->channels),
                        (size_t)acq_n[p][i] * b->channels * sizeof(float));
        }
        b->a_pending.push_back(q);
        sl.acquiring = true;
      }
      if (sl.framer.held) continue;
    }
    BrokerJob job;
    job.sid = sid;
    // ---- at most one window per kind: whole units (do_processing), else, once, the zero-padded unit of
    // do_flush.  The samples are copied further down: only the positions are taken here. ----------------
    const bool flush_fft = sl.flush_requested && !sl.fft_flushed;
    if (metered && sl.flush_requested && !sl.meter.ended) sl.meter.end(sl.framer);   // the stream's end is known from here on
    job.fft = sl.framer.take(kUnitFrame, kBrokerMaxFrames, flush_fft);
    if (flush_fft && (job.fft.flush || !job.fft.count)) sl.fft_flushed = true;   // (no whole frame was left)
    if (job.fft.count) {
      job.fft_idx = active;
      m_nref[active] = static_cast<uint32_t>(job.fft.valid[0]);
      m_ntest[active] = static_cast<uint32_t>(job.fft.valid[1]);
      m_f0[active] = job.fft.first;
      m_nf[active] = job.fft.count;
      m_slot[active] = static_cast<uint32_t>(sid);
      m_tot_f[active] = sl.meter.ended ? sl.meter.total[kUnitFrame] : UINT_MAX;
      m_wf[active] = job.fft.flush ? 0 : job.fft.count;
      frames += job.fft.count;
      max_nf = std::max(max_nf, job.fft.count);
      ++active;
    }
    if (b->advanced) {
      // With the meter on the two paths of a stream stay at a common sample horizon, so that a window's two halves
      // meet in the delivered ring: the blocks go no further than the frame after the last one taken, 1024 (frames + 2)
      // samples.  Whatever blocks are whole while no frame is lie below that, so nothing waits that a tick without the
      // meter would take unless a frame waits too; and 48 blocks a tick outrun 8 frames.  The cap holds through a
      // flush's backlog as well, until the stream's last frame has been taken (above, in this tick at the latest):
      // only the tail of the blocks, and the flush block, run free.
      const bool capped = metered && (!sl.meter.ended || sl.framer.done[kUnitFrame] < sl.meter.total[kUnitFrame]);
      const bool flush_fb = sl.flush_requested && !sl.fb_flushed && !capped;
      unsigned fb_cap = kBrokerMaxBlocks;
      if (capped) {
        const uint64_t reach = 1024ull * ((uint64_t)sl.framer.done[kUnitFrame] + 2) / kFbFrame;
        const uint64_t room = reach > sl.framer.done[kUnitBlock] ? reach - sl.framer.done[kUnitBlock] : 0;
        fb_cap = (unsigned)std::min<uint64_t>(room, kBrokerMaxBlocks);
      }
      if (fb_cap) job.fb = sl.framer.take(kUnitBlock, fb_cap, flush_fb);
      if (flush_fb && (job.fb.flush || !job.fb.count)) {
        sl.fb_flushed = true;
        // the blocks ended without a flush block: the windows that run to the last block are delivered by an entry
        // without units, behind this tick's own in the meter's launch (the back ends never see it).  (A window whose
        // streaming end fell on the last block was stored then already; this stores the same fields again.)
        if (metered && !job.fb.count && sl.meter.total[kUnitFrame]) {
          const unsigned at = (unsigned)S - 1 - fb_closing++;      // (filled from the far end; moved up below)
          b->h_win[at] = FbPairWindow{sl.meter.total[kUnitBlock], 0, 0, static_cast<uint32_t>(sid)};
          m_fb_tot_f[at] = sl.meter.total[kUnitFrame];
          m_fb_tot_b[at] = sl.meter.total[kUnitBlock];
        }
      }
      if (job.fb.count) {
        m_fb_tot_f[fb_active] = sl.meter.ended ? sl.meter.total[kUnitFrame] : UINT_MAX;
        m_fb_tot_b[fb_active] = sl.meter.ended ? sl.meter.total[kUnitBlock] : UINT_MAX;
        job.fb_idx = fb_active;
        m_fb_nref[fb_active] = static_cast<uint32_t>(job.fb.valid[0]);
        m_fb_ntest[fb_active] = static_cast<uint32_t>(job.fb.valid[1]);
        b->h_win[fb_active] =
            FbPairWindow{job.fb.first, job.fb.count, job.fb.prev_blocks, static_cast<uint32_t>(sid)};
        max_nb = std::max(max_nb, job.fb.count);
        ++fb_active;
      }
    }
    if (sl.flush_requested && sl.fft_flushed && (!b->advanced || sl.fb_flushed))
      sl.flush_requested = sl.fft_flushed = sl.fb_flushed = false;
    if (job.fft.count || job.fb.count) {
      b->jobs.push_back(job);
      if (sl.t_ready_us >= 0.) b->parked_wait_us.push_back((float)(t_tick - sl.t_ready_us));
      // more whole units left behind (the per-tick cap)?  They have been waiting since now at the latest.
      sl.t_ready_us = (sl.framer.ready() || sl.flush_requested) ? t_tick : -1.;
    }
  }
  ++b->n_ticks;
  const unsigned n_acq = (unsigned)b->a_pending.size();
  if (!active && !fb_active && !fb_closing && !n_acq) return PEAQ_OK;
  for (unsigned i = 0; i < fb_closing; ++i) {        // the entries without units: behind the tick's own
    const unsigned at = (unsigned)S - 1 - i, to = fb_active + i;
    b->h_win[to] = b->h_win[at];
    m_fb_tot_f[to] = m_fb_tot_f[at];
    m_fb_tot_b[to] = m_fb_tot_b[at];
  }
  // ---- the sessions' new samples into the pinned staging buffers; then drop what both consumers are done
  // with.  (Only ticks consume, and ticks are serialised: the positions recorded above stay valid; a
  // concurrent push may reallocate a FIFO, hence the slot lock around each copy.) ----------------------
  b->stagers->run(b->jobs.size(), [b](size_t i) {
    const BrokerJob& j = b->jobs[i];
    BrokerSlot& sl = *b->slots[j.sid];
    std::lock_guard<std::mutex> lock(sl.mu);
    if (j.fft.count) broker_stage_copy(b, sl, b->fft, j.fft_idx, j.fft);
    if (j.fb.count) broker_stage_copy(b, sl, b->fbs, j.fb_idx, j.fb);
    sl.framer.trim();
  });
  HIP_TRY(hipEventRecord(b->t_begin, b->stream));
  HIP_TRY(hipMemcpyAsync(b->d_meta.p, b->h_meta, (watched ? kMetaRows : metered ? 10 : 7) * S * sizeof(uint32_t), hipMemcpyHostToDevice,
                         b->stream));
  // the meter's launches: the live back ends leave this tick's records at [launch index][unit of the tick], and one
  // small kernel behind each back end walks every session's units through its open windows
  RunOutputs live;
  MeterArgs ma{};
  if (metered) {
    live.live.frames = b->m_ftrc.as<FrameTrace>();
    live.live.frame_stride = kBrokerMaxFrames;
    live.live.blocks = b->m_btrc.as<BlockTrace>();
    live.live.block_stride = kBrokerMaxBlocks;
    live.live.n_uniform = UINT_MAX;
    ma.open = b->m_open.as<PointSnap>();
    ma.ring = b->m_ring.as<PointSnap>();
    ma.window = b->meter.window;
    ma.hop = b->meter.hop;
    ma.k_open = b->meter.k_open;
    ma.ring_depth = b->meter.ring;
    ma.frames = live.live.frames;
    ma.frame_stride = kBrokerMaxFrames;
    ma.blocks = live.live.blocks;
    ma.block_stride = kBrokerMaxBlocks;
  }
  const uint32_t* d_meta = b->d_meta.as<uint32_t>();
  const ModelSetup m = b->model();
  if (active) {
    const size_t stride = b->fft.samples * b->channels;
    for (int p = 0; p < 2; ++p)
      HIP_TRY(hipMemcpyAsync(b->fft.d[p].p, b->fft.h[p], active * stride * sizeof(float), hipMemcpyHostToDevice,
                             b->stream));
    FrontendArgs fa = m.frontend();
    fa.ref = b->fft.d[0].as<float>();
    fa.test = b->fft.d[1].as<float>();
    fa.pair_stride = b->fft.samples;
    fa.n_ref = d_meta;
    fa.n_test = d_meta + S;
    fa.pair_frame0 = d_meta + 2 * S;
    fa.pair_nframes = d_meta + 3 * S;
    fa.frames_per_launch = max_nf;
    fa.records = b->records.as<double>();
    HIP_TRY(launch_frontend(m.fft_bands(), fa, active, b->stream));
    if (watched) {
      WatchArgs wa{};
      wa.ref = fa.ref;
      wa.test = fa.test;
      wa.pair_stride = fa.pair_stride;
      wa.channels = b->channels;
      wa.n_frames = max_nf;
      wa.window = b->align.window;
      wa.rows = b->w_rows.as<double>();
      wa.row_stride = kBrokerMaxFrames;
      wa.state = b->w_state.as<WatchState>();
      wa.s_frames = d_meta + 10 * S;
      wa.s_slot = d_meta + 4 * S;
      HIP_TRY(launch_delay_watch(wa, active, b->stream));
    }
    BackendArgs ba = m.backend(fa);
    ba.frames_per_launch = max_nf;
    ba.state = b->state.as<PairState>();
    ba.pair_slot = d_meta + 4 * S;
    HIP_TRY(launch_backend(ba, active, b->stream, live));
    if (metered) {
      MeterArgs mf = ma;
      mf.rec_stride = max_nf;
      mf.s_unit0 = d_meta + 2 * S;
      mf.s_nunits = d_meta + 3 * S;
      mf.s_slot = d_meta + 4 * S;
      mf.s_total_frames = mf.s_total_units = d_meta + 7 * S;
      HIP_TRY(launch_meter_fft(mf, b->advanced != 0, b->records.as<double>(), b->channels, active, b->stream));
    }
  }
  if (!fb_active && fb_closing)
    HIP_TRY(hipMemcpyAsync(b->d_win.p, b->h_win, fb_closing * sizeof(FbPairWindow), hipMemcpyHostToDevice, b->stream));
  if (fb_active) {
    const size_t stride = b->fbs.samples * b->channels;
    for (int p = 0; p < 2; ++p)
      HIP_TRY(hipMemcpyAsync(b->fbs.d[p].p, b->fbs.h[p], fb_active * stride * sizeof(float), hipMemcpyHostToDevice,
                             b->stream));
    HIP_TRY(hipMemcpyAsync(b->d_win.p, b->h_win, (fb_active + fb_closing) * sizeof(FbPairWindow), hipMemcpyHostToDevice,
                           b->stream));
    FbFrontArgs ff = m.fb_frontend();
    ff.ref = b->fbs.d[0].as<float>();
    ff.test = b->fbs.d[1].as<float>();
    ff.pair_stride = b->fbs.samples;
    ff.n_ref = d_meta + 5 * S;
    ff.n_test = d_meta + 6 * S;
    ff.blocks_per_launch = max_nb;
    ff.fbstate = b->fbstate.as<FbSignalState>();
    ff.hp_scratch = b->hp_rows.as<double>();
    ff.hp_row_stride = kBrokerRowStride;
    ff.records = b->fb_records.as<double>();
    ff.windows = b->d_win.as<FbPairWindow>();
    HIP_TRY(launch_fb_frontend(ff, fb_active, b->stream));
    FbBackendArgs fbk = m.fb_backend(ff);
    fbk.blocks_per_launch = max_nb;
    fbk.state = b->state.as<PairState>();
    HIP_TRY(launch_fb_backend(fbk, fb_active, b->stream, live));
  }
  if (metered && fb_active + fb_closing) {
    MeterArgs mb = ma;
    mb.s_win = b->d_win.as<FbPairWindow>();
    mb.s_total_frames = d_meta + 8 * S;
    mb.s_total_units = d_meta + 9 * S;
    HIP_TRY(launch_meter_fb(mb, b->channels, fb_active + fb_closing, b->stream));
  }
  if (n_acq) {
    // live alignment: one estimate over this tick's probes, its records copied to pinned memory -- enqueued, not waited
    // for: the next tick reads them after its wait for `staged`
    const size_t row = (size_t)b->align.probe * b->channels;
    for (int p = 0; p < 2; ++p)
      HIP_TRY(hipMemcpyAsync(b->a_probe[p].p, b->a_hprobe[p], n_acq * row * sizeof(float), hipMemcpyHostToDevice, b->stream));
    if (int rc = peaq_batch_estimate_delay(c, b->channels, (int)n_acq, b->a_probe[0].as<float>(), b->a_probe[1].as<float>(),
                                           b->align.probe, acq_n[0], acq_n[1], 0, b->align.max_lag,
                                           b->a_rec.as<peaq_delay>(), b->stream))
      return rc;
    HIP_TRY(hipMemcpyAsync(b->a_hrec, b->a_rec.p, n_acq * sizeof(peaq_delay), hipMemcpyDeviceToHost, b->stream));
  }
  HIP_TRY(hipEventRecord(b->t_end, b->stream));
  HIP_TRY(hipEventRecord(b->staged, b->stream));
  b->staged_pending = true;
  b->parked_host_us = now_us() - t_tick;
  ++b->n_launches;
  b->n_frames += frames;
  b->max_active = std::max(b->max_active, std::max(active, fb_active));
  if (n_active_out) *n_active_out = std::max(active, fb_active);
  return PEAQ_OK;
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
    int r = b->fft.alloc(S, kBrokerStageSamples, channels);
    if (r != PEAQ_OK) return r;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&b->h_meta), kMetaRows * S * sizeof(uint32_t), hipHostMallocDefault));
    HIP_TRY(b->d_meta.reserve(kMetaRows * S * sizeof(uint32_t)));
    HIP_TRY(b->records.reserve(S * kBrokerMaxFrames * channels * kRecDoubles * sizeof(double)));
    HIP_TRY(b->state.reserve(S * sizeof(PairState)));
    HIP_TRY(b->result.reserve(sizeof(ResultRecord)));
    HIP_TRY(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&b->staged, hipEventDisableTiming));
    HIP_TRY(hipEventCreate(&b->t_begin));
    HIP_TRY(hipEventCreate(&b->t_end));
    HIP_TRY(launch_state_init(b->state.as<PairState>(), b->advanced, max_sessions, b->stream));
    if (b->advanced) {
      r = b->fbs.alloc(S, kBrokerFbStageSamples, channels);
      if (r != PEAQ_OK) return r;
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
  if (b->h_meta) (void)hipHostFree(b->h_meta);
  if (b->h_win) (void)hipHostFree(b->h_win);
  for (int p = 0; p < 2; ++p)
    if (b->a_hprobe[p]) (void)hipHostFree(b->a_hprobe[p]);
  if (b->a_hrec) (void)hipHostFree(b->a_hrec);
  if (b->staged) (void)hipEventDestroy(b->staged);
  if (b->t_begin) (void)hipEventDestroy(b->t_begin);
  if (b->t_end) (void)hipEventDestroy(b->t_end);
  if (b->stream) (void)hipStreamDestroy(b->stream);
  for (BrokerSlot* s : b->slots) delete s;
  delete b;                         // (the staging and device buffers go with it)
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
      HIP_TRY(launch_points_init(b->m_open.as<PointSnap>() + (size_t)sid * b->meter.k_open, b->meter.k_open, b->stream));
      HIP_TRY(launch_points_init(b->m_ring.as<PointSnap>() + (size_t)sid * b->meter.ring, b->meter.ring, b->stream));
    }
    if (b->align.window)                               // a fresh watch: index 0, nothing complete
      HIP_TRY(hipMemsetAsync(b->w_state.as<WatchState>() + sid, 0, sizeof(WatchState), b->stream));
    sl.meter = MeterStream();
    sl.open = true;
    sl.flush_requested = sl.fft_flushed = sl.fb_flushed = false;
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
  if (broker_is_multi(b)) {
    int local;
    peaq_broker* sh = broker_shard_of(b, session_id, &local);
    if (!sh) return fail(PEAQ_ERR_ARG, "peaq_broker_close: bad session id");
    const int rc = peaq_broker_close(sh, local);
    if (rc == PEAQ_OK) {
      std::lock_guard<std::mutex> place(b->tick_mu);
      --b->shard_open[session_id % (int)b->shards.size()];
    }
    return rc;
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
  if (broker_is_multi(b)) {
    int local;
    peaq_broker* sh = broker_shard_of(b, session_id, &local);
    return sh ? peaq_broker_push(sh, local, pad, data, n) : fail(PEAQ_ERR_ARG, "peaq_broker_push: bad session id");
  }
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
  if (broker_is_multi(b)) {
    int local;
    peaq_broker* sh = broker_shard_of(b, session_id, &local);
    return sh ? peaq_broker_flush(sh, local) : fail(PEAQ_ERR_ARG, "peaq_broker_flush: bad session id");
  }
  BrokerSlot* sl = broker_slot(b, session_id);
  if (!sl) return fail(PEAQ_ERR_ARG, "peaq_broker_flush: bad broker or session id");
  if (b->failed.load()) return broker_failed(b, "peaq_broker_flush");
  std::lock_guard<std::mutex> lock(sl->mu);
  if (!sl->open) return fail(PEAQ_ERR_STATE, "peaq_broker_flush: session is not open");
  sl->flush_requested = true;
  sl->fft_flushed = sl->fb_flushed = false;
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
  return sl->framer.ready() || sl->flush_requested;
}

extern "C" int peaq_broker_results(peaq_broker* b, int session_id, peaq_result* out) {
  if (broker_is_multi(b)) {
    int local;
    peaq_broker* sh = broker_shard_of(b, session_id, &local);
    return sh ? peaq_broker_results(sh, local, out) : fail(PEAQ_ERR_ARG, "peaq_broker_results: bad session id");
  }
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
  if (b->running.load())
    return fail(PEAQ_ERR_ARG, "peaq_broker_set_meter: the tick thread runs; set the meter before peaq_broker_start");
  for (int sid = 0; sid < b->max_sessions; ++sid) {
    std::lock_guard<std::mutex> lock(b->slots[sid]->mu);
    if (b->slots[sid]->open)
      return fail(PEAQ_ERR_ARG, "peaq_broker_set_meter: session " + std::to_string(sid) +
                                    " is open; set the meter before the first peaq_broker_open");
  }
  b->meter.on = false;
  if (off) return PEAQ_OK;
  MeterGeometry g;
  g.set(*cfg);
  const size_t S = (size_t)b->max_sessions;
  HIP_TRY(hipSetDevice(b->ctx->device));
  HIP_TRY(hipStreamSynchronize(b->stream));            // (the buffers may be replaced)
  HIP_TRY(b->m_open.reserve(S * g.k_open * sizeof(PointSnap)));
  HIP_TRY(b->m_ring.reserve(S * g.ring * sizeof(PointSnap)));
  HIP_TRY(b->m_readout.reserve((size_t)g.ring * sizeof(ResultRecord)));
  HIP_TRY(b->m_ftrc.reserve(S * kBrokerMaxFrames * sizeof(FrameTrace)));
  if (b->advanced) HIP_TRY(b->m_btrc.reserve(S * kBrokerMaxBlocks * sizeof(BlockTrace)));
  try {
    b->m_host.resize(g.ring);
  } catch (const std::bad_alloc&) {
    return fail(PEAQ_ERR_NOMEM, "out of host memory");
  }
  b->meter = g;
  b->meter.on = true;
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
  if (b->running.load())
    return fail(PEAQ_ERR_ARG, who + ": the tick thread runs; set the alignment before peaq_broker_start");
  for (int sid = 0; sid < b->max_sessions; ++sid) {
    std::lock_guard<std::mutex> lock(b->slots[sid]->mu);
    if (b->slots[sid]->open)
      return fail(PEAQ_ERR_ARG, who + ": session " + std::to_string(sid) +
                                    " is open; set the alignment before the first peaq_broker_open");
  }
  b->align = LiveAlignGeometry();
  if (off) return PEAQ_OK;
  const size_t S = (size_t)b->max_sessions;
  HIP_TRY(hipSetDevice(b->ctx->device));
  HIP_TRY(hipStreamSynchronize(b->stream));            // (the buffers may be replaced)
  if (cfg->max_lag) {
    const size_t bytes = (size_t)kBrokerAcquirePerTick * probe * b->channels * sizeof(float);
    for (int p = 0; p < 2; ++p) {
      if (b->a_hprobe[p]) (void)hipHostFree(b->a_hprobe[p]);
      b->a_hprobe[p] = nullptr;
      HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&b->a_hprobe[p]), bytes, hipHostMallocDefault));
      HIP_TRY(b->a_probe[p].reserve(bytes));
    }
    HIP_TRY(b->a_rec.reserve(kBrokerAcquirePerTick * sizeof(peaq_delay)));
    if (!b->a_hrec)
      HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&b->a_hrec), kBrokerAcquirePerTick * sizeof(peaq_delay),
                            hipHostMallocDefault));
  }
  if (cfg->watch_frames) {
    HIP_TRY(b->w_rows.reserve(S * kBrokerMaxFrames * kWatchRow * sizeof(double)));
    HIP_TRY(b->w_state.reserve(S * sizeof(WatchState)));
  }
  b->align.max_lag = cfg->max_lag;
  b->align.probe = probe;
  b->align.window = cfg->watch_frames;
  return PEAQ_OK;
}

// The slot's delay as of the last tick enqueued.  A slot that still holds with its flush asked for is driven to its
// acquisition, as peaq_broker_results drives a session to its end.
extern "C" int peaq_broker_align_read(peaq_broker* b, int session_id, peaq_live_delay* out) {
  if (!b || !out) return fail(PEAQ_ERR_ARG, "peaq_broker_align_read: NULL argument");
  if (broker_is_multi(b)) {
    int local;
    peaq_broker* sh = broker_shard_of(b, session_id, &local);
    return sh ? peaq_broker_align_read(sh, local, out) : fail(PEAQ_ERR_ARG, "peaq_broker_align_read: bad session id");
  }
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
      if (!(sl->framer.held && sl->flush_requested)) break;
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
  if (broker_is_multi(b)) {
    int local;
    peaq_broker* sh = broker_shard_of(b, session_id, &local);
    return sh ? peaq_broker_watch_read(sh, local, out) : fail(PEAQ_ERR_ARG, "peaq_broker_watch_read: bad session id");
  }
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
  HIP_TRY(hipMemcpyAsync(&st, b->w_state.as<WatchState>() + session_id, sizeof st, hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  delay_watch_record(st, out);
  return PEAQ_OK;
}

// What was delivered up to the last tick that has been enqueued (the call waits for it); it does not tick.
extern "C" int peaq_broker_meter_read(peaq_broker* b, int session_id, peaq_meter_reading* out, int cap, int* n_read,
                                      uint64_t* dropped) {
  if (!b || !n_read) return fail(PEAQ_ERR_ARG, "peaq_broker_meter_read: NULL argument");
  *n_read = 0;
  if (dropped) *dropped = 0;
  if (cap < 0 || (cap > 0 && !out))
    return fail(PEAQ_ERR_ARG, "peaq_broker_meter_read: cap " + std::to_string(cap) + " with out " + (out ? "set" : "NULL"));
  if (broker_is_multi(b)) {
    int local;
    peaq_broker* sh = broker_shard_of(b, session_id, &local);
    return sh ? peaq_broker_meter_read(sh, local, out, cap, n_read, dropped)
              : fail(PEAQ_ERR_ARG, "peaq_broker_meter_read: bad session id");
  }
  BrokerSlot* sl = broker_slot(b, session_id);
  if (!sl) return fail(PEAQ_ERR_ARG, "peaq_broker_meter_read: bad session id " + std::to_string(session_id));
  std::lock_guard<std::mutex> tick(b->tick_mu);
  if (!b->meter.on) return fail(PEAQ_ERR_ARG, "peaq_broker_meter_read: the meter is off (peaq_broker_set_meter)");
  if (b->failed.load()) return broker_failed(b, "peaq_broker_meter_read");
  std::lock_guard<std::mutex> lock(sl->mu);
  if (!sl->open) return fail(PEAQ_ERR_STATE, "peaq_broker_meter_read: session is not open");
  HIP_TRY(hipSetDevice(b->ctx->device));
  return sl->meter.read(sl->framer, b->meter, b->m_ring.as<PointSnap>() + (size_t)session_id * b->meter.ring, b->m_readout,
                        b->m_host, b->channels, b->stream, b->cfg, out, cap, n_read, dropped);
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
    double host_w = 0., dev_w = 0.;
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
      host_w += (double)s.launches;
      dev_w += (double)s.launches;
      acc.latency_us_mean += s.latency_us_mean * (double)s.latency_samples;
      acc.latency_samples += s.latency_samples;
    }
    if (host_w > 0.) acc.tick_host_us_mean /= host_w;
    if (dev_w > 0.) acc.tick_device_us_mean /= dev_w;
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
    HIP_TRY(hipEventSynchronize(b->staged));
    b->staged_pending = false;
    broker_settle_timing(b);
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

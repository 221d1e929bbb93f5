// peaq_replay.hip -- scores of time spans inside each pair of a batch run: the windows of the basic version
// (peaq_batch_run_windows) and the spans of the advanced version (peaq_batch_run_adv_spans; DESIGN.md 28;
// both in include/peaq_amd.h).
//
// A span's reading is the read-out of the version's accumulators (eleven in the basic, five in the advanced version) that
// were reset just before the span's first unit and then given what the pair's own accumulators were given in the span's
// units: the same set_tentative, the same values, weights and gates, in the same order.  Everything below the
// accumulators is the pair's own, in context.  The units are the FFT back end's frames (2048 samples every 1024) and, in
// the advanced version, the filter-bank back end's blocks (192 samples) as well, on a stream of their own.  The run's
// back ends are the trace instantiations, which leave every frame's and every block's MOV-layer values and gate flags in
// scratch of the context; the bandwidths, the EHS, the energy bits and the two energies are in the FFT front end's
// records of the same launch.  One replay body, a feed per kernel:
//
//   window_replay_kernel     behind every FFT back-end launch of the basic version: the launch's frames into all eleven
//   span_replay_fft_kernel   ... of the advanced version: the launch's frames into SegmentalNMR and EHS
//   span_replay_fb_kernel    behind every filter-bank back-end launch: the launch's blocks into RmsModDiff,
//                            RmsNoiseLoudAsym and AvgLinDist
//
//   One wave serves 64 / (2 L) spans of one pair, L the feed's lanes per channel (16: 2 spans; 4: 8 spans): lane l owns
//   accumulator slot l % L of channel (l / L) & 1 of span slot l / (2 L); the feed says how many of the L it uses.  The
//   twelve fields and the status stay in registers for the whole walk: loaded from the span's snapshot (PointSnap,
//   [pair][span]) at entry if the span meets the launch's units, stored at exit; a wave none of whose spans meets the
//   launch returns before it loads anything.  The wave walks from the smallest first to the largest last unit of its
//   spans, a lane acting on the units of its own span.  A unit's records sit at wave-uniform addresses, to which a lane
//   adds the fixed index of the value it takes; none depends on a loaded or computed value: the loads of unit u + 1 are
//   issued before the adds of unit u, and the only serial chain is the accumulator's own FP64 add.  No atomics, no LDS,
//   no cross-lane traffic; every lane stores what it owns, lane (accumulator 0, channel 0) of a slot the energies and
//   `frames` in the FFT kernels, `fb_blocks` in the filter-bank kernel.  The two kernels of the advanced version run
//   beside each other on two streams and write disjoint words of the same snapshots, as the two points instantiations
//   of the back ends do.
//
// The add rounds as LaneAcc::add does in the shipped kernels, whose disassembly (val, w the arguments of add) has
//   backend_kernel<109, false> (peaq_backend.hip)
//     average (AVG, AVG_LOG, ADB)   num = fma(val, w, num);            den = w + den
//     RMS                           num = fma(val, val * (w * w), num); den = fma(w, w, den)
//     AVG_WINDOW                    ws = (((sq + p0) + p1) + p2) / 4; ws = ws * ws; num = fma(ws, ws, num); den = den + 1
//     FILTERED_MAX                  filt = fma(0.1, val, 0.9 * filt)
//   fb_backend_trace_kernel, fb_backend_points_kernel (the same three sequences in both)
//     RMS        w2 = w * w; t = val * w2; num = fma(val, t, num); den = fma(w, w, den)
//     RMS_ASYM   num = fma(val, val, num); num2 = fma(w, w, num2); den = den + 1
//     AVG        num = fma(w, val, num); den = w + den                       (AvgLinDist: w = 1)
//   backend_trace_kernel<55, true>, backend_points_kernel<55, true> (w is the literal 1 of every route)
//     AVG        num = val + num; den = den + 1          (= fma(val, 1, num), 1 + den: the same bits)
//     EHS's value is the plain product 1000 * ehs
// -- restated here once, with contraction off and the fused operations spelt out, so that a span {0, L} is bit for bit
// the trajectory's point and the end result.  (The two RMS lines are the same operations in the same order, and a fused
// multiply-add does not tell its factors apart.)
#include <hip/hip_runtime.h>

#include "peaq_device.h"
#include "peaq_kernels.h"

namespace peaq {

namespace {

enum { WB_BW_REF, WB_BW_TEST, WB_NMR, WB_WINMOD, WB_ADB, WB_EHS, WB_AVGMOD1, WB_AVGMOD2, WB_NOISELOUD, WB_MFPD,
       WB_RELDIST };                                   // gstpeaq.c:95-108, the order of MB_* in peaq_backend.hip
enum { SA_RMSMOD, SA_NLASYM, SA_SEGNMR, SA_EHS, SA_LINDIST };   // gstpeaq.c:110-116, the order of MA_* in peaq_backend.hip
enum { F_NUM, F_DEN, F_NUM2, F_P0, F_P1, F_P2, F_MX, F_FILT, F_SNUM, F_SDEN, F_SNUM2, F_SMX };
static_assert(kAccFields == 12 && kMaxAcc == 11, "the fields and accumulators of LaneAcc");
constexpr int kTrcPDetect = 12, kTrcSteps = 13;
static_assert(sizeof(FrameTrace) == 16 * sizeof(double) && offsetof(FrameTrace, ch) == 0 &&
                  offsetof(FrameTrace, p_detect) == kTrcPDetect * 8 && offsetof(FrameTrace, steps) == kTrcSteps * 8 &&
                  offsetof(FrameTrace, flags) == 112 && sizeof(BlockTrace) == 12 * sizeof(double) &&
                  offsetof(BlockTrace, ch) == 0 && offsetof(BlockTrace, flags) == 80,
              "the trace records as the replay indexes them");

// Where a lane's two values sit, fixed for the whole walk: `t` an index into the doubles of the unit's trace record, `r`
// into the frame's front-end record(s) (FFT feeds) or the trace record again (filter-bank feed).
struct LaneSrc {
  int t, r;
};

// One unit's records as loaded: the lane's own values and what is the same for the whole wave.
struct Raw {
  double v, w;                  // at LaneSrc's t and r
  double wt, bw_ref;            // basic feed: the lane's channel's weight (trace record) and reference bandwidth
  double p_detect;              // basic feed
  double sig, noise;            // FFT feeds: the frame's energies over the channels
  uint32_t flags;               // kTrace* of the unit's trace record
  int fl;                       // FFT feeds: the front end's flag words of both signals, all channels
};

// what a lane's accumulator is given in one unit
struct Given {
  double v, w;
  bool hit, above;
  double sig, noise;            // (the head lane adds them)
};

// what is the same for the whole wave in a frame's front-end record(s)
__device__ __forceinline__ void frame_scalars(const double* __restrict__ rec, int channels, Raw& x) {
#pragma clang fp contract(off)
  x.fl = (int)rec[kRecFlagsRef] | (int)rec[kRecFlagsTest];
  x.sig = rec[kRecSigE];
  x.noise = rec[kRecNoiseE];
  if (channels == 2) {
    x.fl |= (int)rec[kRecDoubles + kRecFlagsRef] | (int)rec[kRecDoubles + kRecFlagsTest];
    x.sig = x.sig + rec[kRecDoubles + kRecSigE];
    x.noise = x.noise + rec[kRecDoubles + kRecNoiseE];
  } else {
    x.sig = x.sig + 0.;
    x.noise = x.noise + 0.;
  }
}

// ---- the feeds: what differs between the three kernels -------------------------------------------------------------
// kLanes / kUsed: accumulator lanes per channel, and how many of them own an accumulator; kFft: the units are FFT frames
// (window_frames, FrameTrace records, the front end's records beside them; the head lane carries the energies and writes
// `frames`) or filter-bank blocks (span_blocks, BlockTrace records, nothing beside them; the head lane writes
// `fb_blocks`); kModes: the add modes that occur; acc / mode / source of accumulator lane a; load: a unit's records ->
// Raw; feed: ... -> what the lane's accumulator is given.  (In feed the lane's values are in their registers, in one
// place for all lanes: the loads are not moved behind a lane's branch of the pick.)

// basic version, 109-band FFT back end (peaq_backend_fft.inc:362-502): all eleven accumulators
struct BasicFftFeed {
  static constexpr int kLanes = 16, kUsed = 11;
  static constexpr bool kFft = true;
  static constexpr unsigned kModes = 1u << kAvg | 1u << kAvgLog | 1u << kAdb | 1u << kRms | 1u << kAvgWindow | 1u << kFilteredMax;
  static __device__ __forceinline__ int acc(int a) { return a; }
  // gstpeaq.c:528-557 (acc_mode of peaq_backend.hip, basic version)
  static __device__ __forceinline__ int mode(int a) {
    return a == WB_NMR ? kAvgLog : a == WB_WINMOD ? kAvgWindow : a == WB_ADB ? kAdb : a == WB_NOISELOUD ? kRms
           : a == WB_MFPD ? kFilteredMax : kAvg;
  }
  // t: ch[2][6], p_detect, steps of the FrameTrace; r: the lane's channel of the front end's record
  static __device__ __forceinline__ LaneSrc source(int a, int ch) {
    LaneSrc s{6 * ch, kRecBwRef};
    switch (a) {
      case WB_BW_TEST: s.r = kRecBwTest; break;
      case WB_NMR: s.t += 4; break;
      case WB_ADB: s.t = kTrcSteps; break;
      case WB_EHS: s.r = kRecEhs; break;
      case WB_AVGMOD2: s.t += 1; break;
      case WB_NOISELOUD: s.t += 3; break;
      case WB_MFPD: s.t = kTrcPDetect; break;
      case WB_RELDIST: s.t += 5; break;
      default: break;                                  // BW_REF (r), WINMOD and AVGMOD1 (t) take the first
    }
    return s;
  }
  static __device__ __forceinline__ Raw load(const void* __restrict__ trace_rec, const double* __restrict__ rec,
                                             int channels, int ch, const LaneSrc src) {
#pragma clang fp contract(off)
    const double* __restrict__ t = reinterpret_cast<const double*>(trace_rec);
    const double* __restrict__ r = rec + (size_t)ch * kRecDoubles;
    Raw x{};
    x.v = t[src.t];
    x.wt = t[6 * ch + 2];
    x.w = r[src.r];
    x.bw_ref = r[kRecBwRef];
    x.p_detect = t[kTrcPDetect];
    x.flags = reinterpret_cast<const FrameTrace*>(trace_rec)->flags;
    frame_scalars(rec, channels, x);
    return x;
  }
  static __device__ __forceinline__ Given feed(Raw x, int a, int ch) {
#pragma clang fp contract(off)
    asm volatile("" : "+v"(x.v), "+v"(x.wt), "+v"(x.w), "+v"(x.bw_ref));
    const bool mod_open = x.flags & kTraceModOpen, loud_open = x.flags & kTraceLoudOpen;
    Given g;
    g.above = x.flags & kTraceAbove;
    g.sig = x.sig;
    g.noise = x.noise;
    g.w = a == WB_AVGMOD1 || a == WB_AVGMOD2 ? x.wt : 1.;
    g.v = a == WB_RELDIST ? (x.v > 1.41253754462275 ? 1. : 0.) : a == WB_EHS ? 1000. * x.w
          : a == WB_BW_REF || a == WB_BW_TEST ? x.w : x.v;
    g.hit = a == WB_BW_REF || a == WB_BW_TEST                       ? x.bw_ref > 346.
            : a == WB_WINMOD || a == WB_AVGMOD1 || a == WB_AVGMOD2 ? mod_open
            : a == WB_NOISELOUD                                     ? loud_open
            : a == WB_ADB                                           ? ch == 0 && x.p_detect > 0.5
            : a == WB_MFPD                                          ? ch == 0
            : a == WB_EHS                                           ? (x.fl & 2) != 0
                                                                    : true;
    return g;
  }
};

// advanced version, 55-band FFT back end (peaq_backend_fft.inc:502-534): SegmentalNMR, EHS, two idle lanes
struct AdvFftFeed {
  static constexpr int kLanes = 4, kUsed = 2;
  static constexpr bool kFft = true;
  static constexpr unsigned kModes = 1u << kAvg;
  static __device__ __forceinline__ int acc(int a) { return a == 0 ? SA_SEGNMR : SA_EHS; }
  static __device__ __forceinline__ int mode(int) { return kAvg; }   // gstpeaq.c:547-557
  // t: ch[c][0] of the FrameTrace, the segmental NMR; r: channel c's EHS in the frame's front-end records
  static __device__ __forceinline__ LaneSrc source(int, int ch) { return LaneSrc{6 * ch, ch * kRecDoubles + kRecEhs}; }
  static __device__ __forceinline__ Raw load(const void* __restrict__ trace_rec, const double* __restrict__ rec,
                                             int channels, int, const LaneSrc src) {
#pragma clang fp contract(off)
    Raw x{};
    x.v = reinterpret_cast<const double*>(trace_rec)[src.t];
    x.w = rec[src.r];
    x.flags = reinterpret_cast<const FrameTrace*>(trace_rec)->flags;
    frame_scalars(rec, channels, x);
    return x;
  }
  static __device__ __forceinline__ Given feed(Raw x, int a, int) {
#pragma clang fp contract(off)
    asm volatile("" : "+v"(x.v), "+v"(x.w));
    Given g;
    g.above = x.flags & kTraceAbove;
    g.sig = x.sig;
    g.noise = x.noise;
    g.v = a == 1 ? 1000. * x.w : x.v;
    g.w = 1.;
    g.hit = a == 1 ? (x.fl & 2) != 0 : true;
    return g;
  }
};

// advanced version, filter-bank back end (peaq_backend_fb.inc:116-263): RmsModDiff, RmsNoiseLoudAsym, AvgLinDist, one
// idle lane
struct AdvFbFeed {
  static constexpr int kLanes = 4, kUsed = 3;
  static constexpr bool kFft = false;
  static constexpr unsigned kModes = 1u << kRms | 1u << kRmsAsym | 1u << kAvg;
  static __device__ __forceinline__ int acc(int a) { return a == 0 ? SA_RMSMOD : a == 1 ? SA_NLASYM : SA_LINDIST; }
  static __device__ __forceinline__ int mode(int a) { return a == 0 ? kRms : a == 1 ? kRmsAsym : kAvg; }   // gstpeaq.c:547-557
  // both index the BlockTrace's ch[c][0 .. 4]: RmsModDiff, its weight, noise loudness, missing components, linear
  // distortion
  static __device__ __forceinline__ LaneSrc source(int a, int ch) {
    return LaneSrc{5 * ch + (a == 0 ? 0 : a == 1 ? 2 : 4), 5 * ch + (a == 0 ? 1 : 3)};
  }
  static __device__ __forceinline__ Raw load(const void* __restrict__ trace_rec, const double* __restrict__, int, int,
                                             const LaneSrc src) {
    const double* __restrict__ t = reinterpret_cast<const double*>(trace_rec);
    Raw x{};
    x.v = t[src.t];
    x.w = t[src.r];
    x.flags = reinterpret_cast<const BlockTrace*>(trace_rec)->flags;
    return x;
  }
  static __device__ __forceinline__ Given feed(Raw x, int a, int) {
    asm volatile("" : "+v"(x.v), "+v"(x.w));
    Given g;
    g.above = x.flags & kTraceAbove;
    g.sig = x.sig;
    g.noise = x.noise;
    g.v = x.v;
    g.w = a == 2 ? 1. : x.w;
    g.hit = a == 0 ? (x.flags & kTraceModOpen) != 0 : (x.flags & kTraceLoudOpen) != 0;
    return g;
  }
};

// ---- the body ------------------------------------------------------------------------------------------------------
// The replay of units [unit0, unit0 + units_per_launch) of every pair into the spans that meet them.  `records`: the
// FFT front end's records of the launch (FFT feeds only).
template <class Feed>
__device__ __forceinline__ void span_replay(const SpanArgs& spn, const double* __restrict__ records, unsigned unit0,
                                            unsigned units_per_launch, int channels) {
#pragma clang fp contract(off)
  constexpr int L = Feed::kLanes, kSlots = 64 / (2 * L);
  constexpr bool FFT = Feed::kFft;
  const int lane = threadIdx.x & 63;
  const int a = lane % L, ch = (lane / L) & 1, slot = lane / (2 * L);
  const unsigned pair = blockIdx.x;
  const int s0 = kSlots * (int)blockIdx.y;           // the wave's spans: s0 .. s0 + kSlots - 1
  const uint32_t n_ref = spn.n_ref ? spn.n_ref[pair] : spn.n_uniform;
  const uint32_t n_test = spn.n_test ? spn.n_test[pair] : spn.n_uniform;
  const uint32_t l_end = unit0 + units_per_launch;
  // units [first, end) of a span: FFT frames or filter-bank blocks
  auto span_units = [&](WindowSpan s, uint32_t& first, uint32_t& end) {
    if (FFT)
      window_frames(n_ref, n_test, s.start, s.length, first, end);
    else
      span_blocks(n_ref, n_test, s.start, s.length, first, end);
  };
  // the wave's units of this launch, wave-uniform: from the smallest lo to the largest hi of the spans that meet it,
  // [lo, hi) = [first, end) within [unit0, l_end)
  uint32_t u_begin = UINT_MAX, u_end = 0;
  for (int s = 0; s < kSlots; ++s) {
    if (s0 + s >= spn.n_spans) break;
    uint32_t first, end;
    span_units(spn.spans[s0 + s], first, end);
    const uint32_t lo = first > unit0 ? first : unit0, hi = end < l_end ? end : l_end;
    if (lo < hi) {
      u_begin = lo < u_begin ? lo : u_begin;
      u_end = hi > u_end ? hi : u_end;
    }
  }
  if (u_begin >= u_end) return;
  // this lane's span (a slot past n_spans owns nothing)
  const bool have = s0 + slot < spn.n_spans;
  uint32_t my_first = 0, my_lo = 0, my_hi = 0;
  if (have) {
    uint32_t end;
    span_units(spn.spans[s0 + slot], my_first, end);
    my_lo = my_first > unit0 ? my_first : unit0;
    my_hi = end < l_end ? end : l_end;
    if (my_hi < my_lo) my_hi = my_lo;
  }
  const bool used = a < Feed::kUsed;
  const bool own = used && ch < channels && my_lo < my_hi;
  const bool head_lane = own && a == 0 && ch == 0;   // the slot's counts and energies
  const int lane_a = used ? a : 0, lane_ch = ch < channels ? ch : 0;
  const int acc = Feed::acc(lane_a), mode = Feed::mode(lane_a);
  auto occurs = [](int m) { return (Feed::kModes >> m & 1u) != 0; };   // (compile time: what a feed lacks folds away)

  PointSnap* __restrict__ sp = spn.snap + (size_t)pair * spn.n_spans + (have ? s0 + slot : s0);   // (touched by `own` lanes only)
  double f[kAccFields];
  int status = kInit;
  double sig_e = 0., noise_e = 0.;
  if (own) {
#pragma unroll
    for (int k = 0; k < kAccFields; ++k) f[k] = sp->acc[ch][acc][k];
    status = sp->status[acc];
  } else {
#pragma unroll
    for (int k = 0; k < kAccFields; ++k) f[k] = 0.;
  }
  if (FFT && head_lane) {
    sig_e = sp->sig_energy;
    noise_e = sp->noise_energy;
  }

  const LaneSrc src = Feed::source(lane_a, lane_ch);
  const char* __restrict__ trace =
      FFT ? reinterpret_cast<const char*>(spn.frames + (size_t)pair * spn.frame_stride)
          : reinterpret_cast<const char*>(spn.blocks + (size_t)pair * spn.block_stride);
  constexpr size_t kTraceBytes = FFT ? sizeof(FrameTrace) : sizeof(BlockTrace);
  const double* __restrict__ recs = FFT ? records + (size_t)pair * units_per_launch * channels * kRecDoubles : nullptr;
  auto load_of = [&](uint32_t unit) {
    return Feed::load(trace + (size_t)unit * kTraceBytes,
                      FFT ? recs + (size_t)(unit - unit0) * channels * kRecDoubles : nullptr, channels, lane_ch, src);
  };
  Given cur = Feed::feed(load_of(u_begin), lane_a, lane_ch);
  for (uint32_t unit = u_begin; unit < u_end; ++unit) {
    // (the next unit's loads before this unit's adds; the last unit reads itself again)
    const Raw nxt = load_of(unit + 1 < u_end ? unit + 1 : unit);
    if (own && unit >= my_lo && unit < my_hi) {
      // movaccum.c:317-362
      if (!cur.above) {
        if (status == kNormal) {
          f[F_SNUM] = f[F_NUM];
          f[F_SDEN] = f[F_DEN];
          f[F_SNUM2] = f[F_NUM2];
          f[F_SMX] = f[F_MX];
          status = kTentative;
        }
      } else {
        status = kNormal;
      }
      if (FFT && head_lane) {
        sig_e = sig_e + cur.sig;
        noise_e = noise_e + cur.noise;
      }
      // movaccum.c:368-425
      if (cur.hit && status != kInit) {
        const double v = cur.v, w = cur.w;
        if (occurs(kAvgWindow) && mode == kAvgWindow) {
          const double sq = sqrt(v);
          const double p0 = f[F_P0], p1 = f[F_P1], p2 = f[F_P2];
          if (!isnan(p0)) {
            double ws = ((sq + p0) + p1) + p2;
            ws = ws * 0.25;
            ws = ws * ws;
            f[F_NUM] = __builtin_fma(ws, ws, f[F_NUM]);
            f[F_DEN] = f[F_DEN] + 1.;
          }
          f[F_P0] = p1;
          f[F_P1] = p2;
          f[F_P2] = sq;
        } else if (occurs(kFilteredMax) && mode == kFilteredMax) {
          const double filt = __builtin_fma(0.1, v, 0.9 * f[F_FILT]);
          f[F_FILT] = filt;
          if (filt > f[F_MX]) f[F_MX] = filt;
        } else if (occurs(kRms) && mode == kRms) {
          const double w2 = w * w;
          const double t = v * w2;
          f[F_NUM] = __builtin_fma(v, t, f[F_NUM]);
          f[F_DEN] = __builtin_fma(w, w, f[F_DEN]);
        } else if (occurs(kRmsAsym) && mode == kRmsAsym) {
          f[F_NUM] = __builtin_fma(v, v, f[F_NUM]);
          f[F_NUM2] = __builtin_fma(w, w, f[F_NUM2]);
          f[F_DEN] = f[F_DEN] + 1.;
        } else {
          f[F_NUM] = __builtin_fma(v, w, f[F_NUM]);
          f[F_DEN] = w + f[F_DEN];
        }
      }
    }
    cur = Feed::feed(nxt, lane_a, lane_ch);
  }
  if (own) {
#pragma unroll
    for (int k = 0; k < kAccFields; ++k) sp->acc[ch][acc][k] = f[k];
    if (ch == 0) sp->status[acc] = status;
  }
  if (head_lane) {
    if (FFT) {
      sp->frames = my_hi - my_first;
      sp->sig_energy = sig_e;
      sp->noise_energy = noise_e;
    } else {
      sp->fb_blocks = my_hi - my_first;
    }
  }
}

}  // namespace

__global__ __launch_bounds__(64) void window_replay_kernel(SpanArgs spn, const double* __restrict__ records,
                                                           unsigned frame0, unsigned frames_per_launch, int channels) {
  span_replay<BasicFftFeed>(spn, records, frame0, frames_per_launch, channels);
}

__global__ __launch_bounds__(64) void span_replay_fft_kernel(SpanArgs spn, const double* __restrict__ records,
                                                             unsigned frame0, unsigned frames_per_launch, int channels) {
  span_replay<AdvFftFeed>(spn, records, frame0, frames_per_launch, channels);
}

__global__ __launch_bounds__(64) void span_replay_fb_kernel(SpanArgs spn, unsigned block0, unsigned blocks_per_launch,
                                                            int channels) {
  span_replay<AdvFbFeed>(spn, nullptr, block0, blocks_per_launch, channels);
}

// what both launches hold: `advanced` says whether the run has block records, `slots` the kernel's spans per wave
static bool span_args_ok(const SpanArgs& spn, bool advanced, int channels, int slots) {
  return spn.snap && spn.spans && spn.frames && (spn.blocks != nullptr) == advanced && spn.n_spans >= 1 &&
         spn.n_spans <= slots * 65535 && (channels == 1 || channels == 2);
}

hipError_t launch_span_replay_fft(const SpanArgs& spn, bool advanced, const double* records, unsigned frame0,
                                  unsigned frames_per_launch, int channels, unsigned n_pairs, hipStream_t stream) {
  if (n_pairs == 0 || frames_per_launch == 0) return hipSuccess;
  const int slots = advanced ? 8 : 2;                // spans per wave: 64 / (2 kLanes) of the feed
  if (!span_args_ok(spn, advanced, channels, slots) || !records) return hipErrorInvalidValue;
  const auto kernel = advanced ? span_replay_fft_kernel : window_replay_kernel;
  hipLaunchKernelGGL(kernel, dim3(n_pairs, (unsigned)(spn.n_spans + slots - 1) / slots), dim3(64), 0, stream, spn, records,
                     frame0, frames_per_launch, channels);
  return hipGetLastError();
}

hipError_t launch_span_replay_fb(const SpanArgs& spn, unsigned block0, unsigned blocks_per_launch, int channels,
                                 unsigned n_pairs, hipStream_t stream) {
  if (n_pairs == 0 || blocks_per_launch == 0) return hipSuccess;
  if (!span_args_ok(spn, true, channels, 8)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(span_replay_fb_kernel, dim3(n_pairs, (unsigned)(spn.n_spans + 7) / 8), dim3(64), 0, stream, spn, block0,
                     blocks_per_launch, channels);
  return hipGetLastError();
}

}  // namespace peaq

// peaq_replay_feed.h -- what the replays of the batch side (peaq_replay.hip: windows and spans of a pair) and of the live
// side (peaq_meter.hip: the sliding windows of a session) share: where a lane's values sit in a unit's records
// (LaneSrc), a unit's records as loaded (Raw), what an accumulator is given in a unit (Given), the three feeds, and the
// accumulate step.  Device code only; everything is in an unnamed namespace of the including file, like the kernels'
// other helpers.
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
#pragma once
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

// ---- the feeds: what differs between the three kernels of either file ----------------------------------------------
// kLanes / kUsed: accumulator lanes per channel, and how many of them own an accumulator; kFft: the units are FFT frames
// (FrameTrace records, the front end's records beside them; the head lane carries the energies and writes `frames`) or
// filter-bank blocks (BlockTrace records, nothing beside them; the head lane writes `fb_blocks`); kModes: the add modes
// that occur; acc / mode / source of accumulator lane a; load: a unit's records -> Raw; feed: ... -> what the lane's
// accumulator is given.  (In feed the lane's values are in their registers, in one place for all lanes: the loads are
// not moved behind a lane's branch of the pick.)

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

// ---- the accumulate step -------------------------------------------------------------------------------------------
// One unit into one lane's accumulator: the tentative / normal turn (movaccum.c:317-362), the energies (the head lane of
// an FFT feed), the add in the lane's mode (movaccum.c:368-425).  `f` the twelve fields, `status` the accumulator's.
template <class Feed>
__device__ __forceinline__ void replay_accumulate(double (&f)[kAccFields], int& status, double& sig_e, double& noise_e,
                                                  const Given& cur, int mode, bool head_lane) {
#pragma clang fp contract(off)
  auto occurs = [](int m) { return (Feed::kModes >> m & 1u) != 0; };   // (compile time: what a feed lacks folds away)
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
  if (Feed::kFft && head_lane) {
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

}  // namespace

}  // namespace peaq

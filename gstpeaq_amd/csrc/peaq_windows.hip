// peaq_windows.hip -- scores of time windows inside each pair of a batch run (peaq_batch_run_windows, basic version;
// include/peaq_amd.h).
//
// A window's reading is the read-out of eleven accumulators that were reset just before the window's first frame and
// then given what the pair's own accumulators were given in the window's frames: the same set_tentative, the same
// values, weights and gates, in the same order.  Everything below the accumulators is the pair's own, in context.  The
// run's back end is the trace instantiation, which leaves every frame's eight MOV-layer values and its gate flags in a
// scratch of the context; the bandwidths, the EHS, the energy bits and the two energies are in the front end's records
// of the same launch.  window_replay_kernel feeds both to the windows that meet the launch's frames.
//
//   window_replay_kernel   one wave serves two windows of one pair: lane l owns accumulator l & 15 (11 used) of channel
//       (l >> 4) & 1 of window slot l >> 5.  The twelve fields and the status stay in registers for the whole walk:
//       loaded from the window's snapshot (PointSnap, [pair][window]) at entry if the window meets the launch's frames,
//       stored at exit; a wave whose windows both miss the launch returns at once.  A frame's trace record and scalars
//       sit at wave-uniform addresses, to which a lane adds the fixed index of the value it takes; none depends on a
//       computed value: the loads of frame f + 1 are issued before the adds of frame f, and the only serial chain is the accumulator's own FP64 add.  No atomics, no LDS, no cross-lane
//       traffic; every lane stores what it owns, lane 0 of channel 0 of a slot the energies and the frame count.
//
// The add rounds as LaneAcc::add does in backend_kernel<109, false> (peaq_backend.hip), whose disassembly has
//   average (AVG, AVG_LOG, ADB)   num = fma(val, w, num);            den = w + den
//   RMS                           num = fma(val, val * (w * w), num); den = fma(w, w, den)
//   AVG_WINDOW                    ws = (((sq + p0) + p1) + p2) / 4; ws = ws * ws; num = fma(ws, ws, num); den = den + 1
//   FILTERED_MAX                  filt = fma(0.1, val, 0.9 * filt)
// -- restated here with contraction off and the fused operations spelt out, so that a window {0, L} is bit for bit the
// trajectory's point and the end result.
#include <hip/hip_runtime.h>

#include "peaq_device.h"
#include "peaq_kernels.h"

namespace peaq {

namespace {

enum { WB_BW_REF, WB_BW_TEST, WB_NMR, WB_WINMOD, WB_ADB, WB_EHS, WB_AVGMOD1, WB_AVGMOD2, WB_NOISELOUD, WB_MFPD,
       WB_RELDIST };                                   // gstpeaq.c:95-108, the order of MB_* in peaq_backend.hip
enum { F_NUM, F_DEN, F_NUM2, F_P0, F_P1, F_P2, F_MX, F_FILT, F_SNUM, F_SDEN, F_SNUM2, F_SMX };
static_assert(kAccFields == 12 && kMaxAcc == 11, "the fields and accumulators of LaneAcc");

// Where a lane's value sits in a frame's two records, fixed for the whole walk (peaq_backend_fft.inc:362-502): `t`
// an index into the FrameTrace's doubles (ch[2][6], p_detect, steps), `r` into the lane's channel of the front end's
// record; `from_rec` says which of the two the accumulator takes.
struct LaneSrc {
  int t, r;
  bool from_rec;
};
constexpr int kTrcPDetect = 12, kTrcSteps = 13;
static_assert(offsetof(FrameTrace, p_detect) == kTrcPDetect * 8 && offsetof(FrameTrace, steps) == kTrcSteps * 8 &&
                  offsetof(FrameTrace, flags) == 112,
              "the trace record as the replay indexes it");
__device__ __forceinline__ LaneSrc lane_source(int ai, int ch) {
  LaneSrc s{6 * ch, kRecBwRef, false};
  switch (ai) {
    case WB_BW_REF: s.from_rec = true; break;
    case WB_BW_TEST: s.r = kRecBwTest; s.from_rec = true; break;
    case WB_NMR: s.t += 4; break;
    case WB_WINMOD: break;
    case WB_ADB: s.t = kTrcSteps; break;
    case WB_EHS: s.r = kRecEhs; s.from_rec = true; break;
    case WB_AVGMOD1: break;
    case WB_AVGMOD2: s.t += 1; break;
    case WB_NOISELOUD: s.t += 3; break;
    case WB_MFPD: s.t = kTrcPDetect; break;
    case WB_RELDIST: s.t += 5; break;
  }
  return s;
}

// what a lane's accumulator is given in one frame
struct Feed {
  double v, w;
  bool hit, above;
  double sig, noise;            // the frame's energies over the channels (the energy lane adds them)
};

// One frame's trace record and front-end scalars as loaded: the lane's four values (tv, wt: its value and its channel's
// weight in the trace record; rv, bw_ref: its value and its channel's reference bandwidth in the front end's record) and
// what is the same for the whole wave.
struct Raw {
  double tv, wt, rv, bw_ref;
  double p_detect, sig, noise;
  uint32_t flags;
  int fl;
};
__device__ __forceinline__ Raw frame_load(const FrameTrace* __restrict__ tr, const double* __restrict__ rec, int channels,
                                          int ch, const LaneSrc src) {
#pragma clang fp contract(off)
  const double* __restrict__ t = reinterpret_cast<const double*>(tr);
  const double* __restrict__ r = rec + (size_t)ch * kRecDoubles;
  Raw x;
  x.tv = t[src.t];
  x.wt = t[6 * ch + 2];
  x.rv = r[src.r];
  x.bw_ref = r[kRecBwRef];
  x.p_detect = tr->p_detect;
  x.flags = tr->flags;
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
  return x;
}

// ... -> this lane's feed.  (The lane's four values are in their registers here, in one place for all lanes: the loads
// are not moved behind a lane's branch of the pick below.)
__device__ __forceinline__ Feed frame_feed(Raw x, int ai, int ch, const LaneSrc src) {
#pragma clang fp contract(off)
  asm volatile("" : "+v"(x.tv), "+v"(x.wt), "+v"(x.rv), "+v"(x.bw_ref));
  const bool mod_open = x.flags & kTraceModOpen, loud_open = x.flags & kTraceLoudOpen;
  Feed f;
  f.above = x.flags & kTraceAbove;
  f.sig = x.sig;
  f.noise = x.noise;
  f.w = ai == WB_AVGMOD1 || ai == WB_AVGMOD2 ? x.wt : 1.;
  f.v = ai == WB_RELDIST ? (x.tv > 1.41253754462275 ? 1. : 0.) : ai == WB_EHS ? 1000. * x.rv : src.from_rec ? x.rv : x.tv;
  f.hit = ai == WB_BW_REF || ai == WB_BW_TEST                        ? x.bw_ref > 346.
          : ai == WB_WINMOD || ai == WB_AVGMOD1 || ai == WB_AVGMOD2 ? mod_open
          : ai == WB_NOISELOUD                                       ? loud_open
          : ai == WB_ADB                                             ? ch == 0 && x.p_detect > 0.5
          : ai == WB_MFPD                                            ? ch == 0
          : ai == WB_EHS                                             ? (x.fl & 2) != 0
                                                                     : true;
  return f;
}

}  // namespace

__global__ __launch_bounds__(64) void window_replay_kernel(WindowArgs win, const double* __restrict__ records,
                                                           unsigned frame0, unsigned frames_per_launch, int channels) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int ai = lane & 15, ch = (lane >> 4) & 1, slot = lane >> 5;
  const unsigned pair = blockIdx.x;
  const int w0 = 2 * (int)blockIdx.y;                // the wave's two windows: w0, w0 + 1
  const uint32_t n_ref = win.n_ref ? win.n_ref[pair] : win.n_uniform;
  const uint32_t n_test = win.n_test ? win.n_test[pair] : win.n_uniform;
  const uint32_t l_end = frame0 + frames_per_launch;
  // both windows' frames of this launch, wave-uniform: [lo, hi) of [first, end) within [frame0, l_end)
  uint32_t first[2] = {0, 0}, lo[2] = {0, 0}, hi[2] = {0, 0};
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    if (w0 + s >= win.n_windows) continue;
    const WindowSpan ws = win.windows[w0 + s];
    uint32_t end;
    window_frames(n_ref, n_test, ws.start, ws.length, first[s], end);
    lo[s] = first[s] > frame0 ? first[s] : frame0;
    hi[s] = end < l_end ? end : l_end;
    if (hi[s] < lo[s]) hi[s] = lo[s];
  }
  const bool meet0 = lo[0] < hi[0], meet1 = lo[1] < hi[1];
  if (!meet0 && !meet1) return;
  const uint32_t f_begin = !meet1 ? lo[0] : !meet0 ? lo[1] : (lo[0] < lo[1] ? lo[0] : lo[1]);
  const uint32_t f_end = !meet1 ? hi[0] : !meet0 ? hi[1] : (hi[0] > hi[1] ? hi[0] : hi[1]);
  const uint32_t my_lo = slot ? lo[1] : lo[0], my_hi = slot ? hi[1] : hi[0], my_first = slot ? first[1] : first[0];
  const bool own = ai < kMaxAcc && ch < channels && my_lo < my_hi;   // (a slot past n_windows has lo == hi == 0)
  const bool energy_lane = own && ai == 0 && ch == 0;

  PointSnap* __restrict__ sp = win.snap + (size_t)pair * win.n_windows + (w0 + slot);   // (read and written by `own` lanes only)
  double f[kAccFields];
  int status = kInit;
  double sig_e = 0., noise_e = 0.;
  if (own) {
#pragma unroll
    for (int k = 0; k < kAccFields; ++k) f[k] = sp->acc[ch][ai][k];
    status = sp->status[ai];
  } else {
#pragma unroll
    for (int k = 0; k < kAccFields; ++k) f[k] = 0.;
  }
  if (energy_lane) {
    sig_e = sp->sig_energy;
    noise_e = sp->noise_energy;
  }
  // gstpeaq.c:528-557 (acc_mode of peaq_backend.hip, basic version)
  const int mode = ai == WB_NMR ? kAvgLog : ai == WB_WINMOD ? kAvgWindow : ai == WB_ADB ? kAdb : ai == WB_NOISELOUD ? kRms
                   : ai == WB_MFPD ? kFilteredMax : kAvg;
  const int lane_ai = ai < kMaxAcc ? ai : 0, lane_ch = ch < channels ? ch : 0;

  const FrameTrace* __restrict__ trace = win.trace + (size_t)pair * win.trace_stride;
  const double* __restrict__ recs = records + (size_t)pair * frames_per_launch * channels * kRecDoubles;
  const LaneSrc src = lane_source(lane_ai, lane_ch);
  auto load_of = [&](uint32_t frame) {
    return frame_load(trace + frame, recs + (size_t)(frame - frame0) * channels * kRecDoubles, channels, lane_ch, src);
  };
  Feed cur = frame_feed(load_of(f_begin), lane_ai, lane_ch, src);
  for (uint32_t frame = f_begin; frame < f_end; ++frame) {
    // (the next frame's loads before this frame's adds; the last frame reads itself again)
    const Raw nxt = load_of(frame + 1 < f_end ? frame + 1 : frame);
    if (own && frame >= my_lo && frame < my_hi) {
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
      if (energy_lane) {
        sig_e = sig_e + cur.sig;
        noise_e = noise_e + cur.noise;
      }
      // movaccum.c:368-425
      if (cur.hit && status != kInit) {
        const double v = cur.v, w = cur.w;
        if (mode == kAvgWindow) {
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
        } else if (mode == kFilteredMax) {
          const double filt = __builtin_fma(0.1, v, 0.9 * f[F_FILT]);
          f[F_FILT] = filt;
          if (filt > f[F_MX]) f[F_MX] = filt;
        } else if (mode == kRms) {
          const double w2 = w * w;
          f[F_NUM] = __builtin_fma(v, v * w2, f[F_NUM]);
          f[F_DEN] = __builtin_fma(w, w, f[F_DEN]);
        } else {
          f[F_NUM] = __builtin_fma(v, w, f[F_NUM]);
          f[F_DEN] = w + f[F_DEN];
        }
      }
    }
    cur = frame_feed(nxt, lane_ai, lane_ch, src);
  }
  if (own) {
#pragma unroll
    for (int k = 0; k < kAccFields; ++k) sp->acc[ch][ai][k] = f[k];
    if (ch == 0) sp->status[ai] = status;
  }
  if (energy_lane) {
    sp->frames = my_hi - my_first;
    sp->sig_energy = sig_e;
    sp->noise_energy = noise_e;
  }
}

hipError_t launch_window_replay(const WindowArgs& win, const double* records, unsigned frame0, unsigned frames_per_launch,
                                int channels, unsigned n_pairs, hipStream_t stream) {
  if (n_pairs == 0 || frames_per_launch == 0) return hipSuccess;
  if (!win.snap || !win.windows || !win.trace || !records || win.n_windows < 1 || win.n_windows > 2 * 65535 ||
      (channels != 1 && channels != 2))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(window_replay_kernel, dim3(n_pairs, (unsigned)(win.n_windows + 1) / 2), dim3(64), 0, stream, win,
                     records, frame0, frames_per_launch, channels);
  return hipGetLastError();
}

}  // namespace peaq

// peaq_spans.hip -- scores of time spans inside each pair of a batch run, advanced version (peaq_batch_run_adv_spans;
// include/peaq_amd.h).
//
// A span's reading is the read-out of the advanced version's five accumulators that were reset just before the span's
// first FFT frame / first filter-bank block and then given what the pair's own accumulators were given in the span's
// frames and blocks: the same set_tentative, the same values, weights and gates, in the same order.  Everything below the
// accumulators is the pair's own, in context.  The advanced version has two feeds with two units, on two streams: the
// 55-band FFT back end (frames of 2048 samples every 1024: SegmentalNMR, EHS, the energies) and the filter-bank back end
// (blocks of 192 samples: RmsModDiff, RmsNoiseLoudAsym, AvgLinDist).  Both run as their trace instantiations, which
// leave every frame's and every block's MOV-layer values and gate flags in scratch of the context; the EHS, the energy
// bits and the two energies are in the FFT front end's records of the same launch.  One replay body, two kernels:
//
//   span_replay_fft_kernel   behind every FFT back-end launch: the launch's frames into SegmentalNMR and EHS
//   span_replay_fb_kernel    behind every filter-bank back-end launch: the launch's blocks into the other three
//
//   One wave serves eight spans of one pair: lane l owns accumulator slot l & 3 of channel (l >> 2) & 1 of span slot
//   l >> 3 -- SegNMR, EHS and two idle lanes in the FFT kernel; RmsModDiff, RmsNoiseLoudAsym, AvgLinDist and one idle
//   lane in the filter-bank kernel.  The twelve fields and the status stay in registers for the whole walk: loaded from
//   the span's snapshot (PointSnap, [pair][span]) at entry if the span meets the launch's units, stored at exit; a wave
//   none of whose spans meets the launch returns before it loads anything.  The wave walks from the smallest first to
//   the largest last unit of its spans, a lane acting on the units of its own span.  A unit's records sit at
//   wave-uniform addresses, to which a lane adds the fixed index of the value it takes; none depends on a loaded or
//   computed value: the loads of unit u + 1 are issued before the adds of unit u, and the only serial chain is the
//   accumulator's own FP64 add.  No atomics, no LDS, no cross-lane traffic; every lane stores what it owns, lane
//   (accumulator 0, channel 0) of a slot the energies and `frames` in the FFT kernel, `fb_blocks` in the filter-bank
//   kernel.  The two kernels run beside each other on two streams and write disjoint words of the same snapshots, as the
//   two points instantiations of the back ends do.
//
// The add rounds as LaneAcc::add does in the shipped kernels, whose disassembly (val, w the arguments of add) has
//   fb_backend_trace_kernel, fb_backend_points_kernel (the same three sequences in both)
//     RMS        w2 = w * w; t = val * w2; num = fma(val, t, num); den = fma(w, w, den)
//     RMS_ASYM   num = fma(val, val, num); num2 = fma(w, w, num2); den = den + 1
//     AVG        num = fma(w, val, num); den = w + den                       (AvgLinDist: w = 1)
//   backend_trace_kernel<55, true>, backend_points_kernel<55, true> (w is the literal 1 of every route)
//     AVG        num = val + num; den = den + 1          (= fma(val, 1, num), 1 + den: the same bits)
//     EHS's value is the plain product 1000 * ehs
// -- restated here with contraction off and the fused operations spelt out, so that a span {0, L} is bit for bit the
// advanced trajectory's point and the end result.
#include <hip/hip_runtime.h>

#include "peaq_device.h"
#include "peaq_kernels.h"

namespace peaq {

namespace {

enum { SA_RMSMOD, SA_NLASYM, SA_SEGNMR, SA_EHS, SA_LINDIST };   // gstpeaq.c:110-116, the order of MA_* in peaq_backend.hip
enum { F_NUM, F_DEN, F_NUM2, F_P0, F_P1, F_P2, F_MX, F_FILT, F_SNUM, F_SDEN, F_SNUM2, F_SMX };
static_assert(kAccFields == 12 && kMaxAcc >= 5, "the fields and accumulators of LaneAcc");
static_assert(sizeof(FrameTrace) == 16 * sizeof(double) && offsetof(FrameTrace, ch) == 0 &&
                  offsetof(FrameTrace, flags) == 112 && sizeof(BlockTrace) == 12 * sizeof(double) &&
                  offsetof(BlockTrace, ch) == 0 && offsetof(BlockTrace, flags) == 80,
              "the trace records as the replay indexes them");

// Where a lane's two values sit, fixed for the whole walk.  FFT kernel (peaq_backend_fft.inc:502-534): `v` an index into
// the FrameTrace's doubles (ch[c][0], the segmental NMR), `w` into the frame's front-end record(s) (channel c's EHS).
// Filter-bank kernel (peaq_backend_fb.inc:116-263): both index the BlockTrace's doubles (ch[c][0 .. 4]: RmsModDiff, its
// weight, noise loudness, missing components, linear distortion).
struct LaneSrc {
  int v, w;
};
template <bool FB>
__device__ __forceinline__ LaneSrc lane_source(int a, int ch) {
  if (FB) return LaneSrc{5 * ch + (a == 0 ? 0 : a == 1 ? 2 : 4), 5 * ch + (a == 0 ? 1 : 3)};
  return LaneSrc{6 * ch, ch * kRecDoubles + kRecEhs};
}

// One unit's records as loaded: the lane's two values and what is the same for the whole wave.
struct Raw {
  double v, w;
  double sig, noise;            // FFT kernel: the frame's energies over the channels
  uint32_t flags;               // kTrace* of the unit's trace record
  int fl;                       // FFT kernel: the front end's flag words of both signals, all channels
};
template <bool FB>
__device__ __forceinline__ Raw unit_load(const void* __restrict__ trace_rec, const double* __restrict__ rec, int channels,
                                         const LaneSrc src) {
#pragma clang fp contract(off)
  const double* __restrict__ t = reinterpret_cast<const double*>(trace_rec);
  Raw x;
  x.v = t[src.v];
  x.sig = x.noise = 0.;
  x.fl = 0;
  if (FB) {
    x.w = t[src.w];
    x.flags = reinterpret_cast<const BlockTrace*>(trace_rec)->flags;
  } else {
    x.w = rec[src.w];
    x.flags = reinterpret_cast<const FrameTrace*>(trace_rec)->flags;
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
  return x;
}

// what a lane's accumulator is given in one unit
struct Feed {
  double v, w;
  bool hit, above;
  double sig, noise;
};
// ... -> this lane's feed.  (The lane's two values are in their registers here, in one place for all lanes: the loads
// are not moved behind a lane's branch of the pick below.)
template <bool FB>
__device__ __forceinline__ Feed unit_feed(Raw x, int a) {
#pragma clang fp contract(off)
  asm volatile("" : "+v"(x.v), "+v"(x.w));
  Feed f;
  f.above = x.flags & kTraceAbove;
  f.sig = x.sig;
  f.noise = x.noise;
  if (FB) {
    f.v = x.v;
    f.w = a == 2 ? 1. : x.w;
    f.hit = a == 0 ? (x.flags & kTraceModOpen) != 0 : (x.flags & kTraceLoudOpen) != 0;
  } else {
    f.v = a == 1 ? 1000. * x.w : x.v;
    f.w = 1.;
    f.hit = a == 1 ? (x.fl & 2) != 0 : true;
  }
  return f;
}

// units [first, end) of a span: FFT frames or filter-bank blocks
template <bool FB>
__device__ __forceinline__ void span_units(uint32_t n_ref, uint32_t n_test, WindowSpan s, uint32_t& first, uint32_t& end) {
  if (FB)
    span_blocks(n_ref, n_test, s.start, s.length, first, end);
  else
    window_frames(n_ref, n_test, s.start, s.length, first, end);
}

// The replay of units [unit0, unit0 + units_per_launch) of every pair into the spans that meet them.  `records`: the
// FFT front end's records of the launch (FFT kernel only).
template <bool FB>
__device__ __forceinline__ void span_replay(const SpanArgs& spn, const double* __restrict__ records, unsigned unit0,
                                            unsigned units_per_launch, int channels) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int a = lane & 3, ch = (lane >> 2) & 1, slot = lane >> 3;
  const unsigned pair = blockIdx.x;
  const int s0 = 8 * (int)blockIdx.y;                // the wave's eight spans: s0 .. s0 + 7
  const uint32_t n_ref = spn.n_ref ? spn.n_ref[pair] : spn.n_uniform;
  const uint32_t n_test = spn.n_test ? spn.n_test[pair] : spn.n_uniform;
  const uint32_t l_end = unit0 + units_per_launch;
  // the wave's units of this launch, wave-uniform: from the smallest lo to the largest hi of the spans that meet it,
  // [lo, hi) = [first, end) within [unit0, l_end)
  uint32_t u_begin = UINT_MAX, u_end = 0;
  for (int s = 0; s < 8; ++s) {
    if (s0 + s >= spn.n_spans) break;
    uint32_t first, end;
    span_units<FB>(n_ref, n_test, spn.spans[s0 + s], first, end);
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
    span_units<FB>(n_ref, n_test, spn.spans[s0 + slot], my_first, end);
    my_lo = my_first > unit0 ? my_first : unit0;
    my_hi = end < l_end ? end : l_end;
    if (my_hi < my_lo) my_hi = my_lo;
  }
  const bool used = FB ? a < 3 : a < 2;
  const bool own = used && ch < channels && my_lo < my_hi;
  const bool head_lane = own && a == 0 && ch == 0;   // the slot's counts and energies
  const int acc = FB ? (a == 0 ? SA_RMSMOD : a == 1 ? SA_NLASYM : SA_LINDIST) : (a == 0 ? SA_SEGNMR : SA_EHS);
  // gstpeaq.c:547-557 (acc_mode of peaq_backend.hip, advanced version)
  const int mode = FB ? (a == 0 ? kRms : a == 1 ? kRmsAsym : kAvg) : kAvg;

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
  if (!FB && head_lane) {
    sig_e = sp->sig_energy;
    noise_e = sp->noise_energy;
  }

  const int lane_a = used ? a : 0, lane_ch = ch < channels ? ch : 0;
  const LaneSrc src = lane_source<FB>(lane_a, lane_ch);
  const char* __restrict__ trace =
      FB ? reinterpret_cast<const char*>(spn.blocks + (size_t)pair * spn.block_stride)
         : reinterpret_cast<const char*>(spn.frames + (size_t)pair * spn.frame_stride);
  constexpr size_t kTraceBytes = FB ? sizeof(BlockTrace) : sizeof(FrameTrace);
  const double* __restrict__ recs = FB ? nullptr : records + (size_t)pair * units_per_launch * channels * kRecDoubles;
  auto load_of = [&](uint32_t unit) {
    return unit_load<FB>(trace + (size_t)unit * kTraceBytes,
                         FB ? nullptr : recs + (size_t)(unit - unit0) * channels * kRecDoubles, channels, src);
  };
  Feed cur = unit_feed<FB>(load_of(u_begin), lane_a);
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
      if (!FB && head_lane) {
        sig_e = sig_e + cur.sig;
        noise_e = noise_e + cur.noise;
      }
      // movaccum.c:368-425
      if (cur.hit && status != kInit) {
        const double v = cur.v, w = cur.w;
        if (mode == kRms) {
          const double w2 = w * w;
          const double t = v * w2;
          f[F_NUM] = __builtin_fma(v, t, f[F_NUM]);
          f[F_DEN] = __builtin_fma(w, w, f[F_DEN]);
        } else if (mode == kRmsAsym) {
          f[F_NUM] = __builtin_fma(v, v, f[F_NUM]);
          f[F_NUM2] = __builtin_fma(w, w, f[F_NUM2]);
          f[F_DEN] = f[F_DEN] + 1.;
        } else {
          f[F_NUM] = __builtin_fma(w, v, f[F_NUM]);
          f[F_DEN] = w + f[F_DEN];
        }
      }
    }
    cur = unit_feed<FB>(nxt, lane_a);
  }
  if (own) {
#pragma unroll
    for (int k = 0; k < kAccFields; ++k) sp->acc[ch][acc][k] = f[k];
    if (ch == 0) sp->status[acc] = status;
  }
  if (head_lane) {
    if (FB) {
      sp->fb_blocks = my_hi - my_first;
    } else {
      sp->frames = my_hi - my_first;
      sp->sig_energy = sig_e;
      sp->noise_energy = noise_e;
    }
  }
}

}  // namespace

__global__ __launch_bounds__(64) void span_replay_fft_kernel(SpanArgs spn, const double* __restrict__ records,
                                                             unsigned frame0, unsigned frames_per_launch, int channels) {
  span_replay<false>(spn, records, frame0, frames_per_launch, channels);
}

__global__ __launch_bounds__(64) void span_replay_fb_kernel(SpanArgs spn, unsigned block0, unsigned blocks_per_launch,
                                                            int channels) {
  span_replay<true>(spn, nullptr, block0, blocks_per_launch, channels);
}

static bool span_args_ok(const SpanArgs& spn, int channels) {
  return spn.snap && spn.spans && spn.frames && spn.blocks && spn.n_spans >= 1 && spn.n_spans <= 8 * 65535 &&
         (channels == 1 || channels == 2);
}

hipError_t launch_span_replay_fft(const SpanArgs& spn, const double* records, unsigned frame0, unsigned frames_per_launch,
                                  int channels, unsigned n_pairs, hipStream_t stream) {
  if (n_pairs == 0 || frames_per_launch == 0) return hipSuccess;
  if (!span_args_ok(spn, channels) || !records) return hipErrorInvalidValue;
  hipLaunchKernelGGL(span_replay_fft_kernel, dim3(n_pairs, (unsigned)(spn.n_spans + 7) / 8), dim3(64), 0, stream, spn,
                     records, frame0, frames_per_launch, channels);
  return hipGetLastError();
}

hipError_t launch_span_replay_fb(const SpanArgs& spn, unsigned block0, unsigned blocks_per_launch, int channels,
                                 unsigned n_pairs, hipStream_t stream) {
  if (n_pairs == 0 || blocks_per_launch == 0) return hipSuccess;
  if (!span_args_ok(spn, channels)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(span_replay_fb_kernel, dim3(n_pairs, (unsigned)(spn.n_spans + 7) / 8), dim3(64), 0, stream, spn, block0,
                     blocks_per_launch, channels);
  return hipGetLastError();
}

}  // namespace peaq

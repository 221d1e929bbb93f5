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
// The feeds (BasicFftFeed, AdvFftFeed, AdvFbFeed), LaneSrc / Raw / Given and the accumulate step -- with the note on how
// the add rounds -- are in peaq_replay_feed.h, which the live side's replay (peaq_meter.hip) includes as well.
#include <hip/hip_runtime.h>

#include "peaq_device.h"
#include "peaq_kernels.h"
#include "peaq_replay_feed.h"

namespace peaq {

namespace {

// ---- the body ------------------------------------------------------------------------------------------------------
// The replay of units [unit0, unit0 + units_per_launch) of every pair into the spans that meet them.  `records`: the
// FFT front end's records of the launch (FFT feeds only).  The units [first, end) of a span are window_frames' (FFT
// feeds) or span_blocks' (filter-bank feed).
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
    if (own && unit >= my_lo && unit < my_hi) replay_accumulate<Feed>(f, status, sig_e, noise_e, cur, mode, head_lane);
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

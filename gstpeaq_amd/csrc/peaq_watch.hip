// peaq_watch.hip -- the delay watch of a live stream (peaq_session_set_align with watch_frames, peaq_session_watch_read
// in include/peaq_amd.h, "live alignment"): the cross-correlation of the two pads at the lags -31 .. 31
// around the alignment the stream runs at, over tumbling windows of W whole FFT frames, behind the stream's own
// front-end launches and from the samples those have staged.  The watch reports; it never touches the stream.
//
// With r[n], t[n] the mono sums in double of the stream as scored, frame f owns n = 1024 f + 512 .. 1024 f + 1535, and
// every n + d, |d| <= 31, lies inside that frame's 2048 samples: a frame's contribution needs the frame alone.
//
//   delay_watch_frames_kernel   one wave per whole frame of the launch (workgroups of four waves).  The wave puts the
//       frame's r over [512, 1536) and t over [481, 1567) into its own LDS as doubles (16.9 KB per wave).  Lane l < 63
//       owns d = l - 31 and walks n in ascending order, one multiply-add per n: r[n] is the same address in every lane
//       (a broadcast), t[n + d] consecutive doubles across the lanes (64 banks per half wave: no conflict).  Lane 63
//       walks the same loop over r[n] r[n]: e_ref.  e_test is the sum of sixteen squares per lane in ascending n, then
//       the wave's fixed tree.  The frame's row -- 63 lags, e_ref, e_test -- goes to scratch [stream][frame][66].
//   delay_watch_fold_kernel     one wave per stream of the launch, lane = column (lane 0 also carries column 64,
//       e_test).  It adds the launch's rows in frame order to the stream's accumulators; when the count reaches W it
//       copies them with the window's index and first frame to the stream's "latest" row, zeroes them and goes on.
//       Plain vector stores, no atomics: one wave owns a stream's state.
// A broker's launch gives every stream its own count of whole frames and its slot (WatchArgs::s_*): rows the tick uploads.
// Every sum has a fixed order that does not depend on how the stream was cut into launches, so a window's record is the
// same bit for bit for any push pattern and from run to run.
#include <hip/hip_runtime.h>

#include "peaq_device.h"
#include "peaq_kernels.h"
#include "peaq_wave.h"

namespace peaq {

namespace {

constexpr int kWatchR0 = 512, kWatchN = 1024;                  // the n a frame owns, frame-relative: [512, 1536)
constexpr int kWatchT0 = kWatchR0 - kWatchLags;                // t is needed over [481, 1567)
constexpr int kWatchTN = kWatchN + 2 * kWatchLags;             // 1086
constexpr int kWatchTPad = 1088;

__device__ __forceinline__ double watch_mono(const float* __restrict__ x, size_t s, int channels) {
  double v = (double)x[s * channels];
  if (channels == 2) v += (double)x[s * channels + 1];
  return v;
}

__global__ __launch_bounds__(256) void delay_watch_frames_kernel(const WatchArgs a) {
  __shared__ double sh_r[4][kWatchN];
  __shared__ double sh_t[4][kWatchTPad];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t f = 4 * blockIdx.x + wave;
  const unsigned strm = blockIdx.y;
  const uint32_t n_frames = a.s_frames ? min(a.s_frames[strm], a.n_frames) : a.n_frames;
  if (f >= n_frames) return;                         // (wave-uniform; the waves of a workgroup share nothing)
  const size_t s0 = (size_t)strm * a.pair_stride + (size_t)f * kHop;
  double* __restrict__ r = sh_r[wave];
  double* __restrict__ t = sh_t[wave];
  for (int i = lane; i < kWatchN; i += 64) r[i] = watch_mono(a.ref, s0 + kWatchR0 + i, a.channels);
  for (int i = lane; i < kWatchTN; i += 64) t[i] = watch_mono(a.test, s0 + kWatchT0 + i, a.channels);
  wave_lds_fence();
  // lanes 0 .. 62: c[d], t[n + d] at t[n + lane]; lane 63: e_ref
  const bool lag = lane < kWatchCols - 2;
  const int tl = lag ? lane : kWatchLags;
  double acc = 0.;
#pragma unroll 8
  for (int n = 0; n < kWatchN; ++n) {
    const double x = r[n];
    const double y = t[n + tl];
    acc = fma(x, lag ? y : x, acc);
  }
  double et = 0.;
#pragma unroll
  for (int j = 0; j < kWatchN / 64; ++j) {
    const double y = t[kWatchLags + lane + 64 * j];
    et = fma(y, y, et);
  }
  et = wave_sum(et);
  double* __restrict__ row = a.rows + ((size_t)strm * a.row_stride + f) * kWatchRow;
  row[lane] = acc;
  if (lane == 0) row[kWatchCols - 1] = et;
}

__global__ __launch_bounds__(64) void delay_watch_fold_kernel(const WatchArgs a) {
  const int lane = threadIdx.x;
  const unsigned strm = blockIdx.x;
  WatchState* __restrict__ st = a.state + (a.s_slot ? a.s_slot[strm] : strm);
  const double* __restrict__ rows = a.rows + (size_t)strm * a.row_stride * kWatchRow;
  const uint32_t n_frames = a.s_frames ? min(a.s_frames[strm], a.n_frames) : a.n_frames;
  if (!n_frames) return;
  const bool head = lane == 0;
  double acc = st->acc[lane], acc2 = head ? st->acc[kWatchCols - 1] : 0.;
  uint32_t count = st->count;
  uint64_t k = st->index;
  for (uint32_t f = 0; f < n_frames; ++f) {
    acc += rows[(size_t)f * kWatchRow + lane];
    if (head) acc2 += rows[(size_t)f * kWatchRow + kWatchCols - 1];
    if (++count == a.window) {
      st->latest[lane] = acc;
      if (head) {
        st->latest[kWatchCols - 1] = acc2;
        st->latest_index = k;
        st->latest_first = (uint32_t)(k * a.window);
        st->latest_frames = a.window;
      }
      acc = acc2 = 0.;
      count = 0;
      ++k;
    }
  }
  st->acc[lane] = acc;
  if (head) {
    st->acc[kWatchCols - 1] = acc2;
    st->count = count;
    st->index = k;
  }
}

}  // namespace

hipError_t launch_delay_watch(const WatchArgs& a, unsigned n_streams, hipStream_t stream) {
  if (!a.n_frames || !n_streams) return hipSuccess;
  hipLaunchKernelGGL(delay_watch_frames_kernel, dim3((a.n_frames + 3) / 4, n_streams), dim3(256), 0, stream, a);
  hipLaunchKernelGGL(delay_watch_fold_kernel, dim3(n_streams), dim3(64), 0, stream, a);
  return hipGetLastError();
}

}  // namespace peaq

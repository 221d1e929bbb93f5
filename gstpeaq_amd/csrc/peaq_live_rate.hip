// peaq_live_rate.hip -- rate conversion of live streams, window by window (include/peaq_amd.h, "live rate conversion";
// DESIGN.md 34): the host arithmetic that maps raw sample counts to converted ones (peaq_live_rate_ready,
// peaq_live_rate_inputs), and peaq_batch_resample_range, the converter of peaq_resample.hip over SEGMENTS -- a run of
// outputs of one stream from a row that holds the raw samples those outputs read.  Same filter, same plain [L][2K] tap
// table, same chain per output (FP64 multiply-adds in the tap order, one rounding to FP32), so a stream converted in
// segments is bit for bit the stream peaq_batch_resample converts whole.
//
// One kernel, resample_range_kernel.  A workgroup owns kRangeTile consecutive outputs of one segment.  It stages the
// raw samples they read -- one run of at most kRangeTile M / L + 2K + 1 samples, all channels, coalesced -- in LDS
// once, absent samples (outside the stream) as zeros, which leave an FP64 sum as it is.  LANE = OUTPUT: a session's
// window is a frame or two (2048 .. 3072 outputs), a broker's tick has about as much per stream, and with lane = period
// (resample_tile_kernel) a tile would be 64 L' outputs, 10240 at 44.1 kHz, with a fifth of the lanes at work.  Each lane
// walks its tap row in the global table two taps a load (the row is 16-byte aligned: 2K doubles) and its samples in
// LDS, consecutive lanes M / L floats apart; both channels of a stereo stream share the taps.  The table of a rate is
// 84 KB at 44.1 kHz and stays in L2.
#include "peaq_host.h"

namespace {

constexpr int kRangeTile = 256;                                    // outputs per workgroup = threads
constexpr uint32_t kRangeRatioMax = 8, kRangeTapsMax = 520;        // M / L <= 8 (384 kHz), 2K <= 516 of every supported rate
constexpr uint32_t kRangeSpanMax = kRangeTile * kRangeRatioMax + kRangeTapsMax;   // staged samples per channel

struct RangeArgs {
  size_t in_stride, out_stride;   // samples per channel between the rows of in and out
  int channels;
  uint32_t L, M, K;
};

static_assert(sizeof(peaq_rate_segment) == 32, "peaq_rate_segment: three positions and two counts");

// (taps and segments as parameters of their own, as in resample_tile_kernel)
__global__ __launch_bounds__(kRangeTile) void resample_range_kernel(const RangeArgs a,
                                                                     const peaq_rate_segment* __restrict__ a_seg,
                                                                     const float* __restrict__ a_in,
                                                                     float* __restrict__ a_out,
                                                                     const double* __restrict__ a_taps) {
  __shared__ __attribute__((aligned(16))) float span[kRangeSpanMax * 2];
  const peaq_rate_segment sg = a_seg[blockIdx.y];
  const unsigned long long t0 = (unsigned long long)blockIdx.x * kRangeTile;
  if (t0 >= sg.out_count) return;                                  // (the whole workgroup)
  const unsigned count = (unsigned)min((unsigned long long)kRangeTile, sg.out_count - t0);
  const unsigned tid = threadIdx.x;
  const unsigned C = (unsigned)a.channels;
  // the tile's first output in 64 bits, once; the lanes go on from it in 32 (i M < 2^24: M <= 32000)
  const unsigned long long mm0 = (sg.out_first + t0) * a.M;
  const unsigned long long q0 = mm0 / a.L;
  const uint32_t p0 = (uint32_t)(mm0 % a.L);
  // floor(p / L - 1/8) is -1 below an eighth and 0 from there on, as in resample_any_kernel
  auto first_of = [&](unsigned i, uint32_t* p) {
    const uint32_t t = p0 + i * a.M;
    *p = t % a.L;
    return (long long)(q0 + t / a.L) + (8ull * *p < a.L ? -1 : 0) - (long long)a.K + 1;
  };
  uint32_t p_lo, p_hi, p;
  const long long s_lo = first_of(0, &p_lo);                       // n_first is non-decreasing in m
  const unsigned len = (unsigned)(first_of(count - 1, &p_hi) + 2 * (long long)a.K - s_lo);   // <= kRangeSpanMax (host)
  const float* in = a_in + (size_t)blockIdx.y * a.in_stride * C;
  // ---- stage the raw span; absent samples are zeros (h x 0 leaves a sum as it is) ----
  for (unsigned v = tid; v < len * C; v += kRangeTile) {
    const long long s = s_lo + (long long)(C == 2 ? v >> 1 : v);
    const unsigned long long u = (unsigned long long)s;
    const bool there = s >= 0 && u < sg.in_total && u >= sg.in_base && u - sg.in_base < sg.in_have;
    span[v] = there ? in[(size_t)(u - sg.in_base) * C + (C == 2 ? v & 1 : 0)] : 0.f;
  }
  __syncthreads();
  if (tid >= count) return;
  // ---- one output per lane: the chain of resample_any_kernel ----
  const long long n_first = first_of(tid, &p);
  const double2* h = reinterpret_cast<const double2*>(a_taps + (size_t)p * 2 * a.K);
  float* out = a_out + ((size_t)blockIdx.y * a.out_stride + t0 + tid) * C;
  if (C == 2) {
    const float2* x = reinterpret_cast<const float2*>(span) + (n_first - s_lo);
    double acc0 = 0., acc1 = 0.;
    for (uint32_t j = 0; j < a.K; ++j) {
      const double2 t = h[j];
      const float2 xa = x[2 * j], xb = x[2 * j + 1];
      acc0 = __builtin_fma(t.x, (double)xa.x, acc0);
      acc1 = __builtin_fma(t.x, (double)xa.y, acc1);
      acc0 = __builtin_fma(t.y, (double)xb.x, acc0);
      acc1 = __builtin_fma(t.y, (double)xb.y, acc1);
    }
    out[0] = (float)acc0;
    out[1] = (float)acc1;
  } else {
    const float* x = span + (n_first - s_lo);
    double acc = 0.;
    for (uint32_t j = 0; j < a.K; ++j) {
      const double2 t = h[j];
      acc = __builtin_fma(t.x, (double)x[2 * j], acc);
      acc = __builtin_fma(t.y, (double)x[2 * j + 1], acc);
    }
    out[0] = (float)acc;
  }
}

// positions the arithmetic below takes: m M and 8 L n stay far inside 64 bits
constexpr uint64_t kRangePosMax = (1ull << 62) / 48000;

// floor (t_m) = (m M) div L + (8 p < L ? -1 : 0), the sample in front of output m's position
long long floor_pos(const RateGeometry& g, uint64_t m) {
  const unsigned __int128 mm = (unsigned __int128)m * g.M;
  const uint64_t p = (uint64_t)(mm % g.L);
  return (long long)(uint64_t)(mm / g.L) + (8 * p < g.L ? -1 : 0);
}

uint64_t ready_open(const RateGeometry& g, uint64_t n_have) {
  // last (m) = floor ((8 m M - L) / (8 L)) + K < n_have  <=>  8 m M < 8 L (n_have - K) + L = A
  if (n_have < g.K) return 0;
  const unsigned __int128 A = (unsigned __int128)8 * g.L * (n_have - g.K) + g.L;
  return (uint64_t)((A - 1) / (8ull * g.M)) + 1;
}

void span_of(const RateGeometry& g, uint64_t out_first, uint32_t out_count, uint64_t* in_first, uint64_t* in_end) {
  const long long nf = floor_pos(g, out_first) - (long long)g.K + 1;
  *in_first = nf > 0 ? (uint64_t)nf : 0;
  *in_end = out_count ? (uint64_t)(floor_pos(g, out_first + out_count - 1) + (long long)g.K + 1) : *in_first;
}

int check_position(const std::string& who, const char* name, uint64_t v) {
  return v <= kRangePosMax ? PEAQ_OK
                           : fail(PEAQ_ERR_ARG, who + ": " + name + " " + std::to_string(v) + " is past 2^62 / 48000");
}

}  // namespace

// (peaq_host.h: what the stream framer counts with)
uint64_t live_rate_ready(const RateGeometry& g, uint32_t rate, uint64_t n_have, bool ended) {
  return ended ? resampled_length_u64(n_have, rate) : ready_open(g, n_have);
}
void live_rate_span(const RateGeometry& g, uint64_t out_first, uint32_t out_count, uint64_t* in_first, uint64_t* in_end) {
  span_of(g, out_first, out_count, in_first, in_end);
}

extern "C" size_t peaq_rate_segment_size(void) { return sizeof(peaq_rate_segment); }

extern "C" int peaq_live_rate_ready(uint32_t rate, uint64_t n_have, int ended, uint64_t* ready) {
  const std::string who("peaq_live_rate_ready");
  if (!ready) return fail(PEAQ_ERR_ARG, who + ": ready is NULL");
  *ready = 0;
  RateGeometry g;
  if (int rc = resample_geometry(who.c_str(), rate, &g)) return rc;
  if (int rc = check_position(who, "n_have", n_have)) return rc;
  *ready = ended ? resampled_length_u64(n_have, rate) : ready_open(g, n_have);
  return PEAQ_OK;
}

extern "C" int peaq_live_rate_inputs(uint32_t rate, uint64_t out_first, uint32_t out_count, uint64_t* in_first,
                                   uint64_t* in_end) {
  const std::string who("peaq_live_rate_inputs");
  if (!in_first || !in_end) return fail(PEAQ_ERR_ARG, who + ": NULL argument");
  *in_first = *in_end = 0;
  RateGeometry g;
  if (int rc = resample_geometry(who.c_str(), rate, &g)) return rc;
  if (int rc = check_position(who, "out_first", out_first)) return rc;
  span_of(g, out_first, out_count, in_first, in_end);
  return PEAQ_OK;
}

// the launch over checked segments: the rate's plain table (uploaded at the first call), the segments through a pinned
// slot, one grid of (tiles of the longest segment) x segments
static int range_launch(peaq_ctx* c, int channels, uint32_t rate, int n_segments, const peaq_rate_segment* seg,
                        const float* d_in, size_t in_stride, float* d_out, size_t out_stride, uint32_t count_max,
                        hipStream_t stream) {
  std::lock_guard<std::mutex> lock(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  const double* taps = nullptr;
  LenStage* lens = nullptr;
  RateGeometry g;
  if (int rc = resample_plain_table(c, rate, &taps, &g, &lens)) return rc;
  LenSlot* slot = nullptr;
  static_assert(sizeof(peaq_rate_segment) % sizeof(uint32_t) == 0, "segments travel as 32-bit words");
  if (int rc = lens->upload(reinterpret_cast<const uint32_t*>(seg),
                            (size_t)n_segments * (sizeof(peaq_rate_segment) / sizeof(uint32_t)), stream, &slot))
    return rc;
  RangeArgs a{};
  a.in_stride = in_stride;
  a.out_stride = out_stride;
  a.channels = channels;
  a.L = g.L;
  a.M = g.M;
  a.K = g.K;
  const dim3 grid((count_max + kRangeTile - 1) / kRangeTile, (unsigned)n_segments);
  hipLaunchKernelGGL(resample_range_kernel, grid, dim3(kRangeTile), 0, stream, a,
                     slot->dev.as<peaq_rate_segment>(), d_in, d_out, taps);
  HIP_TRY(hipGetLastError());
  return lens->sent(slot, stream);
}

extern "C" int peaq_batch_resample_range(peaq_ctx* c, int channels, uint32_t rate, int n_segments,
                                         const peaq_rate_segment* seg, const float* d_in, size_t in_stride, float* d_out,
                                         size_t out_stride, void* stream_) {
  const std::string who("peaq_batch_resample_range");
  // (what needs no context first)
  RateGeometry g;
  if (int rc = resample_geometry(who.c_str(), rate, &g)) return rc;
  if (int rc = check_channels(who, channels)) return rc;
  if (int rc = check_count(who, n_segments, "n_segments", "segments")) return rc;
  if (!c) return fail(PEAQ_ERR_ARG, who + ": ctx is NULL");
  if (n_segments == 0) return PEAQ_OK;
  if (!seg) return fail(PEAQ_ERR_ARG, who + ": seg is NULL");
  if (!d_in || !d_out) return fail(PEAQ_ERR_ARG, who + ": NULL buffer");
  if (g.M > kRangeRatioMax * g.L || 2 * g.K > kRangeTapsMax - 2)
    return fail(PEAQ_ERR_ARG, who + ": rate " + std::to_string(rate) + " Hz: a tile's raw span does not fit its staging");
  uint32_t count_max = 0;
  for (int i = 0; i < n_segments; ++i) {
    const peaq_rate_segment& s = seg[i];
    const std::string at = who + ": segment " + std::to_string(i);
    if (int rc = check_position(at, "out_first", s.out_first)) return rc;
    if (int rc = check_position(at, "in_base", s.in_base)) return rc;
    if (s.out_count > out_stride)
      return fail(PEAQ_ERR_ARG, at + ": out_count " + std::to_string(s.out_count) + " passes out_stride " +
                                    std::to_string(out_stride));
    if (s.in_have > in_stride)
      return fail(PEAQ_ERR_ARG, at + ": in_have " + std::to_string(s.in_have) + " passes in_stride " +
                                    std::to_string(in_stride));
    count_max = std::max(count_max, s.out_count);
    if (!s.out_count) continue;
    const bool ended = s.in_total != UINT64_MAX;
    if (ended) {
      if (int rc = check_position(at, "in_total", s.in_total)) return rc;
      const uint64_t n_out = resampled_length_u64(s.in_total, rate);
      if (s.out_first + s.out_count > n_out)
        return fail(PEAQ_ERR_ARG, at + ": outputs " + std::to_string(s.out_first) + " + " + std::to_string(s.out_count) +
                                      " pass the " + std::to_string(n_out) + " converted samples of a stream of " +
                                      std::to_string(s.in_total));
    }
    uint64_t lo, hi;
    span_of(g, s.out_first, s.out_count, &lo, &hi);
    if (ended) hi = std::min(hi, s.in_total);
    if (lo < hi && (lo < s.in_base || hi > s.in_base + s.in_have))
      return fail(PEAQ_ERR_ARG, at + ": the outputs read raw samples [" + std::to_string(lo) + ", " + std::to_string(hi) +
                                    "), the row holds [" + std::to_string(s.in_base) + ", " +
                                    std::to_string(s.in_base + s.in_have) + ")");
  }
  if (count_max == 0) return PEAQ_OK;
  return range_launch(c, channels, rate, n_segments, seg, d_in, in_stride, d_out, out_stride, count_max,
                      static_cast<hipStream_t>(stream_));
}

// (peaq_host.h) The same launch for segments the stream framer made (stage_window): they hold what their outputs read
// by construction and their rate was checked when it was set, so nothing is looked at but the strides.
int live_rate_convert(peaq_ctx* c, int channels, uint32_t rate, int n_segments, const peaq_rate_segment* seg,
                      const float* d_in, size_t in_stride, float* d_out, size_t out_stride, hipStream_t stream) {
  uint32_t count_max = 0;
  for (int i = 0; i < n_segments; ++i) {
    if (seg[i].out_count > out_stride || seg[i].in_have > in_stride)
      return fail(PEAQ_ERR_ARG, "live rate conversion: segment " + std::to_string(i) + " passes its staging");
    count_max = std::max(count_max, seg[i].out_count);
  }
  if (count_max == 0) return PEAQ_OK;
  return range_launch(c, channels, rate, n_segments, seg, d_in, in_stride, d_out, out_stride, count_max, stream);
}

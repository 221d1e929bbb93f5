// peaq_track.hip -- a pair's delay as a track: the drift stage's per-window delays kept as a knot per window and a line
// from every knot to the next (host), and the test signal's cut along them (peaq_track_fit, peaq_track_segment,
// peaq_track_index, peaq_track_lengths, peaq_batch_estimate_track, peaq_batch_cut_track, peaq_run_pair_track;
// include/peaq_amd.h).
//
//   track_cut_kernel   peaq_batch_cut_track: drift_cut_kernel's shape (peaq_drift.hip), widened.  A workgroup owns 1024
//       consecutive outputs of one pair, both channels; lane l owns outputs l + 256 j.  A window is at least 4096
//       outputs, so a tile meets at most TWO segments: the index of the knot between them and both (a, e) are uniform
//       over the workgroup, and an output selects its line by comparing its i.  m is monotone within a segment but not
//       across a knot of opposite slopes, so the smallest m of the tile is that of its first output, its last output or
//       one of the two outputs at the knot; at |e| <= 1/64 m moves by at most 17 over the tile (kTrSpread has the
//       arithmetic), and the workgroup stages 1024 + 64 + 20 samples in LDS, the channels of a sample side by side.
//       Taps come per lane from the table in device memory, as in drift_cut_kernel.  Pairs whose segments are all (0, 0)
//       take align_cut_kernel's copy (copy_run, peaq_host.h): their bits are moved.
//   No other kernel: the estimate is the drift stage's (drift_estimate, peaq_drift.hip), then host arithmetic.
#include "peaq_host.h"
#include "peaq_track_math.h"

namespace {

constexpr int kTrK = PEAQ_SUB_HALF;                    // taps each side
constexpr int kTrTaps = 2 * kTrK + 1;                  // 65
constexpr int kTrSteps = PEAQ_SUB_STEPS;               // rows of the table
constexpr int kTrTile = 1024;                          // outputs per workgroup
constexpr int kTrPer = 4;                              // ... per lane, 256 apart
// m_i - m_lo within a tile stays below this.  In grid steps of 1/256 sample, g = rint (256 (a + e i)) moves over the
// tile's outputs by at most 256 |e| per output (4096 in all at 1/64), one more for each of the two roundings at the
// tile's ends, and across a knot by the step between the lines (at most one, PEAQ_TRACK_MAX_STEP) and two more
// roundings: 4096 + 8 at the outside.  m = floor ((g + 128) / 256) then moves by at most 4104 / 256 + 1 = 17.
constexpr int kTrSpread = 20;
constexpr int kTrStage = kTrTile + 2 * kTrK + kTrSpread;   // staged samples
static_assert(kTrTile == 256 * kTrPer, "a lane's share");
static_assert(kTrSteps == 256, "peaq_drift_index: 256 phases per sample");
static_assert(PEAQ_DRIFT_MIN_WINDOW > kTrTile, "a tile meets at most two segments");
static_assert(kTrTile * PEAQ_TRACK_MAX_E * kTrSteps + PEAQ_TRACK_MAX_STEP * kTrSteps + 7 < (kTrSpread - 2) * kTrSteps,
              "the spread of m over a tile");

struct TrackArgs {
  size_t in_stride, out_stride; // samples per channel between pairs
  const uint32_t* n_in;         // device [n_pairs]
  const uint32_t* skip;
  const uint32_t* n_keep;
  const uint32_t* n_seg;        // 0: every segment of the pair is (0, 0), its bits are moved
  const uint32_t* seg_off;      // the pair's first segment in a and e
  const double* a;              // device [sum of n_seg]
  const double* e;
  uint32_t window;
  int channels;
};

template <int C>
__device__ __forceinline__ void tr_cut(const TrackArgs& args, const float* __restrict__ in, float* __restrict__ out,
                                       const double* __restrict__ tab, float* lds, uint32_t n_seg) {
  const unsigned pair = blockIdx.y;
  const long long n_in = args.n_in[pair], n_keep = args.n_keep[pair];
  const long long i0 = (long long)blockIdx.x * kTrTile;            // the tile's first output (below n_keep)
  const long long i_last = min(i0 + kTrTile, n_keep) - 1;          // ... and its last
  // ---- the tile's segments (uniform): k0 that of i0; outputs from `knot` on belong to k0 + 1 ----
  const long long k0 = track_segment(i0, args.window, n_seg);
  const double* __restrict__ sa = args.a + args.seg_off[pair];
  const double* __restrict__ se = args.e + args.seg_off[pair];
  const double a0 = sa[k0], e0 = se[k0];
  double a1 = a0, e1 = e0;
  long long knot = i_last + 1;                                     // (no knot inside the tile)
  if (k0 + 1 < (long long)n_seg) {
    const long long next = (long long)(args.window / 2) + (k0 + 1) * (long long)args.window;
    if (next <= i_last) {
      knot = next;
      a1 = sa[k0 + 1];
      e1 = se[k0 + 1];
    }
  }
  long long m_a, m_b;
  int phi;
  drift_index(a0, e0, i0, &m_a, &phi);
  drift_index(knot <= i_last ? a1 : a0, knot <= i_last ? e1 : e0, i_last, &m_b, &phi);
  long long m_lo = min(m_a, m_b);
  if (knot <= i_last) {                                            // (knot > i0: the knot's segment is not i0's)
    drift_index(a0, e0, knot - 1, &m_a, &phi);
    drift_index(a1, e1, knot, &m_b, &phi);
    m_lo = min(m_lo, min(m_a, m_b));
  }
  const long long s0 = (long long)args.skip[pair] + i0 + m_lo - kTrK;   // input sample under staged position 0
  const float* __restrict__ src = in + (size_t)pair * args.in_stride * C;
  // ---- stage: consecutive lanes read consecutive floats; staged sample v, channel c at lds[C v + c] ----
  for (int f = threadIdx.x; f < kTrStage * C; f += 256) {
    const long long s = s0 + (C == 2 ? f >> 1 : f);
    lds[f] = (s >= 0 && s < n_in) ? src[(size_t)s * C + (C == 2 ? f & 1 : 0)] : 0.f;
  }
  __syncthreads();
  // ---- output j of the lane: i = i0 + l + 256 j; tap o of it meets staged position l + 256 j + (m_i - m_lo) + o ----
  const double* __restrict__ row[kTrPer];
  const float* x[kTrPer];
#pragma unroll
  for (int j = 0; j < kTrPer; ++j) {
    const long long i = min(i0 + (long long)threadIdx.x + 256 * j, i_last);   // (an output past n_keep: computed, not stored)
    const bool second = i >= knot;
    long long m;
    drift_index(second ? a1 : a0, second ? e1 : e0, i, &m, &phi);
    const int dm = max(0, min((int)(m - m_lo), kTrSpread - 1));    // (0 .. 17 by the bounds above: the clamp never acts)
    row[j] = tab + (size_t)(phi + kTrSteps / 2) * kTrTaps;
    x[j] = lds + C * ((int)(i - i0) + dm);
  }
  double acc[C][kTrPer];
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int j = 0; j < kTrPer; ++j) acc[c][j] = 0.;
#pragma unroll 5
  for (int o = 0; o < kTrTaps; ++o) {                              // o = -32 .. 32 of the definition, in that order
#pragma unroll
    for (int j = 0; j < kTrPer; ++j) {
      const double h = row[j][o];
      if (C == 2) {
        const float2 v = *reinterpret_cast<const float2*>(x[j] + 2 * o);
        acc[0][j] = __builtin_fma(h, (double)v.x, acc[0][j]);
        acc[C - 1][j] = __builtin_fma(h, (double)v.y, acc[C - 1][j]);
      } else {
        acc[0][j] = __builtin_fma(h, (double)x[j][o], acc[0][j]);
      }
    }
  }
  // ---- consecutive lanes store consecutive samples ----
  float* __restrict__ dst = out + (size_t)pair * args.out_stride * C;
  const bool pairs8 = C == 2 && ((uintptr_t)dst & 7) == 0;         // (uniform) both channels in one store
#pragma unroll
  for (int j = 0; j < kTrPer; ++j) {
    const long long i = i0 + (long long)threadIdx.x + 256 * j;
    if (i >= n_keep) continue;
    if (pairs8) {
      reinterpret_cast<float2*>(dst)[i] = {(float)acc[0][j], (float)acc[C - 1][j]};
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) dst[(size_t)i * C + c] = (float)acc[c][j];
    }
  }
}

// (the buffers and the table as parameters of their own, as drift_cut_kernel's)
__global__ __launch_bounds__(256, 4) void track_cut_kernel(const TrackArgs args, const float* __restrict__ a_in,
                                                        float* __restrict__ a_out, const double* __restrict__ shift_tab) {
  __shared__ __attribute__((aligned(16))) float lds[2 * kTrStage];
  const unsigned pair = blockIdx.y;
  const uint32_t n_keep = args.n_keep[pair];
  if ((unsigned long long)blockIdx.x * kTrTile >= n_keep) return;  // (the whole workgroup)
  const uint32_t n_seg = args.n_seg[pair];
  if (n_seg == 0) {                                    // (uniform) peaq_batch_cut's copy of this tile's floats
    const size_t count = (size_t)n_keep * args.channels;
    const float* __restrict__ src = a_in + ((size_t)pair * args.in_stride + args.skip[pair]) * args.channels;
    float* __restrict__ dst = a_out + (size_t)pair * args.out_stride * args.channels;
    for (int sub = 0; sub < args.channels; ++sub)      // a tile is `channels` units of 256 x 4 floats
      copy_run(src, dst, count, ((size_t)blockIdx.x * args.channels + sub) * 256, blockIdx.x == 0 && sub == 0, CopyBits());
    return;
  }
  if (args.channels == 2)
    tr_cut<2>(args, a_in, a_out, shift_tab, lds, n_seg);
  else
    tr_cut<1>(args, a_in, a_out, shift_tab, lds, n_seg);
}

#pragma clang fp contract(off)                        // host arithmetic from here on: every operation rounded on its own

int check_track_window(const std::string& w, uint32_t window) {
  if (window < PEAQ_DRIFT_MIN_WINDOW || window > PEAQ_DRIFT_MAX_WINDOW)
    return fail(PEAQ_ERR_ARG, w + ": window " + std::to_string(window) + " is outside 4096 .. 1048576");
  return PEAQ_OK;
}
int check_track_max_e(const std::string& w, double max_e) {
  if (!(max_e > 0. && max_e <= PEAQ_TRACK_MAX_E))
    return fail(PEAQ_ERR_ARG, w + ": max_e " + std::to_string(max_e) + " is outside (0, 0.015625]");
  return PEAQ_OK;
}

// the record of one pair from its windows' records: the drift stage's d_w and validity, then the fit
void track_record(int32_t lag0, uint32_t W, const peaq_delay* dl, const peaq_subdelay* sb, uint32_t window, double min_corr,
                  double max_e, peaq_track* out, double* knots, double* a, double* e) {
  std::vector<double> d(W);
  std::vector<uint8_t> valid(W);
  for (uint32_t w = 0; w < W; ++w) {
    d[w] = (double)dl[w].lag + (double)sb[w].q / 256.;
    valid[w] = std::isfinite(dl[w].norm) && dl[w].norm > 0. && sb[w].flags == 0 &&
               std::fabs(dl[w].peak) >= min_corr * dl[w].norm;
  }
  TrackSummary s;
  track_fit(d.data(), valid.data(), W, window, max_e, knots, a, e, &s);
  peaq_track r;
  std::memset(&r, 0, sizeof r);
  r.lag0 = lag0;
  r.flags = s.flags;
  r.n_windows = W;
  r.n_valid = s.n_valid;
  r.n_filled = s.n_filled;
  r.n_segments = s.n_segments;
  r.d_min = s.d_min;
  r.d_max = s.d_max;
  r.max_abs_e = s.max_abs_e;
  *out = r;
}

}  // namespace

static_assert(kTrackNone == PEAQ_TRACK_F_NONE && kTrackRange == PEAQ_TRACK_F_RANGE, "peaq_track_math.h's flags");

extern "C" size_t peaq_track_size(void) { return sizeof(peaq_track); }

extern "C" int peaq_track_fit(const double* d, const uint8_t* valid, uint32_t n_windows, uint32_t window, double max_e,
                              peaq_track* out, double* knots, double* a, double* e) {
  const std::string w("peaq_track_fit");
  if (!out || !a || !e) return fail(PEAQ_ERR_ARG, w + ": out, a or e is NULL");
  if (n_windows && (!d || !knots)) return fail(PEAQ_ERR_ARG, w + ": d or knots is NULL");
  if (int rc = check_track_window(w, window)) return rc;
  if (n_windows > PEAQ_DRIFT_MAX_WINDOWS)
    return fail(PEAQ_ERR_ARG, w + ": " + std::to_string(n_windows) + " windows are more than " + std::to_string(PEAQ_DRIFT_MAX_WINDOWS));
  if (int rc = check_track_max_e(w, max_e)) return rc;
  TrackSummary s;
  track_fit(d, valid, n_windows, window, max_e, knots, a, e, &s);
  std::memset(out, 0, sizeof *out);
  out->flags = s.flags;
  out->n_windows = n_windows;
  out->n_valid = s.n_valid;
  out->n_filled = s.n_filled;
  out->n_segments = s.n_segments;
  out->d_min = s.d_min;
  out->d_max = s.d_max;
  out->max_abs_e = s.max_abs_e;
  return PEAQ_OK;
}

extern "C" uint32_t peaq_track_segment(int64_t i, uint32_t window, uint32_t n_seg) {
  if (!n_seg || !window) return 0;
  return (uint32_t)track_segment(i, window, n_seg);
}

extern "C" void peaq_track_index(uint32_t window, uint32_t n_seg, const double* a, const double* e, int64_t i, int64_t* m,
                                 int32_t* phi) {
  long long mm = 0;
  int pp = 0;
  if (n_seg && window && a && e) track_index(window, n_seg, a, e, i, &mm, &pp);
  if (m) *m = mm;
  if (phi) *phi = pp;
}

extern "C" void peaq_track_lengths(int32_t lag0, uint32_t window, uint32_t n_seg, const double* a, const double* e,
                                   uint32_t n_ref, uint32_t n_test, uint32_t* skip_ref, uint32_t* skip_test,
                                   uint32_t* n_keep) {
  uint32_t sr, st, common;
  peaq_aligned_lengths(lag0, n_ref, n_test, &sr, &st, &common);
  if (skip_ref) *skip_ref = sr;
  if (skip_test) *skip_test = st;
  if (!n_keep) return;
  const double zero = 0.;
  const bool none = !n_seg || !window || !a || !e;     // (no track: the plain cut's lengths)
  *n_keep = track_keep(none ? 1 : window, none ? 1 : n_seg, none ? &zero : a, none ? &zero : e, st, common, n_test);
}

extern "C" int peaq_batch_estimate_track(peaq_ctx* c, int channels, int n_pairs, const float* d_ref, const float* d_test,
                                         size_t pair_stride, const uint32_t* n_ref, const uint32_t* n_test,
                                         uint32_t n_uniform, const int32_t* lag0, uint32_t window, uint32_t R,
                                         double min_corr, double max_e, uint32_t w_max, peaq_delay* d_win_delay,
                                         peaq_subdelay* d_win_sub, peaq_drift* drift, peaq_track* out, double* knots,
                                         uint32_t seg_stride, double* a, double* e, void* stream_) {
  const std::string w("peaq_batch_estimate_track");
  if (int rc = check_track_max_e(w, max_e)) return rc;
  if (seg_stride < 1 || (uint64_t)seg_stride + 1 < w_max)
    return fail(PEAQ_ERR_ARG, w + ": seg_stride " + std::to_string(seg_stride) + " is below max (w_max - 1, 1) for w_max " +
                                  std::to_string(w_max));
  if (n_pairs > 0 && (!out || !knots || !a || !e)) return fail(PEAQ_ERR_ARG, w + ": NULL out, knots, a or e");
  const size_t np = (size_t)std::max(n_pairs, 0);
  std::vector<peaq_drift> line(drift ? 0 : std::min<size_t>(np, 65535));
  if (!drift) drift = line.data();
  if (int rc = drift_estimate(w, c, channels, n_pairs, d_ref, d_test, pair_stride, n_ref, n_test, n_uniform, lag0, window, R,
                              min_corr, PEAQ_DRIFT_MAX_E, w_max, d_win_delay, d_win_sub, np ? drift : nullptr, stream_))
    return rc;
  if (n_pairs == 0) return PEAQ_OK;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIP_TRY(hipSetDevice(c->device));
  std::vector<peaq_delay> dl(np * w_max);
  std::vector<peaq_subdelay> sb(np * w_max);
  HIP_TRY(hipMemcpyAsync(dl.data(), d_win_delay, dl.size() * sizeof(peaq_delay), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipMemcpyAsync(sb.data(), d_win_sub, sb.size() * sizeof(peaq_subdelay), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  for (size_t p = 0; p < np; ++p) {
    const uint32_t W = drift[p].n_windows;             // (at most w_max: the drift estimate has looked)
    double* kn = knots + p * w_max;
    double* pa = a + p * seg_stride;
    double* pe = e + p * seg_stride;
    std::fill(kn, kn + w_max, 0.);
    std::fill(pa, pa + seg_stride, 0.);
    std::fill(pe, pe + seg_stride, 0.);
    track_record(lag0[p], W, &dl[p * w_max], &sb[p * w_max], window, min_corr, max_e, &out[p], kn, pa, pe);
  }
  return PEAQ_OK;
}

extern "C" int peaq_batch_cut_track(peaq_ctx* c, int channels, int n_pairs, const float* d_in, size_t in_stride,
                                    const uint32_t* n_in, const uint32_t* skip, const uint32_t* n_keep, uint32_t window,
                                    const uint32_t* n_seg, uint32_t seg_stride, const double* a, const double* e,
                                    float* d_out, size_t out_stride, void* stream_) {
  const std::string w("peaq_batch_cut_track");
  if (int rc = check_shape(w, channels, n_pairs)) return rc;
  if (n_pairs > 0 && (!n_in || !skip || !n_keep || !n_seg || !a || !e))
    return fail(PEAQ_ERR_ARG, w + ": NULL n_in, skip, n_keep, n_seg, a or e");
  uint32_t keep_max = 0;
  if (int rc = check_cut_geometry(w, "pair", channels, n_pairs, n_pairs, d_in, in_stride, skip, n_keep, d_out, out_stride,
                                  &keep_max))
    return rc;
  if (int rc = check_lengths(w, n_pairs, n_in, 0, "n_in", in_stride, "in_stride")) return rc;
  if (int rc = check_track_window(w, window)) return rc;
  const size_t np = (size_t)std::max(n_pairs, 0);
  uint64_t total = 0;
  for (size_t p = 0; p < np; ++p) {
    if (n_seg[p] < 1 || n_seg[p] > seg_stride)
      return fail(PEAQ_ERR_ARG, w + ": pair " + std::to_string(p) + ": n_seg " + std::to_string(n_seg[p]) + " is outside 1 .. seg_stride " +
                                    std::to_string(seg_stride));
    total += n_seg[p];
  }
  if (total > PEAQ_TRACK_MAX_SEGMENTS_PER_CALL)
    return fail(PEAQ_ERR_ARG, w + ": " + std::to_string(total) + " segments are more than " +
                                  std::to_string(PEAQ_TRACK_MAX_SEGMENTS_PER_CALL) + " in one call");
  const size_t words = 5 * np + (np & 1);              // the doubles behind them start on 8 bytes
  std::vector<uint32_t> h(words + 4 * (size_t)total);
  size_t off = 0;
  for (size_t p = 0; p < np; ++p) {
    const double* pa = a + p * seg_stride;
    const double* pe = e + p * seg_stride;
    bool plain = true;
    for (uint32_t k = 0; k < n_seg[p]; ++k) {
      const std::string where = w + ": pair " + std::to_string(p) + ", segment " + std::to_string(k);
      if (!(std::fabs(pa[k]) <= PEAQ_DRIFT_MAX_A))
        return fail(PEAQ_ERR_ARG, where + ": a " + std::to_string(pa[k]) + " is outside -1048576 .. 1048576");
      if (!(std::fabs(pe[k]) <= PEAQ_TRACK_MAX_E))
        return fail(PEAQ_ERR_ARG, where + ": e " + std::to_string(pe[k]) + " is outside -0.015625 .. 0.015625");
      if (k && !(track_step(window, pa, pe, k - 1) <= PEAQ_TRACK_MAX_STEP))
        return fail(PEAQ_ERR_ARG, where + ": a step of " + std::to_string(track_step(window, pa, pe, k - 1)) +
                                      " samples from the segment before it is more than 0.00390625");
      plain = plain && pa[k] == 0. && pe[k] == 0.;
      std::memcpy(&h[words + 2 * (off + k)], &pa[k], sizeof(double));
      std::memcpy(&h[words + 2 * (size_t)total + 2 * (off + k)], &pe[k], sizeof(double));
    }
    h[p] = n_in[p];
    h[np + p] = skip[p];
    h[2 * np + p] = n_keep[p];
    h[3 * np + p] = plain ? 0 : n_seg[p];
    h[4 * np + p] = (uint32_t)off;
    off += n_seg[p];
  }
  if (!c) return fail(PEAQ_ERR_ARG, w + ": ctx is NULL");
  if (n_pairs == 0 || keep_max == 0) return PEAQ_OK;

  hipStream_t stream = static_cast<hipStream_t>(stream_);
  std::lock_guard<std::mutex> lock(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  const double* tab = nullptr;
  LenStage* lens = nullptr;
  if (int rc = frac_shift_table(c, &tab, &lens)) return rc;
  LenSlot* slot = nullptr;
  if (int rc = lens->upload(h.data(), h.size(), stream, &slot)) return rc;
  TrackArgs args{};
  args.in_stride = in_stride;
  args.out_stride = out_stride;
  args.n_in = slot->dev.as<uint32_t>();
  args.skip = args.n_in + np;
  args.n_keep = args.skip + np;
  args.n_seg = args.n_keep + np;
  args.seg_off = args.n_seg + np;
  args.a = reinterpret_cast<const double*>(args.n_in + words);
  args.e = args.a + total;
  args.window = window;
  args.channels = channels;
  const unsigned tiles = (unsigned)(((uint64_t)keep_max + kTrTile - 1) / kTrTile);
  hipLaunchKernelGGL(track_cut_kernel, dim3(tiles, (unsigned)n_pairs), dim3(256), 0, stream, args, d_in, d_out, tab);
  const hipError_t launched = hipGetLastError();
  const int sent = lens->sent(slot, stream);           // (also after a failed launch: the copy into the slot is enqueued)
  HIP_TRY(launched);
  return sent;
}

extern "C" int peaq_run_pair_track(peaq_ctx* c, int advanced, int channels, double level_db, uint32_t rate, uint32_t max_lag,
                                   uint32_t window, int mode, double max_gain_db, const float* ref, size_t n_ref,
                                   const float* test, size_t n_test, peaq_delay* delay, peaq_track* track, peaq_gain* gain,
                                   peaq_result* out) {
  const std::string w("peaq_run_pair_track");
  if (int rc = check_track_window(w, window)) return rc;
  const uint32_t R = std::min<uint32_t>(window / 4, 1024);
  if (int rc = check_gain_mode(w, mode, max_gain_db)) return rc;
  if (int rc = check_max_lag(w, max_lag)) return rc;
  if (int rc = check_level(w, level_db)) return rc;
  if (int rc = check_pair_args(w, c, channels, rate, ref, n_ref, test, n_test, out, true)) return rc;
  if (gain) std::memset(gain, 0, sizeof *gain);
  const bool match = (mode & 0xF) != PEAQ_GAIN_OFF;
  // 1, 2: upload, rate conversion
  PairBuffers in;
  if (int rc = upload_pair_48k(c, channels, rate, ref, n_ref, test, n_test, in)) return rc;
  const uint32_t* len = in.len;
  const size_t stride = in.stride;
  // 3, 4: estimate, the track
  DevBuf cut[2], matched, d_dl, d_sb, d_gain;
  peaq_delay rec;
  if (int rc = estimate_one_delay(c, channels, in, max_lag, &rec)) return rc;
  if (delay) *delay = rec;
  const uint32_t W = peaq_drift_windows(rec.lag, len[0], len[1], window);
  if (W > PEAQ_DRIFT_MAX_WINDOWS)
    return fail(PEAQ_ERR_ARG, w + ": " + std::to_string(W) + " windows of " + std::to_string(window) + " samples are more than " +
                                  std::to_string(PEAQ_DRIFT_MAX_WINDOWS) + ": take a longer window");
  uint32_t n_seg = std::max<uint32_t>(W, 2) - 1;
  std::vector<double> knots(std::max<uint32_t>(W, 1)), sa(n_seg, 0.), se(n_seg, 0.);
  peaq_track tr;
  std::memset(&tr, 0, sizeof tr);
  tr.lag0 = rec.lag;
  tr.flags = PEAQ_TRACK_F_NONE;
  tr.n_segments = n_seg;
  if (W >= 1) {                                        // (none: no track whatever)
    HIP_TRY(d_dl.reserve((size_t)W * sizeof(peaq_delay)));
    HIP_TRY(d_sb.reserve((size_t)W * sizeof(peaq_subdelay)));
    if (int rc = peaq_batch_estimate_track(c, channels, 1, in.d(0), in.d(1), stride, len, len + 1, 0, &rec.lag, window, R, 0.5,
                                           PEAQ_TRACK_MAX_E, W, d_dl.as<peaq_delay>(), d_sb.as<peaq_subdelay>(), nullptr, &tr,
                                           knots.data(), n_seg, sa.data(), se.data(), nullptr))
      return rc;
  }
  if (track) *track = tr;
  // 5, 6: plain cut of the reference, track cut of the test signal
  uint32_t skip[2], keep = 0;
  peaq_track_lengths(rec.lag, window, n_seg, sa.data(), se.data(), len[0], len[1], &skip[0], &skip[1], &keep);
  size_t cstride = std::max<size_t>(keep, 2);
  cstride += cstride & 1;
  const size_t cbytes = cstride * channels * sizeof(float);
  for (int i = 0; i < 2; ++i) {
    HIP_TRY(cut[i].reserve(cbytes));
    HIP_TRY(hipMemset(cut[i].p, 0, cbytes));
  }
  if (int rc = peaq_batch_cut(c, channels, 1, in.d(0), stride, &skip[0], &keep, cut[0].as<float>(), cstride, nullptr)) return rc;
  if (int rc = peaq_batch_cut_track(c, channels, 1, in.d(1), stride, &len[1], &skip[1], &keep, window, &n_seg, n_seg, sa.data(),
                                    se.data(), cut[1].as<float>(), cstride, nullptr))
    return rc;
  const float* scored = cut[1].as<float>();
  // 7: the gain of the RESAMPLED test signal, applied into a second buffer
  if (match) {
    const uint32_t zero = 0;
    HIP_TRY(d_gain.reserve(sizeof(peaq_gain)));
    HIP_TRY(matched.reserve(cbytes));
    HIP_TRY(hipMemset(matched.p, 0, cbytes));
    if (int rc = peaq_batch_measure_gain(c, channels, 1, cut[0].as<float>(), cstride, &zero, cut[1].as<float>(), cstride, &zero,
                                         &keep, mode, max_gain_db, d_gain.as<peaq_gain>(), nullptr))
      return rc;
    if (int rc = peaq_batch_cut_scaled(c, channels, 1, cut[1].as<float>(), cstride, &zero, &keep, d_gain.as<peaq_gain>(),
                                       matched.as<float>(), cstride, nullptr))
      return rc;
    scored = matched.as<float>();
  }
  HIP_TRY(hipDeviceSynchronize());
  if (match && gain) HIP_TRY(hipMemcpy(gain, d_gain.p, sizeof(peaq_gain), hipMemcpyDeviceToHost));
  // 8: the one-pair path
  return score_one_pair(c, advanced, channels, level_db, cut[0].as<float>(), scored, cstride, keep, keep, out);
}

// peaq_track.hip -- a pair's delay as a track: the drift stage's per-window delays kept as a knot per window and a line
// from every knot to the next (host), and the test signal's cut along them (peaq_track_fit, peaq_track_segment,
// peaq_track_index, peaq_track_lengths, peaq_batch_estimate_track, peaq_batch_cut_track, peaq_run_pair_track;
// include/peaq_amd.h).
//
//   track_cut_kernel   peaq_batch_cut_track: a workgroup owns 1024 consecutive outputs of one pair, both channels, and
//       makes them in ONE pass of the cuts' shared body (delay_cut_pass, peaq_delay_cut.h) whose outputs choose between
//       two lines.  A window is at least 4096 outputs, so a tile meets at most TWO segments: the index of the knot
//       between them and both (a, e) are uniform over the workgroup, and an output selects its line by comparing its i.
//       m is monotone within a segment but not across a knot of opposite slopes, so the smallest m of the tile is that
//       of its first output, its last output or one of the two outputs at the knot; at |e| <= 1/64 m moves by at most 17
//       over the tile (kTrSpread has the arithmetic): 1024 + 64 + 20 staged samples.  Pairs whose segments are all
//       (0, 0) take align_cut_kernel's copy (cut_tile_copied): their bits are moved.
//   No other kernel: the estimate is the drift stage's (drift_estimate, peaq_drift.hip), then host arithmetic.
#include "peaq_host.h"
#include "peaq_track_math.h"
#include "peaq_delay_cut.h"   // (behind the arithmetic: its pass is rounded as that is)

namespace {

// m_i - m_lo within a tile stays below this.  In grid steps of 1/256 sample, g = rint (256 (a + e i)) moves over the
// tile's outputs by at most 256 |e| per output (4096 in all at 1/64), one more for each of the two roundings at the
// tile's ends, and across a knot by the step between the lines (at most one, PEAQ_TRACK_MAX_STEP) and two more
// roundings: 4096 + 8 at the outside.  m = floor ((g + 128) / 256) then moves by at most 4104 / 256 + 1 = 17.
constexpr int kTrSpread = 20;
constexpr int kTrStage = delay_cut_stage(kTrSpread);   // staged samples
static_assert(PEAQ_DRIFT_MIN_WINDOW > kCutTile, "a tile meets at most two segments");
static_assert(kCutTile * PEAQ_TRACK_MAX_E * kCutSteps + PEAQ_TRACK_MAX_STEP * kCutSteps + 7 < (kTrSpread - 2) * kCutSteps,
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
  const long long i0 = (long long)blockIdx.x * kCutTile;           // the tile's first output (below n_keep)
  const long long i_last = min(i0 + kCutTile, n_keep) - 1;         // ... and its last
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
  const float* __restrict__ src = in + (size_t)pair * args.in_stride * C;
  float* __restrict__ dst = out + (size_t)pair * args.out_stride * C;
  const bool pairs8 = C == 2 && ((uintptr_t)dst & 7) == 0;         // (uniform) both channels in one store
  delay_cut_pass<C, kTrSpread, false>(src, dst, pairs8, n_in, args.skip[pair], i0, i0, i_last, m_lo, kTrStage,
                                      [=](long long i, long long* m, int* ph) {
                                        const bool second = i >= knot;
                                        drift_index(second ? a1 : a0, second ? e1 : e0, i, m, ph);
                                      },
                                      tab, lds);
}

// (the buffers and the table as parameters of their own, as drift_cut_kernel's)
__global__ __launch_bounds__(256, 4) void track_cut_kernel(const TrackArgs args, const float* __restrict__ a_in,
                                                        float* __restrict__ a_out, const double* __restrict__ shift_tab) {
  __shared__ __attribute__((aligned(16))) float lds[2 * kTrStage];
  const unsigned pair = blockIdx.y;
  const uint32_t n_seg = args.n_seg[pair];
  if (cut_tile_copied(a_in, a_out, args.in_stride, args.out_stride, args.skip, args.n_keep[pair], args.channels, n_seg == 0))
    return;
  if (args.channels == 2)
    tr_cut<2>(args, a_in, a_out, shift_tab, lds, n_seg);
  else
    tr_cut<1>(args, a_in, a_out, shift_tab, lds, n_seg);
}

#pragma clang fp contract(off)                        // host arithmetic from here on: every operation rounded on its own

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
  window_delays(dl, sb, W, min_corr, d.data(), valid.data());
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
  if (int rc = check_delay_window(w, window)) return rc;
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
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  DelayCutCall k{w, c, channels, n_pairs, d_in, in_stride, n_in, skip, n_keep, d_out, out_stride, stream};
  if (int rc = k.check(n_seg && a && e, ", n_seg, a or e")) return rc;
  if (int rc = check_delay_window(w, window)) return rc;
  uint64_t total = 0;
  for (size_t p = 0; p < k.np; ++p) {
    if (n_seg[p] < 1 || n_seg[p] > seg_stride)
      return fail(PEAQ_ERR_ARG, w + ": pair " + std::to_string(p) + ": n_seg " + std::to_string(n_seg[p]) + " is outside 1 .. seg_stride " +
                                    std::to_string(seg_stride));
    total += n_seg[p];
  }
  if (total > PEAQ_TRACK_MAX_SEGMENTS_PER_CALL)
    return fail(PEAQ_ERR_ARG, w + ": " + std::to_string(total) + " segments are more than " +
                                  std::to_string(PEAQ_TRACK_MAX_SEGMENTS_PER_CALL) + " in one call");
  k.pack(5, (size_t)total, false);
  for (size_t p = 0; p < k.np; ++p) {
    const double* pa = a + p * seg_stride;
    const double* pe = e + p * seg_stride;
    const size_t first = k.next_line;
    bool plain;
    if (int rc = k.add_lines(p, "segment", n_seg[p], pa, pe, nullptr, PEAQ_TRACK_MAX_E, "-0.015625 .. 0.015625", &plain,
                             [&](uint32_t s, const auto& where) {
                               if (s && !(track_step(window, pa, pe, s - 1) <= PEAQ_TRACK_MAX_STEP))
                                 return fail(PEAQ_ERR_ARG, where() + ": a step of " + std::to_string(track_step(window, pa, pe, s - 1)) +
                                                               " samples from the segment before it is more than 0.00390625");
                               return (int)PEAQ_OK;
                             }))
      return rc;
    k.col(3, p) = plain ? 0 : n_seg[p];                // (0: every segment is (0, 0), the pair's bits are moved)
    k.col(4, p) = (uint32_t)first;
  }
  if (int rc = k.upload()) return rc;
  if (!k.slot) return PEAQ_OK;
  TrackArgs args{};
  args.in_stride = in_stride;
  args.out_stride = out_stride;
  args.n_in = k.dev_col(0);
  args.skip = k.dev_col(1);
  args.n_keep = k.dev_col(2);
  args.n_seg = k.dev_col(3);
  args.seg_off = k.dev_col(4);
  args.a = k.dev_a();
  args.e = k.dev_e();
  args.window = window;
  args.channels = channels;
  hipLaunchKernelGGL(track_cut_kernel, dim3(k.tiles(), (unsigned)n_pairs), dim3(256), 0, stream, args, d_in, d_out, k.tab);
  return k.launched();
}

extern "C" int peaq_run_pair_track(peaq_ctx* c, int advanced, int channels, double level_db, uint32_t rate, uint32_t max_lag,
                                   uint32_t window, int mode, double max_gain_db, const float* ref, size_t n_ref,
                                   const float* test, size_t n_test, peaq_delay* delay, peaq_track* track, peaq_gain* gain,
                                   peaq_result* out) {
  const std::string w("peaq_run_pair_track");
  if (int rc = check_delay_window(w, window)) return rc;
  const uint32_t R = std::min<uint32_t>(window / 4, 1024);
  // 1 .. 3: upload, rate conversion, estimate
  PairBuffers in;
  peaq_delay rec;
  uint32_t W = 0;
  if (int rc = begin_delay_pair(w, c, channels, level_db, rate, max_lag, window, mode, max_gain_db, ref, n_ref, test, n_test,
                                delay, gain, out, in, &rec, &W))
    return rc;
  const uint32_t* len = in.len;
  const size_t stride = in.stride;
  // 4: the track
  DevBuf d_dl, d_sb;
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
  // 5 .. 8: both signals cut to the track's lengths, the test signal along the track; the gain; the score
  uint32_t skip[2], keep = 0;
  peaq_track_lengths(rec.lag, window, n_seg, sa.data(), se.data(), len[0], len[1], &skip[0], &skip[1], &keep);
  return score_cut_pair(c, advanced, channels, level_db, in, skip, keep, mode, max_gain_db, gain,
                        [&](float* d_out, size_t out_stride) {
                          return peaq_batch_cut_track(c, channels, 1, in.d(1), stride, &len[1], &skip[1], &keep, window, &n_seg,
                                                      n_seg, sa.data(), se.data(), d_out, out_stride, nullptr);
                        },
                        out);
}

// peaq_drift.hip -- a pair's delay as one straight line a + e i: per-window delays through the aligner and the sub-sample
// stage, the robust fit on the host, and the test signal's cut along the line (peaq_drift_fit, peaq_drift_index,
// peaq_drift_lengths, peaq_batch_estimate_drift, peaq_batch_cut_drift, peaq_run_pair_drift; include/peaq_amd.h,
// DESIGN.md 17).
//
//   drift_cut_kernel   peaq_batch_cut_drift: a workgroup owns 1024 consecutive outputs of one pair, both channels, and
//       makes them in ONE pass of the cuts' shared body (delay_cut_pass, peaq_delay_cut.h: the staging, the taps per
//       lane, the 65-tap FP64 sum) along the pair's one line.  The outputs of a tile read the input from i0 + m_lo - 32
//       on, m_lo the smaller of the tile's first and last m (m is monotone in i and moves by at most 2 over 1024 outputs
//       at |e| <= 1e-3): 1024 + 64 + 4 staged samples.  The phase stepping every 1 / (256 |e|) outputs, neighbouring
//       lanes mostly read the same tap row.  Pairs with a == 0 and e == 0 take align_cut_kernel's copy
//       (cut_tile_copied): their bits are moved.
//   No other kernel: the estimate runs the aligner's and the sub-sample stage's kernels on copies of the windows
//   (peaq_batch_gather, peaq_batch_estimate_delay, peaq_batch_refine_delay).
#include "peaq_host.h"
#include "peaq_drift_math.h"
#include "peaq_delay_cut.h"   // (behind the arithmetic: its pass is rounded as that is)

namespace {

constexpr int kDrSpread = 4;                           // m_i - m_lo within a tile stays below this (2 at |e| = 1e-3)
constexpr int kDrStage = delay_cut_stage(kDrSpread);   // staged samples
constexpr size_t kDrStagingBudget = (size_t)1 << 30;   // estimate: pairs are taken in groups whose window copies stay below this
static_assert(kCutTile * PEAQ_DRIFT_MAX_E * kCutSteps + 2 < (kDrSpread - 1) * kCutSteps, "the spread of m over a tile");

struct DriftArgs {
  size_t in_stride, out_stride; // samples per channel between pairs
  const uint32_t* n_in;         // device [n_pairs]
  const uint32_t* skip;
  const uint32_t* n_keep;
  const double* a;
  const double* e;
  int channels;
};

template <int C>
__device__ __forceinline__ void dr_cut(const DriftArgs& args, const float* __restrict__ in, float* __restrict__ out,
                                       const double* __restrict__ tab, float* lds, double a, double e) {
  const unsigned pair = blockIdx.y;
  const long long n_in = args.n_in[pair], n_keep = args.n_keep[pair];
  const long long i0 = (long long)blockIdx.x * kCutTile;           // the tile's first output (below n_keep)
  const long long i_last = min(i0 + kCutTile, n_keep) - 1;         // ... and its last
  long long m_a, m_b;
  int phi;
  drift_index(a, e, i0, &m_a, &phi);
  drift_index(a, e, i_last, &m_b, &phi);
  const long long m_lo = min(m_a, m_b);   // (named HERE, ahead of the row pointers: as an argument expression behind them
                                          //  the compiler keeps more loads in flight, 114 registers instead of 103)
  const float* __restrict__ src = in + (size_t)pair * args.in_stride * C;
  float* __restrict__ dst = out + (size_t)pair * args.out_stride * C;
  const bool pairs8 = C == 2 && ((uintptr_t)dst & 7) == 0;         // (uniform) both channels in one store
  delay_cut_pass<C, kDrSpread, false>(src, dst, pairs8, n_in, args.skip[pair], i0, i0, i_last, m_lo, kDrStage,
                                      [=](long long i, long long* m, int* ph) { drift_index(a, e, i, m, ph); },
                                      tab, lds);
}

// (the buffers and the table as parameters of their own, as frac_cut_kernel's)
__global__ __launch_bounds__(256, 4) void drift_cut_kernel(const DriftArgs args, const float* __restrict__ a_in,
                                                        float* __restrict__ a_out, const double* __restrict__ shift_tab) {
  __shared__ __attribute__((aligned(16))) float lds[2 * kDrStage];
  const unsigned pair = blockIdx.y;
  const double a = args.a[pair], e = args.e[pair];
  if (cut_tile_copied(a_in, a_out, args.in_stride, args.out_stride, args.skip, args.n_keep[pair], args.channels,
                      (a == 0.) & (e == 0.)))
    return;
  if (args.channels == 2)
    dr_cut<2>(args, a_in, a_out, shift_tab, lds, a, e);
  else
    dr_cut<1>(args, a_in, a_out, shift_tab, lds, a, e);
}

#pragma clang fp contract(off)                        // host arithmetic from here on: every operation rounded on its own

struct DriftParams {
  uint32_t window, R;
  double min_corr, max_e;
};

int check_drift_params(const std::string& w, const DriftParams& p) {
  if (int rc = check_delay_window(w, p.window)) return rc;
  if (p.R < 1 || p.R > p.window / 4 || p.R > 16384)
    return fail(PEAQ_ERR_ARG, w + ": R " + std::to_string(p.R) + " is outside 1 .. min (window / 4, 16384) = " +
                                  std::to_string(std::min<uint32_t>(p.window / 4, 16384)));
  if (!(p.min_corr >= 0. && p.min_corr <= 1.))
    return fail(PEAQ_ERR_ARG, w + ": min_corr " + std::to_string(p.min_corr) + " is outside 0 .. 1");
  if (!(p.max_e > 0. && p.max_e <= PEAQ_DRIFT_MAX_E))
    return fail(PEAQ_ERR_ARG, w + ": max_e " + std::to_string(p.max_e) + " is outside (0, 0.001]");
  return PEAQ_OK;
}

// the record of one pair from its windows' records
void drift_record(int32_t lag0, uint32_t W, const peaq_delay* dl, const peaq_subdelay* sb, const DriftParams& p,
                  peaq_drift* out) {
  std::vector<double> d(W), x(W);
  std::vector<uint8_t> valid(W);
  window_delays(dl, sb, W, p.min_corr, d.data(), valid.data());
  for (uint32_t w = 0; w < W; ++w) x[w] = (double)w * p.window + (double)(p.window / 2);
  peaq_drift r;
  std::memset(&r, 0, sizeof r);
  r.lag0 = lag0;
  r.n_windows = W;
  r.n_valid = (uint32_t)theil_sen(d.data(), x.data(), valid.data(), W, &r.a, &r.e);
  if (r.n_valid < 3) {
    r.flags = PEAQ_DRIFT_F_NONE;
  } else {
    double ss = 0.;
    for (uint32_t w = 0; w < W; ++w)
      if (valid[w]) {
        const double res = d[w] - r.a - r.e * x[w];
        ss += res * res;
      }
    r.resid_rms = std::sqrt(ss / r.n_valid);
    if (std::fabs(r.e) > p.max_e) {
      r.flags = PEAQ_DRIFT_F_RANGE;
      r.a = r.e = 0.;
    }
  }
  r.ppm = 1e6 * r.e;
  *out = r;
}

// pairs of a group of the estimate, and the bytes of its two staging buffers
PairGroups drift_groups(int channels, int n_pairs, uint32_t window, uint32_t w_max) {
  const size_t per_pair = 2 * (size_t)w_max * window * channels * sizeof(float);
  PairGroups pg = pair_groups(per_pair, n_pairs, kDrStagingBudget);
  pg.group = std::max(1, std::min<int>(pg.group, 65535 / (int)w_max));
  pg.bytes = (size_t)pg.group * per_pair;
  return pg;
}

}  // namespace

extern "C" size_t peaq_drift_size(void) { return sizeof(peaq_drift); }

extern "C" int peaq_drift_fit(const double* d, const double* x, const uint8_t* valid, size_t n, double* a, double* e) {
  const std::string w("peaq_drift_fit");
  if (!a || !e) return fail(PEAQ_ERR_ARG, w + ": a or e is NULL");
  *a = *e = 0.;
  if (n && (!d || !x)) return fail(PEAQ_ERR_ARG, w + ": d or x is NULL");
  if (n > PEAQ_DRIFT_MAX_WINDOWS)
    return fail(PEAQ_ERR_ARG, w + ": " + std::to_string(n) + " points are more than " + std::to_string(PEAQ_DRIFT_MAX_WINDOWS));
  return (int)theil_sen(d, x, valid, n, a, e);
}

extern "C" void peaq_drift_index(double a, double e, int64_t i, int64_t* m, int32_t* phi) {
  long long mm;
  int pp;
  drift_index(a, e, i, &mm, &pp);
  if (m) *m = mm;
  if (phi) *phi = pp;
}

extern "C" void peaq_drift_lengths(int32_t lag0, double a, double e, uint32_t n_ref, uint32_t n_test, uint32_t* skip_ref,
                                   uint32_t* skip_test, uint32_t* n_keep) {
  uint32_t sr, st, common;
  peaq_aligned_lengths(lag0, n_ref, n_test, &sr, &st, &common);
  if (skip_ref) *skip_ref = sr;
  if (skip_test) *skip_test = st;
  if (!n_keep) return;
  *n_keep = drift_keep(a, e, st, common, n_test);
}

extern "C" uint32_t peaq_drift_windows(int32_t lag0, uint32_t n_ref, uint32_t n_test, uint32_t window) {
  if (window < PEAQ_DRIFT_MIN_WINDOW || window > PEAQ_DRIFT_MAX_WINDOW) return 0;
  uint32_t common = 0;
  peaq_aligned_lengths(lag0, n_ref, n_test, nullptr, nullptr, &common);
  return common / window;
}

extern "C" size_t peaq_drift_workspace_bytes(int channels, int n_pairs, uint32_t window, uint32_t w_max) {
  if ((channels != 1 && channels != 2) || n_pairs <= 0 || n_pairs > 65535) return 0;
  if (window < PEAQ_DRIFT_MIN_WINDOW || window > PEAQ_DRIFT_MAX_WINDOW || w_max < 1 || w_max > PEAQ_DRIFT_MAX_WINDOWS) return 0;
  return drift_groups(channels, n_pairs, window, w_max).bytes;
}

// peaq_batch_estimate_drift under the name `w` of the entry point that was called (peaq_track.hip's estimate is this one's)
int drift_estimate(const std::string& w, peaq_ctx* c, int channels, int n_pairs, const float* d_ref, const float* d_test,
                   size_t pair_stride, const uint32_t* n_ref, const uint32_t* n_test, uint32_t n_uniform, const int32_t* lag0,
                   uint32_t window, uint32_t R, double min_corr, double max_e, uint32_t w_max, peaq_delay* d_win_delay,
                   peaq_subdelay* d_win_sub, peaq_drift* out, void* stream_) {
  const DriftParams prm{window, R, min_corr, max_e};
  if (int rc = check_drift_params(w, prm)) return rc;
  if (int rc = check_shape(w, channels, n_pairs)) return rc;
  if (w_max < 1 || w_max > PEAQ_DRIFT_MAX_WINDOWS)
    return fail(PEAQ_ERR_ARG, w + ": w_max " + std::to_string(w_max) + " is outside 1 .. " + std::to_string(PEAQ_DRIFT_MAX_WINDOWS));
  if (n_pairs > 0 && (!d_ref || !d_test || !d_win_delay || !d_win_sub)) return fail(PEAQ_ERR_ARG, w + ": NULL buffer");
  if (n_pairs > 0 && (!lag0 || !out)) return fail(PEAQ_ERR_ARG, w + ": NULL lag0 or out");
  if ((n_ref == nullptr) != (n_test == nullptr))
    return fail(PEAQ_ERR_ARG, w + ": n_ref and n_test must both be given or both be NULL");
  if (int rc = check_lengths(w, n_pairs, n_ref, n_uniform, "n_ref", pair_stride, "pair_stride")) return rc;
  if (int rc = check_lengths(w, n_pairs, n_test, n_uniform, "n_test", pair_stride, "pair_stride")) return rc;
  const size_t np = (size_t)std::max(n_pairs, 0);
  std::vector<uint32_t> skip_r(np), skip_t(np), W(np);
  for (size_t p = 0; p < np; ++p) {
    uint32_t common = 0;
    peaq_aligned_lengths(lag0[p], n_ref ? n_ref[p] : n_uniform, n_test ? n_test[p] : n_uniform, &skip_r[p], &skip_t[p], &common);
    W[p] = common / window;
    if (W[p] > w_max)
      return fail(PEAQ_ERR_ARG, w + ": pair " + std::to_string(p) + ": " + std::to_string(W[p]) + " windows are more than w_max " +
                                    std::to_string(w_max));
  }
  if (!c) return fail(PEAQ_ERR_ARG, w + ": ctx is NULL");
  if (n_pairs == 0) return PEAQ_OK;

  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIP_TRY(hipSetDevice(c->device));
  const PairGroups pg = drift_groups(channels, n_pairs, window, w_max);
  const size_t slots = (size_t)pg.group * w_max;       // window slots of a group: at most 65535
  DevBuf stage[2];                                      // (the call's own: the stages it calls take the context's lock)
  for (DevBuf& b : stage) HIP_TRY(b.reserve(pg.bytes / 2));
  std::vector<uint32_t> src(slots), skip(slots), keep(slots);
  std::vector<int32_t> lag(slots);
  std::vector<peaq_delay> dl(slots);
  std::vector<peaq_subdelay> sb(slots);
  for (int p0 = 0; p0 < n_pairs; p0 += pg.group) {
    const int g = std::min(pg.group, n_pairs - p0);
    const int ns = g * (int)w_max;
    for (int side = 0; side < 2; ++side) {
      for (int p = 0; p < g; ++p)
        for (uint32_t k = 0; k < w_max; ++k) {
          const size_t s = (size_t)p * w_max + k;
          const bool there = k < W[p0 + p];
          src[s] = (uint32_t)p;
          skip[s] = there ? (side ? skip_t : skip_r)[p0 + p] + k * window : 0;
          keep[s] = there ? window : 0;
        }
      if (int rc = peaq_batch_gather(c, channels, g, ns, (side ? d_test : d_ref) + (size_t)p0 * pair_stride * channels,
                                     pair_stride, src.data(), skip.data(), keep.data(), stage[side].as<float>(), window, stream))
        return rc;
    }
    peaq_delay* d_dl = d_win_delay + (size_t)p0 * w_max;
    peaq_subdelay* d_sb = d_win_sub + (size_t)p0 * w_max;
    if (int rc = peaq_batch_estimate_delay(c, channels, ns, stage[0].as<float>(), stage[1].as<float>(), window, keep.data(),
                                           keep.data(), 0, R, d_dl, stream))
      return rc;
    HIP_TRY(hipMemcpyAsync(dl.data(), d_dl, (size_t)ns * sizeof(peaq_delay), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (int s = 0; s < ns; ++s) lag[s] = dl[s].lag;
    if (int rc = peaq_batch_refine_delay(c, channels, ns, stage[0].as<float>(), stage[1].as<float>(), window, keep.data(),
                                         keep.data(), 0, lag.data(), d_sb, stream))
      return rc;
    HIP_TRY(hipMemcpyAsync(sb.data(), d_sb, (size_t)ns * sizeof(peaq_subdelay), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));             // (the staging buffers are free again, too)
    for (int p = 0; p < g; ++p)
      drift_record(lag0[p0 + p], W[p0 + p], &dl[(size_t)p * w_max], &sb[(size_t)p * w_max], prm, &out[p0 + p]);
  }
  return PEAQ_OK;
}

extern "C" int peaq_batch_estimate_drift(peaq_ctx* c, int channels, int n_pairs, const float* d_ref, const float* d_test,
                                         size_t pair_stride, const uint32_t* n_ref, const uint32_t* n_test,
                                         uint32_t n_uniform, const int32_t* lag0, uint32_t window, uint32_t R,
                                         double min_corr, double max_e, uint32_t w_max, peaq_delay* d_win_delay,
                                         peaq_subdelay* d_win_sub, peaq_drift* out, void* stream_) {
  return drift_estimate("peaq_batch_estimate_drift", c, channels, n_pairs, d_ref, d_test, pair_stride, n_ref, n_test, n_uniform,
                        lag0, window, R, min_corr, max_e, w_max, d_win_delay, d_win_sub, out, stream_);
}

extern "C" int peaq_batch_cut_drift(peaq_ctx* c, int channels, int n_pairs, const float* d_in, size_t in_stride,
                                    const uint32_t* n_in, const uint32_t* skip, const uint32_t* n_keep, const double* a,
                                    const double* e, float* d_out, size_t out_stride, void* stream_) {
  const std::string w("peaq_batch_cut_drift");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  DelayCutCall k{w, c, channels, n_pairs, d_in, in_stride, n_in, skip, n_keep, d_out, out_stride, stream};
  if (int rc = k.check(a && e, ", a or e")) return rc;
  k.pack(3, k.np, false);
  bool plain;                                          // (the kernel looks at a and e itself)
  for (size_t p = 0; p < k.np; ++p)
    if (int rc = k.add_lines(p, nullptr, 1, a + p, e + p, nullptr, PEAQ_DRIFT_MAX_E, "-0.001 .. 0.001", &plain,
                             [](uint32_t, const auto&) { return PEAQ_OK; }))
      return rc;
  if (int rc = k.upload()) return rc;
  if (!k.slot) return PEAQ_OK;
  DriftArgs args{};
  args.in_stride = in_stride;
  args.out_stride = out_stride;
  args.n_in = k.dev_col(0);
  args.skip = k.dev_col(1);
  args.n_keep = k.dev_col(2);
  args.a = k.dev_a();
  args.e = k.dev_e();
  args.channels = channels;
  hipLaunchKernelGGL(drift_cut_kernel, dim3(k.tiles(), (unsigned)n_pairs), dim3(256), 0, stream, args, d_in, d_out, k.tab);
  return k.launched();
}

extern "C" int peaq_run_pair_drift(peaq_ctx* c, int advanced, int channels, double level_db, uint32_t rate, uint32_t max_lag,
                                   uint32_t window, int mode, double max_gain_db, const float* ref, size_t n_ref,
                                   const float* test, size_t n_test, peaq_delay* delay, peaq_drift* drift, peaq_gain* gain,
                                   peaq_result* out) {
  const std::string w("peaq_run_pair_drift");
  const DriftParams prm{window, std::min<uint32_t>(window / 4, 1024), 0.5, PEAQ_DRIFT_MAX_E};
  if (int rc = check_drift_params(w, prm)) return rc;
  // 1 .. 3: upload, rate conversion, estimate
  PairBuffers in;
  peaq_delay rec;
  uint32_t W = 0;
  if (int rc = begin_delay_pair(w, c, channels, level_db, rate, max_lag, window, mode, max_gain_db, ref, n_ref, test, n_test,
                                delay, gain, out, in, &rec, &W))
    return rc;
  const uint32_t* len = in.len;
  const size_t stride = in.stride;
  // 4: the line
  DevBuf d_dl, d_sb;
  peaq_drift dr;
  std::memset(&dr, 0, sizeof dr);
  dr.lag0 = rec.lag;
  dr.n_windows = W;
  dr.flags = PEAQ_DRIFT_F_NONE;
  if (W >= 3) {                                        // (fewer: no line whatever they measure)
    HIP_TRY(d_dl.reserve((size_t)W * sizeof(peaq_delay)));
    HIP_TRY(d_sb.reserve((size_t)W * sizeof(peaq_subdelay)));
    if (int rc = peaq_batch_estimate_drift(c, channels, 1, in.d(0), in.d(1), stride, len, len + 1, 0, &rec.lag, prm.window, prm.R,
                                           prm.min_corr, prm.max_e, W, d_dl.as<peaq_delay>(), d_sb.as<peaq_subdelay>(), &dr,
                                           nullptr))
      return rc;
  }
  if (drift) *drift = dr;
  // 5 .. 8: both signals cut to the line's lengths, the test signal along the line; the gain; the score
  uint32_t skip[2], keep = 0;
  peaq_drift_lengths(rec.lag, dr.a, dr.e, len[0], len[1], &skip[0], &skip[1], &keep);
  return score_cut_pair(c, advanced, channels, level_db, in, skip, keep, mode, max_gain_db, gain,
                        [&](float* d_out, size_t out_stride) {
                          return peaq_batch_cut_drift(c, channels, 1, in.d(1), stride, &len[1], &skip[1], &keep, &dr.a, &dr.e,
                                                      d_out, out_stride, nullptr);
                        },
                        out);
}

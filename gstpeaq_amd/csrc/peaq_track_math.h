// peaq_track_math.h -- the arithmetic of the track stage that needs no device (include/peaq_amd.h, "delay track on the
// device"): the per-window delays kept as a track (running median of three, knots for every window, a line per pair of
// neighbouring knots), which segment an output belongs to, where it reads, how many outputs a pair keeps.
// peaq_track.hip wraps these as peaq_track_fit, peaq_track_segment, peaq_track_index and peaq_track_lengths, and its
// kernel evaluates track_segment's arithmetic and drift_index itself; tools/track_host_check.cpp includes this header
// alone, so that the host arithmetic runs under the sanitizers without the device runtime.  Plain C++: every operation
// here is rounded on its own.
#pragma once
#include "peaq_drift_math.h"

#pragma clang fp contract(off)

// what track_fit finds beside the knots and the segments (the fields of peaq_track that are not the caller's)
struct TrackSummary {
  uint32_t flags, n_valid, n_filled, n_segments;
  double d_min, d_max, max_abs_e;
};
constexpr uint32_t kTrackNone = 1, kTrackRange = 2;    // PEAQ_TRACK_F_NONE, PEAQ_TRACK_F_RANGE

// the middle one of three by value
inline double med3(double a, double b, double c) {
  if (a > b) std::swap(a, b);
  if (c < a) return a;
  if (c > b) return b;
  return c;
}

// the centre of window w
inline double track_x(uint32_t w, uint32_t window) { return (double)w * window + (double)(window / 2); }

// the line through (x1, u1) and (x2, u2) taken at x0, in the one form every use of it here has
inline double track_line(double u1, double u2, double x1, double x2, double x0) { return u1 + (u1 - u2) / (x1 - x2) * (x0 - x1); }

// The fit: d[W], valid[W] (NULL: all) -> knots[W], a[S], e[S], S = max (W - 1, 1).  Arrays the caller sized.
inline void track_fit(const double* d, const uint8_t* valid, uint32_t W, uint32_t window, double max_e, double* knots,
                      double* a, double* e, TrackSummary* out) {
  const uint32_t S = std::max<uint32_t>(W, 2) - 1;
  TrackSummary r{};
  r.n_segments = S;
  for (uint32_t w = 0; w < W; ++w) knots[w] = 0.;
  for (uint32_t k = 0; k < S; ++k) a[k] = e[k] = 0.;
  // 1: the valid windows
  std::vector<uint32_t> V;
  for (uint32_t w = 0; w < W; ++w)
    if (!valid || valid[w]) V.push_back(w);
  const size_t nv = V.size();
  r.n_valid = (uint32_t)nv;
  r.n_filled = W - (uint32_t)nv;
  if (nv == 0) {
    r.flags = kTrackNone;
    *out = r;
    return;
  }
  // 2: the running median of three over the raw values; at an end the third value continues the next two
  std::vector<double> t(nv);
  for (size_t j = 0; j < nv; ++j) t[j] = d[V[j]];
  if (nv >= 3) {
    const auto u = [&](size_t j) { return d[V[j]]; };
    const auto x = [&](size_t j) { return track_x(V[j], window); };
    for (size_t j = 1; j + 1 < nv; ++j) t[j] = med3(u(j - 1), u(j), u(j + 1));
    t[0] = med3(u(0), u(1), track_line(u(1), u(2), x(1), x(2), x(0)));
    t[nv - 1] = med3(u(nv - 1), u(nv - 2), track_line(u(nv - 2), u(nv - 3), x(nv - 2), x(nv - 3), x(nv - 1)));
  }
  // 3: a knot for every window
  for (uint32_t w = 0; w < V[0]; ++w) knots[w] = t[0];
  for (size_t j = 0; j < nv; ++j) {
    knots[V[j]] = t[j];
    if (j + 1 == nv) break;
    for (uint32_t w = V[j] + 1; w < V[j + 1]; ++w)
      knots[w] = track_line(t[j], t[j + 1], track_x(V[j], window), track_x(V[j + 1], window), track_x(w, window));
  }
  for (uint32_t w = V[nv - 1] + 1; w < W; ++w) knots[w] = t[nv - 1];
  r.d_min = r.d_max = knots[0];
  for (uint32_t w = 1; w < W; ++w) {
    r.d_min = std::min(r.d_min, knots[w]);
    r.d_max = std::max(r.d_max, knots[w]);
  }
  // 4: a line from every knot to the next
  if (W == 1) {
    a[0] = knots[0];
  } else {
    for (uint32_t k = 0; k < S; ++k) {
      e[k] = (knots[k + 1] - knots[k]) / (double)window;
      a[k] = knots[k] - e[k] * track_x(k, window);
      r.max_abs_e = std::max(r.max_abs_e, std::fabs(e[k]));
    }
  }
  // 5: the range
  if (r.max_abs_e > max_e) {
    r.flags = kTrackRange;
    for (uint32_t k = 0; k < S; ++k) a[k] = e[k] = 0.;
  }
  *out = r;
}

// the segment of output i: the first and the last one extend to the pair's ends (n_seg >= 1)
PEAQ_DRIFT_HD long long track_segment(long long i, uint32_t window, uint32_t n_seg) {
  const long long h = window / 2;
  if (i < h) return 0;
  const long long k = (i - h) / window, last = (long long)n_seg - 1;
  return k < last ? k : last;
}

// where output i reads: drift_index along its segment's line
inline void track_index(uint32_t window, uint32_t n_seg, const double* a, const double* e, long long i, long long* m, int* phi) {
  const long long k = track_segment(i, window, n_seg);
  drift_index(a[k], e[k], i, m, phi);
}

// How many outputs stay: the largest count <= n_common with skip_test + i + m_i < n_test for every i below it.  i + m_i
// does not decrease with i, so drift_keep's binary search carries over: within a segment |e| <= 1/64 moves 256 (a + e i)
// by at most 4 per output, which moves g = rint (...) by at most 5 grid steps; across a knot the two lines meet within
// one grid step (track_fit's do to rounding: a_k + e_k x_{k+1} and a_{k+1} + e_{k+1} x_{k+1} are both s_{k+1} but for
// a few ulps; peaq_batch_cut_track refuses segments that do not), which moves g by at most 2 more.  7 grid steps are
// fewer than the 256 of a sample: m falls by at most 1 where i rises by 1.
inline uint32_t track_keep(uint32_t window, uint32_t n_seg, const double* a, const double* e, uint32_t skip_test,
                           uint32_t n_common, uint32_t n_test) {
  uint64_t lo = 0, hi = n_common;                      // the condition holds below lo and fails from hi on
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    long long m;
    int phi;
    track_index(window, n_seg, a, e, (long long)mid, &m, &phi);
    if ((long long)skip_test + (long long)mid + m < (long long)n_test)
      lo = mid + 1;
    else
      hi = mid;
  }
  return (uint32_t)lo;
}

// the step between segment k and k + 1 where they meet, at x_{k+1} (samples)
inline double track_step(uint32_t window, const double* a, const double* e, uint32_t k) {
  const double x = track_x(k + 1, window);
  return std::fabs((a[k] + e[k] * x) - (a[k + 1] + e[k + 1] * x));
}

// track_host_check.cpp -- the host arithmetic of the track stage (gstpeaq_amd/csrc/peaq_track_math.h: track_fit,
// track_segment, track_index, track_keep, what peaq_track_fit / peaq_track_segment / peaq_track_index /
// peaq_track_lengths wrap) on its own, for the sanitizers: no device runtime, no library.  The inputs are those of
// tests/test_track_host.py.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o track_host_check track_host_check.cpp
//   ./track_host_check        (prints "track_host_check ok", exit status 0)
#include <cstdio>
#include <cstdlib>

#include "../gstpeaq_amd/csrc/peaq_track_math.h"

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);         \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static uint64_t rng_state = 88172645463325252ull;
static double uniform() {                              // xorshift64, (0, 1)
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (double)(rng_state >> 11) / 9007199254740992.;
}
static double grid(double v) { return std::nearbyint(v * 256.) / 256.; }

struct Fit {
  std::vector<double> knots, a, e;
  TrackSummary s;
};
// arrays of exactly the sizes the fit may touch, so that a write past them is the sanitizer's to see
static Fit fit(const std::vector<double>& d, const std::vector<uint8_t>* valid, uint32_t window, double max_e = 1. / 64) {
  const uint32_t W = (uint32_t)d.size(), S = std::max<uint32_t>(W, 2) - 1;
  Fit f;
  f.knots.assign(W, -1.);
  f.a.assign(S, -1.);
  f.e.assign(S, -1.);
  track_fit(d.data(), valid ? valid->data() : nullptr, W, window, max_e, f.knots.data(), f.a.data(), f.e.data(), &f.s);
  return f;
}

int main() {
  // lines on the grid come back as they are, every segment the same line
  for (uint32_t window : {4096u, 5001u, 16384u}) {
    std::vector<double> d(12);
    for (size_t w = 0; w < d.size(); ++w) d[w] = -3.25 + 0.375 * (double)w;
    const Fit f = fit(d, nullptr, window);
    CHECK(f.s.flags == 0 && f.s.n_valid == 12 && f.s.n_filled == 0 && f.s.n_segments == 11);
    CHECK(f.knots == d && f.s.d_min == d.front() && f.s.d_max == d.back());
    for (double e : f.e) CHECK(std::fabs(e - 0.375 / window) <= 1e-12 * 0.375 / window);
  }
  {  // a step survives; a spike inside and at either end does not
    std::vector<double> d{2, 2, 2, 2, 2, 9.25, 9.25, 9.25, 9.25, 9.25, 9.25};
    CHECK(fit(d, nullptr, 16384).knots == d);
    for (size_t at : {0u, 3u, 7u}) {
      std::vector<double> s{1.0, 1.1, 1.2, 1.3, 1.4, 1.5, 1.6, 1.7};
      for (double& v : s) v = grid(v);
      s[at] = at == 0 ? -300. : 250.;
      const Fit f = fit(s, nullptr, 16384);
      CHECK(f.s.flags == 0);
      for (double k : f.knots) CHECK(std::fabs(k) < 2.);
    }
  }
  {  // gaps at the start, in the middle and at the end; nv = 0, 1, 2; W = 0, 1, 2
    std::vector<double> d(10);
    for (size_t w = 0; w < d.size(); ++w) d[w] = 0.5 * (double)w;
    const std::vector<uint8_t> masks[] = {{0, 0, 0, 1, 1, 1, 1, 1, 1, 1}, {1, 1, 1, 0, 0, 0, 1, 1, 1, 1}, {1, 1, 1, 1, 1, 1, 1, 0, 0, 255},
                                          {0, 1, 0, 0, 1, 1, 0, 1, 0, 1}, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 1, 0, 0, 0, 0, 0, 0, 0},
                                          {0, 1, 0, 0, 1, 0, 0, 0, 0, 0}};
    for (const auto& mask : masks) {
      const Fit f = fit(d, &mask, 5001);
      uint32_t nv = 0;
      for (uint8_t v : mask) nv += v != 0;
      CHECK(f.s.n_valid == nv && f.s.n_filled == 10 - nv && f.s.n_segments == 9);
      CHECK((f.s.flags == kTrackNone) == (nv == 0));
      if (nv >= 2)
        for (size_t w = 0; w < d.size(); ++w) CHECK(f.knots[w] >= -1e-9 && f.knots[w] <= 4.5 + 1e-9);
      if (nv == 0)
        for (size_t w = 0; w < d.size(); ++w) CHECK(f.knots[w] == 0.);
    }
    const Fit mid = fit(d, &masks[1], 5001);
    for (size_t w = 0; w < d.size(); ++w) CHECK(std::fabs(mid.knots[w] - d[w]) < 1e-12);
    const Fit none = fit({}, nullptr, 4096);
    CHECK(none.s.flags == kTrackNone && none.s.n_segments == 1 && none.a[0] == 0. && none.e[0] == 0.);
    const Fit one = fit({-12.75}, nullptr, 4096);
    CHECK(one.s.flags == 0 && one.s.n_segments == 1 && one.a[0] == -12.75 && one.e[0] == 0. && one.knots[0] == -12.75);
    const Fit two = fit({1.0, 2.5}, nullptr, 8192);
    CHECK(two.s.n_segments == 1 && two.e[0] == 1.5 / 8192 && two.a[0] == 1.0 - two.e[0] * 4096.);
  }
  // a slope just under and just over max_e
  for (double max_e : {1. / 64, 1e-3}) {
    const double rise = max_e * 4096.;
    const Fit under = fit({0., 0., std::nextafter(rise, 0.), std::nextafter(rise, 0.)}, nullptr, 4096, max_e);
    const Fit over = fit({0., 0., std::nextafter(rise, 1e9), std::nextafter(rise, 1e9)}, nullptr, 4096, max_e);
    CHECK(under.s.flags == 0 && under.e[1] > 0.);
    CHECK(over.s.flags == kTrackRange && over.s.max_abs_e > max_e && over.knots[2] > rise);
    for (size_t k = 0; k < 3; ++k) CHECK(over.a[k] == 0. && over.e[k] == 0.);
  }
  // the segment of an output, an odd window among them
  CHECK(track_segment(2500, 5001, 3) == 0 && track_segment(7500, 5001, 3) == 0 && track_segment(7501, 5001, 3) == 1);
  CHECK(track_segment(1000000, 5001, 3) == 2 && track_segment(0, 4096, 1) == 0 && track_segment(4294967295ll, 4096, 1) == 0);
  CHECK(track_segment(4294967295ll, 4096, 4095) == 4094);
  // random tracks of steep segments: the index along them, the lengths against brute force, i + m_i never decreasing
  for (int trial = 0; trial < 300; ++trial) {
    const uint32_t window = trial & 1 ? 5001 : 4096, W = 1 + (uint32_t)(uniform() * 5);
    std::vector<double> d(W);
    double v = 10. * uniform() - 5.;
    for (uint32_t w = 0; w < W; ++w) {
      v += (uniform() < 0.5 ? -1. : 1.) * (trial % 4 < 2 ? window / 64. : uniform() * window / 200.);
      d[w] = grid(v);
    }
    const Fit f = fit(d, nullptr, window);
    CHECK(f.s.flags == 0 && f.s.max_abs_e <= 1. / 64);
    const uint32_t S = f.s.n_segments;
    for (uint32_t k = 0; k + 1 < S; ++k) CHECK(track_step(window, f.a.data(), f.e.data(), k) < 1e-9);
    const uint32_t n_test = window / 2 + (uint32_t)(uniform() * W * window), skip = (uint32_t)(uniform() * 40);
    const uint32_t common = n_test > skip ? n_test - skip : 0;
    uint32_t want = 0;
    bool open = true;
    long long last = -(1ll << 40);
    for (uint32_t i = 0; i < common; ++i) {
      long long m;
      int phi;
      track_index(window, S, f.a.data(), f.e.data(), i, &m, &phi);
      CHECK(phi >= -128 && phi <= 127);
      CHECK(i + m >= last);
      last = i + m;
      if (open && (long long)skip + i + m < (long long)n_test)
        ++want;
      else
        open = false;
    }
    CHECK(track_keep(window, S, f.a.data(), f.e.data(), skip, common, n_test) == want);
  }
  const double zero = 0.;
  CHECK(track_keep(4096, 1, &zero, &zero, 0, 0, 0) == 0 && track_keep(4096, 1, &zero, &zero, 7, 4294967288u, 4294967295u) == 4294967288u);
  if (failures) return 1;
  std::puts("track_host_check ok");
  return 0;
}

// steps_host_check.cpp -- the host arithmetic of the steps stage (gstpeaq_amd/csrc/peaq_steps_math.h: steps_candidates,
// steps_fit, pieces_find, pieces_index, pieces_keep, what peaq_steps_candidates / peaq_steps_fit / peaq_pieces_index /
// peaq_pieces_lengths wrap) on its own, for the sanitizers: no device runtime, no library.  The inputs are those of
// tests/test_steps_host.py.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o steps_host_check steps_host_check.cpp
//   ./steps_host_check        (prints "steps_host_check ok", exit status 0)
#include <cstdio>
#include <cstdlib>

#include "../gstpeaq_amd/csrc/peaq_steps_math.h"

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

struct Fit {
  std::vector<StepCandidate> cand;
  std::vector<StepFound> found;
  std::vector<uint32_t> b;
  std::vector<double> a, e;
  PiecesSummary s;
};
// arrays of exactly the sizes the fit may touch, so that a write past them is the sanitizer's to see; where[j]: the c
// of candidate j, good[j]: whether its gains pass
static Fit fit(const std::vector<double>& knots, uint32_t window, uint32_t n_common, const std::vector<uint32_t>& where,
               const std::vector<uint8_t>& good, double ratio = 3., double max_e = 1. / 64) {
  const uint32_t W = (uint32_t)knots.size(), S = std::max<uint32_t>(W, 2) - 1;
  Fit f;
  f.cand.resize(S);
  f.cand.resize(steps_candidates(knots.data(), W, window, n_common, 0.75, ratio, f.cand.data()));
  const uint32_t n = (uint32_t)f.cand.size();
  for (uint32_t j = 0; j < n; ++j) {
    const bool ok = j < good.size() ? good[j] : true;
    f.found.push_back({j < where.size() ? where[j] : f.cand[j].lo, 0, f.cand[j].LA, f.cand[j].LB, 1., ok ? 1. : 0., 2.});
  }
  f.b.assign(S + n, 7u);
  f.a.assign(S + n, -1.);
  f.e.assign(S + n, -1.);
  steps_fit(knots.data(), W, window, f.cand.data(), f.found.data(), n, 0.0021, max_e, f.b.data(), f.a.data(), f.e.data(), &f.s);
  CHECK(f.s.n_pieces >= 1 && f.s.n_pieces <= S + n && f.b[0] == 0);
  for (uint32_t j = 1; j < f.s.n_pieces; ++j) CHECK(f.b[j] > f.b[j - 1]);
  return f;
}

// pieces_keep against a look at every output
static uint32_t keep_brute(const Fit& f, uint32_t skip_test, uint32_t n_common, uint32_t n_test) {
  for (uint32_t i = 0; i < n_common; ++i) {
    long long m;
    int phi;
    pieces_index(f.s.n_pieces, f.b.data(), f.a.data(), f.e.data(), i, &m, &phi);
    if ((long long)skip_test + i + m >= (long long)n_test) return i;
  }
  return n_common;
}

int main() {
  {  // a drift and a bend: no candidate, the track's own segments
    for (uint32_t window : {4096u, 5001u, 16384u}) {
      std::vector<double> d(12), bend;
      for (size_t w = 0; w < d.size(); ++w) d[w] = -3.25 + 0.375 * (double)w;
      for (int w = 0; w < 6; ++w) bend.push_back(0.8 * w);
      for (int w = 0; w < 6; ++w) bend.push_back(4.0 - 0.8 * w);
      for (const auto& knots : {d, bend}) {
        const Fit f = fit(knots, window, 12 * window + 5, {}, {});
        CHECK(f.cand.empty() && f.s.n_pieces == 11 && f.s.flags == 0 && f.s.n_accepted == 0);
        for (uint32_t k = 0; k < 11; ++k) {
          double a, e;
          steps_segment(knots.data(), 12, window, k, &a, &e);
          CHECK(f.b[k] == steps_start(k, window) && f.a[k] == a && f.e[k] == e);
        }
      }
    }
    CHECK(fit({}, 4096, 100, {}, {}).s.n_pieces == 1);
    CHECK(fit({-12.75}, 4096, 5000, {}, {}).a[0] == -12.75);
  }
  for (uint32_t k : {0u, 3u, 6u}) {  // one step in the first, a middle and the last segment
    std::vector<double> knots(8, 37.5);
    for (uint32_t w = k + 1; w < 8; ++w) knots[w] += 9.;
    const uint32_t c = steps_start(k, 4096) + 1000;
    const Fit f = fit(knots, 4096, 8 * 4096 + 777, {c}, {1});
    CHECK(f.cand.size() == 1 && f.cand[0].k == k && f.cand[0].LA == 38 && f.cand[0].LB == 46);
    CHECK(f.s.n_accepted == 1 && f.s.n_pieces == 8 && f.s.flags == 0);
    for (uint32_t j = 0; j < 8; ++j) CHECK(f.e[j] == 0. && f.a[j] == (f.b[j] < c ? 37.5 : 46.5));
    const Fit weak = fit(knots, 4096, 8 * 4096 + 777, {c}, {0});
    CHECK(weak.s.n_accepted == 0 && weak.s.n_pieces == 7 && weak.found[0].flags == kStepWeak);
  }
  {  // c before and behind its segment's own outputs, at the interval's ends
    std::vector<double> knots(8, -2.25);
    for (uint32_t w = 4; w < 8; ++w) knots[w] -= 20.;
    const uint32_t start = steps_start(3, 4096), end = steps_start(4, 4096);
    for (uint32_t c : {start - 700, end + 900, 3u * 4096, 5u * 4096, start, end}) {
      const Fit f = fit(knots, 4096, 8 * 4096 + 777, {c}, {1});
      CHECK(f.s.n_accepted == 1 && f.s.n_pieces == 7);
      for (uint32_t j = 0; j < 7; ++j) CHECK(f.a[j] == (f.b[j] < c ? -2.25 : -22.25));
    }
  }
  {  // steps in adjacent segments (ratio 1): flat lines, each c held at the border where the other reaches across
    const std::vector<double> knots{0., 0., 0., 6., 12., 12., 12.};
    for (auto cc : {std::pair<uint32_t, uint32_t>{2 * 4096 + 3000, 3 * 4096 + 3500}, {4 * 4096 - 5, 3 * 4096 + 5}, {2 * 4096, 5 * 4096}}) {
      const Fit f = fit(knots, 4096, 7 * 4096, {cc.first, cc.second}, {1, 1}, 1.);
      CHECK(f.cand.size() == 2 && f.s.n_accepted == 2);
      for (uint32_t j = 0; j < f.s.n_pieces; ++j) CHECK(f.e[j] == 0. && (j == 0 || f.a[j] >= f.a[j - 1]));
    }
  }
  {  // flagged through a step alone: unflagged once it is accepted, flagged and zeroed when it is not
    std::vector<double> knots(11, 0.25);
    for (uint32_t w = 6; w < 11; ++w) knots[w] += 300.;
    const Fit f = fit(knots, 16384, 11 * 16384, {5 * 16384 + 8192 + 4321}, {1});
    CHECK(f.s.flags == 0 && f.s.n_accepted == 1 && f.s.max_abs_e == 0. && f.s.n_pieces == 11);
    const Fit g = fit(knots, 16384, 11 * 16384, {5 * 16384 + 8192 + 4321}, {0});
    CHECK(g.s.flags == kPiecesRange && g.s.n_pieces == 10 && g.s.max_abs_e > 1. / 64);
    for (uint32_t j = 0; j < 10; ++j) CHECK(g.a[j] == 0. && g.e[j] == 0.);
  }
  // random tracks: every candidate somewhere in its interval, some weak; then index and keep against brute force
  for (int trial = 0; trial < 300; ++trial) {
    const uint32_t W = 2 + (uint32_t)(uniform() * 12), window = uniform() < 0.5 ? 4096 : 5001;
    std::vector<double> knots(W);
    double v = 0.;
    for (uint32_t w = 0; w < W; ++w) {
      v += 0.6 * (uniform() - 0.5);
      if (w && uniform() < 0.2) v += uniform() < 0.5 ? -300. : 20.;
      knots[w] = std::nearbyint(v * 256.) / 256.;
    }
    const uint32_t n_common = W * window + (uint32_t)(uniform() * window);
    const double ratio = uniform() < 0.5 ? 1. : 3.;
    std::vector<StepCandidate> cd(W);
    cd.resize(steps_candidates(knots.data(), W, window, n_common, 0.75, ratio, cd.data()));
    std::vector<uint32_t> where;
    std::vector<uint8_t> good;
    for (const StepCandidate& c : cd) {
      where.push_back(c.lo + (uint32_t)(uniform() * (c.hi - c.lo + 1)));
      good.push_back(uniform() < 0.7);
    }
    const Fit f = fit(knots, window, n_common, where, good, ratio);
    if (f.s.flags) continue;
    const uint32_t n_test = n_common - (uint32_t)(uniform() * 400), skip = (uint32_t)(uniform() * 50);
    CHECK(pieces_keep(f.s.n_pieces, f.b.data(), f.a.data(), f.e.data(), skip, n_common, n_test) == keep_brute(f, skip, n_common, n_test));
  }
  {  // jumps of +-5000, pieces of 1 and 5 outputs, slopes of +-1/64: index and keep
    Fit f;
    f.b = {0, 1000, 1001, 1006, 1306, 5000};
    f.a = {0.3, 5000.25, -5000.0, 17.5, -3.75, 2.0};
    f.e = {1e-3, -1. / 64, 1. / 64, 0., 3e-4, -2e-3};
    f.s.n_pieces = 6;
    for (long long i : {0ll, 999ll, 1000ll, 1001ll, 1005ll, 1006ll, 4999ll, 5000ll, 11999ll}) {
      long long m, want;
      int phi, wphi;
      pieces_index(6, f.b.data(), f.a.data(), f.e.data(), i, &m, &phi);
      const uint32_t j = pieces_find(f.b.data(), 6, i);
      CHECK(f.b[j] <= i && (j == 5 || i < f.b[j + 1]));
      drift_index(f.a[j], f.e[j], i, &want, &wphi);
      CHECK(m == want && phi == wphi && phi >= -128 && phi <= 127);
    }
    for (uint32_t n_test : {12000u, 9500u, 6100u, 900u})
      for (uint32_t skip : {0u, 37u})
        CHECK(pieces_keep(6, f.b.data(), f.a.data(), f.e.data(), skip, 11000, n_test) == keep_brute(f, skip, 11000, n_test));
  }
  if (failures) return 1;
  std::printf("steps_host_check ok\n");
  return 0;
}

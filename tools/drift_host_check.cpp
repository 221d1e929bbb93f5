// drift_host_check.cpp -- the host arithmetic of the drift stage (gstpeaq_amd/csrc/peaq_drift_math.h: drift_index,
// drift_keep, theil_sen, what peaq_drift_index / peaq_drift_lengths / peaq_drift_fit wrap, and window_delays) on its
// own, for the sanitizers: no device runtime, no library.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o drift_host_check drift_host_check.cpp
//   ./drift_host_check        (prints "drift_host_check ok", exit status 0)
#include <cstdio>
#include <cstdlib>

#include "../gstpeaq_amd/csrc/peaq_drift_math.h"

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

int main() {
  long long m;
  int phi;
  // the index: the grid points of a flat line, the half-way cases, far positions on both sides
  for (int q = -128; q < 128; ++q) {
    drift_index(q / 256., 0., 4000000000ll + q, &m, &phi);
    CHECK(m == 0 && phi == q);
  }
  drift_index(-0.5, 0., 0, &m, &phi);
  CHECK(m == 0 && phi == -128);
  drift_index(0.5, 0., 0, &m, &phi);
  CHECK(m == 1 && phi == -128);
  drift_index(1. / 512, 0., 0, &m, &phi);               // g = 0.5 rounds to 0
  CHECK(m == 0 && phi == 0);
  drift_index(3. / 512, 0., 0, &m, &phi);               // g = 1.5 rounds to 2
  CHECK(m == 0 && phi == 2);
  const long long far[] = {-2147483648ll, -100000, -1, 0, 1, 4294967295ll, 4294967296ll, 8589934592ll};
  for (long long i : far)
    for (double e : {1e-3, -1e-3, 3.73e-5})
      for (double a : {-1048576., -0.37, 17.5, 1048576.}) {
        drift_index(a, e, i, &m, &phi);
        CHECK(phi >= -128 && phi <= 127);
        const double pos = a + e * (double)i;
        CHECK(std::fabs((double)m + phi / 256. - pos) <= 1. / 256 + 1e-6);
      }
  // the lengths against brute force, empty signals included
  for (int trial = 0; trial < 4000; ++trial) {
    const uint32_t n_test = (uint32_t)(uniform() * 700), skip = (uint32_t)(uniform() * (n_test + 1));
    const uint32_t common = (uint32_t)(uniform() * (n_test - std::min(skip, n_test) + 1));
    const double a = 12. * uniform() - 6., e = 2e-3 * uniform() - 1e-3;
    uint32_t want = 0;
    for (; want < common; ++want) {
      drift_index(a, e, want, &m, &phi);
      if (!((long long)skip + want + m < (long long)n_test)) break;
    }
    CHECK(drift_keep(a, e, skip, common, n_test) == want);
  }
  CHECK(drift_keep(-2.25, -1e-3, 7, 4294967288u, 4294967295u) == 4294967288u);
  CHECK(drift_keep(0., 0., 0, 0, 0) == 0);
  // the fit: exact lines come back, outliers are outvoted, masks and short sets
  for (size_t n : {0u, 1u, 2u, 3u, 4u, 7u, 64u, 301u}) {
    std::vector<double> d(n), x(n);
    std::vector<uint8_t> valid(n, 1);
    for (size_t w = 0; w < n; ++w) {
      x[w] = 16384. * w + 8192.;
      d[w] = 3.5 + x[w] / 8192.;                        // exact in double
    }
    double a = 1., e = 1.;
    CHECK(theil_sen(d.data(), x.data(), nullptr, n, &a, &e) == n);
    if (n >= 3)
      CHECK(a == 3.5 && e == 1. / 8192);
    else
      CHECK(a == 0. && e == 0.);
    for (size_t w = 0; w < n; w += 4) d[w] = 1000. * uniform();          // a quarter of gross outliers
    theil_sen(d.data(), x.data(), valid.data(), n, &a, &e);
    if (n >= 7) CHECK(a == 3.5 && e == 1. / 8192);
    for (size_t w = 0; w < n; w += 4) valid[w] = 0;
    const size_t nv = theil_sen(d.data(), x.data(), valid.data(), n, &a, &e);
    CHECK(nv == n - (n + 3) / 4);
    if (nv >= 3) CHECK(a == 3.5 && e == 1. / 8192);
  }
  {
    std::vector<double> d(4096), x(4096);              // the largest set the stage takes: 8.4 M slopes
    for (size_t w = 0; w < d.size(); ++w) {
      x[w] = 4096. * w + 2048.;
      d[w] = -2. + x[w] / 16384. + (uniform() - 0.5) / 256.;
    }
    double a, e;
    CHECK(theil_sen(d.data(), x.data(), nullptr, d.size(), &a, &e) == 4096);
    CHECK(std::fabs(e - 1. / 16384) < 1e-9 && std::fabs(a + 2.) < 1e-3);
  }
  {
    // the windows' delays and which of them count, on records laid out here (the library's are peaq_delay, peaq_subdelay)
    struct Delay { int lag; double peak, norm; };
    struct Sub { int q; unsigned flags; };
    const Delay dl[] = {{37, 0.9, 1.}, {-3, -0.6, 1.}, {5, 0.49, 1.}, {5, 0.5, 1.}, {1, 1., 0.}, {1, 1., NAN}, {2, 3., INFINITY}, {9, 1., 1.}};
    const Sub sb[] = {{128, 0}, {-64, 0}, {0, 0}, {1, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 1}};
    const uint8_t want[] = {1, 1, 0, 1, 0, 0, 0, 0};    // below min_corr; no energy; NaN; Inf; flagged by the refinement
    double d[8];
    uint8_t valid[8];
    window_delays(dl, sb, 8, 0.5, d, valid);
    for (int w = 0; w < 8; ++w) CHECK(valid[w] == want[w]);
    CHECK(d[0] == 37.5 && d[1] == -3.25 && d[3] == 5. + 1. / 256);
    window_delays(dl, sb, 0, 0.5, nullptr, nullptr);   // no window: nothing is touched
  }
  if (failures) return 1;
  std::puts("drift_host_check ok");
  return 0;
}

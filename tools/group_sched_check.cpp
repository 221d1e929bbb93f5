// group_sched_check.cpp -- the front end's band sums by read slots (gstpeaq_amd/csrc/peaq_group_sched.h, group_bands of
// peaq_frontend.hip) in plain C++ on the REAL band tables (linked against peaq_tables.cpp), against the plain loop of
// fftearmodel.c:604-620: no device runtime, no library.  Every band is summed with the slot count of its half (the
// middle band, which its lane sums twice, with both), on a spectrum of exactly the kernel's length followed by exactly
// group_zero_words zero words -- so that a read beyond either end is an error under the address sanitizer.
//   clang++ -std=c++17 -O1 -g -ffp-contract=off [-fsanitize=address,undefined -fno-sanitize-recover=all] -I../gstpeaq_amd/csrc
//           -I../include -o group_sched_check group_sched_check.cpp ../gstpeaq_amd/csrc/peaq_tables.cpp
//   ./group_sched_check
// One line per band count and case, "NB case sums N mismatches M", and one "NB slots ..." line with the largest number
// of whole pairs in each half beside the slot count; exit status 0.  tests/test_group_schedule_host.py builds and runs it
// and holds every M to 0: the sums must be the plain loop's bit for bit, the floor of 1e-12 included.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../gstpeaq_amd/csrc/peaq_group_sched.h"
#include "../gstpeaq_amd/csrc/peaq_tables.h"

static uint64_t rng_state = 88172645463325252ull;
static double uniform() {                              // xorshift64, (0, 1)
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (double)(rng_state >> 11) / 9007199254740992.;
}

static double plain_loop(const peaq::BandTables& t, int b, const double* sp) {
  double p = t.wlo[b] * sp[t.lo[b]] + t.whi[b] * sp[t.hi[b]];
  for (int k = t.lo[b] + 1; k < t.hi[b]; ++k) p += sp[k];
  return p < 1e-12 ? 1e-12 : p;
}
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

struct Tally {
  long sums = 0, mismatches = 0;
};
// all bands of one spectrum, each with the slots of its half; sp[zero ..] are the zero words
static void compare(const peaq::BandTables& t, const double* sp, int zero, Tally& y) {
  const int nb = t.bands;
  for (int b = 0; b < nb; ++b) {
    const double want = plain_loop(t, b, sp);
    const int slots = group_band_is_wide(nb, b) ? group_wide_pairs(nb) : group_narrow_pairs(nb);
    y.mismatches += !same_bits(group_band_scheduled(slots, t.lo[b], t.hi[b], t.wlo[b], t.whi[b], sp, zero), want);
    ++y.sums;
    if (b == group_lanes(nb) - 1 && nb - 1 - b == b) {   // the middle lane sums its band as a wide one as well
      y.mismatches += !same_bits(group_band_scheduled(group_wide_pairs(nb), t.lo[b], t.hi[b], t.wlo[b], t.whi[b], sp, zero), want);
      ++y.sums;
    }
  }
}

static int run(int nb) {
  auto tp = std::make_unique<peaq::BandTables>();
  const peaq::BandTables& t = *tp;
  peaq::build_fft_band_tables(nb, *tp);
  int narrow_max = 0, wide_max = 0, widest = 0;
  for (int b = 0; b < nb; ++b) {
    int& m = group_band_is_wide(nb, b) ? wide_max : narrow_max;
    const int pairs = group_pairs(t.lo[b], t.hi[b]);
    m = pairs > m ? pairs : m;
    widest = t.hi[b] - t.lo[b] - 1 > widest ? t.hi[b] - t.lo[b] - 1 : widest;
  }
  std::printf("%d slots narrow_max %d narrow_slots %d wide_max %d wide_slots %d widest_interior %d misfit %d\n", nb, narrow_max,
              group_narrow_pairs(nb), wide_max, group_wide_pairs(nb), widest, peaq::fft_band_sums_misfit(t));
  // a table that does not fit must be told: one band of each half made one pair too long
  {
    auto bad = std::make_unique<peaq::BandTables>(t);
    bad->hi[0] = bad->lo[0] + 2 * group_narrow_pairs(nb) + 3;
    const int first = peaq::fft_band_sums_misfit(*bad);
    *bad = t;
    bad->lo[nb - 1] = bad->hi[nb - 1] - 2 * group_wide_pairs(nb) - 3;
    std::printf("%d misfit_detected narrow %d wide %d\n", nb, first, peaq::fft_band_sums_misfit(*bad));
  }
  const int zero = kGroupSpectrumBins;
  std::vector<double> sp(kGroupSpectrumBins + group_zero_words(nb), 0.);
  Tally y;
  for (int rep = 0; rep < 16; ++rep) {                 // powers over 24 decades, bin by bin
    for (int k = 0; k < kGroupSpectrumBins; ++k) sp[k] = std::pow(10., -18. + 24. * uniform());
    compare(t, sp.data(), zero, y);
  }
  std::printf("%d random sums %ld mismatches %ld\n", nb, y.sums, y.mismatches);
  y = Tally();
  for (int rep = 0; rep < 4; ++rep) {                  // ... and of one size, where every bin's last bits reach the sum
    for (int k = 0; k < kGroupSpectrumBins; ++k) sp[k] = 0.5 + uniform();
    compare(t, sp.data(), zero, y);
  }
  std::printf("%d level sums %ld mismatches %ld\n", nb, y.sums, y.mismatches);
  y = Tally();
  std::fill(sp.begin(), sp.end(), 0.);
  compare(t, sp.data(), zero, y);                      // the floor
  std::printf("%d zeros sums %ld mismatches %ld\n", nb, y.sums, y.mismatches);
  y = Tally();
  long seen = 0;                                       // one bin walked over every position the bands touch
  for (int k = t.lo[0]; k <= t.hi[nb - 1]; ++k) {
    sp[k] = 0.3 + k * 1e-3;
    compare(t, sp.data(), zero, y);
    for (int b = 0; b < nb; ++b)                       // (and every position is seen by some band at all)
      if (k >= t.lo[b] && k <= t.hi[b]) {
        ++seen;
        break;
      }
    sp[k] = 0.;
  }
  std::printf("%d walk sums %ld mismatches %ld\n", nb, y.sums, y.mismatches + (t.hi[nb - 1] - t.lo[0] + 1 - seen));
  return 0;
}

int main() {
  run(109);
  run(55);
  return 0;
}

// peaq_spread_sched.h -- the schedule of the front end's upward spreading (peaq_frontend.hip, Kabal (27)): which lane
// adds which term of which source at which step.  Plain constexpr functions of the band count, usable from host code:
// the kernel takes its constants from here, tools/spread_sched_check.cpp simulates the same schedule on a 64-element
// array against the reference's double loop, and the static_asserts at the end prove the cover.
//
// The setting: lane L owns the bands 2 L and 2 L + 1 ("source L", "target L"), kLanes = (NB - 1) / 2 is the last lane
// with a band.  The accumulators travel: at step k (counted down) a source adds what it sends k lanes up to the pair
// of sums standing in its own lane, then all sums move one lane up.  A pair (S, k) is wanted when S + k <= kLanes.
//
// One stream walking k = kLanes .. 1 in every lane leaves most lanes idle at the far distances: at distance K only the
// sources S <= kLanes - K have a target.  So the far distances K0 + 1 .. kLanes ("helper stream", H of them) run
// CONCURRENTLY with the main stream's first H steps k = K0 .. K0 - H + 1, in lanes 32 + S that hold a copy of source S
// and that the main stream's sums do not reach yet; the same instructions, another lane, distance k + H.  While the
// helper runs, a lane adds only from its activation step on (k <= act): a term for a band that does not exist would
// otherwise walk up from the main lanes into the helper's.  At the boundary (behind step k = kBoundary) the helper's
// finished sums stand `spread_home_shift` lanes below their home lanes, are taken out and handed home; the lanes
// >= 32 go on with their own source at distance kBoundary - 1 (none of them has a target farther than that).
#pragma once

constexpr int kSpreadWave = 64;
constexpr int kSpreadHelperBase = 32;                  // helper lane of source S: 32 + S

constexpr int spread_lanes(int nb) { return (nb - 1) / 2; }
// The helper may run while lane 31 is still empty BEFORE the move of a step (main sums stand in lanes <= kLanes - k):
// kLanes - k < 31 for every k >= K0 - H + 1, and the main stream needs a step k >= 1 for each of the helper's.
constexpr int spread_helper_steps(int nb) {
  const int by_half = (kSpreadHelperBase - 1) / 2, by_steps = spread_lanes(nb) / 2;
  return by_half < by_steps ? by_half : by_steps;
}
constexpr int spread_k0(int nb) { return spread_lanes(nb) - spread_helper_steps(nb); }        // the main stream's first distance = the step count
constexpr int spread_boundary(int nb) { return spread_k0(nb) - spread_helper_steps(nb) + 1; }  // the last step the helper runs in
// the step from which lane `lane` adds while the helper runs (below 1: never)
constexpr int spread_act(int nb, int lane) {
  return lane < kSpreadHelperBase ? spread_lanes(nb) - lane : spread_k0(nb) - (lane - kSpreadHelperBase);
}
// behind the boundary step's move the helper's sum for target M stands in lane M - spread_home_shift
constexpr int spread_home_shift(int nb) { return spread_helper_steps(nb) + spread_boundary(nb) - (kSpreadHelperBase + 1); }
// Exponents of a^0.4 (two bands per lane step) in the start terms of source band 2 L + s:
constexpr int spread_exp_upper(int nb, int s) { return 2 * (spread_boundary(nb) - 1) - s; }    // lanes >= 32, behind the boundary
constexpr int spread_exp_helper(int nb) { return 2 * spread_helper_steps(nb); }                // main = upper x this, copy = main x this
constexpr int spread_exp_main(int nb, int s) { return spread_exp_upper(nb, s) + spread_exp_helper(nb); }   // = 2 K0 - s

// Every wanted pair is covered exactly once, nothing unwanted is added while the helper runs, the main sums stay out
// of the helper's lanes and the helper's sums end `spread_home_shift` below home.
constexpr bool spread_schedule_covers(int nb) {
  const int kl = spread_lanes(nb), h = spread_helper_steps(nb), k0 = spread_k0(nb), kb = spread_boundary(nb);
  if (h < 1 || kb < 2 || k0 + h != kl || kl >= kSpreadWave || kSpreadHelperBase + h > kSpreadWave) return false;
  int count[kSpreadWave][kSpreadWave] = {};            // [source][distance]
  for (int k = k0; k >= 1; --k) {
    for (int lane = 0; lane < kSpreadWave; ++lane) {
      const bool helper_phase = k >= kb;
      if (helper_phase && k > spread_act(nb, lane)) continue;
      const bool copy = helper_phase && lane >= kSpreadHelperBase;
      const int src = copy ? lane - kSpreadHelperBase : lane, dist = copy ? k + h : k;
      if (src + dist <= kl) {
        ++count[src][dist];
        if (helper_phase && !copy && lane + 1 >= kSpreadHelperBase) return false;   // a main sum about to enter lane 32
      } else if (helper_phase) {
        return false;                                  // an unwanted term added where it could reach the helper
      }
      // where the sum this term goes into stands once the boundary is passed (helper) / at the end (others)
      if (copy && lane + (k - kb + 1) + spread_home_shift(nb) != src + dist) return false;
    }
  }
  for (int s = 0; s <= kl; ++s)
    for (int k = 1; k < kSpreadWave; ++k)
      if (count[s][k] != (s + k <= kl ? 1 : 0)) return false;
  return spread_exp_main(nb, 0) == 2 * k0 && spread_exp_upper(nb, 1) >= 1;
}
static_assert(spread_schedule_covers(109) && spread_k0(109) == 39 && spread_boundary(109) == 25, "upward spreading, 109 bands");
static_assert(spread_schedule_covers(55) && spread_k0(55) == 14 && spread_boundary(55) == 2, "upward spreading, 55 bands");

// spread_sched_check.cpp -- the front end's two-stream upward spreading (gstpeaq_amd/csrc/peaq_spread_sched.h, the
// loop of peaq_frontend.hip) simulated on a 64-element "wave" in plain C++, against the O(B^2) double loop of Kabal
// (27): no device runtime, no library.  A lane move is an array shift, the half-wave swap a copy of the lower half,
// the activation step a condition; the arithmetic and its order are the kernel's.
//   g++ -std=c++17 -O1 -g [-fsanitize=address,undefined -fno-sanitize-recover=all] -o spread_sched_check spread_sched_check.cpp
//   ./spread_sched_check      (one line per band count and input: "NB steps max_rel_err exact_zeros"; exit status 0)
// tests/test_spread_schedule_host.py builds and runs it and holds the figures to their bounds.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../gstpeaq_amd/csrc/peaq_spread_sched.h"

#pragma STDC FP_CONTRACT OFF

static uint64_t rng_state = 88172645463325252ull;
static double uniform() {                              // xorshift64, (0, 1)
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (double)(rng_state >> 11) / 9007199254740992.;
}

static double pow_const(double x, int e) {             // by squaring, as the kernel's
  double pw = 1., sq = x;
  for (; e; e >>= 1) {
    if (e & 1) pw *= sq;
    if (e >> 1) sq *= sq;
  }
  return pw;
}

constexpr int W = kSpreadWave;
static void shift_up(double (&x)[W]) {                 // lane i <- lane i - 1, zero into lane 0
  for (int i = W - 1; i > 0; --i) x[i] = x[i - 1];
  x[0] = 0.;
}
static void lower_halves(double (&dst)[W], const double (&a)[W], const double (&b)[W]) {
  for (int i = 0; i < W; ++i) dst[i] = i < W / 2 ? a[i] : b[i - W / 2];
}

// up[b] = sum over i < b of ene[i] a[i]^(b - i), by the schedule; returns the number of steps
template <int NB>
static int spread_up_scheduled(const double* ene_b, const double* a_b, double* up_b) {
  constexpr int kLanes = spread_lanes(NB), kHelper = spread_helper_steps(NB), kFirst = spread_k0(NB),
                kBoundary = spread_boundary(NB);
  double ene[2][W], ae[2][W], far[2][W], far_copy[2][W], upper[2][W], back2[2][W];
  for (int lane = 0; lane < W; ++lane)
    for (int s = 0; s < 2; ++s) {
      const int b = 2 * lane + s;
      if (b < NB) {
        const double t2 = a_b[b], t4 = t2 * t2;
        ene[s][lane] = ene_b[b];
        ae[s][lane] = t2;
        upper[s][lane] = ene_b[b] * pow_const(t2, spread_exp_upper(NB, s));
        const double ph = pow_const(t2, spread_exp_helper(NB));
        far[s][lane] = upper[s][lane] * ph;
        far_copy[s][lane] = far[s][lane] * ph;
        back2[s][lane] = t4 > 1e-290 ? 1. / t4 : 0.;
      } else {
        ene[s][lane] = ae[s][lane] = far[s][lane] = far_copy[s][lane] = upper[s][lane] = back2[s][lane] = 0.;
      }
    }
  double u[W], v[W], wa0[W], wa1[W], wb0[W], wb1[W], up0[W] = {}, up1[W] = {};
  lower_halves(u, far[0], far_copy[0]);
  lower_halves(v, far[1], far_copy[1]);
  lower_halves(wa0, ae[0], ae[0]);
  lower_halves(wa1, ae[1], ae[1]);
  lower_halves(wb0, back2[0], back2[0]);
  lower_halves(wb1, back2[1], back2[1]);
  int steps = 0;
  for (int k = kFirst; k >= kBoundary; --k, ++steps) {
    for (int lane = 0; lane < W; ++lane)
      if (k <= spread_act(NB, lane)) {
        up0[lane] += u[lane];
        up0[lane] += v[lane];
        up1[lane] = std::fma(wa0[lane], u[lane], up1[lane]);
        up1[lane] = std::fma(wa1[lane], v[lane], up1[lane]);
      }
    shift_up(up0);
    shift_up(up1);
    for (int lane = 0; lane < W; ++lane) {
      u[lane] *= wb0[lane];
      v[lane] *= wb1[lane];
    }
  }
  double home0[W], home1[W];
  for (int lane = 0; lane < W; ++lane) {
    const bool lower = lane < kSpreadHelperBase;
    const int to = (lane + spread_home_shift(NB) + W) & (W - 1);
    home0[to] = lower ? 0. : up0[lane];
    home1[to] = lower ? 0. : up1[lane];
    if (!lower) {
      up0[lane] = up1[lane] = 0.;
      u[lane] = upper[0][lane];
      v[lane] = upper[1][lane];
    }
  }
  for (int k = kBoundary - 1; k >= 1; --k, ++steps) {
    for (int lane = 0; lane < W; ++lane) {
      up0[lane] += u[lane];
      up0[lane] += v[lane];
      up1[lane] = std::fma(ae[0][lane], u[lane], up1[lane]);
      up1[lane] = std::fma(ae[1][lane], v[lane], up1[lane]);
    }
    shift_up(up0);
    shift_up(up1);
    for (int lane = 0; lane < W; ++lane) {
      u[lane] *= back2[0][lane];
      v[lane] *= back2[1][lane];
    }
  }
  for (int lane = 0; lane <= kLanes; ++lane) {
    up0[lane] += home0[lane];
    up1[lane] += home1[lane];
    up1[lane] = std::fma(ae[0][lane], ene[0][lane], up1[lane]);
    up_b[2 * lane] = up0[lane];
    if (2 * lane + 1 < NB) up_b[2 * lane + 1] = up1[lane];
  }
  (void)kHelper;
  return steps;
}

template <int NB>
static int run(const char* name, int mode) {
  double ene[NB], a[NB], got[NB], want[NB] = {};
  for (int b = 0; b < NB; ++b) {
    a[b] = 0.3 + 0.699 * uniform();
    ene[b] = std::pow(10., -3. + 15. * uniform());      // [1e-3, 1e12]
    if (mode == 1) ene[b] = 0.;                          // no source at all
    if (mode == 2 && b < NB - 9) ene[b] = 0.;            // sources in the top lanes only
    if (mode == 3) a[b] = b % 3 ? 0.999 : 0.3;           // the steepest and the flattest slopes side by side
  }
  for (int i = 0; i + 1 < NB; ++i) {                     // Kabal (27) as the reference walks it
    double r = ene[i];
    for (int j = i + 1; j < NB; ++j) {
      r *= a[i];
      want[j] += r;
    }
  }
  const int steps = spread_up_scheduled<NB>(ene, a, got);
  double worst = 0.;
  bool zeros = true;
  for (int b = 0; b < NB; ++b) {
    if (want[b] == 0.)
      zeros = zeros && got[b] == 0.;
    else
      worst = std::fmax(worst, std::fabs(got[b] - want[b]) / want[b]);
  }
  std::printf("%d %s steps %d max_rel_err %.3e exact_zeros %d\n", NB, name, steps, worst, zeros ? 1 : 0);
  return 0;
}

int main() {
  static const char* names[] = {"random", "silent", "top_only", "slopes"};
  for (int mode = 0; mode < 4; ++mode) {
    run<109>(names[mode], mode);
    run<55>(names[mode], mode);
  }
  return 0;
}

// peaq_steps_math.h -- the arithmetic of the steps stage that needs no device (include/peaq_amd.h, "delay steps on the
// device"): which segments of a track look like a step of the delay (steps_candidates), a track rebuilt as pieces that
// jump where a step was located (steps_fit), where an output reads along pieces (pieces_index), how many outputs a pair
// keeps (pieces_keep).  peaq_steps.hip wraps these as peaq_steps_candidates, peaq_steps_fit, peaq_pieces_index and
// peaq_pieces_lengths, and its cut kernel evaluates pieces_find's search and drift_index itself;
// tools/steps_host_check.cpp includes this header alone, so that the host arithmetic runs under the sanitizers without
// the device runtime.  Plain C++: every operation here is rounded on its own.
#pragma once
#include "peaq_track_math.h"

#pragma clang fp contract(off)

constexpr uint32_t kStepNone = 1, kStepSpan = 2, kStepWeak = 4;   // PEAQ_STEP_F_NONE, _SPAN, _WEAK
constexpr uint32_t kPiecesRange = 2;                              // PEAQ_PIECES_F_RANGE

// one candidate: the segment, the interval that is searched, the two integer delays
struct StepCandidate {
  uint32_t k, lo, hi;
  int32_t LA, LB;
};
// what the locator found for one candidate (the fields of peaq_step the fit reads and writes)
struct StepFound {
  uint32_t c, flags;
  int32_t LA, LB;
  double gain_left, gain_right, norm;
};
struct PiecesSummary {
  uint32_t flags, n_candidates, n_accepted, n_pieces;
  double max_abs_e;
};

// segment k's line from the knots: track_fit's item 4, the same operations (so the same bits where the track kept them)
inline void steps_segment(const double* knots, uint32_t W, uint32_t window, uint32_t k, double* a, double* e) {
  if (W < 2) {
    *e = 0.;
    *a = W ? knots[0] : 0.;
    return;
  }
  *e = (knots[k + 1] - knots[k]) / (double)window;
  *a = knots[k] - *e * track_x(k, window);
}

// the first output of segment k: the first segment starts with the pair
inline uint32_t steps_start(uint32_t k, uint32_t window) { return k ? window / 2 + k * window : 0; }

// (i) the candidates among the S = max (W - 1, 1) segments of a track, in the order of k.  out: room for S entries.
inline uint32_t steps_candidates(const double* knots, uint32_t W, uint32_t window, uint32_t n_common, double min_step,
                                 double ratio, StepCandidate* out) {
  if (W < 2) return 0;
  const uint32_t S = W - 1;
  uint32_t n = 0;
  for (uint32_t k = 0; k < S; ++k) {
    const double D = std::fabs(knots[k + 1] - knots[k]);
    const double Dl = k ? std::fabs(knots[k] - knots[k - 1]) : 0.;
    const double Dr = k + 1 < S ? std::fabs(knots[k + 2] - knots[k + 1]) : 0.;
    if (!(D >= min_step) || !(D >= ratio * std::max(Dl, Dr))) continue;
    const double la = std::rint(knots[k]), lb = std::rint(knots[k + 1]);
    if (!(std::fabs(la) <= 2147483647.) || !(std::fabs(lb) <= 2147483647.) || la == lb) continue;
    StepCandidate c;
    c.k = k;
    c.lo = k * window;
    c.hi = (uint32_t)std::min<uint64_t>((uint64_t)(k + 2) * window, n_common);
    c.LA = (int32_t)la;
    c.LB = (int32_t)lb;
    if (c.lo >= c.hi) continue;                        // (n_common below the track's own windows: nothing to search)
    out[n++] = c;
  }
  return n;
}

// (ii) .. (iv): the pieces of one pair.  cand[n_cand] are steps_candidates' for the same knots; found[n_cand] the
// locator's records for them, whose flags gain kStepWeak where a step is not accepted.  b, a, e: room for
// S + n_cand entries.  A piece that would be empty is left out.
inline void steps_fit(const double* knots, uint32_t W, uint32_t window, const StepCandidate* cand, StepFound* found,
                      uint32_t n_cand, double min_gain, double max_e, uint32_t* b, double* a, double* e, PiecesSummary* out) {
  const uint32_t S = std::max<uint32_t>(W, 2) - 1;
  PiecesSummary r{};
  r.n_candidates = n_cand;
  // (ii) which segments step, and where
  std::vector<uint8_t> stepped(S, 0);
  std::vector<uint32_t> at(S, 0);
  for (uint32_t j = 0; j < n_cand; ++j) {
    StepFound& f = found[j];
    const bool ok = f.flags == 0 && std::min(f.gain_left, f.gain_right) >= min_gain * f.norm;
    if (!ok) {
      f.flags |= kStepWeak;
      continue;
    }
    stepped[cand[j].k] = 1;
    at[cand[j].k] = std::min(std::max(f.c, cand[j].lo), cand[j].hi);
    ++r.n_accepted;
  }
  // (iii) the pieces, in the order of the segments
  const uint64_t kEnd = ~0ull;                         // the last segment runs to the pair's end
  uint32_t n = 0;
  const auto put = [&](uint64_t from, uint64_t to, double pa, double pe) {
    if (from >= to) return;
    b[n] = (uint32_t)from;
    a[n] = pa;
    e[n] = pe;
    ++n;
  };
  for (uint32_t k = 0; k < S; ++k) {
    const uint64_t start = steps_start(k, window), end = k + 1 < S ? steps_start(k + 1, window) : kEnd;
    const bool left_steps = k && stepped[k - 1], right_steps = k + 1 < S && stepped[k + 1];
    double ak, ek;
    steps_segment(knots, W, window, k, &ak, &ek);
    if (!stepped[k]) {                                 // the track's segment, shortened where a neighbour's step reaches in
      const uint64_t from = left_steps ? std::max<uint64_t>(start, at[k - 1]) : start;
      const uint64_t to = right_steps ? std::min<uint64_t>(end, at[k + 1]) : end;
      put(from, to, ak, ek);
      continue;
    }
    // a step: the left neighbour's line up to c, the right neighbour's from c on; c reaches into a neighbour that is
    // no step itself, else it stops at the segment's own border
    uint64_t c = at[k];
    uint64_t from = start, to = end;
    if (c < start) {
      if (left_steps) c = start;
      else from = c;
    }
    if (c > end) {
      if (right_steps) c = end;
      else to = c;
    }
    double al = knots[k], el = 0., ar = W >= 2 ? knots[k + 1] : knots[k], er = 0.;
    if (k && !left_steps) steps_segment(knots, W, window, k - 1, &al, &el);
    if (k + 1 < S && !right_steps) steps_segment(knots, W, window, k + 1, &ar, &er);
    put(from, c, al, el);
    put(c, to, ar, er);
  }
  if (n == 0 || b[0] != 0) {                           // (cannot happen: the first segment or its pieces start at 0)
    n = 1;
    b[0] = 0;
    a[0] = e[0] = 0.;
  }
  // (iv) the range
  for (uint32_t j = 0; j < n; ++j) r.max_abs_e = std::max(r.max_abs_e, std::fabs(e[j]));
  if (r.max_abs_e > max_e) {
    r.flags = kPiecesRange;
    for (uint32_t j = 0; j < n; ++j) a[j] = e[j] = 0.;
  }
  r.n_pieces = n;
  *out = r;
}

// the piece of output i: the largest j with b[j] <= i (b[0] = 0, b strictly increasing, n >= 1, i >= 0)
PEAQ_DRIFT_HD uint32_t pieces_find(const uint32_t* b, uint32_t n, long long i) {
  uint32_t lo = 0, hi = n;                             // b[lo] <= i < b[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if ((long long)b[mid] <= i)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// where output i reads: drift_index along its piece's line
inline void pieces_index(uint32_t n, const uint32_t* b, const double* a, const double* e, long long i, long long* m, int* phi) {
  const uint32_t j = pieces_find(b, n, i);
  drift_index(a[j], e[j], i, m, phi);
}

// How many outputs stay: the largest count <= n_common with skip_test + i + m_i < n_test for every i below it.  Across a
// breakpoint i + m_i may fall by any amount (a negative jump), so no search over the whole pair finds it.  INSIDE a
// piece, |e| <= 1/64 moves 256 (a + e i) by at most 4 per output, which moves g = rint (...) by at most 5 grid steps,
// fewer than the 256 of a sample: m falls by at most 1 where i rises by 1, i + m_i does not decrease, and the outputs
// of a piece that fail the condition are its last ones.  So: piece by piece in their order, a binary search for the
// piece's first failing output; the first piece that has one ends the count there.
inline uint32_t pieces_keep(uint32_t n, const uint32_t* b, const double* a, const double* e, uint32_t skip_test,
                            uint32_t n_common, uint32_t n_test) {
  for (uint32_t j = 0; j < n; ++j) {
    if (b[j] >= n_common) break;
    const uint64_t end = j + 1 < n ? std::min<uint64_t>(b[j + 1], n_common) : n_common;
    uint64_t lo = b[j], hi = end;                      // the condition holds below lo and fails from hi on (within the piece)
    while (lo < hi) {
      const uint64_t mid = lo + (hi - lo) / 2;
      long long m;
      int phi;
      drift_index(a[j], e[j], (long long)mid, &m, &phi);
      if ((long long)skip_test + (long long)mid + m < (long long)n_test)
        lo = mid + 1;
      else
        hi = mid;
    }
    if (lo < end) return (uint32_t)lo;
  }
  return n_common;
}

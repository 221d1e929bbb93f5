// peaq_drift_math.h -- the arithmetic of the drift stage that needs no device (include/peaq_amd.h, "constant drift on the
// device"): where an output of the drift cut reads, how many outputs a pair keeps, the Theil-Sen fit.  peaq_drift.hip
// wraps these as peaq_drift_index, peaq_drift_lengths and peaq_drift_fit, and its kernel evaluates drift_index itself;
// tools/drift_host_check.cpp includes this header alone, so that the host arithmetic runs under the sanitizers without
// the device runtime.  Plain C++: every operation here is rounded on its own.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define PEAQ_DRIFT_HD __host__ __device__ __forceinline__
#else
#define PEAQ_DRIFT_HD inline
#endif

#pragma clang fp contract(off)

// peaq_drift_index (include/peaq_amd.h): the same FP64 operations on the host and on the device
PEAQ_DRIFT_HD void drift_index(double a, double e, long long i, long long* m, int* phi) {
  const long long g = (long long)__builtin_rint(256. * __builtin_fma(e, (double)i, a));
  *m = (g + 128) >> 8;                                 // floor: the shift of a signed value is arithmetic
  *phi = (int)(g - 256 * *m);
}

// how many outputs stay: the largest count <= n_common with skip_test + i + m_i < n_test for every i below it.  i + m_i
// never decreases with i (|e| < 1), so the outputs centred inside the signal's end are the first of them.
inline uint32_t drift_keep(double a, double e, uint32_t skip_test, uint32_t n_common, uint32_t n_test) {
  uint64_t lo = 0, hi = n_common;                      // the condition holds below lo and fails from hi on
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    long long m;
    int phi;
    drift_index(a, e, (long long)mid, &m, &phi);
    if ((long long)skip_test + (long long)mid + m < (long long)n_test)
      lo = mid + 1;
    else
      hi = mid;
  }
  return (uint32_t)lo;
}

// The delay d[w] of every window and whether it counts, from the windows' records of the aligner (Delay: lag, peak,
// norm) and of the sub-sample stage (Sub: q, flags) -- the public header's peaq_delay and peaq_subdelay, which this
// header does not need to know (tools/drift_host_check.cpp runs it on records of its own): a window counts where it
// has energy, a grid point, and a peak of min_corr of the norm.
template <typename Delay, typename Sub>
inline void window_delays(const Delay* dl, const Sub* sb, uint32_t W, double min_corr, double* d, uint8_t* valid) {
  for (uint32_t w = 0; w < W; ++w) {
    d[w] = (double)dl[w].lag + (double)sb[w].q / 256.;
    valid[w] = std::isfinite(dl[w].norm) && dl[w].norm > 0. && sb[w].flags == 0 &&
               std::fabs(dl[w].peak) >= min_corr * dl[w].norm;
  }
}

// the middle one of v's values, the mean of the two middle ones for an even count (what a sort would put there)
inline double median_of(std::vector<double>& v) {
  const size_t n = v.size(), h = n / 2;
  std::nth_element(v.begin(), v.begin() + h, v.end());
  const double hi = v[h];
  if (n & 1) return hi;
  const double lo = *std::max_element(v.begin(), v.begin() + h);
  return (lo + hi) / 2.;
}

// the fit over the valid points; the number of them
inline size_t theil_sen(const double* d, const double* x, const uint8_t* valid, size_t n, double* a, double* e) {
  std::vector<size_t> idx;
  for (size_t w = 0; w < n; ++w)
    if (!valid || valid[w]) idx.push_back(w);
  *a = *e = 0.;
  const size_t nv = idx.size();
  if (nv < 3) return nv;
  std::vector<double> v;
  v.reserve(nv * (nv - 1) / 2);
  for (size_t i = 0; i < nv; ++i)
    for (size_t j = i + 1; j < nv; ++j) v.push_back((d[idx[j]] - d[idx[i]]) / (x[idx[j]] - x[idx[i]]));
  const double slope = median_of(v);
  v.clear();
  for (size_t i = 0; i < nv; ++i) v.push_back(d[idx[i]] - slope * x[idx[i]]);
  *a = median_of(v);
  *e = slope;
  return nv;
}


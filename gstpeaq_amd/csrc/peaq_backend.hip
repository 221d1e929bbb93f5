// peaq_backend.hip -- the stateful half of the PEAQ path: everything that
// carries state from one frame to the next.  One workgroup per pair, one
// wavefront per channel, frames processed in order; a lane owns two critical
// bands (one for the 40-band filter bank) and keeps their recurrent state in
// registers; lane i additionally owns MOV accumulator i of its channel (its
// twelve fields and the per-band constants live in LDS).
//
// Reference functions restated here (file:line under /root/reference/src):
//   time smearing                    fftearmodel.c:496-504
//   level + pattern adaptation       leveladapter.c:243-340
//   modulation patterns              modpatt.c:223-251
//   loudness gate                    earmodel.c:891-907, gstpeaq.c:841-845
//   modulation difference MOVs       movs.c:205-254
//   noise loudness MOVs              movs.c:354-371, 551-577, 679-743
//   NMR / relative disturbed frames  movs.c:1002-1022
//   detection probability MOVs       movs.c:1224-1276
//   accumulation + tentative logic   movaccum.c:317-425, gstpeaq.c:858-920, 965-1010
//   read-out, DI, ODG                movaccum.c:438-481, nn.c:187-216,304-335,372-375
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdlib>

#include "peaq_device.h"
#include "peaq_kernels.h"
#include "peaq_wave.h"
#ifdef PEAQ_DEV_PROBES                               // VARIANT builds only (csrc/Makefile): never in the product library
#define PEAQ_DEV_TU_BACKEND
#include "dev_probes.inc"
#endif
#ifndef PEAQ_DEV_SPIN_INSTEAD_OF_BACKEND
#define PEAQ_DEV_SPIN_INSTEAD_OF_BACKEND(a, block, stream)
#endif

namespace peaq {

constexpr int kLdsBands = 128;      // 2 bands x 64 lanes: every lane may store, only valid bands are read
// pattern-adaptation ratios in LDS: kPaPad zeros, 128 band slots (zero beyond the last band), spare
constexpr int kPaPad = 4, kPaStride = kPaPad + kLdsBands + 4;

// ---------------------------------------------------------------------------
// MOV accumulator owned by one lane (movaccum.c)
// ---------------------------------------------------------------------------
// The twelve fields live in LDS (field k of the accumulator at f[k * kAccLdsStride]); they are
// touched once per frame, registers are better spent on the band state.
constexpr int kAccLdsStride = 16;
struct LaneAcc {
  double* f;
  int mode, status;
  enum { NUM, DEN, NUM2, P0, P1, P2, MX, FILT, S_NUM, S_DEN, S_NUM2, S_MX };
  __device__ __forceinline__ double& at(int k) const { return f[k * kAccLdsStride]; }

  __device__ __forceinline__ void load(double* lds, const double* g, int mode_, int status_) {
    f = lds;
#pragma unroll
    for (int k = 0; k < kAccFields; ++k) at(k) = g[k];
    mode = mode_;
    status = status_;
  }
  __device__ __forceinline__ void store(double* g) const {
#pragma unroll
    for (int k = 0; k < kAccFields; ++k) g[k] = at(k);
  }
  // movaccum.c:317-362
  __device__ __forceinline__ void set_tentative(bool tentative) {
    if (tentative) {
      if (status == kNormal) {
        at(S_NUM) = at(NUM);
        at(S_DEN) = at(DEN);
        at(S_NUM2) = at(NUM2);
        at(S_MX) = at(MX);         // FILTERED_MAX: only `max`, not the filter state (:343-346)
        status = kTentative;
      }
    } else {
      status = kNormal;
    }
  }
  // movaccum.c:368-425
  __device__ __forceinline__ void add(double val, double w) {
    if (status == kInit) return;
    switch (mode) {
      case kRms:
        w *= w;
        at(NUM) += w * val * val;
        at(DEN) += w;
        break;
      case kRmsAsym:
        at(NUM) += val * val;
        at(NUM2) += w * w;
        at(DEN) += 1.;
        break;
      case kAvg:
      case kAvgLog:
      case kAdb:
        at(NUM) += w * val;
        at(DEN) += w;
        break;
      case kAvgWindow: {
        const double sq = sqrt(val);
        const double p0 = at(P0), p1 = at(P1), p2 = at(P2);
        if (!isnan(p0)) {
          double ws = ((sq + p0) + p1) + p2;
          ws /= 4.;
          ws *= ws;
          ws *= ws;
          at(NUM) += ws;
          at(DEN) += 1.;
        }
        at(P0) = p1;
        at(P1) = p2;
        at(P2) = sq;
        break;
      }
      case kFilteredMax: {
        const double filt = 0.9 * at(FILT) + 0.1 * val;
        at(FILT) = filt;
        if (filt > at(MX)) at(MX) = filt;
        break;
      }
    }
  }
};

__device__ __forceinline__ int acc_mode(bool advanced, int i) {
  // gstpeaq.c:528-557
  if (advanced) return i == 0 ? kRms : i == 1 ? kRmsAsym : kAvg;
  switch (i) {
    case 2: return kAvgLog;
    case 3: return kAvgWindow;
    case 4: return kAdb;
    case 8: return kRms;
    case 9: return kFilteredMax;
    default: return kAvg;
  }
}

// value of one channel's accumulator (movaccum.c:448-477, per-channel term)
__device__ __forceinline__ double acc_channel_value(int mode, bool tentative, const double* f) {
  const double num = tentative ? f[8] : f[0], den = tentative ? f[9] : f[1];
  const double num2 = tentative ? f[10] : f[2], mx = tentative ? f[11] : f[6];
  switch (mode) {
    case kAvg: return num / den;
    case kAvgLog: return 10. * log10(num / den);
    case kAvgWindow:
    case kRms: return sqrt(num / den);
    case kRmsAsym: return sqrt(num / den) + 0.5 * sqrt(num2 / den);
    case kFilteredMax: return mx;
    case kAdb: return den > 0 ? (num == 0. ? -0.5 : log10(num / den)) : 0.;
  }
  return 0.;
}

// ---------------------------------------------------------------------------
// shared per-frame building blocks; SLOTS bands per lane, band b = SLOTS*lane + s
// ---------------------------------------------------------------------------
template <int NB, int SLOTS>
struct BandLane {
  int lane;
  __device__ __forceinline__ int band(int s) const { return SLOTS * lane + s; }
  __device__ __forceinline__ bool valid(int s) const { return band(s) < NB; }
};

// Per-band constants as the building blocks see them: straight from the tables in global memory
// (filter-bank back end), or from a copy in LDS (FFT back end: nine tables x two bands would
// otherwise sit in 36 registers for the whole frame loop -- or be spilled).
struct GlobalTabs {
  const BandTables* __restrict__ p;
  __device__ __forceinline__ double adapt_tc(int b) const { return p->adapt_tc[b]; }
  __device__ __forceinline__ double ear_tc(int b) const { return p->ear_tc[b]; }
  __device__ __forceinline__ double threshold(int b) const { return p->threshold[b]; }
  __device__ __forceinline__ double loud_factor(int b) const { return p->loud_factor[b]; }
  __device__ __forceinline__ double exc_threshold(int b) const { return p->exc_threshold[b]; }
  __device__ __forceinline__ double internal_noise(int b) const { return p->internal_noise[b]; }
  __device__ __forceinline__ double noise_pow03(int b) const { return p->noise_pow03[b]; }
  __device__ __forceinline__ double mask_diff(int b) const { return p->mask_diff[b]; }
  __device__ __forceinline__ double ln_internal_noise(int b) const { return p->ln_internal_noise[b]; }
  __device__ __forceinline__ double inv_window_count(int b) const { return p->inv_window_count[b]; }
  __device__ __forceinline__ double deriv_factor() const { return p->deriv_factor; }
  // transcendentals of the MOV layer: the logarithm from the table in LDS (see LdsTabs)
  const double* ltab;
  const double* etab;               // ... and the exponential from its own (exp_tab, peaq_wave.h)
#if defined(PEAQ_LEDGER_FP32_BACKEND) || defined(PEAQ_NO_LOGTAB_BE)
  __device__ __forceinline__ double log(double x) const { return be_log(x); }
  __device__ __forceinline__ double exp(double x) const { return be_exp(x); }
  __device__ __forceinline__ double pow(double x, double y) const { return be_pow(x, y); }
#else
  __device__ __forceinline__ double log(double x) const { return log_tab(x, ltab); }
  __device__ __forceinline__ double exp(double x) const { return exp_tab(x, etab); }
  __device__ __forceinline__ double pow(double x, double y) const { return exp_tab(y * log_tab(x, ltab), etab); }
#endif
};
enum { T_ADAPT, T_EAR, T_THR, T_LOUDF, T_EXCTHR, T_INOISE, T_NPOW03, T_MASK, T_ISN, T_ISN03, T_LNINOISE, T_RCNT, T_COUNT };
struct LdsTabs {
  const double* t;                  // [T_COUNT][kBandStride] in LDS
  int off;                          // 0, but opaque to the compiler (re-read per frame, not hoisted)
  double deriv;
  __device__ __forceinline__ double at(int tab, int b) const { return t[off + tab * kBandStride + b]; }
  __device__ __forceinline__ double adapt_tc(int b) const { return at(T_ADAPT, b); }
  __device__ __forceinline__ double ear_tc(int b) const { return at(T_EAR, b); }
  __device__ __forceinline__ double threshold(int b) const { return at(T_THR, b); }
  __device__ __forceinline__ double loud_factor(int b) const { return at(T_LOUDF, b); }
  __device__ __forceinline__ double exc_threshold(int b) const { return at(T_EXCTHR, b); }
  __device__ __forceinline__ double internal_noise(int b) const { return at(T_INOISE, b); }
  __device__ __forceinline__ double noise_pow03(int b) const { return at(T_NPOW03, b); }
  __device__ __forceinline__ double mask_diff(int b) const { return at(T_MASK, b); }
  __device__ __forceinline__ double ln_internal_noise(int b) const { return at(T_LNINOISE, b); }
  __device__ __forceinline__ double inv_window_count(int b) const { return at(T_RCNT, b); }
  __device__ __forceinline__ double deriv_factor() const { return deriv; }
  // transcendentals of the MOV layer: the logarithm from the 129-entry table in LDS (log_tab, peaq_wave.h) --
  // ten logarithms per band and frame are a tenth of this kernel's vector instructions otherwise
  const double* ltab;               // [kLogTabEntries][2] in LDS
  // (the exponential stays the polynomial here: this kernel runs beside the front end, whose LDS array is the busier
  // unit -- with exp_tab the basic step measured 0 ... - 1 %, the filter-bank back end above + 0.8 % on its pass)
#if defined(PEAQ_LEDGER_FP32_BACKEND) || defined(PEAQ_NO_LOGTAB_BE)
  __device__ __forceinline__ double log(double x) const { return be_log(x); }
  __device__ __forceinline__ double exp(double x) const { return be_exp(x); }
  __device__ __forceinline__ double pow(double x, double y) const { return be_pow(x, y); }
#else
  __device__ __forceinline__ double log(double x) const { return log_tab(x, ltab); }
  __device__ __forceinline__ double exp(double x) const { return be_exp(x); }
  __device__ __forceinline__ double pow(double x, double y) const { return be_exp(y * log_tab(x, ltab)); }
#endif
};

// leveladapter.c:243-340.  e_ref/e_test: excitation patterns of this frame.
// st: [6][SLOTS] state (filt_ref, filt_test, num, den, pattcorr_ref, pattcorr_test)
template <int NB, int SLOTS, class TAB>
__device__ __forceinline__ void level_adapt(const BandLane<NB, SLOTS>& bl, const TAB& bt,
                                            const double (&e_ref)[SLOTS], const double (&e_test)[SLOTS],
                                            double (&st)[6][SLOTS], double* pa_lds /* [2][kPaStride], zero padded */,
                                            double (&ad_ref)[SLOTS], double (&ad_test)[SLOTS]) {
  double num = 0., den = 0.;
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    if (bl.valid(s)) {
      const double a = bt.adapt_tc(bl.band(s));
      st[0][s] = a * st[0][s] + (1 - a) * e_ref[s];          // (42)/(43) in BS.1387
      st[1][s] = a * st[1][s] + (1 - a) * e_test[s];
      num += sqrt_pos(st[0][s] * st[1][s]);                  // (45)
      den += st[1][s];
    }
  }
  wave_sum2(num, den, num, den);
  // lev = (num / den)^2 and its reciprocal, once per wave; the quotients of the per-band loop below
  // are products with reciprocals that exist anyway (1 ulp from the reference's divisions)
  const double n2 = num * num, d2 = den * den;
  const double lev = div_fast(n2, d2), inv_lev = div_fast(d2, n2);
  double lc_ref[SLOTS], lc_test[SLOTS];
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    if (lev > 1) {                                           // (46)/(47)
      lc_ref[s] = e_ref[s] * inv_lev;
      lc_test[s] = e_test[s];
    } else {
      lc_ref[s] = e_ref[s];
      lc_test[s] = e_test[s] * lev;
    }
    double pr = 0., pt = 0.;
    if (bl.valid(s)) {
      const double a = bt.adapt_tc(bl.band(s));
      st[2][s] = a * st[2][s] + lc_test[s] * lc_ref[s];      // (48): no (1-a) gain, leveladapter.c:293-298
      st[3][s] = a * st[3][s] + lc_ref[s] * lc_ref[s];
      if (st[2][s] >= st[3][s]) {                            // (49)
        pr = 1.;
        pt = div_fast(st[3][s], st[2][s]);
      } else {
        pr = div_fast(st[2][s], st[3][s]);
        pt = 1.;
      }
    }
    pa_lds[kPaPad + bl.band(s)] = pr;                        // 0 for the slots beyond the last band
    pa_lds[kPaStride + kPaPad + bl.band(s)] = pt;
  }
  wave_lds_fence();
  constexpr int M1 = NB / 36, M2 = NB / 25;                  // leveladapter.c:315-316
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    ad_ref[s] = 0.;
    ad_test[s] = 0.;
    if (bl.valid(s)) {
      const int k = bl.band(s);
      // (50)/(51): window [k - m1, k + m2] summed in ascending order like the reference.  The
      // array is zero outside [0, NB), so the full window [k - M1, k + M2] gives the same sums
      // bit for bit (x + 0 = x) with compile-time offsets from one address.
      double rr = 0., rt = 0.;
#pragma unroll
      for (int j = -M1; j <= M2; ++j) {
        rr += pa_lds[kPaPad + k + j];
        rt += pa_lds[kPaStride + kPaPad + k + j];
      }
      const double rcnt = bt.inv_window_count(k);            // 1 / (m1 + m2 + 1)
      rr *= rcnt;
      rt *= rcnt;
      const double a = bt.adapt_tc(k);
      st[4][s] = a * st[4][s] + (1 - a) * rr;
      st[5][s] = a * st[5][s] + (1 - a) * rt;
      ad_ref[s] = lc_ref[s] * st[4][s];                      // (52)/(53)
      ad_test[s] = lc_test[s] * st[5][s];
    }
  }
  wave_lds_fence();
}

// modpatt.c:223-251; st: prev_loud, filt_loud, filt_dloud
// PIN (summary instantiation, whose test-side state comes from LDS): the two filters spelt out as the compiler contracts
// them where the state sits in registers -- filt_dloud rounds (1 - a) dl and fuses a st, filt_loud rounds a st and fuses
// (1 - a) loud.  With the state from LDS it fuses a st in both, and the results would not be peaq_batch_run's to the bit.
template <int NB, int SLOTS, class TAB, bool PIN = false>
__device__ __forceinline__ void modulation(const BandLane<NB, SLOTS>& bl, const TAB& bt,
                                           const double (&loud)[SLOTS], double (&st)[3][SLOTS],
                                           double (&mod)[SLOTS]) {
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    mod[s] = 0.;
    if (bl.valid(s)) {
      const double a = bt.adapt_tc(bl.band(s));
      const double dl = bt.deriv_factor() * fabs(loud[s] - st[0][s]);
      if (PIN) {
        st[2][s] = __builtin_fma(a, st[2][s], (1 - a) * dl);
        st[1][s] = __builtin_fma(1. - a, loud[s], a * st[1][s]);
      } else {
        st[2][s] = a * st[2][s] + (1 - a) * dl;
        st[1][s] = a * st[1][s] + (1. - a) * loud[s];
      }
      mod[s] = div_fast(st[2][s], 1. + st[1][s] * (1. / 0.3));
      st[0][s] = loud[s];
    }
  }
}

// earmodel.c:891-907
template <int NB, int SLOTS, class TAB>
__device__ __forceinline__ double total_loudness_part(const BandLane<NB, SLOTS>& bl, const TAB& bt,
                                                      const double (&exc)[SLOTS]) {
  double t = 0.;
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    if (bl.valid(s)) {
      const int b = bl.band(s);
      const double thr = bt.threshold(b);
      const double l = bt.loud_factor(b) * (bt.pow(1. - thr + div_fast(thr * exc[s], bt.exc_threshold(b)), 0.23) - 1.);
      t += fmax(l, 0.);
    }
  }
  return t;
}

// movs.c:709-743.  `lead`: the factor (ethres / stest)^0.23 per slot -- computed here (KEEP: and handed back) or taken
// from a call with the same thres_fac, s0 and mod_test (USE): RmsNoiseLoudAsym's missing-components term and AvgLinDist
// (movs.c:551-577, 679-706) share it, a logarithm and an exponential per band and block.
enum LeadMode { LEAD_OWN, LEAD_KEEP, LEAD_USE };
// (the lane's part of the sum over the bands: callers with several sums in a frame take them through ONE reduction,
// wave_sum2 / wave_sum4, and finish with noise_loudness_total)
// TERMS (pattern-bands and summary instantiations only): every slot's term of that sum also goes to terms[s], 0 for a
// slot beyond the last band -- the very value the sum adds, so a band below the hinge reads exactly 0.
template <int NB, int SLOTS, class TAB, LeadMode LM = LEAD_OWN, bool TERMS = false>
__device__ __forceinline__ double noise_loudness_part(const BandLane<NB, SLOTS>& bl, const TAB& bt,
                                                      double alpha, double thres_fac, double s0,
                                                      const double (&mod_ref)[SLOTS], const double (&mod_test)[SLOTS],
                                                      const double (&e_ref)[SLOTS], const double (&e_test)[SLOTS],
                                                      double* lead = nullptr, double* terms = nullptr) {
  double nl = 0.;
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    if (TERMS) terms[s] = 0.;
    if (bl.valid(s)) {
      const double sref = thres_fac * mod_ref[s] + s0;
      const double stest = thres_fac * mod_test[s] + s0;
      const double ethres = bt.internal_noise(bl.band(s));
      const double beta = bt.exp(div_fast(-alpha * (e_test[s] - e_ref[s]), e_ref[s]));
      // (ethres / stest)^0.23 from the logarithms: ln ethres is a table entry
      double ld;
      if (LM == LEAD_USE)
        ld = lead[s];
      else
        ld = bt.exp(0.23 * (bt.ln_internal_noise(bl.band(s)) - bt.log(stest)));
      if (LM == LEAD_KEEP) lead[s] = ld;
      if (!TERMS) {
        nl += ld *
              (bt.pow(1. + div_fast(fmax(stest * e_test[s] - sref * e_ref[s], 0.), ethres + sref * e_ref[s] * beta), 0.23) -
               1.);
      } else {                                       // the same product, named: the sum adds what the caller stores
        const double t =
            ld *
            (bt.pow(1. + div_fast(fmax(stest * e_test[s] - sref * e_ref[s], 0.), ethres + sref * e_ref[s] * beta), 0.23) - 1.);
        nl += t;
        terms[s] = t;
      }
    }
  }
  return nl;
}
template <int NB>
__device__ __forceinline__ double noise_loudness_total(double sum, double nl_min) {
  const double nl = sum * (24. / NB);
  return nl < nl_min ? 0. : nl;
}

// movs.c:224-251: returns d1 (un-normalised), d2, weight
// TERMS (pattern-bands and summary instantiations only): every slot's terms of the three sums also go to
// terms[0..2][s], 0 for a slot beyond the last band.
template <int NB, int SLOTS, class TAB, bool TERMS = false>
__device__ __forceinline__ void mod_difference(const BandLane<NB, SLOTS>& bl, const TAB& bt,
                                               double lev_wt, const double (&mr)[SLOTS], const double (&mt)[SLOTS],
                                               const double (&loud_ref)[SLOTS], double& d1, double& d2, double& wt,
                                               double (*terms)[SLOTS] = nullptr) {
  double a1 = 0., a2 = 0., aw = 0.;
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    if (TERMS) terms[0][s] = terms[1][s] = terms[2][s] = 0.;
    if (bl.valid(s)) {
      const double diff = fabs(mr[s] - mt[s]);
      if (!TERMS) {
        a1 += div_fast(diff, 1. + mr[s]);
        a2 += div_fast((mt[s] >= mr[s] ? 1. : .1) * diff, 0.01 + mr[s]);
        aw += div_fast(loud_ref[s], loud_ref[s] + lev_wt * bt.noise_pow03(bl.band(s)));
      } else {                                       // the same quotients, named: the sums add what the caller stores
        a1 += terms[0][s] = div_fast(diff, 1. + mr[s]);
        a2 += terms[1][s] = div_fast((mt[s] >= mr[s] ? 1. : .1) * diff, 0.01 + mr[s]);
        aw += terms[2][s] = div_fast(loud_ref[s], loud_ref[s] + lev_wt * bt.noise_pow03(bl.band(s)));
      }
    }
  }
  double unused;
  wave_sum4(a1, a2, aw, 0., d1, d2, wt, unused);
}

// ---------------------------------------------------------------------------
// Reading points of a trajectory (PointArgs, peaq_batch_run_trajectory): point k of a pair falls on the frame (FB:
// block) after which the pair has processed F(a_k) frames (B(a_k) blocks), a_k = min((k + 1) interval, n_ref, n_test),
// F(a) = a >= 2048 ? (a - 2048) / 1024 + 1 : 0 (do_processing, gstpeaq.c:596-611), B(a) = a / 192.  Every quantity is
// wave-uniform: the first pending point is found once per workgroup, then one comparison per frame (block) tells
// whether the next one is due.  The walk's state is in LDS, one copy per wave that all its lanes write alike, and is
// read back as scalars where it is used: kept in registers across the frame loop it cost the basic back end registers
// it does not have.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_uniform(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
template <bool FB>
struct PointWalk {
  PointSnap* row;                   // this pair's snapshots
  uint32_t n_min, interval;
  int n_points, k;                  // k: the next point to take
  uint32_t due;                     // F(a_k) / B(a_k): the count after which point k is taken (UINT_MAX: none left)
  __device__ __forceinline__ static uint32_t count(uint32_t a) {
    return FB ? a / kFbFrame : a >= (uint32_t)kFrame ? (a - kFrame) / kHop + 1 : 0u;
  }
  __device__ __forceinline__ void set_due(int k1) {
    k = k1;
    if (k1 >= n_points) {
      due = UINT_MAX;
      return;
    }
    const uint64_t t = (uint64_t)(k1 + 1) * interval;
    due = count(t < n_min ? (uint32_t)t : n_min);
  }
  // c0: frames (blocks) the pair has processed before this launch -- the first pending point has a count above it
  __device__ __forceinline__ void init(const PointArgs& p, unsigned pair, uint32_t c0) {
    row = p.snap + (size_t)pair * p.n_points;
    const uint32_t nr = p.n_ref ? p.n_ref[pair] : p.n_uniform, nt = p.n_test ? p.n_test[pair] : p.n_uniform;
    n_min = nr < nt ? nr : nt;
    interval = p.interval;
    n_points = p.n_points;
    const uint64_t thr = FB ? (uint64_t)kFbFrame * (c0 + 1ull) : (uint64_t)kFrame + (uint64_t)kHop * c0;   // a_k >= thr
    const uint64_t k0 = n_min < thr ? (uint64_t)n_points : (thr + interval - 1) / interval - 1;
    set_due(k0 < (uint64_t)n_points ? (int)k0 : n_points);
  }
  // the snapshot to write after count c, or nullptr; advances to the next point
  __device__ __forceinline__ PointSnap* take(uint32_t c) {
    if (wave_uniform(due) != c) return nullptr;
    const int k1 = (int)wave_uniform((uint32_t)k);
    const uint64_t r = reinterpret_cast<uint64_t>(row);
    PointSnap* sp = reinterpret_cast<PointSnap*>(((uint64_t)wave_uniform((uint32_t)(r >> 32)) << 32) |
                                                 wave_uniform((uint32_t)r)) + k1;
    set_due(k1 + 1);
    return sp;
  }
};

// ---------------------------------------------------------------------------
// Band traces (BandArgs, peaq_batch_run_bands): one plane's two values of a lane -- its bands 2 lane and 2 lane + 1 --
// as one 16-byte store into the row of (pair, frame, channel), `cell` = (pair frame_stride + frame) channels + channel.
// The plane test is on a kernel argument, so wave-uniform; the row's pad entry (band NB of NB + 1) belongs to the lane
// that owns band NB - 1, whose v1 the caller hands over as 0, and the lanes beyond it store nothing.
// ---------------------------------------------------------------------------
// (ARGS: BandArgs, or PatternBandArgs of peaq_batch_run_pattern_bands -- the same rows and slots)
template <int NB, class ARGS>
__device__ __forceinline__ void band_store(const ARGS& bnd, uint32_t bit, size_t cell, int lane, double v0, double v1) {
  if (!(bnd.planes & bit)) return;
  const unsigned n_planes = __builtin_popcount(bnd.planes), slot = __builtin_popcount(bnd.planes & (bit - 1u));
  // (a uniform row address and the lane's 32-bit byte offset: the store takes them as they are, no 64-bit lane address)
  char* __restrict__ row = reinterpret_cast<char*>(bnd.bands + (cell * n_planes + slot) * band_row(NB));
  unsigned off = (unsigned)lane * 16u;
  asm volatile("" : "+v"(off));                      // (made here, not kept as a 64-bit lane address across the frame loop)
  if (2 * lane < NB) *reinterpret_cast<double2*>(row + off) = make_double2(v0, v1);
}

// Filter-bank band traces (FbBandArgs, peaq_batch_run_fb_bands): one plane's value of a lane -- its band -- into the row
// of `row0` + the plane's slot, rows of kFbBands doubles.  The plane test is on a kernel argument, so wave-uniform, and
// so is the row address; the lane adds a 32-bit byte offset, and the lanes beyond the last band store nothing.
__device__ __forceinline__ void fb_band_store(const FbBandArgs& bnd, uint32_t bit, size_t row0, int lane, double v) {
  if (!(bnd.planes & bit)) return;
  const unsigned slot = __builtin_popcount(bnd.planes & (bit - 1u));
  char* __restrict__ row = reinterpret_cast<char*>(bnd.bands + (row0 + slot) * kFbBands);
  unsigned off = (unsigned)lane * 8u;
  asm volatile("" : "+v"(off));                      // (made here, not kept as a 64-bit lane address across the block loop)
  if (lane < kFbBands) *reinterpret_cast<double*>(row + off) = v;
}

// Filter-bank band summary (FbSummaryArgs, peaq_batch_run_fb_band_summary): a channel's running rows sit in LDS, rows of
// kFbSumRow doubles; lane b owns entry b of every row and is the only one to touch it (no barrier).  Lane 40 owns the
// denominators and is handed the denominator's increment in place of a band value, lane 41 the zero behind them.
__device__ __forceinline__ double fb_summary_pick(int lane, double band_value, double den) {
  return lane < kFbBands ? band_value : lane == kFbBands ? den : 0.;
}
__device__ __forceinline__ void fb_summary_add(double* entry, bool own, double v) {
  if (own) *entry += v;
}
// the rows of one channel, a lane's entry of each: LDS <-> the caller's array, LDS -> the saved copy
__device__ __forceinline__ void fb_summary_copy(double* dst, const double* src, bool own) {
  if (!own) return;
#pragma unroll
  for (int k = 0; k < kFbSumRows; ++k) {
    asm volatile("" ::: "memory");                   // row by row (rare): one row's register, not seven at once
    dst[k * kFbSumRow] = src[k * kFbSumRow];
  }
}

// ---------------------------------------------------------------------------
// Band summary (SummaryArgs, peaq_batch_run_band_summary): a channel's running rows sit in LDS, rows of ROW doubles; a
// lane owns the two entries 2 lane and 2 lane + 1 of every row and is the only one to touch them (no barrier).  NB is
// odd, so the lane that owns band NB - 1 owns the row's denominator (entry NB) as its second entry: callers hand that
// lane the denominator's increment in place of a band value (`last`).
// ---------------------------------------------------------------------------
// row += (v0, v1): one 16-byte read-modify-write
__device__ __forceinline__ void summary_add(double* row, bool own, double v0, double v1) {
  if (!own) return;
  double2* __restrict__ p = reinterpret_cast<double2*>(row);
  double2 v = *p;
  v.x += v0;
  v.y += v1;
  *p = v;
}
// row = max (row, (v0, v1)); the denominator counts
__device__ __forceinline__ void summary_max(double* row, bool own, bool last, double v0, double v1) {
  if (!own) return;
  double2* __restrict__ p = reinterpret_cast<double2*>(row);
  double2 v = *p;
  if (v0 > v.x) v.x = v0;
  if (last)
    v.y += 1.;
  else if (v1 > v.y)
    v.y = v1;
  *p = v;
}
// the R rows of one channel, a lane's entries of each: LDS <-> the caller's array, LDS -> the saved copy
template <int R, int ROW>
__device__ __forceinline__ void summary_copy(double* dst, const double* src, bool own) {
  if (!own) return;
#pragma unroll
  for (int k = 0; k < R; ++k) {
    asm volatile("" ::: "memory");                   // row by row (rare): one row's registers, not R rows' at once
    *reinterpret_cast<double2*>(dst + k * ROW) = *reinterpret_cast<const double2*>(src + k * ROW);
  }
}

// ---------------------------------------------------------------------------
// FFT-model back end.  ADV = false: basic version (109 bands, 11 MOVs).
// ADV = true: the FFT part of the advanced version (55 bands; SegmentalNMR, EHS).
// ---------------------------------------------------------------------------
enum { MB_BW_REF, MB_BW_TEST, MB_NMR, MB_WINMOD, MB_ADB, MB_EHS, MB_AVGMOD1, MB_AVGMOD2, MB_NOISELOUD, MB_MFPD,
       MB_RELDIST };                                         // gstpeaq.c:95-108
enum { MA_RMSMOD, MA_NLASYM, MA_SEGNMR, MA_EHS, MA_LINDIST };   // gstpeaq.c:86-93

struct BackendShared {
  double pa[2][2][kPaStride];       // [wave][ref/test][pad + band] pattern-adaptation ratios
  double pc[2][kLdsBands];          // exponents xb of the detection probabilities 1 - 0.5^xb, per channel
  double qc[2][kLdsBands];
  double acc[2][kAccFields][kAccLdsStride];   // [channel][field][accumulator]
  int gate[2];
};

// 3 waves per SIMD requested: the back end runs BESIDE the front end of the next chunk (which
// holds 3 x 168 VGPRs per SIMD); with the default budget (256) it could never be co-scheduled
// DBG = true (basic version only, peaq_debug_backend): the per-frame patterns are also written to
// a.debug for the stage-level parity tests; the arithmetic is the same instantiation otherwise.
// PTS = true (backend_points_kernel, trajectory launches only): after each frame the reading points that fall on it
// get a snapshot (PointWalk); the arithmetic is the same as the plain instantiation's.
// TRC = true (backend_trace_kernel, trace launches only): the MOV values are computed for every frame, as with DBG, and
// one lane per (frame, channel) writes them as a compact record (TraceArgs) -- no pattern dump.
// BND = true (backend_bands_kernel, band-trace launches only): every lane stores the per-band values of its two bands
// where they come up (BandArgs, band_store); the arithmetic and the gates are the plain instantiation's.
// PBD = true (backend_pattern_bands_kernel, pattern-band launches of the basic version only): the modulation differences
// and the noise loudness are evaluated for every frame, as with TRC, and every lane stores its two bands' terms and
// patterns where they come up (PatternBandArgs, band_store); the accumulators see what the gates admit.
// SUM = true (backend_summary_kernel, summary launches only): every lane adds its two bands' values of the counted
// frames to the channel's running rows in LDS where they come up (SummaryArgs, summary_add); the arithmetic and the
// gates are the plain instantiation's, and a frame whose gate is closed evaluates nothing more than there.
// WARM = true (the plain instantiations, which every scoring run goes through): channel 0's wave asks the next frame's
// record(s) into L2 behind the frame's own loads.  It holds one register through the frame, which the 109-band
// instantiations with an output of their own, and the debug one, do not have to spare without spilling: they run
// without it.  -DPEAQ_BE_NO_WARM (VARIANT builds): no kernel has it, for the A/B of the touch alone.
#ifdef PEAQ_BE_NO_WARM
constexpr bool kBackendWarm = false;
#else
constexpr bool kBackendWarm = true;
#endif
template <int NB, bool ADV, bool DBG = false>
__global__ __launch_bounds__(128, 3) void backend_kernel(BackendArgs a) {
  constexpr bool PTS = false, TRC = false, LIVE = false, BND = false, PBD = false, SUM = false, WARM = kBackendWarm && !DBG;
  constexpr SummaryArgs sum{};
  constexpr PointArgs pts{};
  constexpr TraceArgs trc{};
  constexpr BandArgs bnd{};
  constexpr PatternBandArgs pbd{};
#include "peaq_backend_fft.inc"
}
// The points instantiation is a kernel of its own name with the same body (not a fourth template parameter of
// backend_kernel, not a call of a common device function: either would change the plain kernels' code or names).
template <int NB, bool ADV>
__global__ __launch_bounds__(128, 3) void backend_points_kernel(BackendArgs a, PointArgs pts) {
  constexpr bool DBG = false, PTS = true, TRC = false, LIVE = false, BND = false, PBD = false, SUM = false, WARM = false;
  constexpr SummaryArgs sum{};
  constexpr TraceArgs trc{};
  constexpr BandArgs bnd{};
  constexpr PatternBandArgs pbd{};
#include "peaq_backend_fft.inc"
}
// the trace instantiation: a third kernel of its own name with the same body
template <int NB, bool ADV>
__global__ __launch_bounds__(128, 3) void backend_trace_kernel(BackendArgs a, TraceArgs trc) {
  constexpr bool DBG = false, PTS = false, TRC = true, LIVE = false, BND = false, PBD = false, SUM = false, WARM = false;
  constexpr SummaryArgs sum{};
  constexpr PointArgs pts{};
  constexpr BandArgs bnd{};
  constexpr PatternBandArgs pbd{};
#include "peaq_backend_fft.inc"
}
// the live instantiation (a metered session's launches): the trace instantiation, but record f of a launch sits at
// [launch index][f - first frame of the launch] -- the feed of peaq_meter.hip, in a scratch of one launch
template <int NB, bool ADV>
__global__ __launch_bounds__(128, 3) void backend_live_kernel(BackendArgs a, TraceArgs trc) {
  constexpr bool DBG = false, PTS = false, TRC = true, LIVE = true, BND = false, PBD = false, SUM = false, WARM = false;
  constexpr SummaryArgs sum{};
  constexpr PointArgs pts{};
  constexpr BandArgs bnd{};
  constexpr PatternBandArgs pbd{};
#include "peaq_backend_fft.inc"
}
// the live-band instantiation (the launches of a metered session with the band meter on): the live instantiation, and
// the planes of `bnd` at the same launch-relative index beside the trace record -- the feed of peaq_meter_bands.hip.
// (A name of its own that contains neither the live nor the bands kernels' names.)
template <int NB, bool ADV>
__global__ __launch_bounds__(128, 3) void backend_liveband_kernel(BackendArgs a, TraceArgs trc, BandArgs bnd) {
  constexpr bool DBG = false, PTS = false, TRC = true, LIVE = true, BND = true, PBD = false, SUM = false, WARM = false;
  constexpr SummaryArgs sum{};
  constexpr PointArgs pts{};
  constexpr PatternBandArgs pbd{};
#include "peaq_backend_fft.inc"
}
// the bands instantiation: a fourth kernel of its own name with the same body
template <int NB, bool ADV>
__global__ __launch_bounds__(128, 3) void backend_bands_kernel(BackendArgs a, BandArgs bnd) {
  constexpr bool DBG = false, PTS = false, TRC = false, LIVE = false, BND = true, PBD = false, SUM = false, WARM = false;
  constexpr SummaryArgs sum{};
  constexpr PointArgs pts{};
  constexpr TraceArgs trc{};
  constexpr PatternBandArgs pbd{};
#include "peaq_backend_fft.inc"
}
// the pattern-bands instantiation (basic version only): a fifth kernel of its own name with the same body
template <int NB, bool ADV>
__global__ __launch_bounds__(128, 3) void backend_pattern_bands_kernel(BackendArgs a, PatternBandArgs pbd) {
  static_assert(!ADV, "the 55-band path has no pattern layer");
  constexpr bool DBG = false, PTS = false, TRC = false, LIVE = false, BND = false, PBD = true, SUM = false, WARM = false;
  constexpr SummaryArgs sum{};
  constexpr PointArgs pts{};
  constexpr TraceArgs trc{};
  constexpr BandArgs bnd{};
#include "peaq_backend_fft.inc"
}
// the summary instantiation: a sixth kernel of its own name with the same body
template <int NB, bool ADV>
__global__ __launch_bounds__(128, 3) void backend_summary_kernel(BackendArgs a, SummaryArgs sum) {
  constexpr bool DBG = false, PTS = false, TRC = false, LIVE = false, BND = false, PBD = false, SUM = true, WARM = false;
  constexpr PointArgs pts{};
  constexpr TraceArgs trc{};
  constexpr BandArgs bnd{};
  constexpr PatternBandArgs pbd{};
#include "peaq_backend_fft.inc"
}

// Which outputs may meet which launch (x = refused with hipErrorInvalidValue, . = accepted, and then the first of sum,
// pbd, bnd, trc, pts, a.debug decides the kernel):
//
//                with:  sum  pbd  bnd  trc  pts  a.debug  a.pair_frame0  a.pair_slot  a.advanced
//   out.sum              -    x    x    x    x      x           x             x            .
//   out.pbd              x    -    x    x    x      x           x             .            x
//   out.bnd              x    x    -    x    x      x           x             .            .
//   out.trc              x    x    x    -    .      .           .             .            .
//   out.pts              x    x    x    .    -      .           .             .            .
//
//   out.spn              x    x    x  needs   x      x           x             x     as spn.blocks
//   out.live             x    x    x    x    x      x           .             .            .
//   out.live_bnd       needs out.live, and is held to what out.live is held to
//
// The rows-per-band outputs (bnd, pbd, sum) belong to a run's own launches: each stands alone.  The trace and the
// points are not held against each other, the debug dump or a broker's windows: the trace wins over the points, either
// wins over a.debug.  out.fbnd is the filter-bank path's and is not looked at here.  out.spn (peaq_batch_run_windows,
// peaq_batch_run_adv_spans) launches nothing here: its replay (peaq_replay.hip) reads what the trace instantiation of a
// run's own launch leaves -- the basic or the 55-band one, as a.advanced says --, so it needs out.trc and nothing else of
// the run's own outputs.  out.live (a metered session's launches: the feed of peaq_meter.hip, launch-relative) stands
// alone among the outputs -- out.spn included -- and is the one that goes with a launch's own frame windows and slots; it
// needs live.frames.  out.live_bnd (the band meter) selects the live-band instantiations: the same launch with the planes
// of live_bnd beside the records; without out.live, without live_bnd.frame_stride or with planes that the version does
// not have it is refused.
hipError_t launch_backend(const BackendArgs& a, unsigned n_pairs, hipStream_t stream, const RunOutputs& out) {
  if (n_pairs == 0) return hipSuccess;
  const dim3 block(64 * a.channels);
  PEAQ_DEV_SPIN_INSTEAD_OF_BACKEND(a, block, stream)
  const bool pts = out.has_pts(), trc = out.has_trc(), bnd = out.has_bnd(), pbd = out.has_pbd(), sum = out.has_sum();
  const int alone = bnd + pbd + sum;                 // at most one of these, and none with ...
  if (alone && (alone + pts + trc + (a.debug != nullptr) + (a.pair_frame0 != nullptr) > 1 || (pbd && a.advanced) ||
                (sum && a.pair_slot)))
    return hipErrorInvalidValue;
  if (out.has_spn() && (!trc || alone || pts || a.debug || a.pair_frame0 || a.pair_slot ||
                        (a.advanced != 0) != (out.spn.blocks != nullptr)))   // (block records: the advanced version's)
    return hipErrorInvalidValue;
  if (out.has_live_bnd() && (!out.has_live() || !out.live_bnd.frame_stride || !out.live_bnd.planes ||
                             (out.live_bnd.planes & ~(a.advanced ? kBandAdvanced : kBandAll))))
    return hipErrorInvalidValue;
  if (out.has_live()) {
    if (alone || pts || trc || out.has_spn() || a.debug || !out.live.frames) return hipErrorInvalidValue;
    if (out.has_live_bnd() && !a.advanced)
      hipLaunchKernelGGL((backend_liveband_kernel<109, false>), dim3(n_pairs), block, 0, stream, a, out.live, out.live_bnd);
    else if (out.has_live_bnd())
      hipLaunchKernelGGL((backend_liveband_kernel<55, true>), dim3(n_pairs), block, 0, stream, a, out.live, out.live_bnd);
    else if (!a.advanced)
      hipLaunchKernelGGL((backend_live_kernel<109, false>), dim3(n_pairs), block, 0, stream, a, out.live);
    else
      hipLaunchKernelGGL((backend_live_kernel<55, true>), dim3(n_pairs), block, 0, stream, a, out.live);
    return hipGetLastError();
  }
  if (sum && !a.advanced)
    hipLaunchKernelGGL((backend_summary_kernel<109, false>), dim3(n_pairs), block, 0, stream, a, out.sum);
  else if (sum)
    hipLaunchKernelGGL((backend_summary_kernel<55, true>), dim3(n_pairs), block, 0, stream, a, out.sum);
  else if (pbd)
    hipLaunchKernelGGL((backend_pattern_bands_kernel<109, false>), dim3(n_pairs), block, 0, stream, a, out.pbd);
  else if (bnd && !a.advanced)
    hipLaunchKernelGGL((backend_bands_kernel<109, false>), dim3(n_pairs), block, 0, stream, a, out.bnd);
  else if (bnd)
    hipLaunchKernelGGL((backend_bands_kernel<55, true>), dim3(n_pairs), block, 0, stream, a, out.bnd);
  else if (trc && !a.advanced)
    hipLaunchKernelGGL((backend_trace_kernel<109, false>), dim3(n_pairs), block, 0, stream, a, out.trc);
  else if (trc)
    hipLaunchKernelGGL((backend_trace_kernel<55, true>), dim3(n_pairs), block, 0, stream, a, out.trc);
  else if (pts && !a.advanced)
    hipLaunchKernelGGL((backend_points_kernel<109, false>), dim3(n_pairs), block, 0, stream, a, out.pts);
  else if (pts)
    hipLaunchKernelGGL((backend_points_kernel<55, true>), dim3(n_pairs), block, 0, stream, a, out.pts);
  else if (!a.advanced && a.debug)
    hipLaunchKernelGGL((backend_kernel<109, false, true>), dim3(n_pairs), block, 0, stream, a);
  else if (a.debug)
    hipLaunchKernelGGL((backend_kernel<55, true, true>), dim3(n_pairs), block, 0, stream, a);
  else if (!a.advanced)
    hipLaunchKernelGGL((backend_kernel<109, false>), dim3(n_pairs), block, 0, stream, a);
  else
    hipLaunchKernelGGL((backend_kernel<55, true>), dim3(n_pairs), block, 0, stream, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Filter-bank back end of the advanced version (gstpeaq.c:965-1010): 40 bands,
// one band per lane, blocks of 192 samples in order.
// ---------------------------------------------------------------------------
struct FbBackendShared {
  double pa[2][2][kPaStride];
  double acc[2][kAccFields][kAccLdsStride];
  int gate[2];
};

// DBG = true (peaq_debug_backend_advanced): the block's MOV values are computed for every block and written to
// a.debug; the arithmetic is the same instantiation otherwise.
// (held to 128 registers -- 44 B of them spilled around the block loop, none inside: beside the FP64 bank this kernel
// runs in the place of ONE of a CU's two bank workgroups, 272 registers per SIMD lane, and two of its waves fit there
// instead of one: + 0.5 % on the advanced pass)
// PTS = true (fb_backend_points_kernel, trajectory launches only): after each block the reading points that fall on it
// get the snapshot of the accumulators this path owns (0, 1, 4).
// TRC = true (fb_backend_trace_kernel, trace launches only): the block's MOV values are computed for every block, as
// with DBG, and one lane per (block, channel) writes them into the pair's block record (TraceArgs).
// BND = true (fb_backend_bands_kernel, filter-bank band-trace launches only): the block's MOV values are computed for
// every block, as with TRC, and every lane below 40 stores its band's value of the requested planes where it comes up
// (FbBandArgs, fb_band_store); the accumulators see what the gates admit, as in the plain instantiation.
// FSUM = true (fb_band_summary_kernel, filter-bank summary launches only): every lane below 40 adds its band's terms of
// the counted blocks to the channel's running rows in LDS where they come up (FbSummaryArgs, fb_summary_add); the
// arithmetic and the gates are the plain instantiation's, and a block whose gate is closed evaluates nothing more.
template <bool DBG>
__global__ __launch_bounds__(128, 4) void fb_backend_kernel(FbBackendArgs a) {
  constexpr bool PTS = false, TRC = false, LIVE = false, BND = false, FSUM = false;
  constexpr PointArgs pts{};
  constexpr TraceArgs trc{};
  constexpr FbBandArgs bnd{};
  constexpr FbSummaryArgs fsum{};
#include "peaq_backend_fb.inc"
}
// the points instantiation (see backend_points_kernel)
__global__ __launch_bounds__(128, 4) void fb_backend_points_kernel(FbBackendArgs a, PointArgs pts) {
  constexpr bool DBG = false, PTS = true, TRC = false, LIVE = false, BND = false, FSUM = false;
  constexpr TraceArgs trc{};
  constexpr FbBandArgs bnd{};
  constexpr FbSummaryArgs fsum{};
#include "peaq_backend_fb.inc"
}
// the trace instantiation (see backend_trace_kernel)
__global__ __launch_bounds__(128, 4) void fb_backend_trace_kernel(FbBackendArgs a, TraceArgs trc) {
  constexpr bool DBG = false, PTS = false, TRC = true, LIVE = false, BND = false, FSUM = false;
  constexpr PointArgs pts{};
  constexpr FbBandArgs bnd{};
  constexpr FbSummaryArgs fsum{};
#include "peaq_backend_fb.inc"
}
// the live instantiation (see backend_live_kernel)
__global__ __launch_bounds__(128, 4) void fb_backend_live_kernel(FbBackendArgs a, TraceArgs trc) {
  constexpr bool DBG = false, PTS = false, TRC = true, LIVE = true, BND = false, FSUM = false;
  constexpr PointArgs pts{};
  constexpr FbBandArgs bnd{};
  constexpr FbSummaryArgs fsum{};
#include "peaq_backend_fb.inc"
}
// the bands instantiation (see backend_bands_kernel)
__global__ __launch_bounds__(128, 4) void fb_backend_bands_kernel(FbBackendArgs a, FbBandArgs bnd) {
  constexpr bool DBG = false, PTS = false, TRC = false, LIVE = false, BND = true, FSUM = false;
  constexpr PointArgs pts{};
  constexpr TraceArgs trc{};
  constexpr FbSummaryArgs fsum{};
#include "peaq_backend_fb.inc"
}
// the summary instantiation (see backend_summary_kernel); a name of its own that the other kernels' names do not contain
__global__ __launch_bounds__(128, 4) void fb_band_summary_kernel(FbBackendArgs a, FbSummaryArgs fsum) {
  constexpr bool DBG = false, PTS = false, TRC = false, LIVE = false, BND = false, FSUM = true;
  constexpr PointArgs pts{};
  constexpr TraceArgs trc{};
  constexpr FbBandArgs bnd{};
#include "peaq_backend_fb.inc"
}

//                with:  fsum  fbnd  trc  pts  a.debug  a.windows
//   out.fsum              -     x    x    x      x         x          (a run's own launches only)
//   out.fbnd              x     -    x    x      x         x          (a run's own launches only)
//   out.trc               x     x    -    .      .         .
//   out.pts               x     x    .    -      .         .
//   out.spn               x     x  needs  x      x         x          (a run's own launches only)
//   out.live              x     x    x    x      x         .          (needs live.blocks; refused with out.spn too)
// out.fsum is also refused together with out.sum: a run has one summary, and the two share the context's saved copy.
// out.bnd, out.pbd and out.sum are the FFT path's and are otherwise not looked at here.
hipError_t launch_fb_backend(const FbBackendArgs& a, unsigned n_pairs, hipStream_t stream, const RunOutputs& out) {
  if (n_pairs == 0) return hipSuccess;
  const bool pts = out.has_pts(), trc = out.has_trc(), bnd = out.has_fbnd(), fsum = out.has_fsum();
  if ((bnd || fsum) && (pts || trc || a.debug || a.windows || (bnd && fsum) || (fsum && out.has_sum())))
    return hipErrorInvalidValue;
  if (out.has_spn() && (!trc || !out.trc.blocks || pts || bnd || fsum || a.debug || a.windows))
    return hipErrorInvalidValue;
  if (out.has_live()) {
    if (bnd || fsum || pts || trc || out.has_spn() || a.debug || !out.live.blocks) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fb_backend_live_kernel, dim3(n_pairs), dim3(64 * a.channels), 0, stream, a, out.live);
    return hipGetLastError();
  }
  if (fsum)
    hipLaunchKernelGGL(fb_band_summary_kernel, dim3(n_pairs), dim3(64 * a.channels), 0, stream, a, out.fsum);
  else if (bnd)
    hipLaunchKernelGGL(fb_backend_bands_kernel, dim3(n_pairs), dim3(64 * a.channels), 0, stream, a, out.fbnd);
  else if (trc)
    hipLaunchKernelGGL(fb_backend_trace_kernel, dim3(n_pairs), dim3(64 * a.channels), 0, stream, a, out.trc);
  else if (pts)
    hipLaunchKernelGGL(fb_backend_points_kernel, dim3(n_pairs), dim3(64 * a.channels), 0, stream, a, out.pts);
  else if (a.debug)
    hipLaunchKernelGGL(fb_backend_kernel<true>, dim3(n_pairs), dim3(64 * a.channels), 0, stream, a);
  else
    hipLaunchKernelGGL(fb_backend_kernel<false>, dim3(n_pairs), dim3(64 * a.channels), 0, stream, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// state initialisation (gstpeaq.c:357-361, movaccum.c:276-299, *_state_alloc: zeros)
// ---------------------------------------------------------------------------
__global__ void state_init_kernel(PairState* st, unsigned n_pairs) {
  const unsigned pair = blockIdx.x;
  if (pair >= n_pairs) return;
  PairState* ps = st + pair;
  double* raw = reinterpret_cast<double*>(ps);
  for (unsigned i = threadIdx.x; i < sizeof(PairState) / sizeof(double); i += blockDim.x) raw[i] = 0.;
  __syncthreads();
  if (threadIdx.x == 0) {
    ps->loudness_reached = UINT_MAX;
    for (int i = 0; i < kMaxAcc; ++i) ps->status[i] = kInit;
    for (int c = 0; c < 2; ++c)
      for (int i = 0; i < kMaxAcc; ++i) {
        // AVG_WINDOW history starts as NaN sentinels (movaccum.c:293)
        ps->ch[c].acc[i][3] = ps->ch[c].acc[i][4] = ps->ch[c].acc[i][5] = __builtin_nan("");
      }
  }
}

hipError_t launch_state_init(PairState* state, int /*advanced*/, unsigned n_pairs, hipStream_t stream) {
  if (n_pairs == 0) return hipSuccess;
  hipLaunchKernelGGL(state_init_kernel, dim3(n_pairs), dim3(256), 0, stream, state, n_pairs);
  return hipGetLastError();
}

// trajectories: a snapshot holds what state_init_kernel leaves in the fields it copies -- zeros (status kInit,
// energies, counts, accumulators) but the AVG_WINDOW history's NaN sentinels; one thread per double
static_assert(kInit == 0, "points_init_kernel writes status as zero");
__global__ void points_init_kernel(double* __restrict__ raw, size_t n_doubles) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_doubles) return;
  const unsigned j = (unsigned)(i % kSnapDoubles);
  double v = 0.;
  if (j >= (unsigned)kSnapAccHead) {
    const unsigned f = (j - kSnapAccHead) % kAccFields;
    if (f >= 3 && f <= 5) v = __builtin_nan("");     // movaccum.c:293
  }
  raw[i] = v;
}

hipError_t launch_points_init(PointSnap* snap, size_t n_snaps, hipStream_t stream) {
  if (n_snaps == 0) return hipSuccess;
  const size_t n = n_snaps * kSnapDoubles;
  hipLaunchKernelGGL(points_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                     reinterpret_cast<double*>(snap), n);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// read-out: one thread per pair (movaccum.c:438-481, gstpeaq.c:1013-1078, nn.c)
// ---------------------------------------------------------------------------
__constant__ double nb_amin[11] = {393.916656, 361.965332, -24.045116, 1.110661, -0.206623, 0.074318,
                                   1.113683, 0.950345, 0.029985, 0.000101, 0.};
__constant__ double nb_amax[11] = {921, 881.131226, 16.212030, 107.137772, 2.886017, 13.933351,
                                   63.257874, 1145.018555, 14.819740, 1., 1.};
__constant__ double nb_wx[11][3] = {{-0.502657, 0.436333, 1.219602},  {4.307481, 3.246017, 1.123743},
                                    {4.984241, -2.211189, -0.192096}, {0.051056, -1.762424, 4.331315},
                                    {2.321580, 1.789971, -0.754560},  {-5.303901, -3.452257, -10.814982},
                                    {2.730991, -6.111805, 1.519223},  {0.624950, -1.331523, -5.955151},
                                    {3.102889, 0.871260, -5.922878},  {-1.051468, -0.939882, -0.142913},
                                    {-1.804679, -0.503610, -0.620456}};
__constant__ double nb_wxb[3] = {-2.518254, 0.654841, -2.207228};
__constant__ double nb_wy[3] = {-3.817048, 4.107138, 4.629582};
__constant__ double na_amin[5] = {13.298751, 0.041073, -25.018791, 0.061560, 0.02452};
__constant__ double na_amax[5] = {2166.5, 13.24326, 13.46708, 10.226771, 14.224874};
__constant__ double na_wx[5][5] = {{21.211773, -39.013052, -1.382553, -14.545348, -0.320899},
                                   {-8.981803, 19.956049, 0.935389, -1.686586, -3.238586},
                                   {1.633830, -2.877505, -7.442935, 5.606502, -1.783120},
                                   {6.103821, 19.587435, -0.240284, 1.088213, -0.511314},
                                   {11.556344, 3.892028, 9.720441, -3.287205, -11.031250}};
__constant__ double na_wxb[5] = {1.330890, 2.686103, 2.096598, -1.327851, 3.087055};
__constant__ double na_wy[5] = {-4.696996, -3.289959, 7.004782, 6.651897, 4.009144};

// One pair's read-out from its readable state -- a PairState (finalize_kernel) or a reading point's snapshot
// (finalize_points_kernel): both go through this one function, so a point and the end result are the same arithmetic.
// acc0 / acc1: the accumulators [kMaxAcc][kAccFields] of channel 0 / 1.
__device__ __forceinline__ ResultRecord finalize_state(const int32_t* status, const double (*acc0)[kAccFields],
                                                       const double (*acc1)[kAccFields], double sig_energy,
                                                       double noise_energy, double frames, double fb_blocks,
                                                       int advanced, int channels, int clamp_movs) {
  ResultRecord r;
  const int n_movs = advanced ? 5 : 11;
  for (int i = 0; i < 11; ++i) r.movs[i] = 0.;
  for (int i = 0; i < n_movs; ++i) {
    const int mode = acc_mode(advanced, i);
    // basic: ADB and MFPD have ONE channel (gstpeaq.c:580-584)
    const int nch = (!advanced && (i == MB_ADB || i == MB_MFPD)) ? 1 : channels;
    const bool tent = status[i] == kTentative;
    double v = 0.;
    for (int c = 0; c < nch; ++c) v += acc_channel_value(mode, tent, (c ? acc1 : acc0)[i]);
    r.movs[i] = v / nch;
  }
  double di;
  if (!advanced) {
    double x[3] = {nb_wxb[0], nb_wxb[1], nb_wxb[2]};
    for (int i = 0; i < 11; ++i) {
      double m = (r.movs[i] - nb_amin[i]) / (nb_amax[i] - nb_amin[i]);
      if (clamp_movs) m = m < 0. ? 0. : m > 1. ? 1. : m;                 // CLAMP_MOVS, nn.c:202-207
      for (int j = 0; j < 3; ++j) x[j] += nb_wx[i][j] * m;
    }
    di = -0.307594;
    for (int j = 0; j < 3; ++j) di += nb_wy[j] / (1 + exp(-x[j]));
  } else {
    double x[5];
    for (int j = 0; j < 5; ++j) x[j] = na_wxb[j];
    for (int i = 0; i < 5; ++i) {
      double m = (r.movs[i] - na_amin[i]) / (na_amax[i] - na_amin[i]);
      if (clamp_movs) m = m < 0. ? 0. : m > 1. ? 1. : m;                 // nn.c:320-325
      for (int j = 0; j < 5; ++j) x[j] += na_wx[i][j] * m;
    }
    di = -1.360308;
    for (int j = 0; j < 5; ++j) di += na_wy[j] / (1 + exp(-x[j]));
  }
  r.di = di;
  r.odg = -3.98 + (0.22 - -3.98) / (1 + exp(-di));          // nn.c:92-93,372-375
  r.totalsnr = 10 * log10(sig_energy / noise_energy);
  r.frames = frames;
  r.fb_blocks = fb_blocks;
  return r;
}

__global__ void finalize_kernel(const PairState* __restrict__ st, int advanced, int channels, unsigned n_pairs,
                                ResultRecord* __restrict__ out, int clamp_movs) {
  const unsigned pair = blockIdx.x * blockDim.x + threadIdx.x;
  if (pair >= n_pairs) return;
  const PairState* ps = st + pair;
  out[pair] = finalize_state(ps->status, ps->ch[0].acc, ps->ch[1].acc, ps->sig_energy, ps->noise_energy,
                             (double)ps->frame_counter, (double)ps->fb_counter, advanced, channels, clamp_movs);
}

// one thread per (pair, point): out[pair][point]
__global__ void finalize_points_kernel(const PointSnap* __restrict__ snap, int advanced, int channels, size_t n_snaps,
                                       ResultRecord* __restrict__ out, int clamp_movs) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_snaps) return;
  const PointSnap* sp = snap + i;
  out[i] = finalize_state(sp->status, sp->acc[0], sp->acc[1], sp->sig_energy, sp->noise_energy, (double)sp->frames,
                          (double)sp->fb_blocks, advanced, channels, clamp_movs);
}

// band summary: a pair whose accumulators end tentative counts nothing after its last frame above the data boundary
// (movaccum.c:443-447 reads data_saved): its rows go back to the copy the back end took when it turned tentative.  One
// workgroup per pair.
__global__ void summary_restore_kernel(const PairState* __restrict__ st, int status_idx, double* __restrict__ rows,
                                       const double* __restrict__ saved, unsigned n_pairs, unsigned pair_doubles) {
  const unsigned pair = blockIdx.x;
  if (pair >= n_pairs || st[pair].status[status_idx] != kTentative) return;
  const size_t base = (size_t)pair * pair_doubles;
  for (unsigned i = threadIdx.x; i < pair_doubles; i += blockDim.x) rows[base + i] = saved[base + i];
}

hipError_t launch_summary_restore(const PairState* state, int advanced, const SummaryArgs& sum, unsigned n_pairs,
                                  unsigned pair_doubles, hipStream_t stream) {
  if (n_pairs == 0) return hipSuccess;
  // (the accumulator whose tentative state the back end's summary rows follow)
  hipLaunchKernelGGL(summary_restore_kernel, dim3(n_pairs), dim3(256), 0, stream, state,
                     advanced ? (int)MA_SEGNMR : (int)MB_NMR, sum.rows, sum.saved, n_pairs, pair_doubles);
  return hipGetLastError();
}

// (the filter-bank summary's rows follow the RmsModDiff accumulator: all three of that path see the same set_tentative)
hipError_t launch_fb_summary_restore(const PairState* state, const FbSummaryArgs& fsum, unsigned n_pairs,
                                     unsigned pair_doubles, hipStream_t stream) {
  if (n_pairs == 0) return hipSuccess;
  hipLaunchKernelGGL(summary_restore_kernel, dim3(n_pairs), dim3(256), 0, stream, state, (int)MA_RMSMOD, fsum.rows,
                     fsum.saved, n_pairs, pair_doubles);
  return hipGetLastError();
}

hipError_t launch_finalize(const PairState* state, int advanced, int channels, unsigned n_pairs, ResultRecord* out,
                           hipStream_t stream, const Settings& cfg) {
  if (n_pairs == 0) return hipSuccess;
  hipLaunchKernelGGL(finalize_kernel, dim3((n_pairs + 63) / 64), dim3(64), 0, stream, state, advanced, channels,
                     n_pairs, out, cfg.clamp_movs);
  return hipGetLastError();
}

hipError_t launch_finalize_points(const PointSnap* snap, int advanced, int channels, unsigned n_pairs, int n_points,
                                  ResultRecord* out, hipStream_t stream, const Settings& cfg) {
  const size_t n = (size_t)n_pairs * (size_t)(n_points > 0 ? n_points : 0);
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(finalize_points_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, snap, advanced,
                     channels, n, out, cfg.clamp_movs);
  return hipGetLastError();
}

}  // namespace peaq

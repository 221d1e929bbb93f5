// peaq_frontend.hip -- the stateless half of the FFT ear model, one workgroup
// of two wavefronts per (pair, frame, channel): wave 0 transforms the reference
// frame, wave 1 the test frame, with IDENTICAL instruction streams (identical
// inputs must give bit-identical spectra, otherwise the reference's
// "identical signals" behaviour -- exact zeros in the noise spectrum and in the
// EHS log-ratio, SURVEY.md Appendix B.10 -- is lost).
//
// Per wave (reference fftearmodel.c:433-515 up to `unsmeared_excitation`):
//   Hann window * samples            :451-452   (window evaluated from 4 per-lane values)
//   2048-point real DFT              :457   (as a 1024-point complex Stockham
//                                            FFT 16x16x4 in registers + LDS and
//                                            the even/odd split, two mirror bins per step)
//   power spectrum * level factor    :464-466
//   outer/middle ear weighting       :470-472
//   grouping into critical bands     :604-620
//   + internal noise                 :483-485
//   level-dependent spreading        :637-676
//   energy flag                      :508-514
// plus the frame's stateless MOV ingredients:
//   ref wave : data-boundary detector      gstpeaq.c:1081-1099 (before the FFT)
//   both     : totalsnr energies           gstpeaq.c:913-918 (with the frame load)
//   both     : bandwidths                  movs.c:776-809 (from the spectra in registers)
//   both     : log ratio of the spectra    movs.c:1383-1391
//   ref wave : error harmonic structure    movs.c:1279-1315,1393-1441 (correlation through
//                                          512-point FFTs like the reference, window, 256-point FFT, peak)
//   test wave: noise-in-bands for NMR      movs.c:992-1000
//
// What bounds this kernel (measured): not the FP64 pipe and not HBM bandwidth but
// latency -- of the vector-memory pipe (hence: one coalesced load path, lane-major tables instead
// of gathers, an L2 prefetch for the workgroups to come) and of the LDS crossbar (hence: DPP /
// permlane reductions and scans, band sums fetched two bins per read in batches that are in flight together).
//
// LDS per wave ("unit"), 10304 B: the 8.5 KiB FFT exchange buffer (real and
// imaginary parts go through it one after the other) is reused for the weighted
// spectrum Pw[0..775] and 4 KiB of scratch; the unweighted spectrum never leaves the
// registers (the bandwidth MOVs are found with two wave reductions).  That is
// what lets six workgroups = three waves per SIMD share a CU.
//
// The basic version launches frontend_pair_kernel<109> instead (further down): ONE wave per
// (pair, frame, channel) that carries reference and test together -- the window, the twiddle powers, the item decoding
// and the table reads exist once, there is no barrier and nothing is handed between waves, and each signal's dependent
// chains have the other's to issue beside them; 251 registers, two waves per SIMD, 18.2 KiB of LDS.  The advanced
// version stays on frontend_kernel<55>; PEAQ_AMD_FE=two_waves selects frontend_kernel<109> for the basic one again.
#include <hip/hip_runtime.h>

#include "peaq_device.h"
#include "peaq_kernels.h"
#include "peaq_group_sched.h"
#include "peaq_spread_sched.h"
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "peaq_wave.h"

namespace peaq {

// LDS per wave ("unit"): 1288 doubles = 10304 B.  During the FFT the first 1088 doubles are the
// exchange buffer (one real component of the 1024 complex points at a time, padded); afterwards
// Pw[0..775] (weighted power spectrum) followed by 512 doubles of scratch.
#ifndef PEAQ_FE_PREFETCH_ITEMS
#define PEAQ_FE_PREFETCH_ITEMS 64
#endif
constexpr int kPrefetchItems = PEAQ_FE_PREFETCH_ITEMS;            // L2 prefetch distance in work items (see the kernel)
constexpr int kUnitDoubles = 1288;
constexpr int kOffPw = 0;                     // Pw[776]
constexpr int kOffScratch = 776;              // 512 doubles
constexpr int kPwLen = 776;
static_assert(kPwLen == kGroupSpectrumBins, "the band sums' schedule is held against this length (peaq_group_sched.h)");
constexpr int kOffLogTab = 2 * kUnitDoubles;       // the logarithm table (log_tab, peaq_wave.h) behind both units
constexpr int kLogTabDoubles = 2 * kLogTabEntries + 2;   // the table + two spare words, per wave
constexpr int kLdsDoubles = 2 * kUnitDoubles + 2 * kLogTabDoubles;
#ifndef PEAQ_FE_WAVES
#define PEAQ_FE_WAVES 3
#endif
constexpr int kWavesPerSimd = PEAQ_FE_WAVES;

// W_32^q = exp(-2 pi i q / 32), q = 0..15
__device__ constexpr double kW32re[16] = {1., 0.98078528040323044913, 0.92387953251128675613, 0.83146961230254523708,
                                          0.70710678118654752440, 0.55557023301960222474, 0.38268343236508977173,
                                          0.19509032201612826785, 0., -0.19509032201612826785, -0.38268343236508977173,
                                          -0.55557023301960222474, -0.70710678118654752440, -0.83146961230254523708,
                                          -0.92387953251128675613, -0.98078528040323044913};
__device__ constexpr double kW32im[16] = {-0., -0.19509032201612826785, -0.38268343236508977173, -0.55557023301960222474,
                                          -0.70710678118654752440, -0.83146961230254523708, -0.92387953251128675613,
                                          -0.98078528040323044913, -1., -0.98078528040323044913, -0.92387953251128675613,
                                          -0.83146961230254523708, -0.70710678118654752440, -0.55557023301960222474,
                                          -0.38268343236508977173, -0.19509032201612826785};

__device__ __forceinline__ int pad16(int i) { return i + (i >> 4); }   // complex index -> padded slot

// entry e of the lane-major twiddle table (peaq_device.h): one coalesced 16-byte load
__device__ __forceinline__ cplx tw_lane(const CommonTables* __restrict__ ct, int e, int lane) {
  const double2 v = *reinterpret_cast<const double2*>(ct->tw_lane[e][lane]);
  return {v.x, v.y};
}
__device__ __forceinline__ cplx csqr(cplx a) { return {a.re * a.re - a.im * a.im, 2. * (a.re * a.im)}; }
// x^e by squaring, for an e >= 1 that is a constant where this is inlined
__device__ __forceinline__ double pow_const(double x, int e) {
  double pw = 1., sq = x;
#pragma unroll
  for (; e; e >>= 1) {
    if (e & 1) pw *= sq;
    if (e >> 1) sq *= sq;
  }
  return pw;
}

// dft8 (peaq_wave.h) for inputs whose upper half is purely imaginary: x[4..7].re are taken as zero and never read.
// Same values as dft8 on {0, x[4 + n].im}, bar the sign of a zero (x.re + 0 turns -0 into +0, this does not).
__device__ __forceinline__ void dft8_imag_upper(cplx (&x)[8]) {
  constexpr double c = 0.70710678118654752440;
  cplx a0 = {x[0].re, x[0].im + x[4].im}, a1 = {x[1].re, x[1].im + x[5].im};
  cplx a2 = {x[2].re, x[2].im + x[6].im}, a3 = {x[3].re, x[3].im + x[7].im};
  cplx b0 = {x[0].re, x[0].im - x[4].im}, b1 = {x[1].re, x[1].im - x[5].im};
  cplx b2 = {x[2].re, x[2].im - x[6].im}, b3 = {x[3].re, x[3].im - x[7].im};
  b1 = {c * (b1.re + b1.im), c * (b1.im - b1.re)};      // * W8^1 = (1 - i) / sqrt 2
  b2 = cmul_mi(b2);                                       // * W8^2 = -i
  b3 = {c * (b3.im - b3.re), -c * (b3.re + b3.im)};      // * W8^3 = (-1 - i) / sqrt 2
  dft4(a0, a1, a2, a3);
  dft4(b0, b1, b2, b3);
  x[0] = a0; x[2] = a1; x[4] = a2; x[6] = a3;
  x[1] = b0; x[3] = b1; x[5] = b2; x[7] = b3;
}

// One exchange step of the Stockham FFT through the wave's 8.5 KiB buffer: all 16 points
// go out at wr(r) and come back from rd(r), first the real then the imaginary parts.
template <typename WR, typename RD>
__device__ __forceinline__ void exchange16(cplx (&z)[16], double* buf, WR wr, RD rd) {
#pragma unroll
  for (int r = 0; r < 16; ++r) buf[pad16(wr(r))] = z[r].re;
  wave_lds_fence();
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r].re = buf[pad16(rd(r))];
  wave_lds_fence();
#pragma unroll
  for (int r = 0; r < 16; ++r) buf[pad16(wr(r))] = z[r].im;
  wave_lds_fence();
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r].im = buf[pad16(rd(r))];
  wave_lds_fence();
}

// ---------------------------------------------------------------------------
// 2048-point real DFT of one frame held as z[r] = x[2n] + i x[2n+1], n = lane + 64 r.
// On return p[s] is the power spectrum at bin spec_bin(s, lane) (registers) and Pw of the unit
// holds the weighted power spectrum of bins 0..775.
// ---------------------------------------------------------------------------
// `before_split` is called ahead of the fence in front of the split: the caller's place for requests whose values it
// needs right behind this function (a callback and not an array handed back: the compiler keeps such an array in
// scratch, 64 bytes per lane in both instantiations).
template <typename F>
__device__ __forceinline__ void frame_power_spectrum(cplx (&z)[16], double (&p)[16], double* unit, int lane,
                                                     const CommonTables* __restrict__ ct,
                                                     double level_factor, F&& before_split) {
  // Table values whose use lies behind an LDS exchange are requested BEFORE it, by hand: wave_lds_fence() is an
  // acquire-release fence, the compiler may not lift a later global load over it, and a load issued behind the fence is
  // waited for a few instructions later -- a full round trip through the vector-memory pipe with nothing to cover it.
  const cplx w256 = tw_lane(ct, 2, lane);            // pass 2's W_256^k: has pass 1 and the exchange to arrive
  // pass 1: radix 16, sub-transform size 1 -> out[16 lane + r]; pass 2 reads in[lane + 64 r]
  dft16(z);
  exchange16(z, unit, [&](int r) { return 16 * lane + r; }, [&](int r) { return lane + 64 * r; });
  // pass 2: radix 16, sub-transform size 16
  {
    {
      // twiddles W_256^(r k), k = lane & 15, r = 1..15: one table read, three squarings (r = 2, 4, 8),
      // the rest as products
      // (applied as soon as they exist: only w1..w8 stay live, the register budget is 168)
      cplx w[9];
      w[1] = w256;                                   // W_256^k; the other powers by squaring
      w[2] = csqr(w[1]);
      w[4] = csqr(w[2]);
      w[8] = csqr(w[4]);
      w[3] = cmul(w[1], w[2]);
      w[5] = cmul(w[4], w[1]);
      w[6] = cmul(w[4], w[2]);
      w[7] = cmul(w[4], w[3]);
#pragma unroll
      for (int r = 1; r < 8; ++r) {
        z[8 + r] = cmul(z[8 + r], cmul(w[8], w[r]));
        z[r] = cmul(z[r], w[r]);
      }
      z[8] = cmul(z[8], w[8]);
    }
    dft16(z);
    // out[j + 16 r] with j = 16 (lane - k) + k; pass 3 (radix 4, sub-transform size 256) wants in[lane + 64 m + 256 r']
    // in slot m + 4 r', i.e. slot s = in[lane + 64 (s & 3) + 256 (s >> 2)].  Written out: the element of row a =
    // lane >> 4, column k, register 4 g + p lands in row p, column k, slot 4 a + g -- the column stays, rows and
    // registers trade places.  That is four 4 x 4 row/register transposes (one per g) on the permlane swaps and a
    // renaming of registers: 64 vector instructions instead of 64 LDS instructions and four waits for the LDS
    // queue (the first exchange moves data across columns and stays on LDS).
#ifndef PEAQ_FE_LDS_EXCHANGE2
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      rows_transpose4(z[4 * g].re, z[4 * g + 1].re, z[4 * g + 2].re, z[4 * g + 3].re);
      rows_transpose4(z[4 * g].im, z[4 * g + 1].im, z[4 * g + 2].im, z[4 * g + 3].im);
    }
#pragma unroll
    for (int a2 = 0; a2 < 4; ++a2)                   // slot 4 a + g <- register 4 g + a
#pragma unroll
      for (int g = a2 + 1; g < 4; ++g) {
        const cplx t = z[4 * a2 + g];
        z[4 * a2 + g] = z[4 * g + a2];
        z[4 * g + a2] = t;
      }
#else
    const int k = lane & 15, j = (lane - k) * 16 + k;
    exchange16(z, unit, [&](int r) { return j + 16 * r; },
               [&](int s) { return lane + 64 * (s & 3) + 256 * (s >> 2); });
#endif
  }
  // the split's W_2048^lane and ear weights (fftearmodel.c:470-472), requested ahead of the fence in front of the split:
  // they have pass 3 to arrive
  const cplx wl = tw_lane(ct, 0, lane);
  double2 ew[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) ew[q] = *reinterpret_cast<const double2*>(ct->ear_w2_pair[q][lane]);
  {
    // W_1024^(r i), i = lane + 64 m: W_1024^lane from the table, times W_16^m (constants), squared and cubed
    constexpr double c1 = 0.92387953251128673848, s1 = 0.38268343236508977173, c2 = 0.70710678118654752440;
    const cplx wb = tw_lane(ct, 1, lane);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const cplx w1 = m == 0 ? wb : m == 1 ? cmul(wb, {c1, -s1}) : m == 2 ? cmul(wb, {c2, -c2}) : cmul(wb, {s1, -c1});
      const cplx w2 = csqr(w1), w3 = cmul(w2, w1);
      z[m + 4] = cmul(z[m + 4], w1);
      z[m + 8] = cmul(z[m + 8], w2);
      z[m + 12] = cmul(z[m + 12], w3);
      dft4(z[m], z[m + 4], z[m + 8], z[m + 12]);
    }
  }
  // z[q] = Z[lane + 64 q].  Even/odd split, two bins per step: with E = (Z[k] + conj Z[1024-k]) / 2,
  // O = (Z[k] - conj Z[1024-k]) / 2i the real signal's spectrum is X[k] = E + W_2048^k O and
  // X[1024-k] = conj(E - W_2048^k O), so a lane that owns k = lane + 64 q (q = 0..7) also produces
  // the power of the mirror bin 1024 - k from the same E and O.  Z[1024-k] lives in lane 64 - lane,
  // slot 15 - q (lane 0: own slot 16 - q, Z[1024] = Z[0]) -- a lane permutation, done bin by bin
  // through the crossbar.  The halvings are exact and folded into the level factor.
  // W_2048^k = W_2048^lane * W_32^q, the second factor is a compile-time constant.
  // Slot q of p[] holds bin lane + 64 q, slot 8 + q the mirror bin (spec_bin() below); lane 0's
  // q = 0 mirror would be bin 1024, which nothing reads: it carries the self-mirrored bin 512.
  before_split();
  wave_lds_fence();                                  // the exchange buffer is about to become Pw
  const int partner = (64 - lane) & 63;
  const double lf4 = 0.25 * level_factor;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int k = lane + 64 * q;
    cplx zm = {__shfl(z[15 - q].re, partner, 64), __shfl(z[15 - q].im, partner, 64)};
    if (lane == 0) zm = z[(16 - q) & 15];
    const cplx e2 = {z[q].re + zm.re, z[q].im - zm.im};               // 2 E
    const cplx o2 = {z[q].im + zm.im, zm.re - z[q].re};               // 2 O
    const cplx wq = {kW32re[q], kW32im[q]};
    const cplx t = cmul(q == 0 ? wl : cmul(wl, wq), o2);
    const cplx xp = cadd(e2, t), xm = csub(e2, t);
    p[q] = (xp.re * xp.re + xp.im * xp.im) * lf4;                     // fftearmodel.c:464-466
    double pm = (xm.re * xm.re + xm.im * xm.im) * lf4;
    int km = 1024 - k;
    if (q == 0 && lane == 0) {                                        // bin 512 = conj Z[512]
      pm = (z[8].re * z[8].re + z[8].im * z[8].im) * level_factor;
      km = 512;
    }
    p[8 + q] = pm;
    unit[kOffPw + k] = p[q] * ew[q].x;                                // fftearmodel.c:470-472
    if (km < kPwLen) unit[kOffPw + km] = pm * ew[q].y;
  }
  wave_lds_fence();
}

// spectrum bin held in slot s of frame_power_spectrum's p[]
__device__ __forceinline__ int spec_bin(int s, int lane) {
  if (s < 8) return lane + 64 * s;
  if (lane == 0 && s == 8) return 512;
  return 1024 - lane - 64 * (s - 8);
}

// critical-band grouping of a spectrum held in LDS (fftearmodel.c:604-620).  The interior bins are
// fetched eight at a time, so that a band of 25 bins costs four LDS round trips instead of 25; beyond
// the band the lane reads sp[zero] -- a slot the caller has set to 0 -- so that the sum needs no
// second predicate (adding +0 is exact); the order of the additions is that of the plain loop.
struct BandEdge {                                    // one band's row of the grouping tables (fftearmodel.c:730-760)
  int lo, hi;
  double wlo, whi;
};
// Requested well before the band sum that uses it: the four values come through L2 with a different band per lane,
// and a band sum that starts by waiting for them waits the longest part of its own duration.
__device__ __forceinline__ BandEdge load_band_edge(const BandTables* __restrict__ bt, int b) {
  return {bt->lo[b], bt->hi[b], bt->wlo[b], bt->whi[b]};
}
__device__ __forceinline__ double group_band(const BandEdge& e, const double* sp, int zero) {
  const int lo = e.lo, hi = e.hi;
  double p = e.wlo * sp[lo] + e.whi * sp[hi];
  for (int k0 = lo + 1; k0 < hi; k0 += 8) {
    typedef const __attribute__((address_space(3))) double* lds_cptr;
    const lds_cptr q = (lds_cptr)sp + k0, z = (lds_cptr)sp + zero;
    const int n = hi - k0;                           // bins left
    double v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      // one compare and one select per slot; the constant j goes into the read's offset field
      lds_cptr qj = j < n ? q : z - j;
      asm("" : "+v"(qj));
      v[j] = qj[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) p += v[j];
  }
  return p < 1e-12 ? 1e-12 : p;
}
// A lane's two band sums -- band e1 of the narrow half, band e2 of the wide half -- by the schedule of
// peaq_group_sched.h: no loop, the interior bins two per read (ds_read2_b64: slot j reads base + 2 j and base + 2 j + 1,
// the constant in the offset fields, one compare and one select per slot), a fixed number of slots per band, the odd
// bin hi - 1 in a read of its own.  Beyond the band a slot reads zero words: sp[zero .. zero + group_zero_words - 1],
// which the caller has set.  The first batch is the whole narrow band and the wide band's edges, then the wide band's slots go
// out group_batch_pairs at a time: all reads of a batch are issued before the first of them is waited for -- the
// scheduling barrier keeps the sums behind the reads, left to itself the scheduler sinks every read to its addition, a
// round trip each (the LDS queue returns in order, so the additions then wait with a count that goes down, not for 0).
// The order of the additions is that of the plain loop and of group_band above, the sums are the same bit for bit.
// -DPEAQ_FE_GROUP_LOOP (VARIANT builds): the loop of group_band at every site, as it was.
template <int NB>
__device__ __forceinline__ void group_bands(const BandEdge& e1, const BandEdge& e2, const double* sp, int zero, double& s1,
                                            double& s2) {
#ifdef PEAQ_FE_GROUP_LOOP
  s1 = group_band(e1, sp, zero);
  s2 = group_band(e2, sp, zero);
#else
  typedef const __attribute__((address_space(3))) double* lds_cptr;
  constexpr int kNarrow = group_narrow_pairs(NB), kWide = group_wide_pairs(NB), kBatch = group_batch_pairs(NB);
  static_assert(kNarrow > 0 && kWide > 0, "band sums: no slot counts for this band count");
  static_assert(2 * kWide + 1 < 256, "band sums: the slot's constant must fit the read's 8-bit offset fields");
  const lds_cptr base = (lds_cptr)sp, z = base + zero;
  auto slot = [&](lds_cptr q, int pairs, int j, double& v0, double& v1) {
    lds_cptr qj = group_slot_live(pairs, j) ? q : z;
    asm("" : "+v"(qj));                              // (keeps the select on the base, the constant in the offset fields)
    v0 = qj[2 * j];
    v1 = qj[2 * j + 1];
  };
  const int pairs1 = group_pairs(e1.lo, e1.hi), pairs2 = group_pairs(e2.lo, e2.hi);
  const lds_cptr q1 = base + e1.lo + 1, q2 = base + e2.lo + 1;
  {
    double v[2 * kNarrow];
    const double lo1 = base[e1.lo], hi1 = base[e1.hi];
#pragma unroll
    for (int j = 0; j < kNarrow; ++j) slot(q1, pairs1, j, v[2 * j], v[2 * j + 1]);
    const double last1 = base[group_leftover_index(e1.lo, e1.hi, zero)];
    const double lo2 = base[e2.lo], hi2 = base[e2.hi];
    __builtin_amdgcn_sched_barrier(0);
    double p = e1.wlo * lo1 + e1.whi * hi1;
#pragma unroll
    for (int j = 0; j < 2 * kNarrow; ++j) p += v[j];
    p += last1;
    s1 = p < 1e-12 ? 1e-12 : p;
    s2 = e2.wlo * lo2 + e2.whi * hi2;
  }
#pragma unroll
  for (int j0 = 0; j0 < kWide; j0 += kBatch) {
    constexpr int kSlots = kBatch;
    const bool last = j0 + kBatch >= kWide;
    double v[2 * kSlots], last2 = 0.;
#pragma unroll
    for (int i = 0; i < kSlots; ++i)
      if (j0 + i < kWide) slot(q2, pairs2, j0 + i, v[2 * i], v[2 * i + 1]);
    if (last) last2 = base[group_leftover_index(e2.lo, e2.hi, zero)];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < kSlots; ++i)
      if (j0 + i < kWide) {
        s2 += v[2 * i];
        s2 += v[2 * i + 1];
      }
    if (last) s2 += last2;
  }
  s2 = s2 < 1e-12 ? 1e-12 : s2;
#endif
}

// Noise spectrum for the NMR MOVs (movs.c:992-996), r - 2 sqrt(r t) + t bin by bin, in place over the test unit's weighted
// spectrum: all loads first, then the arithmetic, then the stores.  Two adjacent bins per lane and step: 16-byte LDS
// operations (the unit is 16-byte aligned), 7 + 7 reads and 7 writes instead of the 13 + 13 and 13 of one bin per lane;
// the same arithmetic per bin, the same bits.  -DPEAQ_FE_NOISE_SINGLE (VARIANT builds): one bin per lane and step, as it was.
__device__ __forceinline__ void noise_spectrum_in_place(const double* pw_ref, double* pw_test, int lane) {
#ifndef PEAQ_FE_NOISE_SINGLE
  static_assert(kPwLen % 2 == 0, "noise spectrum: two bins per lane");
  constexpr int kPairs = kPwLen / 2, kSteps = (kPairs + 63) / 64;
  double2 r[kSteps], t[kSteps];
#pragma unroll
  for (int i = 0; i < kSteps; ++i) {
    const int k = lane + 64 * i < kPairs ? 2 * (lane + 64 * i) : 0;
    r[i] = *reinterpret_cast<const double2*>(pw_ref + k);
    t[i] = *reinterpret_cast<const double2*>(pw_test + k);
  }
  wave_lds_fence();
#pragma unroll
  for (int i = 0; i < kSteps; ++i)
    if (lane + 64 * i < kPairs)
      *reinterpret_cast<double2*>(pw_test + 2 * (lane + 64 * i)) =
          make_double2(r[i].x - 2 * sqrt_pos(r[i].x * t[i].x) + t[i].x, r[i].y - 2 * sqrt_pos(r[i].y * t[i].y) + t[i].y);
#else
  constexpr int kSteps = (kPwLen + 63) / 64;
  double r[kSteps], t[kSteps];
#pragma unroll
  for (int i = 0; i < kSteps; ++i) {
    const int k = lane + 64 * i < kPwLen ? lane + 64 * i : 0;
    r[i] = pw_ref[k];
    t[i] = pw_test[k];
  }
  wave_lds_fence();
#pragma unroll
  for (int i = 0; i < kSteps; ++i)
    if (lane + 64 * i < kPwLen) pw_test[lane + 64 * i] = r[i] - 2 * sqrt_pos(r[i] * t[i]) + t[i];
#endif
}

// ---------------------------------------------------------------------------
// Data-boundary detector (gstpeaq.c:1081-1099), bit-exact: the reference keeps
// a FLOAT running sum of |x| over 5 samples and tests it from i = 5 on.  The
// exact 5-sample window sums decide unless they come within the float sum's
// worst-case drift (< 5e-7 over 2048 steps) of the threshold; only then one
// lane replays the sequential float recurrence.  `ax` = |x| staged in LDS.
// ---------------------------------------------------------------------------
__device__ __forceinline__ int boundary_detect(const float* ax, int n, int lane) {
  const double thr = 200. / 32768;
  double wmax = 0.;
  for (int i = 5 + lane; i < n; i += 64) {
    const double w = (double)ax[i] + (double)ax[i - 1] + (double)ax[i - 2] + (double)ax[i - 3] + (double)ax[i - 4];
    wmax = fmax(wmax, w);
  }
  wmax = wave_max(wmax);
  if (wmax >= thr + 1e-6) return 1;
  if (wmax < thr - 1e-6) return 0;
  int res = 0;
  if (lane == 0) {
    float sum = 0;
    for (int i = 0; i < 5; ++i) sum = (float)((double)sum + (double)ax[i]);
    for (int i = 5; i < n; ++i) {
      sum = (float)((double)sum + ((double)ax[i] - (double)ax[i - 5]));
      if ((double)sum >= thr) {
        res = 1;
        break;
      }
    }
  }
  return __builtin_amdgcn_readfirstlane(res);
}

// XCD-aware bijective remap (the dispatcher places block b on XCD b % 8): work
// items that share input cache lines -- the two channels of a frame and the
// 50 %-overlapping neighbour frames -- become neighbours on ONE XCD's L2.
__device__ __forceinline__ unsigned xcd_remap(unsigned b, unsigned n) {
  const unsigned q = n >> 3, r = n & 7, xcd = b & 7, slot = b >> 3;
  const unsigned base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + slot;
}

// ---------------------------------------------------------------------------
// Frame access.  A frame is read through a raw buffer resource (scalar registers: base = the
// frame's first sample, size = what is left of the signal from there, at most one frame): lanes
// add 32-bit offsets, and everything beyond the signal's end reads as zero -- the zero padding of
// the flush frame (gstpeaq.c:733-738) costs nothing and there is only one load path (gfx950
// checks the range of a multi-dword buffer load dword by dword, and dword alignment is enough).
// ---------------------------------------------------------------------------
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

struct FrameSrc {
  __amdgpu_buffer_rsrc_t rs;
  int channels, chan;
  // frame starting at sample s0 of a signal with n_valid samples per channel
  __device__ __forceinline__ void set(const float* x, long long s0, long long n_valid, int channels_, int chan_) {
    channels = channels_;
    chan = chan_;
    long long l = n_valid - s0;
    l = l < 0 ? 0 : l > kFrame ? kFrame : l;
    const unsigned long long v = reinterpret_cast<unsigned long long>(x + s0 * channels);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);           // wave-uniform by construction: say so
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    float* p = reinterpret_cast<float*>(((unsigned long long)hi << 32) | lo);
    rs = __builtin_amdgcn_make_buffer_rsrc(p, 0, __builtin_amdgcn_readfirstlane((int)l * channels * 4), 0x00020000);
  }
  // byte offset of this lane's first sample pair; pair lane + 64 r sits r * row_bytes() further on
  __device__ __forceinline__ int lane_offset(int lane) const { return channels == 1 ? lane * 8 : lane * 16 + chan * 4; }
  // samples 2 n and 2 n + 1 of this channel, n = lane + 64 r: ONE lane offset for all r (voff = lane_offset),
  // the row as the instruction's scalar offset -- no vector arithmetic per load; the range check covers
  // vector + scalar + immediate offset (tools/probes/oob_soffset.hip)
  __device__ __forceinline__ void load2(int r, int voff, float& x0, float& x1) const {
    if (channels == 1) {
      const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, r * 512, 0);
      x0 = __uint_as_float(v.x);
      x1 = __uint_as_float(v.y);
    } else {
      // two 4-byte loads of this channel rather than 16 bytes of both: half the data through the
      // return path of the vector-memory pipe (its busiest part), no selects, and the sibling
      // channel's workgroup finds the lines in L2 either way (+2 % measured)
      x0 = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff, r * 1024, 0));
      x1 = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff + 8, r * 1024, 0));
    }
  }
};

// Phase timing for tools/fe_profile.py (development builds with -DPEAQ_FE_PROFILE only): the cycles
// between consecutive marks are summed per wave role and phase.
#ifdef PEAQ_FE_PROFILE
#define FE_MARK(i)                                                                     \
  do {                                                                                 \
    const unsigned long long now_ = __builtin_readcyclecounter();                      \
    if (a.prof && lane == 0 && (blockIdx.x & 127) == 5) atomicAdd(a.prof + sig * 16 + (i), now_ - prof_t_); \
    prof_t_ = __builtin_readcyclecounter();                                            \
  } while (0)
#else
#define FE_MARK(i) do { } while (0)
#endif

template <int NB>
__global__ __launch_bounds__(128, kWavesPerSimd)
#ifdef PEAQ_FE_NUM_VGPR
__attribute__((amdgpu_num_vgpr(PEAQ_FE_NUM_VGPR)))
#endif
void frontend_kernel(FrontendArgs a) {
  extern __shared__ double lds[];
  // a fresh wave gets its frame requested before its older neighbours on the SIMD issue their next arithmetic:
  // what it waits for longest is that frame (+ 0.5 % measured; back to normal once the loads are out)
  __builtin_amdgcn_s_setprio(3);
#ifndef PEAQ_FE_LAZY_KERNARGS
  // Everything the start-up needs of the argument block is "used" HERE: the compiler then issues the scalar loads
  // together and waits once.  Left to itself it fetches the block piece by piece where the pieces are first needed --
  // five dependent round trips through the scalar cache (~ 1.4 k cycles between a wave's first instruction and its
  // first sample load, profiles/r06_frontend_phases.json phases 15 + 13).
  asm volatile("" ::"s"(a.ref), "s"(a.test), "s"(a.pair_stride), "s"(a.n_ref), "s"(a.n_test), "s"(a.n_uniform_ref),
               "s"(a.n_uniform_test), "s"(a.n_frames), "s"(a.n_frames_uniform), "s"(a.frame_origin), "s"(a.off_ref),
               "s"(a.off_test), "s"(a.channels), "s"(a.frame0), "s"(a.frames_per_launch), "s"(a.fpl_magic), "s"(a.common),
               "s"(a.records), "s"(a.pair_frame0), "s"(gridDim.x));
#endif
  const int lane = threadIdx.x & 63;
  // 0 = reference wave, 1 = test wave; wave-uniform, so keep it (and all that hangs on it) scalar
  const int sig = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#ifdef PEAQ_FE_PROFILE
  unsigned long long prof_t_ = __builtin_readcyclecounter();
  if (a.prof && lane == 0 && (blockIdx.x & 127) == 5) atomicAdd(a.prof + 32 + sig, 1ull);   // one workgroup in 128 is sampled
#endif
  double* unit = lds + sig * kUnitDoubles;
  double* scratch = unit + kOffScratch;
  const CommonTables* __restrict__ ct = a.common;
  const BandTables* __restrict__ bt = a.bands;

  // ---- which (pair, frame, channel) -------------------------------------------
  // item = (pair * frames_per_launch + fl) * channels + chan, taken apart without integer divisions
  // (channels is 1 or 2; the launch carries the reciprocal of frames_per_launch)
  auto decode = [&](unsigned it, unsigned& pair_, unsigned& fl_) {
    const unsigned t = it >> (a.channels - 1);
    pair_ = a.frames_per_launch == 1 ? t : __umulhi(t, a.fpl_magic);   // (the reciprocal of 1 does not fit)
    fl_ = t - pair_ * a.frames_per_launch;
    return (int)(it & (unsigned)(a.channels - 1));
  };
  const unsigned item = xcd_remap(blockIdx.x, gridDim.x);
  unsigned pair, fl;
  const int chan = decode(item, pair, fl);
  FE_MARK(15);                                       // wave start-up: first instructions, kernel arguments
  const unsigned n_ref = a.n_ref ? a.n_ref[pair] : a.n_uniform_ref;
  const unsigned n_test = a.n_test ? a.n_test[pair] : a.n_uniform_test;
  unsigned frame, frame_origin;
  if (a.pair_frame0) {                               // broker launch: this pair's own window
    if (fl >= a.pair_nframes[pair]) return;
    frame_origin = a.pair_frame0[pair];
    frame = frame_origin + fl;
  } else {
    frame = a.frame0 + fl;
    frame_origin = a.frame_origin;
    const unsigned n_frames = a.n_frames ? a.n_frames[pair] : a.n_frames_uniform;
    if (frame >= n_frames) return;                   // whole workgroup leaves together
  }
  const size_t pair_off = (size_t)pair * a.pair_stride * a.channels;
  FrameSrc src_ref, src_test;
  {
    const long long s0 = (long long)(frame - frame_origin) * kHop;
    src_ref.set(a.ref + pair_off, s0 + a.off_ref, (long long)n_ref, a.channels, chan);
    src_test.set(a.test + pair_off, s0 + a.off_test, (long long)n_test, a.channels, chan);
  }
  const FrameSrc& src = sig ? src_test : src_ref;
  double* __restrict__ rec =
      a.records + ((size_t)(pair * a.frames_per_launch + fl) * a.channels + chan) * kRecDoubles;
  // ---- load + window (fftearmodel.c:451-452), energy flag (:508-514), totalsnr energies over the hop
  // (gstpeaq.c:913-918; float products): the reference wave sums ref^2 from its own samples, the test
  // wave fetches the reference's first 1024 samples in the same batch of loads for (ref - test)^2.
  // The window is evaluated, not read: sample k = 2 (lane + 64 r) + j has the angle
  // theta(2 lane + j) + r d, d = 2 pi 128 / 2047, so w = A (1 - cos) = A - (A cos th) C_r + (A sin th) S_r
  // from four per-lane values and 32 literals -- 2 KB instead of 16 KB through the vector memory
  // pipe per wave, which is what the first phase of this kernel waits for.
  constexpr double kHannA = 0.81649658092772603273;             // sqrt(8/3) / 2
  constexpr double kHannC[16] = {1.0, 0.923806101034885660186, 0.7068354246185547448714, 0.3821516543455241229047,
                                 -0.0007673650086148258012924, -0.3835694472988822502431, -0.7079202261619581075015,
                                 -0.9243926006499437062869, -0.9999988223018871071366, -0.9232174254904238786877,
                                 -0.7057489581976599840459, -0.3807329612736016723471, 0.002302093218395832312485,
                                 0.3849863367942118830771, 0.7090033602727326108775, 0.9249769229541590372578};
  constexpr double kHannS[16] = {0.0, 0.382860663545790020567, 0.7073780336597309217442, 0.92409962292005024589,
                                 0.99999970557542843387, 0.923512035167290059731, 0.7062923993579444458354,
                                 0.3814424201155840173045, -0.001534729565367423810065, -0.3842780051874341062575,
                                 -0.7084620018059667117941, -0.924685034052046356158, -0.9999973501798961346679,
                                 -0.9229222721777677728372, -0.705205101457706221079, -0.3800232782373413192215};
  const double2 hl0 = *reinterpret_cast<const double2*>(&ct->hann_lane[lane][0]);
  const double2 hl1 = *reinterpret_cast<const double2*>(&ct->hann_lane[lane][2]);
  double* ltab = lds + kOffLogTab + sig * kLogTabDoubles;   // this wave's copy of the logarithm table (filled below)
  FE_MARK(13);                                       // work-item decoding, pointers
  cplx z[16];
  float amax = 0.f;
  double energy = 0., hop = 0.;                      // hop: sum ref^2 (reference wave) / sum (ref - test)^2 (test wave)
  {
    const int voff = src.lane_offset(lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = lane + 64 * r;
      float x0, x1;
      src.load2(r, voff, x0, x1);
      const double w0 = fma(hl0.y, kHannS[r], fma(-hl0.x, kHannC[r], kHannA));
      const double w1 = fma(hl1.y, kHannS[r], fma(-hl1.x, kHannC[r], kHannA));
      z[r] = {w0 * (double)x0, w1 * (double)x1};
      if (r >= 8) {                                  // samples 1024..2047; float products, double sum
        energy += (double)(x0 * x0);
        energy += (double)(x1 * x1);
      } else if (sig == 0) {
        hop += (double)(x0 * x0);
        hop += (double)(x1 * x1);
      } else {
        float r0, r1;
        src_ref.load2(r, voff, r0, r1);               // same channel count and channel: same lane offset
        hop += (double)((r0 - x0) * (r0 - x0));
        hop += (double)((r1 - x1) * (r1 - x1));
      }
      // a single sample above the threshold settles the boundary detector; sample 0
      // is excluded because the first tested window is [1..5]
      amax = fmaxf(amax, n == 0 ? fabsf(x1) : fmaxf(fabsf(x0), fabsf(x1)));
    }
  }
  // ---- L2 prefetch for a workgroup further down this XCD's queue.  A fresh wave has nothing to do
  // until its frame has arrived, and under load the half of it that no earlier frame has touched
  // takes thousands of cycles to come from HBM.  So every channel-0 workgroup touches, one dword per
  // 128-byte line, the not yet seen samples of the frame that the workgroup kPrefetchItems items
  // further on will load: by then they sit in this XCD's L2 (items are dealt to an XCD in order).
  // The value is never used; one compare at the end of the kernel keeps the loads alive.
  float pf_keep = 0.f;
  if (chan == 0 && !a.pair_frame0) {
    const unsigned it2 = item + kPrefetchItems;
    if (it2 < gridDim.x) {
      unsigned pair2, fl2;
      decode(it2, pair2, fl2);
      const unsigned n2 = sig ? (a.n_test ? a.n_test[pair2] : a.n_uniform_test) : (a.n_ref ? a.n_ref[pair2] : a.n_uniform_ref);
      // frame 0 of a chunk is new as a whole, later ones share their first half with their predecessor
      const long long s2 = (long long)(a.frame0 + fl2 - a.frame_origin) * kHop + (fl2 == 0 ? 0 : kHop);
      FrameSrc pf;
      pf.set((sig ? a.test : a.ref) + (size_t)pair2 * a.pair_stride * a.channels, s2 + (sig ? a.off_test : a.off_ref),
             (long long)n2, a.channels, 0);
      pf_keep = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(pf.rs, lane * 128, 0, 0));
      if (fl2 == 0 && a.channels == 2)               // 16 KiB: a second row of 64 lines
        pf_keep += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(pf.rs, (64 + lane) * 128, 0, 0));
    }
  }

  __builtin_amdgcn_s_setprio(0);
#ifdef PEAQ_FE_PROFILE
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  FE_MARK(14);                                       // sample loads + window
  wave_sum2(hop, energy, hop, energy);
  if (lane == 0) rec[sig ? kRecNoiseE : kRecSigE] = hop;
  const int energy_flag = energy >= 8000. / (32768. * 32768.);

  int above = 0;
  if (sig == 0) {
    if (__any((double)amax >= 200. / 32768 + 1e-6)) {   // (a vote: nobody needs the maximum itself)
      above = 1;
    } else {
      // quiet frame: stage |x| (8 KiB, start of the still unused FFT buffer) and decide exactly
      float* ax = reinterpret_cast<float*>(unit);
      int lane_q = lane;                             // opaque copy: recompute the indices here rather
      asm volatile("" : "+v"(lane_q));               // than keep 16 of them alive from the first loop
      const int voff_q = src.lane_offset(lane_q);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = lane_q + 64 * r;
        float x0, x1;
        src.load2(r, voff_q, x0, x1);
        reinterpret_cast<float2*>(ax)[n] = make_float2(fabsf(x0), fabsf(x1));
      }
      wave_lds_fence();
      above = boundary_detect(ax, kFrame, lane);
      wave_lds_fence();
    }
  }

  if (lane == 0)                                     // out now: nothing of this stays live over the transform
    rec[sig ? kRecFlagsTest : kRecFlagsRef] = (double)(above | (energy_flag << 1));

  FE_MARK(0);                                        // load, window, flags
  double pspec[16];                                  // unweighted power spectrum, bin lane + 64 q
  // This wave's share of the logarithm table is requested ahead of the split's fences (behind them it would be waited
  // for at once; at the start of the kernel the three loads would sit in front of the frame's own) ...
  double2 lt0, lt1, lt2;
  frame_power_spectrum(z, pspec, unit, lane, ct, a.level_factor, [&] {
    lt0 = *reinterpret_cast<const double2*>(ct->log_tab[lane]);
    lt1 = *reinterpret_cast<const double2*>(ct->log_tab[64 + lane]);
    lt2 = *reinterpret_cast<const double2*>(ct->log_tab[128]);
  });
  // the band edges of this lane's two band sums (a narrow and a wide band, see below), requested now
  const int gb1 = lane < (NB + 1) / 2 ? lane : 0, gb2 = lane < (NB + 1) / 2 ? NB - 1 - lane : 0;
  const BandEdge edge1 = load_band_edge(bt, gb1), edge2 = load_band_edge(bt, gb2);
  // ... and goes into LDS here (log_tab, peaq_wave.h): every wave fills its OWN copy -- no workgroup barrier stands
  // between the transform and the first logarithm any more.
  {
    reinterpret_cast<double2*>(ltab)[lane] = lt0;
    reinterpret_cast<double2*>(ltab)[64 + lane] = lt1;
    if (lane == 0) reinterpret_cast<double2*>(ltab)[128] = lt2;
    wave_lds_fence();
  }
  FE_MARK(1);                                        // FFT + split
  // ---- bandwidths (movs.c:776-809) on the unweighted spectra, straight from the registers.  The three
  // steps hand a number from one wave to the other twice -- the test wave's zero threshold to the reference
  // wave's search, the reference bandwidth to the test wave's search -- and ride on the two workgroup barriers
  // the kernel has anyway (after the spreading phase, after the log ratios) instead of two of their own:
  // a barrier is where a wave waits for its partner on another SIMD, and fewer of them is what makes the
  // workgroup less sensitive to whatever else runs on either SIMD.  The spectra stay in
  // registers until then.  The advanced version has no bandwidth MOVs (gstpeaq.c:924-959): its 55-band kernel
  // skips all of this.
  constexpr bool kAdvanced = NB == 55;
  int bw_ref = 0, bw_test = 0;
  double* xch = lds + kOffLogTab + 2 * kLogTabEntries;   // [2] exchanged scalars: the spare words behind the first table
  double thr = 0.;                                   // powers are >= 0
  // One compare per slot; the rest is scalar: the compare's lane mask says which bins of the slot
  // pass, its highest (slots 0..7: bin = 64 q + lane) or lowest (mirror slots: bin = 1024 - 64 q - lane)
  // set bit below the limit is the slot's top bin.  Returns the highest such bin + 1 over all slots, 0 if none.
  // The slots are walked from the top of the spectrum down -- mirror slots q = 0..7 (bins 1023..513), bin 512 (lane 0
  // of mirror slot 0, spec_bin), direct slots q = 7..0 -- and the first slot with a hit ends the search, as the
  // reference's own loop does (movs.c:776-809); the ballot is wave-uniform, so the exit is a scalar branch.
  auto top_bin = [&](double level, int limit, bool or_equal) {
    bool hit512 = false;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      unsigned long long m = __ballot(or_equal ? pspec[8 + q] >= level : pspec[8 + q] > level);
      if (q == 0) {                                // lane 0 carries bin 512 here: its turn comes behind slot 7
        hit512 = (m & 1ull) && 512 < limit;
        m &= ~1ull;
      }
      const int lo = 1024 - 64 * q - limit + 1;    // lanes lo .. 63 hold bins below the limit
      m &= lo >= 64 ? 0ull : lo <= 0 ? ~0ull : ~0ull << lo;
      if (m) return 1024 - 64 * q - __builtin_ctzll(m) + 1;
    }
    if (hit512) return 513;
#pragma unroll
    for (int q = 7; q >= 0; --q) {
      unsigned long long m = __ballot(or_equal ? pspec[q] >= level : pspec[q] > level);
      const int nl = limit - 64 * q;               // lanes 0 .. nl - 1 hold bins below the limit
      m &= nl >= 64 ? ~0ull : nl <= 0 ? 0ull : (1ull << nl) - 1ull;
      if (m) return 64 * q + 64 - __builtin_clzll(m);
    }
    return 0;
  };
  if (!kAdvanced && sig == 1) {
    // zero threshold = max over bins 921..1023 of the test spectrum: the mirror bins 1024 - (lane + 64 q)
    // of q = 0 (lanes 1..63) and q = 1 (lanes 0..39); read by the reference wave behind the next barrier
    if (lane >= 1) thr = pspec[8];
    if (lane <= 39) thr = fmax(thr, pspec[9]);
    thr = wave_max(thr);
    if (lane == 0) xch[0] = thr;
  }

  FE_MARK(2);                                        // the test wave's zero threshold
  const double* pw_ref = lds + kOffPw;
  double* pw_test = lds + kUnitDoubles + kOffPw;
  double* sa = lds + kOffScratch;                            // [512] the reference unit's scratch
  double* sb = lds + kUnitDoubles + kOffScratch;             // [512] the test unit's scratch
  // Advanced version (55 bands): of the test signal only the weighted spectrum is used -- noise in bands and EHS,
  // process_fft_block_advanced gstpeaq.c:924-959 -- so its wave has no band phase of its own.  The waves meet ONCE, here,
  // with both weighted spectra in LDS; from there on two one-way flags in LDS replace the barrier (round 6: behind a
  // second barrier the reference wave ran the whole error-harmonic structure alone, 8.7 k cycles in which the test wave's
  // slot stood empty -- a fifth of the workgroup's life):
  //   test wave:  log ratios (into ITS scratch area) -> noise spectrum in place -> flag 1 -> waits for flag 0 -> the
  //               error-harmonic structure, exchanging through its scratch area and the REFERENCE wave's spectrum
  //               (dead once that wave has its band sums: flag 0);
  //   ref wave:   band sums -> flag 0 -> spreading, record -> waits for flag 1 -> the noise spectrum's band sums.
  int* adv_flag = reinterpret_cast<int*>(lds + kOffLogTab + kLogTabDoubles + 2 * kLogTabEntries);   // the second table's spare words
  auto wait_flag = [&](int i) {
    while (__builtin_amdgcn_readfirstlane(*(volatile int*)(adv_flag + i)) == 0) __builtin_amdgcn_s_sleep(1);
    wave_lds_fence();
  };
  if constexpr (kAdvanced) {
    if (sig == 0 && lane == 0) {
      adv_flag[0] = 0;
      adv_flag[1] = 0;
    }
    __syncthreads();
    if (sig == 1) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {                  // movs.c:1383-1391: d[k] = ln(Pw_test / Pw_ref), k < 512
        const int k = lane + 64 * j;
        const double fr = pw_ref[k], ft = pw_test[k];
        sb[k] = (fr == 0. && ft == 0.) ? 0. : FE_LOG_NONNEG(ft / fr, ltab);   // +-inf when one side is digital silence
      }
      FE_MARK(8);                                    // log ratios
      wave_lds_fence();
      noise_spectrum_in_place(pw_ref, pw_test, lane);   // movs.c:992-996, as in the basic version below
      wave_lds_fence();
      if (lane == 0) adv_flag[1] = 1;                // the noise spectrum stands (LDS operations of a wave execute in order)
      FE_MARK(10);                                   // test wave: noise spectrum
    }
  }
  // ---- critical bands, internal noise, spreading ------------------------------------
  if (!kAdvanced || sig == 0) {
    // lane owns bands 2 lane and 2 lane + 1
    const double* pw = unit + kOffPw;
    constexpr int kZeroSlot = kOffScratch + 400 - kOffPw;   // a free word of the scratch area, as an index into Pw
    // the zero words of the band sums' idle slots (free: the band sums' exchange space ends at scratch[383]); in the
    // advanced version they serve the noise spectrum's band sums as well -- nothing writes here in between
    static_assert(400 + group_zero_words(NB) <= 512 && group_zero_words(NB) / 2 <= 64, "band sums: the zero words lie in the scratch area");
    if (lane < group_zero_words(NB) / 2) *reinterpret_cast<double2*>(scratch + 400 + 2 * lane) = make_double2(0., 0.);
    wave_lds_fence();
    // Band sums with a balanced assignment -- lane L adds up band L (narrow) and band NB-1-L (wide):
    // the longest loop is ~27 bins instead of the ~50 of two adjacent top bands -- handed over to
    // the two-adjacent-bands layout of everything that follows through LDS.
    double* ppx = scratch + 256;                       // [128]
    // ... and the per-band constants of the spreading phase, requested before the band sums run
    const int b0 = 2 * lane;
    double c_noise[2], c_lnauc[2], c_gil[2];
    const double c_dz02 = bt->dz02, c_ale = bt->aLe;   // (two scalars of the same tables, used behind the band sums' fences)
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const int b = b0 + s2 < NB ? b0 + s2 : 0;
      c_noise[s2] = bt->internal_noise[b];
      c_lnauc[s2] = bt->ln_aUC[b];
      c_gil[s2] = bt->gIL[b];
    }
    if (lane < (NB + 1) / 2) {
      const int b1 = lane, b2 = NB - 1 - lane;
      double s1, s2;                                   // (the middle lane's two bands are one: it stores the same sum twice)
      group_bands<NB>(edge1, edge2, pw, kZeroSlot, s1, s2);
      ppx[b1] = s1;
      ppx[b2] = s2;
    }
    wave_lds_fence();
    if (kAdvanced && lane == 0) adv_flag[0] = 1;       // this wave has read its weighted spectrum for the last time
    FE_MARK(3);                                        // band grouping
    // Upward spreading, Kabal (27): E2[j] += Ene[i] a_i^(j-i) for j > i, a_i = aUCEe[i] -- the reference's O(B^2) loop
    // (fftearmodel.c:657-667).  Every band's contributions are a geometric sequence along the target bands; they used
    // to be scattered into LDS with one atomic per step -- 40 % of the time of an LDS array that was 54 % busy, and an
    // LDS store costs this kernel more than two FP64 instructions (profiles/r05_ab_basic.txt).  Now the ACCUMULATORS travel instead: the pair of sums for the bands
    // of lane M sits in lane M - k while the sources add what they send k lanes up, and moves one lane up (two DPP
    // moves per double, zeros entering at lane 0) after every step, k = kLanes .. 1 -- so it arrives home complete,
    // and sums for bands that do not exist leave at the top.  Walking k DOWN means walking each source's sequence
    // from its far end: u = Ene[2L] a^(2k), v = Ene[2L+1] a'^(2k-1) start at k = kLanes from one exponential each
    // and go back two bands per step with 1 / a^2; what a lane adds per step is (u + v, a u + a' v).
    //
    // Two streams (peaq_spread_sched.h): at distance K only the sources L <= kLanes - K have a target, so the far
    // distances K0 + 1 .. kLanes run in the lanes 32 + L, on a copy of source L (v_permlane32_swap), WHILE the lanes
    // below 32 run the main stream's first steps k = K0 .. kBoundary: the same instructions, kHelper = kLanes - K0 lanes
    // of distance apart -- K0 = 39 steps instead of 54 at 109 bands, 14 instead of 27 at 55.  While both run, a lane adds
    // only from its step `act` on, so that no sum of a band that does not exist walks into the helper's lanes; behind
    // the boundary step the helper's finished sums go home through LDS (fetched behind the loop), its lanes are
    // cleared, and the lanes >= 32 carry on with their own source at distance kBoundary - 1 -- their first with a target.
    // -DPEAQ_FE_SPREAD_ONE_STREAM (VARIANT builds): the single stream k = kLanes .. 1 in every lane, as it was.
    constexpr int kLanes = spread_lanes(NB);           // the farthest lane a band reaches: band 0 -> band NB - 1
#ifdef PEAQ_FE_SPREAD_ONE_STREAM
    constexpr int kHelper = 0, kFirst = kLanes, kBoundary = kLanes + 1;
    constexpr int kExpUpper = 2 * kLanes, kExpHelper = 0;
    constexpr int kUnrollMain = 9;
#else
    constexpr int kUnrollMain = 8;
    constexpr int kHelper = spread_helper_steps(NB), kFirst = spread_k0(NB), kBoundary = spread_boundary(NB);
    constexpr int kExpUpper = spread_exp_upper(NB, 0), kExpHelper = spread_exp_helper(NB);
#endif
    // far: the source's term at the first distance of its stream (main: 2 kFirst (- 1) bands up; the copies' start is
    // kExpHelper / 2 lanes farther); upper: the same at distance kBoundary - 1; back2 = a^-2
    double ene[2], ae[2], far[2], back2[2];
    [[maybe_unused]] double far_copy[2], upper[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int b = b0 + s;
      if (b < NB) {
        const double pp = ppx[b] + c_noise[s];                                                       // :483-485
        // Kabal (23)-(24); fftearmodel.c:649-656.  a^y evaluated as exp(y ln a); the three powers of
        // aUCE share one exponential (t = aUCE^0.2: aUCE^0.4 = t^2, aUCE = t^5), and En^0.4 takes its
        // logarithm as ln Pp - ln(gIL + gIU - 1) instead of dividing first
        const double ln_pp = FE_LOG(pp, ltab);
        const double ln_a = c_lnauc[s] + c_dz02 * ln_pp;
        const double t = exp_fast(0.2 * ln_a), t2 = t * t;
        const double a_uce = t2 * t2 * t;
        const double g_iu = div_fast(1. - exp_fast((double)(NB - b) * ln_a), 1. - a_uce);
        ae[s] = t2;
        ene[s] = exp_fast(0.4 * (ln_pp - FE_LOG(c_gil[s] + g_iu - 1., ltab)));
        // a^(0.4 e) = t2^e by squaring: the exponents are compile-time constants (about ten multiplications for an
        // exponential), and the squares are shared between the start terms
        upper[s] = ene[s] * pow_const(t2, kExpUpper - s);
        if constexpr (kHelper > 0) {
          const double ph = pow_const(t2, kExpHelper);
          far[s] = upper[s] * ph;
          far_copy[s] = far[s] * ph;
        } else {
          far[s] = upper[s];
        }
        // (a^-0.8; 0 where a^0.8 underflows -- never with finite samples, the internal noise bounds Pp from below -- so
        // that such a source sends nothing instead of 0 x inf: the walk's rounding, ~ kLanes ulp on the near terms and
        // ~ 1e-14 relative in all, is DESIGN.md 3's)
        const double t4 = t2 * t2;
        back2[s] = t4 > 1e-290 ? div_fast(1., t4) : 0.;
      } else {
        ae[s] = 0.;
        ene[s] = 0.;
        far[s] = 0.;
        far_copy[s] = 0.;
        upper[s] = 0.;
        back2[s] = 0.;
      }
    }
    FE_MARK(4);                                        // logarithms / exponentials per band
    double up0 = 0., up1 = 0.;                         // E2up of the bands 2 (lane + k), 2 (lane + k) + 1 while in flight
    {
      double u = far[0], v = far[1];
      [[maybe_unused]] double2 home = make_double2(0., 0.);
      if constexpr (kHelper > 0) {
        // lanes >= 32: source lane - 32 at the helper's first distance
        u = lower_halves(far[0], far_copy[0]);
        v = lower_halves(far[1], far_copy[1]);
        const double wa0 = lower_halves(ae[0], ae[0]), wa1 = lower_halves(ae[1], ae[1]);
        const double wb0 = lower_halves(back2[0], back2[0]), wb1 = lower_halves(back2[1], back2[1]);
        const int act = lane < kSpreadHelperBase ? kLanes - lane : kFirst - (lane - kSpreadHelperBase);   // spread_act
#pragma unroll 5
        for (int k = kFirst; k >= kBoundary; --k) {
          if (k <= act) {
            asm volatile("");                          // keeps this an EXEC mask: as four selects a step it gains 0.4 % instead of 2 % (profiles/r08_ab_basic.txt)
            up0 += u;
            up0 += v;
            up1 = fma(wa0, u, up1);
            up1 = fma(wa1, v, up1);
          }
          up0 = lane_below(up0);
          up1 = lane_below(up1);
          u *= wb0;
          v *= wb1;
        }
        // the helper's sums stand spread_home_shift lanes below home; every lane writes (zeros outside the helper's), so
        // that every lane may read: the band sums' exchange space is free (ppx was read for the last time above)
        const bool lower = lane < kSpreadHelperBase;
        double2* hx = reinterpret_cast<double2*>(ppx);
        hx[(lane + spread_home_shift(NB) + kSpreadWave) & (kSpreadWave - 1)] = lower ? make_double2(0., 0.) : make_double2(up0, up1);
        wave_lds_fence();
        home = hx[lane];
        up0 = lower ? up0 : 0.;
        up1 = lower ? up1 : 0.;
        u = lower ? u : upper[0];
        v = lower ? v : upper[1];
      }
#pragma unroll kUnrollMain
      for (int k = kBoundary - 1; k >= 1; --k) {
        up0 += u;
        up0 += v;
        up1 = fma(ae[0], u, up1);
        up1 = fma(ae[1], v, up1);
        up0 = lane_below(up0);
        up1 = lane_below(up1);
        u *= back2[0];
        v *= back2[1];
      }
      if constexpr (kHelper > 0) {
        up0 += home.x;
        up1 += home.y;
      }
      up1 = fma(ae[0], ene[0], up1);                   // band 2 lane to its own neighbour 2 lane + 1
    }
    FE_MARK(5);                                        // upward spreading
    // downward spreading, Kabal (28): E2[i-1] = aLe E2[i] + Ene[i-1]  (suffix scan)
    double dn0, dn1;
    {
      const double al = c_ale;
      const double v = wave_suffix_geometric(ene[0] + al * ene[1], al * al, lane);   // pair-local, then over the lanes
      const double nxt = lane_above(v);                // E2down[2 lane + 2]; 0 beyond the last lane
      dn0 = v;
      dn1 = ene[1] + al * nxt;
    }
    // (25): the excitation is E2^(1/0.4) / normalisation; the record carries E2^(1/4), from which the back
    // end gets E and E^0.3 by multiplications (excitation_from_root, peaq_device.h)
    double root[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const double e2 = (s ? dn1 : dn0) + (s ? up1 : up0);   // band 2 lane + s
      root[s] = b0 + s < NB ? sqrt_pos(sqrt_pos(e2)) : 0.;
    }
    if (b0 < kBandStride)
      *reinterpret_cast<double2*>(rec + (sig ? kRecRootTest : kRecRootRef) + b0) = make_double2(root[0], root[1]);

  }
  FE_MARK(6);                                        // downward spreading, excitation, record
  if constexpr (kAdvanced) {
    if (sig == 0) {
      // the band sums of the noise spectrum (movs.c:997-1000), which the test wave has left in its unit
      const BandEdge e1 = load_band_edge(bt, gb1), e2 = load_band_edge(bt, gb2);   // (asked for again, not held since the transform)
      wait_flag(1);
      const int zero_at = (int)(scratch + 400 - pw_test);   // the zero words of this wave's first band sums, still standing
      if (lane < (NB + 1) / 2) {
        const int b1 = lane, b2 = NB - 1 - lane;
        double s1, s2;
        group_bands<NB>(e1, e2, pw_test, zero_at, s1, s2);
        rec[kRecNoise + b1] = s1;
        rec[kRecNoise + b2] = s2;
      } else if (lane < (NB + 1) / 2 + kBandStride - NB) {
        rec[kRecNoise + NB + lane - (NB + 1) / 2] = 0.;  // padding slots of the band vector
      }
      if (lane == 0) {
        rec[kRecBwRef] = 0.;
        rec[kRecBwTest] = 0.;
      }
    } else {
      wait_flag(0);                                  // the reference wave's spectrum is free: half of the EHS's exchange space
    }
    FE_MARK(7);
  } else {
    __syncthreads();                                 // both spectra are in LDS (and the test wave's threshold)
    FE_MARK(7);                                      // barrier
    if (sig == 0) {
      bw_ref = top_bin(10. * xch[0], 921, false);
      if (lane == 0) xch[1] = (double)bw_ref;        // read by the test wave behind the next barrier
    }
  }

  // ---- error harmonic structure, part 1 (movs.c:1383-1391): d[k] = ln(Pw_test / Pw_ref), k < 512.
  // The test wave takes 5 of the 8 values per lane: its tail (noise spectrum) is the shorter one, but with 6 the
  // reference wave stood 1.3 k cycles at the barrier behind this loop.
  if constexpr (!kAdvanced) {
    double* dlog = sa;
#ifndef PEAQ_FE_RATIOS_REF
#define PEAQ_FE_RATIOS_REF 3                         // (2 / 3 / 4 / 1 of the 8: 28.81 / 28.95 / 28.90 / 28.69 M, profiles/r06_ab_basic.txt)
#endif
    constexpr int kRefRatios = PEAQ_FE_RATIOS_REF;
    static_assert(kRefRatios >= 1 && kRefRatios <= 4, "the reference wave takes 1..4 of the 8 ratios per lane, the test wave the rest");
#pragma unroll
    for (int j = 0; j < 8 - kRefRatios; ++j) {
      if (sig == 0 && j >= kRefRatios) break;
      const int k = (sig == 0 ? 0 : 64 * kRefRatios) + lane + 64 * j;
      const double fr = pw_ref[k], ft = pw_test[k];
      dlog[k] = (fr == 0. && ft == 0.) ? 0. : FE_LOG_NONNEG(ft / fr, ltab);   // +-inf when one side is digital silence
    }
  }
  if constexpr (!kAdvanced) {
    FE_MARK(8);                                      // log ratios
    __syncthreads();
    FE_MARK(9);                                      // barrier
  }
  if (!kAdvanced && sig == 1) {
    bw_ref = (int)xch[1];
    if (bw_ref > 346) bw_test = top_bin(3.16227766016838 * thr, bw_ref, true);
  }

  if (!kAdvanced && sig == 1) {
    // ---- noise spectrum for the NMR MOVs (movs.c:992-996): two bins per lane and step, in place
    // over this unit's weighted spectrum (nobody reads it any more); then the band grouping ------
    wave_lds_fence();
    {
      noise_spectrum_in_place(pw_ref, pw_test, lane);
      // the reference spectrum is dead now (read for the last time above): its first words are the band sums' zero words
      if (lane < group_zero_words(NB) / 2) *reinterpret_cast<double2*>(lds + kOffPw + 2 * lane) = make_double2(0., 0.);
    }
    wave_lds_fence();
    if (lane < (NB + 1) / 2) {                        // balanced assignment as above, straight to the record
      const int b1 = lane, b2 = NB - 1 - lane;
      double s1, s2;
      group_bands<NB>(edge1, edge2, pw_test, kOffPw - kUnitDoubles, s1, s2);
      rec[kRecNoise + b1] = s1;
      rec[kRecNoise + b2] = s2;
    } else if (lane < (NB + 1) / 2 + kBandStride - NB) {
      rec[kRecNoise + NB + lane - (NB + 1) / 2] = 0.;  // padding slots of the band vector
    }
    if (lane == 0) {
      rec[kRecBwRef] = (double)bw_ref;
      rec[kRecBwTest] = (double)bw_test;
    }
    FE_MARK(10);                                     // test wave: noise spectrum + grouping
  } else if (kAdvanced ? sig == 1 : sig == 0) {
    // (basic version: the reference wave; advanced version: the test wave, whose exchange buffers are its own scratch
    // area and the reference unit's spectrum)
    double* const sa = kAdvanced ? lds + kOffPw : lds + kOffScratch;
    // ---- error harmonic structure, part 2: c[l] = sum_{k<256} d[k] d[k+l], l < 256, the way the
    // reference does it (movs.c:1279-1315): with A = DFT_512(d[0..255], zero padded) and
    // B = DFT_512(d[0..511]) the sums are the inverse DFT of B conj(A).  Both transforms of real data
    // come out of ONE complex 512-point FFT of a + i b (8 points per lane, radix 8 x 8 x 8, real and
    // imaginary parts exchanged through the two scratch areas); the Hermitian product goes back
    // through a 256-point complex FFT (the inverse real transform by the half-size trick).
    // All five twiddle entries of the transforms below are requested here, ahead of the exchanges and fences their
    // uses sit behind (see frame_power_spectrum): register pressure is at its lowest on this wave, and the first of
    // them is needed a whole dft8 and an exchange from now.
    const cplx w64 = tw_lane(ct, 4, lane);                             // W_64^(lane & 7)
    const cplx w512 = tw_lane(ct, 3, lane);                            // W_512^lane
    cplx ft1[3];                                                     // fft256's passes 1..3, see there
#pragma unroll
    for (int i = 0; i < 3; ++i) ft1[i] = tw_lane(ct, 5 + i, lane);
    cplx u[8];
    double g[4], run_in;                             // window-energy increments of this lane's four lags
    {
      const double* d = kAdvanced ? sb : sa;           // (advanced version: written by the test wave, see above)
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const double v = d[lane + 64 * r];
        u[r] = {r < 4 ? v : 0., v};
      }
      // running window energy dk[l] = d0 + sum_{j<l} (d[j+256]^2 - d[j]^2)   (:1413-1418); d0 = c[0]
      // is added once it exists
      double tot = 0.;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int j = 4 * lane + t;
        const double hi = d[j + 256], lo = d[j];
        g[t] = hi * hi - lo * lo;
        tot += g[t];
      }
      run_in = wave_prefix_sum(tot, lane) - tot;     // exclusive scan over the lanes
    }
    wave_lds_fence();
    // exchange steps of the 512-point Stockham FFT; the index swizzles keep the 8-byte stores of a
    // 16-lane group on distinct banks (reads lane + 64 r are consecutive anyway)
    auto exchange8 = [&](auto wr, auto swz) {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int i = swz(wr(r));
        sa[i] = u[r].re;
        sb[i] = u[r].im;
      }
      wave_lds_fence();
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int i = swz(lane + 64 * r);
        u[r] = {sa[i], sb[i]};
      }
      wave_lds_fence();
    };
    auto twiddle8 = [&](cplx w1) {                   // u[r] *= w1^r, r = 1..7
      cplx w[8];
      w[1] = w1;
      w[2] = csqr(w[1]);
      w[4] = csqr(w[2]);
      w[3] = cmul(w[1], w[2]);
      w[5] = cmul(w[4], w[1]);
      w[6] = cmul(w[4], w[2]);
      w[7] = cmul(w[4], w[3]);
#pragma unroll
      for (int r = 1; r < 8; ++r) u[r] = cmul(u[r], w[r]);
    };
    dft8_imag_upper(u);                                              // sub-transform size 1 -> out[8 lane + r]; Re u[4..7] = 0
    exchange8([&](int r) { return 8 * lane + r; }, [](int i) { return i ^ ((i >> 4) & 7); });
    {
      const int k = lane & 7;
      twiddle8(w64);                                                 // W_64^(r k)
      dft8(u);                                                       // size 8 -> out[8 (lane - k) + k + 8 r]
      const int j = (lane - k) * 8 + k;
      exchange8([&](int r) { return j + 8 * r; }, [](int i) { return i ^ (((i >> 6) & 1) << 3); });
    }
    twiddle8(w512);                                                  // W_512^(r lane)
    dft8(u);                                                         // u[r] = (A + i B)[lane + 64 r]
    FE_MARK(10);                                     // reference wave: 512-point FFT
    // the window of part 3 (one of two tables, see there), requested two transforms ahead of its use
    const double* __restrict__ win = a.cfg.centre_ehs_window ? ct->ehs_window_centred : ct->ehs_window;
    double wv[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) wv[m] = win[lane + 64 * m];
    // Separate the two spectra and multiply, bins k = lane + 64 r < 256 (and 256 itself in lane 0);
    // the mirror bin 512 - k sits in lane 64 - lane, slot 7 - r (lane 0: own slot 8 - r).
    // 2A = Z[k] + conj Z[512-k], 2B = (Z[k] - conj Z[512-k]) / i, C = B conj(A); all factors of two
    // (and the reference's 1/512) are applied at the very end.
    const int partner = (64 - lane) & 63;
    cplx cc[4];
    double c256 = 0.;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      cplx zm = {__shfl(u[7 - r].re, partner, 64), __shfl(u[7 - r].im, partner, 64)};
      if (lane == 0) zm = u[(8 - r) & 7];
      const cplx a2 = {u[r].re + zm.re, u[r].im - zm.im};
      const cplx b2 = {u[r].im + zm.im, zm.re - u[r].re};
      cc[r] = {b2.re * a2.re + b2.im * a2.im, b2.im * a2.re - b2.re * a2.im};
    }
    if (lane == 0) c256 = (2. * u[4].re) * (2. * u[4].im);           // bin 256: A and B are real there
    // Inverse real transform by the half-size trick: with E = C[k] + conj C[256-k],
    // O = (C[k] - conj C[256-k]) W_512^-k the sequence Z[k] = E + i O (k < 256) is the DFT of
    // c[2m] + i c[2m+1].  C[256-k]: lane 64 - lane, slot 3 - r (lane 0: own slot 4 - r, C[256] for r = 0).
    // The inverse 256-point transform runs as a forward one on conj Z.
    cplx v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      cplx cm = {__shfl(cc[3 - r].re, partner, 64), __shfl(cc[3 - r].im, partner, 64)};
      if (lane == 0) cm = r == 0 ? cplx{c256, 0.} : cc[4 - r];
      const cplx e = {cc[r].re + cm.re, cc[r].im - cm.im};
      const cplx od = {cc[r].re - cm.re, cc[r].im + cm.im};
      // W_512^-k = conj(W_512^lane W_8^r)
      constexpr double c8 = 0.70710678118654752440;
      const cplx wkf = r == 0 ? w512 : r == 1 ? cmul(w512, {c8, -c8}) : r == 2 ? cmul_mi(w512) : cmul(w512, {-c8, -c8});
      const cplx o = cmul(od, {wkf.re, -wkf.im});
      v[r] = {e.re - o.im, -(e.im + o.re)};                          // conj(E + i O)
    }
    // twiddles of fft256's passes 1..3, W_{4p}^(r k): W_16^(lane & 3), W_64^(lane & 15), W_256^lane from the table,
    // squared and cubed -- ONE set for both runs of the transform (the fences between the runs keep the compiler
    // from seeing that the second run's loads and products repeat the first's)
    cplx ft2[3], ft3[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      ft2[i] = csqr(ft1[i]);
      ft3[i] = cmul(ft2[i], ft1[i]);
    }
    wave_lds_fence();
    double2* xb = reinterpret_cast<double2*>(sa);        // 256 complex
    auto fft256 = [&](cplx (&w)[4]) {
#pragma unroll
      for (int pass = 0; pass < 4; ++pass) {
        const int p = 1 << (2 * pass);
        const int k = lane & (p - 1);
        if (pass > 0) {
          if (pass < 3) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const double2 x = xb[lane + 64 * r];
              w[r] = {x.x, x.y};
            }
          }
          w[1] = cmul(w[1], ft1[pass - 1]);
          w[2] = cmul(w[2], ft2[pass - 1]);
          w[3] = cmul(w[3], ft3[pass - 1]);
        }
        dft4(w[0], w[1], w[2], w[3]);
        if (pass < 2) {
          const int j = (lane - k) * 4 + k;
          wave_lds_fence();
#pragma unroll
          for (int r = 0; r < 4; ++r) xb[j + r * p] = make_double2(w[r].re, w[r].im);
          wave_lds_fence();
        } else if (pass == 2) {
          // out[64 (lane >> 4) + (lane & 15) + 16 r], read back as in[lane + 64 r']: row and register trade
          // places, the column stays -- a row/register transpose on the permlane swaps, no LDS
          rows_transpose4(w[0].re, w[1].re, w[2].re, w[3].re);
          rows_transpose4(w[0].im, w[1].im, w[2].im, w[3].im);
        }
      }
    };
    fft256(v);
    // v[r] = conj of (256 x) (c[2m] + i c[2m+1]), m = lane + 64 r; lags below 256 <=> r < 2.
    // Scale: 1/4 (A, B) x 1/2 (E, O) x 1/256 (inverse transform) x ... the reference's 1/512 IS that
    // transform's normalisation -> 1/2048 in all.
    wave_lds_fence();
    {
      double2* cb = reinterpret_cast<double2*>(sb);      // c[l], l < 256, as 128 pairs
      constexpr double kScale = 1. / 2048.;
      cb[lane] = make_double2(v[0].re * kScale, -v[0].im * kScale);
      cb[lane + 64] = make_double2(v[1].re * kScale, -v[1].im * kScale);
      // ... and in the same round trip the running window energy WITHOUT its start value d0 = c[0] (which only
      // exists once the correlation has been read back): dk[l] - d0 = sum_{j<l} (d[j+256]^2 - d[j]^2), l = 4 lane + t
      double run = run_in;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        sa[4 * lane + t] = run;
        run += g[t];
      }
    }
    wave_lds_fence();
    FE_MARK(11);                                     // reference wave: product + inverse transform
    // ---- part 3 (movs.c:1393-1441): lane owns lags lane + 64 m ------------------------------------------
    double c[4], dk[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      c[m] = sb[lane + 64 * m];
      dk[m] = sa[lane + 64 * m];
    }
    const double d0 = read_lane<0>(c[0]);
    double cavg = 0.;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      // NaN when d0 = 0 (identical signals), as in the reference.  (d0 + dk: the reference runs dk = d0;
      // dk += d[i+256]^2 - d[i]^2 (movs.c:1413-1418) -- here the increments are summed first, as a prefix over the
      // lanes, and d0 is added last: the same sum in another order, last-bit differences where d0 dwarfs the
      // increments; DESIGN.md 4, "not bit-exact by design")
      c[m] *= rsqrt_pos(d0 * (d0 + dk[m]));
      cavg += c[m];
    }
    // the mean is removed before the window (the shipped EHS_SUBTRACT_DC_BEFORE_WINDOW, movs.c:1409-1421) or
    // as the DC bin after the transform (:1429-1433); the window is the one of :1366-1367 or the centred
    // one of :1363-1364 (settings.h:56, 66 as run-time switches)
    cavg = a.cfg.ehs_dc_before_window ? wave_sum(cavg) / 256. : 0.;
    cplx w4[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) w4[m] = {(c[m] - cavg) * wv[m], 0.};
    wave_lds_fence();
    fft256(w4);
    if (!a.cfg.ehs_dc_before_window && lane == 0) w4[0].re = 0.;   // bin 0 sits in slot 0 of lane 0
    // w4[r] = C[lane + 64 r]; EHS = highest |C|^2 that exceeds its left neighbour, bins 1..128
    const double s0 = w4[0].re * w4[0].re + w4[0].im * w4[0].im;
    const double s1 = w4[1].re * w4[1].re + w4[1].im * w4[1].im;
    const double s2 = w4[2].re * w4[2].re + w4[2].im * w4[2].im;
    const double s0_up = lane_below(s0), s1_up = lane_below(s1);
    const double s0_last = read_lane<63>(s0), s1_last = read_lane<63>(s1);
    const double prev0 = s0_up;                           // valid for lane >= 1
    const double prev1 = lane == 0 ? s0_last : s1_up;
    double best = 0.;
    if (lane >= 1 && s0 > prev0) best = s0;
    if (s1 > prev1 && s1 > best) best = s1;
    if (lane == 0 && s2 > s1_last && s2 > best) best = s2;
    best = wave_max(best);
    if (lane == 0) rec[kRecEhs] = best;
    FE_MARK(12);                                     // reference wave: normalise, window, 256-point FFT, peak
  }
  if (pf_keep == 123456.789f) rec[kRecScalars + 15] = 1.;   // never true (samples lie in [-1, 1]): keeps the prefetch alive
}

// ===========================================================================
// frontend_pair_kernel -- the same frame in ONE wave: a workgroup of 64 lanes carries the reference AND the test signal
// of its (pair, frame, channel).  What the two waves of frontend_kernel each evaluate for themselves -- the window, the
// twiddle powers, the item decoding, the table reads, the logarithm table -- exists once; nothing is handed between
// waves, so there is no barrier and no flag; and every dependent chain of one signal has the other signal's to issue
// beside it.  The price is registers: both spectra live side by side (<= 256 registers, two waves per SIMD).
// The arithmetic per signal is frontend_kernel's, instruction for instruction (the same device functions, applied to
// both signals from one place in the source, so that identical signals keep giving identical spectra).
//
// LDS, 18592 B per workgroup (<= 20 KiB: eight workgroups per CU):
//   [0, 776)      Pw of the reference  -- during the FFT, with the scratch area: the ONE 8.5 KiB exchange buffer both
//   [776, 1288)   scratch                 signals' first exchanges go through, one after the other
//   [1288, 2064)  Pw of the test signal, later the noise spectrum in place
//   [2064, 2324)  the logarithm table
// ===========================================================================
constexpr int kPairOffPwRef = 0;
constexpr int kPairOffScratch = kPwLen;              // 512 doubles
constexpr int kPairOffPwTest = kPairOffScratch + 512;
constexpr int kPairOffLogTab = kPairOffPwTest + kPwLen;
constexpr int kPairLdsDoubles = kPairOffLogTab + kLogTabDoubles;
static_assert(kPairLdsDoubles * sizeof(double) <= 20480, "one-wave front end: eight workgroups per CU in 160 KiB of LDS");
static_assert(kPairOffPwTest >= 1088 && kPairOffPwTest % 2 == 0, "the exchange buffer ends before the test spectrum; 16-byte alignment");

// frame_power_spectrum for both signals of a frame: every twiddle set is computed once and applied to both z arrays
template <typename F>
__device__ __forceinline__ void pair_power_spectra(cplx (&zr)[16], cplx (&zt)[16], double (&pr)[16], double (&pt)[16],
                                                   double* buf, double* pw_r, double* pw_t, int lane,
                                                   const CommonTables* __restrict__ ct, double level_factor,
                                                   F&& behind_pass2_twiddles) {
  const cplx w256 = tw_lane(ct, 2, lane);
  auto wr1 = [&](int r) { return 16 * lane + r; };
  auto rd1 = [&](int r) { return lane + 64 * r; };
  // pass 1; the test signal's butterflies have the reference's exchange to run beside
  dft16(zr);
  exchange16(zr, buf, wr1, rd1);
  dft16(zt);
  exchange16(zt, buf, wr1, rd1);
  // pass 2
  {
    cplx w[9];
    w[1] = w256;
    w[2] = csqr(w[1]);
    w[4] = csqr(w[2]);
    w[8] = csqr(w[4]);
    w[3] = cmul(w[1], w[2]);
    w[5] = cmul(w[4], w[1]);
    w[6] = cmul(w[4], w[2]);
    w[7] = cmul(w[4], w[3]);
#pragma unroll
    for (int r = 1; r < 8; ++r) {
      const cplx w8r = cmul(w[8], w[r]);
      zr[8 + r] = cmul(zr[8 + r], w8r);
      zt[8 + r] = cmul(zt[8 + r], w8r);
      zr[r] = cmul(zr[r], w[r]);
      zt[r] = cmul(zt[r], w[r]);
    }
    zr[8] = cmul(zr[8], w[8]);
    zt[8] = cmul(zt[8], w[8]);
  }
  behind_pass2_twiddles();                           // (every global load requested before w256 has arrived by now)
  auto pass2_tail = [&](cplx (&z)[16]) {
    dft16(z);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      rows_transpose4(z[4 * g].re, z[4 * g + 1].re, z[4 * g + 2].re, z[4 * g + 3].re);
      rows_transpose4(z[4 * g].im, z[4 * g + 1].im, z[4 * g + 2].im, z[4 * g + 3].im);
    }
#pragma unroll
    for (int a2 = 0; a2 < 4; ++a2)
#pragma unroll
      for (int g = a2 + 1; g < 4; ++g) {
        const cplx t = z[4 * a2 + g];
        z[4 * a2 + g] = z[4 * g + a2];
        z[4 * g + a2] = t;
      }
  };
  pass2_tail(zr);
  pass2_tail(zt);
  const cplx wl = tw_lane(ct, 0, lane);
  // (the ear weights of the first kEwAhead steps of the split only: with both z arrays live there is no room for all
  // eight over pass 3 -- step q of the split requests those of step q + kEwAhead)
  constexpr int kEwAhead = 2;
  double2 ew[8];
#pragma unroll
  for (int q = 0; q < kEwAhead; ++q) ew[q] = *reinterpret_cast<const double2*>(ct->ear_w2_pair[q][lane]);
  {
    constexpr double c1 = 0.92387953251128673848, s1 = 0.38268343236508977173, c2 = 0.70710678118654752440;
    const cplx wb = tw_lane(ct, 1, lane);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const cplx w1 = m == 0 ? wb : m == 1 ? cmul(wb, {c1, -s1}) : m == 2 ? cmul(wb, {c2, -c2}) : cmul(wb, {s1, -c1});
      const cplx w2 = csqr(w1), w3 = cmul(w2, w1);
      auto pass3 = [&](cplx (&z)[16]) {
        z[m + 4] = cmul(z[m + 4], w1);
        z[m + 8] = cmul(z[m + 8], w2);
        z[m + 12] = cmul(z[m + 12], w3);
        dft4(z[m], z[m + 4], z[m + 8], z[m + 12]);
      };
      pass3(zr);
      pass3(zt);
    }
  }
  wave_lds_fence();                                  // the exchange buffer is about to become the two Pw
  const int partner = (64 - lane) & 63;
  // (wave-uniform: held in scalar registers, the split has no vector register to spare)
  const double lf4v = 0.25 * level_factor;
  const double lf4 = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(lf4v)),
                                      __builtin_amdgcn_readfirstlane(__double2loint(lf4v)));
  // Lane 0's mirror bins are its OWN slots 16 - q, one up from the slot 15 - q every other lane's partner holds.  Taken
  // inside the loop, as frontend_kernel does, that keeps slot 16 - q of BOTH signals live a step longer: eight registers
  // too many here.  So lane 0 moves its upper slots one down beforehand (the same selects, in another place; slot j
  // takes from j + 1, which is still untouched) and the loop exchanges slot 15 - q for every lane alike.  Bin 512, which
  // lane 0 forms from its slot 8, first.
  double p512_r, p512_t;
  auto lane0_slots = [&](cplx (&z)[16], double& p512) {
    p512 = (z[8].re * z[8].re + z[8].im * z[8].im) * level_factor;
#pragma unroll
    for (int j = 8; j < 16; ++j)
      if (lane == 0) z[j] = z[(j + 1) & 15];
  };
  lane0_slots(zr, p512_r);
  lane0_slots(zt, p512_t);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    if (q + kEwAhead < 8) ew[q + kEwAhead] = *reinterpret_cast<const double2*>(ct->ear_w2_pair[q + kEwAhead][lane]);
    const int k = lane + 64 * q;
    const cplx wq = {kW32re[q], kW32im[q]};
    const cplx wk = q == 0 ? wl : cmul(wl, wq);
    auto split = [&](cplx (&z)[16], double (&p)[16], double* pw, double p512) {
      const cplx zm = {__shfl(z[15 - q].re, partner, 64), __shfl(z[15 - q].im, partner, 64)};
      const cplx e2 = {z[q].re + zm.re, z[q].im - zm.im};
      const cplx o2 = {z[q].im + zm.im, zm.re - z[q].re};
      const cplx t = cmul(wk, o2);
      const cplx xp = cadd(e2, t), xm = csub(e2, t);
      p[q] = (xp.re * xp.re + xp.im * xp.im) * lf4;
      double pm = (xm.re * xm.re + xm.im * xm.im) * lf4;
      int km = 1024 - k;
      if (q == 0 && lane == 0) {
        pm = p512;
        km = 512;
      }
      p[8 + q] = pm;
      pw[k] = p[q] * ew[q].x;
      if (km < kPwLen) pw[km] = pm * ew[q].y;
    };
    split(zr, pr, pw_r, p512_r);
    split(zt, pt, pw_t, p512_t);
  }
  wave_lds_fence();
}

// the bandwidth search of frontend_kernel (movs.c:776-809) on a spectrum held as frame_power_spectrum leaves it
__device__ __forceinline__ int pair_top_bin(const double (&ps)[16], double level, int limit, bool or_equal) {
  bool hit512 = false;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    unsigned long long m = __ballot(or_equal ? ps[8 + q] >= level : ps[8 + q] > level);
    if (q == 0) {
      hit512 = (m & 1ull) && 512 < limit;
      m &= ~1ull;
    }
    const int lo = 1024 - 64 * q - limit + 1;
    m &= lo >= 64 ? 0ull : lo <= 0 ? ~0ull : ~0ull << lo;
    if (m) return 1024 - 64 * q - __builtin_ctzll(m) + 1;
  }
  if (hit512) return 513;
#pragma unroll
  for (int q = 7; q >= 0; --q) {
    unsigned long long m = __ballot(or_equal ? ps[q] >= level : ps[q] > level);
    const int nl = limit - 64 * q;
    m &= nl >= 64 ? ~0ull : nl <= 0 ? 0ull : (1ull << nl) - 1ull;
    if (m) return 64 * q + 64 - __builtin_clzll(m);
  }
  return 0;
}

// Error harmonic structure from the log ratios d[0..511] (movs.c:1279-1315, 1393-1441): frontend_kernel's parts 2 and 3,
// exchanging through sa and sb (512 doubles each; d may be sb).  Returns the EHS value (every lane).
__device__ __forceinline__ double pair_ehs(const double* d, double* sa, double* sb, int lane,
                                           const CommonTables* __restrict__ ct, const Settings& cfg) {
  const cplx w64 = tw_lane(ct, 4, lane);
  const cplx w512 = tw_lane(ct, 3, lane);
  cplx ft1[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) ft1[i] = tw_lane(ct, 5 + i, lane);
  cplx u[8];
  double g[4], run_in;
  {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const double v = d[lane + 64 * r];
      u[r] = {r < 4 ? v : 0., v};
    }
    double tot = 0.;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int j = 4 * lane + t;
      const double hi = d[j + 256], lo = d[j];
      g[t] = hi * hi - lo * lo;
      tot += g[t];
    }
    run_in = wave_prefix_sum(tot, lane) - tot;
  }
  wave_lds_fence();
  auto exchange8 = [&](auto wr, auto swz) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int i = swz(wr(r));
      sa[i] = u[r].re;
      sb[i] = u[r].im;
    }
    wave_lds_fence();
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int i = swz(lane + 64 * r);
      u[r] = {sa[i], sb[i]};
    }
    wave_lds_fence();
  };
  auto twiddle8 = [&](cplx w1) {
    cplx w[8];
    w[1] = w1;
    w[2] = csqr(w[1]);
    w[4] = csqr(w[2]);
    w[3] = cmul(w[1], w[2]);
    w[5] = cmul(w[4], w[1]);
    w[6] = cmul(w[4], w[2]);
    w[7] = cmul(w[4], w[3]);
#pragma unroll
    for (int r = 1; r < 8; ++r) u[r] = cmul(u[r], w[r]);
  };
  dft8_imag_upper(u);
  exchange8([&](int r) { return 8 * lane + r; }, [](int i) { return i ^ ((i >> 4) & 7); });
  {
    const int k = lane & 7;
    twiddle8(w64);
    dft8(u);
    const int j = (lane - k) * 8 + k;
    exchange8([&](int r) { return j + 8 * r; }, [](int i) { return i ^ (((i >> 6) & 1) << 3); });
  }
  twiddle8(w512);
  dft8(u);
  const double* __restrict__ win = cfg.centre_ehs_window ? ct->ehs_window_centred : ct->ehs_window;
  double wv[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) wv[m] = win[lane + 64 * m];
  const int partner = (64 - lane) & 63;
  cplx cc[4];
  double c256 = 0.;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    cplx zm = {__shfl(u[7 - r].re, partner, 64), __shfl(u[7 - r].im, partner, 64)};
    if (lane == 0) zm = u[(8 - r) & 7];
    const cplx a2 = {u[r].re + zm.re, u[r].im - zm.im};
    const cplx b2 = {u[r].im + zm.im, zm.re - u[r].re};
    cc[r] = {b2.re * a2.re + b2.im * a2.im, b2.im * a2.re - b2.re * a2.im};
  }
  if (lane == 0) c256 = (2. * u[4].re) * (2. * u[4].im);
  cplx v[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    cplx cm = {__shfl(cc[3 - r].re, partner, 64), __shfl(cc[3 - r].im, partner, 64)};
    if (lane == 0) cm = r == 0 ? cplx{c256, 0.} : cc[4 - r];
    const cplx e = {cc[r].re + cm.re, cc[r].im - cm.im};
    const cplx od = {cc[r].re - cm.re, cc[r].im + cm.im};
    constexpr double c8 = 0.70710678118654752440;
    const cplx wkf = r == 0 ? w512 : r == 1 ? cmul(w512, {c8, -c8}) : r == 2 ? cmul_mi(w512) : cmul(w512, {-c8, -c8});
    const cplx o = cmul(od, {wkf.re, -wkf.im});
    v[r] = {e.re - o.im, -(e.im + o.re)};
  }
  cplx ft2[3], ft3[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    ft2[i] = csqr(ft1[i]);
    ft3[i] = cmul(ft2[i], ft1[i]);
  }
  wave_lds_fence();
  double2* xb = reinterpret_cast<double2*>(sa);
  auto fft256 = [&](cplx (&w)[4]) {
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
      const int p = 1 << (2 * pass);
      const int k = lane & (p - 1);
      if (pass > 0) {
        if (pass < 3) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double2 x = xb[lane + 64 * r];
            w[r] = {x.x, x.y};
          }
        }
        w[1] = cmul(w[1], ft1[pass - 1]);
        w[2] = cmul(w[2], ft2[pass - 1]);
        w[3] = cmul(w[3], ft3[pass - 1]);
      }
      dft4(w[0], w[1], w[2], w[3]);
      if (pass < 2) {
        const int j = (lane - k) * 4 + k;
        wave_lds_fence();
#pragma unroll
        for (int r = 0; r < 4; ++r) xb[j + r * p] = make_double2(w[r].re, w[r].im);
        wave_lds_fence();
      } else if (pass == 2) {
        rows_transpose4(w[0].re, w[1].re, w[2].re, w[3].re);
        rows_transpose4(w[0].im, w[1].im, w[2].im, w[3].im);
      }
    }
  };
  fft256(v);
  wave_lds_fence();
  {
    double2* cb = reinterpret_cast<double2*>(sb);
    constexpr double kScale = 1. / 2048.;
    cb[lane] = make_double2(v[0].re * kScale, -v[0].im * kScale);
    cb[lane + 64] = make_double2(v[1].re * kScale, -v[1].im * kScale);
    double run = run_in;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      sa[4 * lane + t] = run;
      run += g[t];
    }
  }
  wave_lds_fence();
  double c[4], dk[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    c[m] = sb[lane + 64 * m];
    dk[m] = sa[lane + 64 * m];
  }
  const double d0 = read_lane<0>(c[0]);
  double cavg = 0.;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    c[m] *= rsqrt_pos(d0 * (d0 + dk[m]));
    cavg += c[m];
  }
  cavg = cfg.ehs_dc_before_window ? wave_sum(cavg) / 256. : 0.;
  cplx w4[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) w4[m] = {(c[m] - cavg) * wv[m], 0.};
  wave_lds_fence();
  fft256(w4);
  if (!cfg.ehs_dc_before_window && lane == 0) w4[0].re = 0.;
  const double s0 = w4[0].re * w4[0].re + w4[0].im * w4[0].im;
  const double s1 = w4[1].re * w4[1].re + w4[1].im * w4[1].im;
  const double s2 = w4[2].re * w4[2].re + w4[2].im * w4[2].im;
  const double s0_up = lane_below(s0), s1_up = lane_below(s1);
  const double s0_last = read_lane<63>(s0), s1_last = read_lane<63>(s1);
  const double prev0 = s0_up;
  const double prev1 = lane == 0 ? s0_last : s1_up;
  double best = 0.;
  if (lane >= 1 && s0 > prev0) best = s0;
  if (s1 > prev1 && s1 > best) best = s1;
  if (lane == 0 && s2 > s1_last && s2 > best) best = s2;
  return wave_max(best);
}

template <int NB>
__global__ __launch_bounds__(64, 2) void frontend_pair_kernel(FrontendArgs a) {
  static_assert(NB == 109, "the one-wave front end is the basic version's (the advanced one has no band phase for the test signal)");
  extern __shared__ double lds[];
  __builtin_amdgcn_s_setprio(3);
  asm volatile("" ::"s"(a.ref), "s"(a.test), "s"(a.pair_stride), "s"(a.n_ref), "s"(a.n_test), "s"(a.n_uniform_ref),
               "s"(a.n_uniform_test), "s"(a.n_frames), "s"(a.n_frames_uniform), "s"(a.frame_origin), "s"(a.off_ref),
               "s"(a.off_test), "s"(a.channels), "s"(a.frame0), "s"(a.frames_per_launch), "s"(a.fpl_magic), "s"(a.common),
               "s"(a.records), "s"(a.pair_frame0), "s"(gridDim.x));
  const int lane = threadIdx.x;
  [[maybe_unused]] constexpr int sig = 0;            // (FE_MARK: one role)
#ifdef PEAQ_FE_PROFILE
  unsigned long long prof_t_ = __builtin_readcyclecounter();
  if (a.prof && lane == 0 && (blockIdx.x & 127) == 5) atomicAdd(a.prof + 32, 1ull);
#endif
  double* pw_ref = lds + kPairOffPwRef;
  double* pw_test = lds + kPairOffPwTest;
  double* scratch = lds + kPairOffScratch;
  double* ltab = lds + kPairOffLogTab;
  const CommonTables* __restrict__ ct = a.common;
  const BandTables* __restrict__ bt = a.bands;

  // ---- which (pair, frame, channel): as frontend_kernel ---------------------------------------------------------
  auto decode = [&](unsigned it, unsigned& pair_, unsigned& fl_) {
    const unsigned t = it >> (a.channels - 1);
    pair_ = a.frames_per_launch == 1 ? t : __umulhi(t, a.fpl_magic);
    fl_ = t - pair_ * a.frames_per_launch;
    return (int)(it & (unsigned)(a.channels - 1));
  };
  const unsigned item = xcd_remap(blockIdx.x, gridDim.x);
  unsigned pair, fl;
  const int chan = decode(item, pair, fl);
  FE_MARK(15);
  const unsigned n_ref = a.n_ref ? a.n_ref[pair] : a.n_uniform_ref;
  const unsigned n_test = a.n_test ? a.n_test[pair] : a.n_uniform_test;
  unsigned frame, frame_origin;
  if (a.pair_frame0) {
    if (fl >= a.pair_nframes[pair]) return;
    frame_origin = a.pair_frame0[pair];
    frame = frame_origin + fl;
  } else {
    frame = a.frame0 + fl;
    frame_origin = a.frame_origin;
    const unsigned n_frames = a.n_frames ? a.n_frames[pair] : a.n_frames_uniform;
    if (frame >= n_frames) return;
  }
  const size_t pair_off = (size_t)pair * a.pair_stride * a.channels;
  FrameSrc src_ref, src_test;
  {
    const long long s0 = (long long)(frame - frame_origin) * kHop;
    src_ref.set(a.ref + pair_off, s0 + a.off_ref, (long long)n_ref, a.channels, chan);
    src_test.set(a.test + pair_off, s0 + a.off_test, (long long)n_test, a.channels, chan);
  }
  double* __restrict__ rec =
      a.records + ((size_t)(pair * a.frames_per_launch + fl) * a.channels + chan) * kRecDoubles;
  // ---- load + window: one lane offset, two buffer resources; the window values once per row -----------------------
  constexpr double kHannA = 0.81649658092772603273;
  constexpr double kHannC[16] = {1.0, 0.923806101034885660186, 0.7068354246185547448714, 0.3821516543455241229047,
                                 -0.0007673650086148258012924, -0.3835694472988822502431, -0.7079202261619581075015,
                                 -0.9243926006499437062869, -0.9999988223018871071366, -0.9232174254904238786877,
                                 -0.7057489581976599840459, -0.3807329612736016723471, 0.002302093218395832312485,
                                 0.3849863367942118830771, 0.7090033602727326108775, 0.9249769229541590372578};
  constexpr double kHannS[16] = {0.0, 0.382860663545790020567, 0.7073780336597309217442, 0.92409962292005024589,
                                 0.99999970557542843387, 0.923512035167290059731, 0.7062923993579444458354,
                                 0.3814424201155840173045, -0.001534729565367423810065, -0.3842780051874341062575,
                                 -0.7084620018059667117941, -0.924685034052046356158, -0.9999973501798961346679,
                                 -0.9229222721777677728372, -0.705205101457706221079, -0.3800232782373413192215};
  const double2 hl0 = *reinterpret_cast<const double2*>(&ct->hann_lane[lane][0]);
  const double2 hl1 = *reinterpret_cast<const double2*>(&ct->hann_lane[lane][2]);
  FE_MARK(13);
  cplx zr[16], zt[16];
  float amax = 0.f;
  double energy_r = 0., energy_t = 0., hop_r = 0., hop_t = 0.;   // hop: sum ref^2 / sum (ref - test)^2
  {
    const int voff = src_ref.lane_offset(lane);      // same channel count and channel: one lane offset for both
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = lane + 64 * r;
      float x0, x1, y0, y1;
      src_ref.load2(r, voff, x0, x1);
      src_test.load2(r, voff, y0, y1);
      const double w0 = fma(hl0.y, kHannS[r], fma(-hl0.x, kHannC[r], kHannA));
      const double w1 = fma(hl1.y, kHannS[r], fma(-hl1.x, kHannC[r], kHannA));
      zr[r] = {w0 * (double)x0, w1 * (double)x1};
      zt[r] = {w0 * (double)y0, w1 * (double)y1};
      if (r >= 8) {
        energy_r += (double)(x0 * x0);
        energy_r += (double)(x1 * x1);
        energy_t += (double)(y0 * y0);
        energy_t += (double)(y1 * y1);
      } else {
        hop_r += (double)(x0 * x0);
        hop_r += (double)(x1 * x1);
        hop_t += (double)((x0 - y0) * (x0 - y0));
        hop_t += (double)((x1 - y1) * (x1 - y1));
      }
      amax = fmaxf(amax, n == 0 ? fabsf(x1) : fmaxf(fabsf(x0), fabsf(x1)));
    }
  }
  // ---- L2 prefetch: this wave touches BOTH signals' next frame for the item kPrefetchItems further on ---------------
  float pf_keep = 0.f;
  if (chan == 0 && !a.pair_frame0) {
    const unsigned it2 = item + kPrefetchItems;
    if (it2 < gridDim.x) {
      unsigned pair2, fl2;
      decode(it2, pair2, fl2);
      const long long s2 = (long long)(a.frame0 + fl2 - a.frame_origin) * kHop + (fl2 == 0 ? 0 : kHop);
      const size_t off2 = (size_t)pair2 * a.pair_stride * a.channels;
      FrameSrc pfr, pft;
      pfr.set(a.ref + off2, s2 + a.off_ref, (long long)(a.n_ref ? a.n_ref[pair2] : a.n_uniform_ref), a.channels, 0);
      pft.set(a.test + off2, s2 + a.off_test, (long long)(a.n_test ? a.n_test[pair2] : a.n_uniform_test), a.channels, 0);
      pf_keep = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(pfr.rs, lane * 128, 0, 0));
      pf_keep += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(pft.rs, lane * 128, 0, 0));
      if (fl2 == 0 && a.channels == 2) {
        pf_keep += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(pfr.rs, (64 + lane) * 128, 0, 0));
        pf_keep += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(pft.rs, (64 + lane) * 128, 0, 0));
      }
    }
  }
  __builtin_amdgcn_s_setprio(0);
#ifdef PEAQ_FE_PROFILE
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  FE_MARK(14);
  // (the reduction tree of wave_sum2, twice over: the sums are frontend_kernel's bit for bit)
  wave_sum4(hop_r, energy_r, hop_t, energy_t, hop_r, energy_r, hop_t, energy_t);
  if (lane == 0) {
    rec[kRecSigE] = hop_r;
    rec[kRecNoiseE] = hop_t;
  }
  const int eflag_r = energy_r >= 8000. / (32768. * 32768.), eflag_t = energy_t >= 8000. / (32768. * 32768.);
  int above = 0;
  if (__any((double)amax >= 200. / 32768 + 1e-6)) {
    above = 1;
  } else {
    float* ax = reinterpret_cast<float*>(lds);       // 8 KiB of the still unused exchange buffer
    int lane_q = lane;
    asm volatile("" : "+v"(lane_q));
    const int voff_q = src_ref.lane_offset(lane_q);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = lane_q + 64 * r;
      float x0, x1;
      src_ref.load2(r, voff_q, x0, x1);
      reinterpret_cast<float2*>(ax)[n] = make_float2(fabsf(x0), fabsf(x1));
    }
    wave_lds_fence();
    above = boundary_detect(ax, kFrame, lane);
    wave_lds_fence();
  }
  if (lane == 0) {
    rec[kRecFlagsRef] = (double)(above | (eflag_r << 1));
    rec[kRecFlagsTest] = (double)(eflag_t << 1);
  }
  FE_MARK(0);
  constexpr int kGroupLanes = (NB + 1) / 2;
  int bw_ref = 0, bw_test = 0;
  {
    double pr[16], pt[16];                           // the unweighted power spectra: they die with the bandwidths
    double2 lt0, lt1, lt2;
    // (the prefetched words end their life where the transform has waited for a younger load anyway -- loads return in
    // order --: one register less over the split, where there is none to spare)
    pair_power_spectra(zr, zt, pr, pt, lds, pw_ref, pw_test, lane, ct, a.level_factor,
                       [&] { asm volatile("" ::"v"(pf_keep)); });
    // the logarithm table, requested only now (no register is free for it over the transform; the barrier keeps the
    // scheduler from lifting the loads back up) and stored behind the bandwidth searches, which cover its way
    __builtin_amdgcn_sched_barrier(0);
    lt0 = *reinterpret_cast<const double2*>(ct->log_tab[lane]);
    lt1 = *reinterpret_cast<const double2*>(ct->log_tab[64 + lane]);
    lt2 = *reinterpret_cast<const double2*>(ct->log_tab[128]);
    FE_MARK(1);
    // ---- bandwidths (movs.c:776-809), straight from the registers: zero threshold = max over bins 921..1023 of the
    // test spectrum, then the two searches
    double thr = 0.;
    if (lane >= 1) thr = pt[8];
    if (lane <= 39) thr = fmax(thr, pt[9]);
    thr = wave_max(thr);
    bw_ref = pair_top_bin(pr, 10. * thr, 921, false);
    if (bw_ref > 346) bw_test = pair_top_bin(pt, 3.16227766016838 * thr, bw_ref, true);
    if (lane == 0) {
      rec[kRecBwRef] = (double)bw_ref;
      rec[kRecBwTest] = (double)bw_test;
    }
    reinterpret_cast<double2*>(ltab)[lane] = lt0;
    reinterpret_cast<double2*>(ltab)[64 + lane] = lt1;
    if (lane == 0) reinterpret_cast<double2*>(ltab)[128] = lt2;
  }
  const int gb1 = lane < kGroupLanes ? lane : 0, gb2 = lane < kGroupLanes ? NB - 1 - lane : 0;
  const BandEdge edge1 = load_band_edge(bt, gb1), edge2 = load_band_edge(bt, gb2);
  FE_MARK(2);
  // ---- critical bands, internal noise, spreading: both signals step by step ------------------------------------------
  {
    constexpr int kZeroAt = 400;                     // zero words of the band sums' idle slots: scratch[400 ..]
    static_assert(kZeroAt + group_zero_words(NB) <= 512 && group_zero_words(NB) / 2 <= 64, "band sums: the zero words lie in the scratch area");
    if (lane < group_zero_words(NB) / 2) *reinterpret_cast<double2*>(scratch + kZeroAt + 2 * lane) = make_double2(0., 0.);
    wave_lds_fence();
    double* const ppx[2] = {scratch + 256, scratch};   // [128] each: band sums, then the helper stream's way home
    const double* const pw[2] = {pw_ref, pw_test};
    const int b0 = 2 * lane;
    double c_noise[2], c_lnauc[2], c_gil[2];
    const double c_dz02 = bt->dz02, c_ale = bt->aLe;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const int b = b0 + s2 < NB ? b0 + s2 : 0;
      c_noise[s2] = bt->internal_noise[b];
      c_lnauc[s2] = bt->ln_aUC[b];
      c_gil[s2] = bt->gIL[b];
    }
    if (lane < kGroupLanes) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        double s1, s2;
        group_bands<NB>(edge1, edge2, pw[g], (int)(scratch + kZeroAt - pw[g]), s1, s2);
        ppx[g][lane] = s1;
        ppx[g][NB - 1 - lane] = s2;
      }
    }
    wave_lds_fence();
    FE_MARK(3);
    constexpr int kLanes = spread_lanes(NB);
    constexpr int kHelper = spread_helper_steps(NB), kFirst = spread_k0(NB), kBoundary = spread_boundary(NB);
    constexpr int kExpUpper = spread_exp_upper(NB, 0), kExpHelper = spread_exp_helper(NB);
    static_assert(kHelper > 0, "upward spreading: the two-stream schedule");
    double ene[2][2], ae[2][2], far[2][2], back2[2][2], far_copy[2][2], upper[2][2];   // [signal][band of the lane]
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int b = b0 + s;
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        if (b < NB) {
          const double pp = ppx[g][b] + c_noise[s];
          const double ln_pp = FE_LOG(pp, ltab);
          const double ln_a = c_lnauc[s] + c_dz02 * ln_pp;
          const double t = exp_fast(0.2 * ln_a), t2 = t * t;
          const double a_uce = t2 * t2 * t;
          const double g_iu = div_fast(1. - exp_fast((double)(NB - b) * ln_a), 1. - a_uce);
          ae[g][s] = t2;
          ene[g][s] = exp_fast(0.4 * (ln_pp - FE_LOG(c_gil[s] + g_iu - 1., ltab)));
          upper[g][s] = ene[g][s] * pow_const(t2, kExpUpper - s);
          const double ph = pow_const(t2, kExpHelper);
          far[g][s] = upper[g][s] * ph;
          far_copy[g][s] = far[g][s] * ph;
          const double t4 = t2 * t2;
          back2[g][s] = t4 > 1e-290 ? div_fast(1., t4) : 0.;
        } else {
          ae[g][s] = 0.;
          ene[g][s] = 0.;
          far[g][s] = 0.;
          far_copy[g][s] = 0.;
          upper[g][s] = 0.;
          back2[g][s] = 0.;
        }
      }
    }
    FE_MARK(4);
    // upward spreading (peaq_spread_sched.h, per signal): four accumulators and four walking terms per step
    double up0[2] = {0., 0.}, up1[2] = {0., 0.};
    {
      double u[2], v[2], wa0[2], wa1[2], wb0[2], wb1[2];
      double2 home[2];
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        u[g] = lower_halves(far[g][0], far_copy[g][0]);
        v[g] = lower_halves(far[g][1], far_copy[g][1]);
        wa0[g] = lower_halves(ae[g][0], ae[g][0]);
        wa1[g] = lower_halves(ae[g][1], ae[g][1]);
        wb0[g] = lower_halves(back2[g][0], back2[g][0]);
        wb1[g] = lower_halves(back2[g][1], back2[g][1]);
      }
      const int act = lane < kSpreadHelperBase ? kLanes - lane : kFirst - (lane - kSpreadHelperBase);   // spread_act
#pragma unroll 5
      for (int k = kFirst; k >= kBoundary; --k) {
        if (k <= act) {
          asm volatile("");                          // keeps this an EXEC mask (see frontend_kernel)
#pragma unroll
          for (int g = 0; g < 2; ++g) {
            up0[g] += u[g];
            up0[g] += v[g];
            up1[g] = fma(wa0[g], u[g], up1[g]);
            up1[g] = fma(wa1[g], v[g], up1[g]);
          }
        }
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          up0[g] = lane_below(up0[g]);
          up1[g] = lane_below(up1[g]);
          u[g] *= wb0[g];
          v[g] *= wb1[g];
        }
      }
      const bool lower = lane < kSpreadHelperBase;
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        double2* hx = reinterpret_cast<double2*>(ppx[g]);
        hx[(lane + spread_home_shift(NB) + kSpreadWave) & (kSpreadWave - 1)] = lower ? make_double2(0., 0.) : make_double2(up0[g], up1[g]);
      }
      wave_lds_fence();
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        home[g] = reinterpret_cast<const double2*>(ppx[g])[lane];
        up0[g] = lower ? up0[g] : 0.;
        up1[g] = lower ? up1[g] : 0.;
        u[g] = lower ? u[g] : upper[g][0];
        v[g] = lower ? v[g] : upper[g][1];
      }
#pragma unroll 8
      for (int k = kBoundary - 1; k >= 1; --k) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          up0[g] += u[g];
          up0[g] += v[g];
          up1[g] = fma(ae[g][0], u[g], up1[g]);
          up1[g] = fma(ae[g][1], v[g], up1[g]);
          up0[g] = lane_below(up0[g]);
          up1[g] = lane_below(up1[g]);
          u[g] *= back2[g][0];
          v[g] *= back2[g][1];
        }
      }
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        up0[g] += home[g].x;
        up1[g] += home[g].y;
        up1[g] = fma(ae[g][0], ene[g][0], up1[g]);
      }
    }
    FE_MARK(5);
    // downward spreading, Kabal (28), and the roots (25)
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const double al = c_ale;
      const double v = wave_suffix_geometric(ene[g][0] + al * ene[g][1], al * al, lane);
      const double nxt = lane_above(v);
      const double dn0 = v, dn1 = ene[g][1] + al * nxt;
      double root[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const double e2 = (s ? dn1 : dn0) + (s ? up1[g] : up0[g]);
        root[s] = b0 + s < NB ? sqrt_pos(sqrt_pos(e2)) : 0.;
      }
      if (b0 < kBandStride)
        *reinterpret_cast<double2*>(rec + (g ? kRecRootTest : kRecRootRef) + b0) = make_double2(root[0], root[1]);
    }
  }
  FE_MARK(6);
  // ---- error harmonic structure, part 1 (movs.c:1383-1391): d[k] = ln(Pw_test / Pw_ref), k < 512, all eight per lane,
  // into the scratch area (whose band-sum words have been read for the last time)
  wave_lds_fence();
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = lane + 64 * j;
    const double fr = pw_ref[k], ft = pw_test[k];
    scratch[k] = (fr == 0. && ft == 0.) ? 0. : FE_LOG_NONNEG(ft / fr, ltab);   // +-inf when one side is digital silence
  }
  FE_MARK(8);
  // ---- noise spectrum for the NMR MOVs (movs.c:992-996) in place over the test spectrum, and its band sums; the
  // reference spectrum is dead behind it: its first words become the band sums' zero words, then all of it the EHS's
  // exchange space
  wave_lds_fence();
  noise_spectrum_in_place(pw_ref, pw_test, lane);
  if (lane < group_zero_words(NB) / 2) *reinterpret_cast<double2*>(pw_ref + 2 * lane) = make_double2(0., 0.);
  wave_lds_fence();
  if (lane < kGroupLanes) {
    double s1, s2;
    group_bands<NB>(edge1, edge2, pw_test, kPairOffPwRef - kPairOffPwTest, s1, s2);
    rec[kRecNoise + lane] = s1;
    rec[kRecNoise + NB - 1 - lane] = s2;
  } else if (lane < kGroupLanes + kBandStride - NB) {
    rec[kRecNoise + NB + lane - kGroupLanes] = 0.;   // padding slots of the band vector
  }
  wave_lds_fence();
  FE_MARK(10);
  const double ehs = pair_ehs(scratch, pw_ref, scratch, lane, ct, a.cfg);
  if (lane == 0) rec[kRecEhs] = ehs;
  FE_MARK(12);
}

// Which front end the basic version launches -- batch, sessions, broker and stage entries alike, so that a stream read
// through a session and the same samples in a batch stay the same bit for bit (tests/test_gpu_backend_record_fetch.py,
// the trajectory and broker tests hold them to that; the two kernels agree to a few ulp, not to the bit): the one-wave
// kernel, or with PEAQ_AMD_FE=two_waves (development: A/B runs and the comparison tests, no variant build)
// frontend_kernel<109>.  The environment is read once; select_frontend() overrides it within a process.
static int g_fe_override = -1;                       // -1: the environment decides; 0: one wave; 1: two waves
int select_frontend(int two_waves) {
  const int before = g_fe_override;
  g_fe_override = two_waves < 0 ? -1 : two_waves ? 1 : 0;
  return before;
}
static bool frontend_two_waves() {
  static const bool env = [] { const char* e = std::getenv("PEAQ_AMD_FE"); return e && std::strcmp(e, "two_waves") == 0; }();
  return g_fe_override < 0 ? env : g_fe_override != 0;
}

static hipError_t launch_frontend_as(bool one_wave, int bands, const FrontendArgs& a, unsigned n_pairs, hipStream_t stream) {
  const unsigned grid = n_pairs * a.frames_per_launch * a.channels;
  if (grid == 0) return hipSuccess;
  if ((unsigned long long)n_pairs * a.frames_per_launch * a.channels >= (1ull << 26)) return hipErrorInvalidValue;
  FrontendArgs args = a;
  args.fpl_magic = (unsigned)(((1ull << 32) + a.frames_per_launch - 1) / a.frames_per_launch);
  if (a.frames_per_launch > 1) {
    // mulhi(t, magic) == t / d for every t of this grid?  (magic d - 2^32) t < 2^32 decides
    const unsigned long long err = (unsigned long long)args.fpl_magic * a.frames_per_launch - (1ull << 32);
    const unsigned long long t_max = (unsigned long long)n_pairs * a.frames_per_launch - 1;
    if (err && t_max >= ((1ull << 32) + err - 1) / err) return hipErrorInvalidValue;
  }
#ifndef PEAQ_FE_LDS_PAD
#define PEAQ_FE_LDS_PAD 0                    // occupancy experiments (VARIANT builds): LDS bytes a workgroup claims on top
#endif
  const size_t lds = kLdsDoubles * sizeof(double) + PEAQ_FE_LDS_PAD;
  if (bands == 109 && one_wave)
    hipLaunchKernelGGL(frontend_pair_kernel<109>, dim3(grid), dim3(64), kPairLdsDoubles * sizeof(double), stream, args);
  else if (bands == 109)
    hipLaunchKernelGGL(frontend_kernel<109>, dim3(grid), dim3(128), lds, stream, args);
  else if (bands == 55)
    hipLaunchKernelGGL(frontend_kernel<55>, dim3(grid), dim3(128), lds, stream, args);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_frontend(int bands, const FrontendArgs& a, unsigned n_pairs, hipStream_t stream) {
  return launch_frontend_as(bands == 109 && !frontend_two_waves(), bands, a, n_pairs, stream);
}

}  // namespace peaq

// peaq_frac.hip -- the constant sub-sample part of a pair's delay: estimate on a grid of 1 / PEAQ_SUB_STEPS samples and
// the test signal's cut through a fractional-delay filter (peaq_batch_refine_delay, peaq_batch_cut_shifted,
// peaq_subsample_tables, peaq_subdelay_workspace_bytes, peaq_run_pair_subsample; include/peaq_amd.h).
//
//   frac_corr_kernel   one workgroup per chunk of kFrChunk reference samples of one pair: the 33 sums
//       c_k = sum_n r[n] t[n + lag + k] over the chunk's n, in FP64.  Lane l owns the 16 consecutive n from 16 l on: its
//       r values sit in registers, the t values its 16 x 33 products meet come from the chunk's window in LDS, in three
//       passes of eleven sums: 26 reads per pass, each feeding up to 11 multiply-adds.  A lane adds its terms of one k in
//       the order of n; then the wave (peaq::wave_sum), then the four waves ((0 + 1) + (2 + 3)).  A term exists where
//       both indices lie inside their signals; waves whose windows lie inside both take the unguarded copy of the same
//       instructions.  One partial per k to the scratch; no atomics.
//   frac_sum_kernel    one workgroup per pair: thread t adds the partials of chunks t, t + 256, ... in chunk order, then
//       the same fixed tree; the 33 sums go to the pair's last scratch row.
//   frac_pick_kernel   one workgroup per pair, one lane per grid point q: v(q) from the 33 sums and the correlation
//       table, the largest, the tie rule, the record.
//   frac_cut_kernel    peaq_batch_cut_shifted: a workgroup owns 1024 outputs of one pair, both channels.  It stages
//       1024 + 64 samples per channel in LDS (absent ones as zeros), a lane owns 4 adjacent outputs per channel and
//       walks the 68 samples under them once -- 17 reads of 16 bytes per channel, every sample feeding up to 4
//       multiply-adds per channel -- with the pair's tap row, uniform in the workgroup, from scalar loads.  Pairs with
//       q == 0 take align_cut_kernel's copy instead (cut_tile_copied, peaq_delay_cut.h): their bits are moved.
#include "peaq_delay_cut.h"

namespace {

constexpr int kFrR = PEAQ_SUB_LAGS;                    // integer lags each side
constexpr int kFrNK = 2 * kFrR + 1;                    // 33 sums per pair
constexpr int kFrK = PEAQ_SUB_HALF;                    // taps each side
constexpr int kFrTaps = 2 * kFrK + 1;                  // 65
constexpr int kFrSteps = PEAQ_SUB_STEPS;               // grid points per sample = rows of both tables
constexpr double kFrBeta = 8.49;                       // the converter's Kaiser window
constexpr double kFrTie = 1e-12;                       // of max |c_k|: values of v this close to the largest count as tied
constexpr uint32_t kFrChunk = 4096;                    // reference samples per workgroup of frac_corr_kernel
constexpr int kFrOwn = 16;                             // ... per lane
constexpr int kFrWin = kFrChunk + 2 * kFrR;            // test samples a chunk's products meet
constexpr int kFrWinPad = kFrWin + kFrWin / 16 + 2;    // in LDS: one double of padding per 16 (al_pad16's reason); 16-byte size
constexpr size_t kFrPartial = kFrNK * sizeof(double);
constexpr size_t kFrScratchBudget = (size_t)256 << 20; // pairs are taken in groups whose partials stay below this
constexpr int kFrTile = 1024;                          // outputs per channel per workgroup of frac_cut_kernel
constexpr int kFrPer = 4;                              // ... per lane
constexpr int kFrStage = kFrTile + 2 * kFrK;           // staged samples per channel
constexpr int kFrPitch = kFrStage + 16;                // floats between the channels' LDS rows: a multiple of 4, 16 mod 32
static_assert(kFrChunk == 256 * kFrOwn && kFrTile == 256 * kFrPer && kFrTile == kCutTile, "a lane's share; the cuts' tile");
static_assert(kFrStage % 4 == 0 && kFrPitch % 4 == 0 && kFrPitch % 32 == 16, "16-byte LDS reads; the channels' stores on different banks");
static_assert(kFrSteps == 256, "frac_pick_kernel: one lane per grid point");

struct RefineArgs {
  const float* ref;             // first pair of the group
  const float* test;
  size_t stride;
  const uint32_t* n_ref;        // device, first pair of the group
  const uint32_t* n_test;
  const int32_t* lag;
  int channels;
  uint32_t nch_max;             // chunks of the call's longest reference; a pair's scratch is [nch_max + 1][33]
  double* part;
  peaq_subdelay* out;           // first pair of the group
};

__device__ __forceinline__ int fr_pad16(int i) { return i + (i >> 4); }

constexpr int kFrPass = 11;                            // sums per pass of a lane over its samples
static_assert(kFrNK % kFrPass == 0, "whole passes");

// mono sum of sample s, in double (C: a constant, so that a load is a load and not a branch)
template <int C>
__device__ __forceinline__ double fr_mono(const float* __restrict__ x, long long s) {
  if (C == 2) return (double)x[2 * s] + (double)x[2 * s + 1];
  return (double)x[s];
}

template <int CH>
__device__ __forceinline__ void fr_corr(const RefineArgs& a, double* tw, double (*sh)[kFrNK]) {
  const unsigned pair = blockIdx.y, chunk = blockIdx.x;
  const long long n_ref = a.n_ref[pair], n_test = a.n_test[pair];
  const long long n0 = (long long)chunk * kFrChunk;
  if (n0 >= n_ref) return;                             // (the whole workgroup)
  constexpr int C = CH;
  const float* __restrict__ ref = a.ref + (size_t)pair * a.stride * C;
  const float* __restrict__ test = a.test + (size_t)pair * a.stride * C;
  const long long t0 = n0 + (long long)a.lag[pair] - kFrR;   // test sample under window position 0
#pragma unroll 4
  for (int v = threadIdx.x; v < kFrWin; v += 256) {
    const long long s = t0 + v;
    tw[fr_pad16(v)] = (s >= 0 && s < n_test) ? fr_mono<CH>(test, s) : 0.;
  }
  const long long m0 = n0 + (long long)kFrOwn * threadIdx.x;      // the lane's first reference sample
  const long long first = t0 + (long long)kFrOwn * threadIdx.x;   // the test sample under its window position 0
  const bool whole = m0 + kFrOwn <= n_ref && first >= 0 && first + kFrOwn + 2 * kFrR <= n_test;
  const bool guard = __builtin_amdgcn_ballot_w64(!whole) != 0;    // (per wave) a term of this wave may not exist
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double* lane_tw = tw + fr_pad16(kFrOwn * (int)threadIdx.x);   // (16 l + u pads to 17 l + pad16 (u))
  if (!guard) {
    // Three passes of eleven sums: the lane's 16 samples stay in registers, a pass reads the 26 window positions its
    // 16 x 11 products meet, once each, and a sum's terms arrive in the order of m.  (All 33 sums in one pass need
    // 66 registers of accumulators beside the samples and whatever reads are in flight: more than 128.)
    double r[kFrOwn];
#pragma unroll
    for (int m = 0; m < kFrOwn; ++m) r[m] = fr_mono<CH>(ref, m0 + m);
#pragma unroll 1
    for (int k0 = 0; k0 < kFrNK; k0 += kFrPass) {
      double acc[kFrPass];
#pragma unroll
      for (int k = 0; k < kFrPass; ++k) acc[k] = 0.;
      const int p0 = kFrOwn * (int)threadIdx.x + k0;
#pragma unroll
      for (int u = 0; u < kFrOwn + kFrPass - 1; ++u) {
        const double t = tw[fr_pad16(p0 + u)];
#pragma unroll
        for (int m = 0; m < kFrOwn; ++m) {
          const int k = u - m;
          if (k >= 0 && k < kFrPass) acc[k] = __builtin_fma(r[m], t, acc[k]);
        }
      }
#pragma unroll
      for (int k = 0; k < kFrPass; ++k) {
        const double s = peaq::wave_sum(acc[k]);
        if (lane == 0) sh[wave][k0 + k] = s;
      }
    }
  } else {
    // the pair's first and last waves: the same chains sum by sum, a term only where both of its samples exist
#pragma unroll 1
    for (int k = 0; k < kFrNK; ++k) {
      double s = 0.;
#pragma unroll 1
      for (int m = 0; m < kFrOwn; ++m) {
        const long long ti = first + m + k;
        if (m0 + m < n_ref && ti >= 0 && ti < n_test) s = __builtin_fma(fr_mono<CH>(ref, m0 + m), lane_tw[fr_pad16(m + k)], s);
      }
      s = peaq::wave_sum(s);
      if (lane == 0) sh[wave][k] = s;
    }
  }
  __syncthreads();
  if (threadIdx.x < kFrNK)
    a.part[((size_t)pair * (a.nch_max + 1) + chunk) * kFrNK + threadIdx.x] =
        (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
}

__global__ __launch_bounds__(256, 4) void frac_corr_kernel(const RefineArgs a) {
  __shared__ double tw[kFrWinPad];
  __shared__ double sh[4][kFrNK];
  if (a.channels == 2)
    fr_corr<2>(a, tw, sh);
  else
    fr_corr<1>(a, tw, sh);
}

__host__ __device__ inline uint32_t frac_chunks(uint32_t n) { return (uint32_t)(((uint64_t)n + kFrChunk - 1) / kFrChunk); }

// (three passes of eleven sums: 33 accumulators beside 33 loads in flight do not fit 128 registers)
__global__ __launch_bounds__(256, 4) void frac_sum_kernel(const RefineArgs a) {
  constexpr int kPass = 11;
  static_assert(kFrNK % kPass == 0, "whole passes");
  __shared__ double sh[4][kPass];
  const unsigned pair = blockIdx.x;
  const uint32_t nch = frac_chunks(a.n_ref[pair]);
  double* P = a.part + (size_t)pair * (a.nch_max + 1) * kFrNK;
#pragma unroll 1
  for (int k0 = 0; k0 < kFrNK; k0 += kPass) {
    double s[kPass];
#pragma unroll
    for (int k = 0; k < kPass; ++k) s[k] = 0.;
    for (uint32_t ch = threadIdx.x; ch < nch; ch += 256) {   // chunk order
#pragma unroll
      for (int k = 0; k < kPass; ++k) s[k] += P[(size_t)ch * kFrNK + k0 + k];
    }
    block_sum4(s, sh);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < kPass; ++k) P[(size_t)a.nch_max * kFrNK + k0 + k] = s[k];
    }
    __syncthreads();                                   // (sh is written again in the next pass)
  }
}

// (the table as a parameter of its own, as the converter's taps: DESIGN.md 10)
__global__ __launch_bounds__(256, 4) void frac_pick_kernel(const RefineArgs a, const double* __restrict__ corr_tab) {
  __shared__ double sh_d[4];
  __shared__ unsigned sh_u[4];
  const unsigned pair = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const double* __restrict__ c = a.part + ((size_t)pair * (a.nch_max + 1) + a.nch_max) * kFrNK;
  const long long n_ref = a.n_ref[pair], n_test = a.n_test[pair];
  const int32_t lag = a.lag[pair];
  const long long mag = lag < 0 ? -(long long)lag : (long long)lag;
  double cmax = 0.;
  bool finite = true;
  for (int k = 0; k < kFrNK; ++k) {                   // (every thread alike)
    finite = finite && isfinite(c[k]);
    cmax = fmax(cmax, fabs(c[k]));
  }
  peaq_subdelay rec;
  rec.lag = lag;
  rec.q = 0;
  rec.frac = 0.;
  rec.peak = 0.;
  rec.c0 = c[kFrR];
  rec.flags = 0;
  rec.reserved = 0;
  if (mag >= n_ref || mag >= n_test || !finite || cmax == 0.) {   // (uniform) no overlap, a NaN or Inf, silence
    rec.flags = PEAQ_SUB_F_NONE;
    if (mag >= n_ref || mag >= n_test) rec.c0 = 0.;    // (nothing was summed for this pair, or nothing that counts)
  } else {
    const double s = c[kFrR] < 0. ? -1. : 1.;
    const double* __restrict__ row = corr_tab + (size_t)tid * kFrNK;
    double v = 0.;
    for (int k = 0; k < kFrNK; ++k) v = __dadd_rn(v, __dmul_rn(c[k], row[k]));   // k = -16 .. 16, product and sum rounded apart
    v *= s;
    double best = peaq::wave_max(v);
    if (lane == 0) sh_d[wave] = best;
    __syncthreads();
    best = fmax(fmax(sh_d[0], sh_d[1]), fmax(sh_d[2], sh_d[3]));
    const int q = (int)tid - kFrSteps / 2;
    unsigned key = 0xFFFFFFFFu;                        // 2 |q| + (q < 0): the smaller |q|, then the positive one
    if (v >= best - kFrTie * cmax) key = 2u * (unsigned)abs(q) + (q < 0 ? 1u : 0u);
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, w, 64));
    if (lane == 0) sh_u[wave] = key;
    __syncthreads();
    key = min(min(sh_u[0], sh_u[1]), min(sh_u[2], sh_u[3]));
    if (!isfinite(best) || key == 0xFFFFFFFFu) {       // (uniform) sums beyond FP64
      rec.flags = PEAQ_SUB_F_NONE;
    } else {
      const int qb = (key & 1u) ? -(int)(key >> 1) : (int)(key >> 1);
      if ((int)tid == qb + kFrSteps / 2) {             // the winner writes: v is its own
        rec.q = qb;
        rec.frac = (double)qb / kFrSteps;
        rec.peak = v * s;
        if (qb == -kFrSteps / 2 || qb == kFrSteps / 2 - 1) rec.flags = PEAQ_SUB_F_EDGE;
        a.out[pair] = rec;
      }
      return;
    }
  }
  if (tid == 0) a.out[pair] = rec;
}

struct ShiftArgs {
  size_t in_stride, out_stride; // samples per channel between pairs
  const uint32_t* n_in;         // device [n_pairs]
  const uint32_t* skip;
  const uint32_t* n_keep;
  const int32_t* q;
  int channels;
};

constexpr int kFrGroups = (kFrTaps + kFrPer - 1 + 3) / 4;   // 17 reads of 16 bytes per channel cover the 68 positions

// positions 4 g .. 4 g + 3 of the lane's window: one read of 16 bytes per channel, each sample into the outputs it meets
template <int C, bool EDGE>
__device__ __forceinline__ void fr_group(double (&acc)[C][kFrPer], const float* mine, const double* __restrict__ h, int g) {
  float4 x[C];
#pragma unroll
  for (int c = 0; c < C; ++c) x[c] = *reinterpret_cast<const float4*>(mine + c * kFrPitch + 4 * g);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int p = 4 * g + e;                                       // position under the lane's window
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const double xv = (double)(e == 0 ? x[c].x : e == 1 ? x[c].y : e == 2 ? x[c].z : x[c].w);
#pragma unroll
      for (int j = 0; j < kFrPer; ++j) {
        const int o = p - j;                                       // tap index o + 32 of the definition
        if (!EDGE || (o >= 0 && o < kFrTaps)) acc[c][j] = __builtin_fma(h[o], xv, acc[c][j]);
      }
    }
  }
}

template <int C>
__device__ __forceinline__ void fr_shift(const ShiftArgs& a, const float* __restrict__ in, float* __restrict__ out,
                                         const double* __restrict__ h, float* lds) {
  const unsigned pair = blockIdx.y;
  const long long n_in = a.n_in[pair], n_keep = a.n_keep[pair];
  const long long i0 = (long long)blockIdx.x * kFrTile;            // the tile's first output
  const long long s0 = (long long)a.skip[pair] + i0 - kFrK;        // input sample under staged position 0
  const float* __restrict__ src = in + (size_t)pair * a.in_stride * C;
  // ---- stage: consecutive lanes read consecutive floats; channel c of staged sample v at lds[c * pitch + v] ----
  for (int f = threadIdx.x; f < kFrStage * C; f += 256) {
    const int v = C == 2 ? f >> 1 : f, c = C == 2 ? f & 1 : 0;
    const long long s = s0 + v;
    lds[c * kFrPitch + v] = (s >= 0 && s < n_in) ? src[(size_t)s * C + c] : 0.f;
  }
  __syncthreads();
  // ---- outputs j = 0 .. 3 at staged positions 4 l + 32 + j: sample 4 l + x meets tap x - j of output j ----
  double acc[C][kFrPer];
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int j = 0; j < kFrPer; ++j) acc[c][j] = 0.;
  const float* mine = lds + kFrPer * threadIdx.x;
  // group g: positions 4 g .. 4 g + 3, taps 4 g - 3 .. 4 g + 3.  The first and the last group meet taps that do not
  // exist (EDGE: decided while compiling); the fifteen between them are a loop, so that a trip holds its own few taps
  // in scalar registers and its own two reads in vector registers instead of the whole row and window.
  fr_group<C, true>(acc, mine, h, 0);
#pragma unroll 1
  for (int g = 1; g < kFrGroups - 1; ++g) fr_group<C, false>(acc, mine, h, g);
  fr_group<C, true>(acc, mine, h, kFrGroups - 1);
  // ---- the lane's 4 x C consecutive floats ----
  const long long i = i0 + (long long)kFrPer * threadIdx.x;
  float* __restrict__ dst = out + ((size_t)pair * a.out_stride + (size_t)i) * C;
  if (i + kFrPer <= n_keep && ((uintptr_t)dst & 15) == 0) {
    if (C == 2) {
      reinterpret_cast<float4*>(dst)[0] = {(float)acc[0][0], (float)acc[C - 1][0], (float)acc[0][1], (float)acc[C - 1][1]};
      reinterpret_cast<float4*>(dst)[1] = {(float)acc[0][2], (float)acc[C - 1][2], (float)acc[0][3], (float)acc[C - 1][3]};
    } else {
      reinterpret_cast<float4*>(dst)[0] = {(float)acc[0][0], (float)acc[0][1], (float)acc[0][2], (float)acc[0][3]};
    }
  } else {
#pragma unroll
    for (int j = 0; j < kFrPer; ++j)
#pragma unroll
      for (int c = 0; c < C; ++c)
        if (i + j < n_keep) dst[j * C + c] = (float)acc[c][j];
  }
}

// (the buffers and the table as parameters of their own: only a __restrict__ read-only PARAMETER lets the compiler fetch
// the taps with scalar loads)
__global__ __launch_bounds__(256, 4) void frac_cut_kernel(const ShiftArgs a, const float* __restrict__ a_in,
                                                       float* __restrict__ a_out, const double* __restrict__ shift_tab) {
  __shared__ __attribute__((aligned(16))) float lds[2 * kFrPitch];
  const unsigned pair = blockIdx.y;
  // (the helper's own test of the tile, made here in front of q: this kernel's filter tiles are 1.4 % slower when q is
  // asked for beside n_keep as the other cuts ask for their scalars -- its taps are scalar loads behind the same wait)
  const uint32_t n_keep = a.n_keep[pair];
  if ((unsigned long long)blockIdx.x * kFrTile >= n_keep) return;
  const int q = a.q[pair];
  if (cut_tile_copied(a_in, a_out, a.in_stride, a.out_stride, a.skip, n_keep, a.channels, q == 0)) return;
  const double* __restrict__ h = shift_tab + (size_t)(q + kFrSteps / 2) * kFrTaps;
  if (a.channels == 2)
    fr_shift<2>(a, a_in, a_out, h, lds);
  else
    fr_shift<1>(a, a_in, a_out, h, lds);
}

// ---------------------------------------------------------------------------
// the two tables, host, double (include/peaq_amd.h: the definitions)
// ---------------------------------------------------------------------------
// I0 by the two Chebyshev expansions of the Cephes library (i0.c: [0, 8] and (8, inf)), in double and in that code's
// order of operations.  It is what numpy.i0 evaluates, so a table rebuilt from the header's formulas with numpy agrees
// with this one to 1e-15; the expansions themselves are good to about 1e-15 relative, far below what the window needs.
constexpr double kFrI0A[30] = {
    -4.4153416464793395e-18, 3.3307945188222384e-17, -2.431279846547955e-16,
    1.715391285555133e-15, -1.1685332877993451e-14, 7.676185498604936e-14,
    -4.856446783111929e-13, 2.95505266312964e-12, -1.726826291441556e-11,
    9.675809035373237e-11, -5.189795601635263e-10, 2.6598237246823866e-09,
    -1.300025009986248e-08, 6.046995022541919e-08, -2.670793853940612e-07,
    1.1173875391201037e-06, -4.4167383584587505e-06, 1.6448448070728896e-05,
    -5.754195010082104e-05, 0.00018850288509584165, -0.0005763755745385824,
    0.0016394756169413357, -0.004324309995050576, 0.010546460394594998,
    -0.02373741480589947, 0.04930528423967071, -0.09490109704804764,
    0.17162090152220877, -0.3046826723431984, 0.6767952744094761,
};
constexpr double kFrI0B[25] = {
    -7.233180487874754e-18, -4.830504485944182e-18, 4.46562142029676e-17,
    3.461222867697461e-17, -2.8276239805165836e-16, -3.425485619677219e-16,
    1.7725601330565263e-15, 3.8116806693526224e-15, -9.554846698828307e-15,
    -4.150569347287222e-14, 1.54008621752141e-14, 3.8527783827421426e-13,
    7.180124451383666e-13, -1.7941785315068062e-12, -1.3215811840447713e-11,
    -3.1499165279632416e-11, 1.1889147107846439e-11, 4.94060238822497e-10,
    3.3962320257083865e-09, 2.266668990498178e-08, 2.0489185894690638e-07,
    2.8913705208347567e-06, 6.889758346916825e-05, 0.0033691164782556943,
    0.8044904110141088,
};

#pragma clang fp contract(off)
template <int N>
double fr_chbevl(double x, const double (&c)[N]) {
  double b0 = c[0], b1 = 0., b2 = 0.;
  for (int i = 1; i < N; ++i) {
    b2 = b1;
    b1 = b0;
    b0 = x * b1 - b2 + c[i];
  }
  return 0.5 * (b0 - b2);
}

double fr_i0(double x) {
  x = std::fabs(x);
  if (x <= 8.) return std::exp(x) * fr_chbevl(x / 2. - 2., kFrI0A);
  return std::exp(x) * fr_chbevl(32. / x - 2., kFrI0B) / std::sqrt(x);
}

double fr_window(double x, double half, double i0b) {
  const double u = std::fabs(x) / half;
  if (!(u < 1.)) return 0.;
  return fr_i0(kFrBeta * std::sqrt(1. - u * u)) / i0b;
}

double fr_sinc(double x) {
  if (x == 0.) return 1.;
  const double px = M_PI * x;
  return std::sin(px) / px;
}

struct FracTables {
  std::vector<double> corr, shift;   // [256][33], [256][65]
  FracTables() : corr((size_t)kFrSteps * kFrNK), shift((size_t)kFrSteps * kFrTaps) {
    const double i0b = fr_i0(kFrBeta);
    for (int q = -kFrSteps / 2; q < kFrSteps / 2; ++q) {
      const double tau = (double)q / kFrSteps;
      for (int k = -kFrR; k <= kFrR; ++k)
        corr[(size_t)(q + kFrSteps / 2) * kFrNK + (k + kFrR)] = fr_sinc(tau - k) * fr_window(tau - k, kFrR + 1., i0b);
      for (int o = -kFrK; o <= kFrK; ++o)
        shift[(size_t)(q + kFrSteps / 2) * kFrTaps + (o + kFrK)] =
            q == 0 ? (o == 0 ? 1. : 0.) : fr_sinc(o - tau) * fr_window(o - tau, kFrK + 1., i0b);
    }
  }
};

const FracTables& frac_tables() {
  static const FracTables t;
  return t;
}

// partials, then the sums
size_t frac_per_pair(uint32_t n_max) { return ((size_t)std::max<uint32_t>(frac_chunks(n_max), 1) + 1) * kFrPartial; }

}  // namespace

struct FracState {
  DevBuf corr, shift;           // the two tables, uploaded once
  bool tables = false;
  StageScratch scratch;         // the partials and sums of a group of pairs
  LenStage lens;                // refine: [n_ref | n_test | lag]; cut_shifted: [n_in | skip | n_keep | q]
};

void frac_release(peaq_ctx* c) { release_stage(c->fr); }

// the context's stage state, its tables on the device (the first call of a context copies them, blocking, as the
// converter does its taps)
static int frac_state(peaq_ctx* c, FracState** out) {
  if (!c->fr) c->fr = new FracState;
  FracState* st = c->fr;
  if (!st->tables) {
    const FracTables& t = frac_tables();
    HIP_TRY(st->corr.reserve(t.corr.size() * sizeof(double)));
    HIP_TRY(st->shift.reserve(t.shift.size() * sizeof(double)));
    HIP_TRY(hipMemcpy(st->corr.p, t.corr.data(), t.corr.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(st->shift.p, t.shift.data(), t.shift.size() * sizeof(double), hipMemcpyHostToDevice));
    st->tables = true;
  }
  *out = st;
  return PEAQ_OK;
}

// what the drift cut (peaq_drift.hip) shares with this stage: the shift table on the context's device and the length
// slots.  The caller holds the context's lock and has selected the device.
int frac_shift_table(peaq_ctx* c, const double** shift, LenStage** lens) {
  FracState* st = nullptr;
  if (int rc = frac_state(c, &st)) return rc;
  *shift = st->shift.as<double>();
  *lens = &st->lens;
  return PEAQ_OK;
}

extern "C" size_t peaq_subdelay_size(void) { return sizeof(peaq_subdelay); }

extern "C" size_t peaq_subdelay_workspace_bytes(int channels, int n_pairs, uint32_t n_max) {
  if (channels != 1 && channels != 2) return 0;
  return pair_groups(frac_per_pair(n_max), n_pairs, kFrScratchBudget).bytes;
}

extern "C" int peaq_subsample_tables(double* corr, double* shift) {
  if (!corr && !shift) return fail(PEAQ_ERR_ARG, "peaq_subsample_tables: corr and shift are both NULL");
  const FracTables& t = frac_tables();
  if (corr) std::memcpy(corr, t.corr.data(), t.corr.size() * sizeof(double));
  if (shift) std::memcpy(shift, t.shift.data(), t.shift.size() * sizeof(double));
  return PEAQ_OK;
}

extern "C" int peaq_batch_refine_delay(peaq_ctx* c, int channels, int n_pairs, const float* d_ref, const float* d_test,
                                       size_t pair_stride, const uint32_t* n_ref, const uint32_t* n_test,
                                       uint32_t n_uniform, const int32_t* lag, peaq_subdelay* d_out, void* stream_) {
  const std::string w("peaq_batch_refine_delay");
  if (int rc = check_shape(w, channels, n_pairs)) return rc;
  if (n_pairs > 0 && (!d_ref || !d_test || !d_out)) return fail(PEAQ_ERR_ARG, w + ": NULL buffer");
  if (n_pairs > 0 && !lag) return fail(PEAQ_ERR_ARG, w + ": NULL lag");
  if ((n_ref == nullptr) != (n_test == nullptr))
    return fail(PEAQ_ERR_ARG, w + ": n_ref and n_test must both be given or both be NULL");
  const size_t np = (size_t)std::max(n_pairs, 0);
  uint32_t n_max = 0;                                  // (the chunks are the reference's)
  if (int rc = check_lengths(w, n_pairs, n_ref, n_uniform, "n_ref", pair_stride, "pair_stride", &n_max)) return rc;
  if (int rc = check_lengths(w, n_pairs, n_test, n_uniform, "n_test", pair_stride, "pair_stride")) return rc;
  std::vector<uint32_t> h(3 * np);
  for (size_t p = 0; p < np; ++p) {
    h[p] = n_ref ? n_ref[p] : n_uniform;
    h[np + p] = n_test ? n_test[p] : n_uniform;
    std::memcpy(&h[2 * np + p], &lag[p], sizeof(uint32_t));
  }
  if (!c) return fail(PEAQ_ERR_ARG, w + ": ctx is NULL");
  if (n_pairs == 0) return PEAQ_OK;

  hipStream_t stream = static_cast<hipStream_t>(stream_);
  std::lock_guard<std::mutex> lock(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  FracState* st = nullptr;
  if (int rc = frac_state(c, &st)) return rc;
  const uint32_t nch = std::max<uint32_t>(frac_chunks(n_max), 1);
  const PairGroups pg = pair_groups(frac_per_pair(n_max), n_pairs, kFrScratchBudget);
  const int group = pg.group;
  if (int rc = st->scratch.acquire(pg.bytes, stream)) return rc;
  LenSlot* slot = nullptr;
  if (int rc = st->lens.upload(h.data(), h.size(), stream, &slot)) return rc;
  RefineArgs a{};
  a.stride = pair_stride;
  a.channels = channels;
  a.nch_max = nch;
  a.part = st->scratch.buf.as<double>();
  hipError_t launched = hipSuccess;
  for (int p0 = 0; p0 < n_pairs; p0 += group) {
    const unsigned g = (unsigned)std::min(group, n_pairs - p0);
    a.ref = d_ref + (size_t)p0 * pair_stride * channels;
    a.test = d_test + (size_t)p0 * pair_stride * channels;
    a.n_ref = slot->dev.as<uint32_t>() + p0;
    a.n_test = a.n_ref + np;
    a.lag = reinterpret_cast<const int32_t*>(a.n_test + np);
    a.out = d_out + p0;
    if (n_max) hipLaunchKernelGGL(frac_corr_kernel, dim3(nch, g), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(frac_sum_kernel, dim3(g), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(frac_pick_kernel, dim3(g), dim3(256), 0, stream, a, st->corr.as<double>());
    launched = hipGetLastError();
    if (launched != hipSuccess) break;
  }
  // (also after a failed launch: what was enqueued before it still reads the slot and the scratch)
  const hipError_t marked = st->scratch.mark(stream);
  const int sent = st->lens.sent(slot, stream);
  HIP_TRY(launched);
  HIP_TRY(marked);
  return sent;
}

extern "C" int peaq_batch_cut_shifted(peaq_ctx* c, int channels, int n_pairs, const float* d_in, size_t in_stride,
                                      const uint32_t* n_in, const uint32_t* skip, const uint32_t* n_keep, const int32_t* q,
                                      float* d_out, size_t out_stride, void* stream_) {
  const std::string w("peaq_batch_cut_shifted");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  DelayCutCall k{w, c, channels, n_pairs, d_in, in_stride, n_in, skip, n_keep, d_out, out_stride, stream};
  if (int rc = k.check(q, " or q")) return rc;
  k.pack(4, 0, false);
  for (size_t p = 0; p < k.np; ++p) {
    if (q[p] < -kFrSteps / 2 || q[p] > kFrSteps / 2 - 1)
      return fail(PEAQ_ERR_ARG, w + ": pair " + std::to_string(p) + ": q " + std::to_string(q[p]) + " is outside -128 .. 127");
    std::memcpy(&k.col(3, p), &q[p], sizeof(uint32_t));
  }
  if (int rc = k.upload()) return rc;
  if (!k.slot) return PEAQ_OK;
  ShiftArgs a{};
  a.in_stride = in_stride;
  a.out_stride = out_stride;
  a.n_in = k.dev_col(0);
  a.skip = k.dev_col(1);
  a.n_keep = k.dev_col(2);
  a.q = reinterpret_cast<const int32_t*>(k.dev_col(3));
  a.channels = channels;
  hipLaunchKernelGGL(frac_cut_kernel, dim3(k.tiles(), (unsigned)n_pairs), dim3(256), 0, stream, a, d_in, d_out, k.tab);
  return k.launched();
}

extern "C" int peaq_run_pair_subsample(peaq_ctx* c, int advanced, int channels, double level_db, uint32_t rate,
                                       uint32_t max_lag, int mode, double max_gain_db, const float* ref, size_t n_ref,
                                       const float* test, size_t n_test, peaq_delay* delay, peaq_subdelay* subdelay,
                                       peaq_gain* gain, peaq_result* out) {
  const std::string w("peaq_run_pair_subsample");
  // 1 .. 3: upload, rate conversion, estimate
  PairBuffers in;
  peaq_delay rec;
  if (int rc = begin_delay_pair(w, c, channels, level_db, rate, max_lag, 0, mode, max_gain_db, ref, n_ref, test, n_test, delay,
                                gain, out, in, &rec, nullptr))
    return rc;
  const uint32_t* len = in.len;
  const size_t stride = in.stride;
  // 4: refine
  DevBuf d_sub;
  HIP_TRY(d_sub.reserve(sizeof(peaq_subdelay)));
  if (int rc = peaq_batch_refine_delay(c, channels, 1, in.d(0), in.d(1), stride, len, len + 1, 0, &rec.lag,
                                       d_sub.as<peaq_subdelay>(), nullptr))
    return rc;
  HIP_TRY(hipDeviceSynchronize());
  peaq_subdelay sub;
  HIP_TRY(hipMemcpy(&sub, d_sub.p, sizeof sub, hipMemcpyDeviceToHost));
  if (subdelay) *subdelay = sub;
  // 5 .. 8: both signals cut to their common part, the test signal through the shift filter; the gain; the score
  uint32_t skip[2], common = 0;
  peaq_aligned_lengths(rec.lag, len[0], len[1], &skip[0], &skip[1], &common);
  return score_cut_pair(c, advanced, channels, level_db, in, skip, common, mode, max_gain_db, gain,
                        [&](float* d_out, size_t out_stride) {
                          return peaq_batch_cut_shifted(c, channels, 1, in.d(1), stride, &len[1], &skip[1], &common, &sub.q, d_out,
                                                        out_stride, nullptr);
                        },
                        out);
}

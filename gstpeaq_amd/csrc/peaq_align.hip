// peaq_align.hip -- time alignment in front of the batch driver (peaq_batch_estimate_delay, peaq_batch_cut,
// peaq_aligned_lengths, peaq_run_pair_aligned; include/peaq_amd.h).  The delay of a pair is the integer lag of the
// largest |cross-correlation| of the two mono sums over [-max_lag, max_lag]; the correlation is evaluated in the
// blocked frequency-domain form, which is exact for linear correlation:
//
//   H = 512.  Reference block j = r[jH .. jH + H) zero-padded to 2H, test window k = t[kH .. kH + 2H).
//   A_s[b] = sum_j conj(R_j[b]) T_{j+s}[b];  the inverse transform of A_s holds, at m = 0 .. H, the lags sH + m
//   (m + n <= 2H - 1 for n < H: nothing wraps).  Segments s = -S .. S - 1, S = ceil(max_lag / H), cover every lag
//   of [-SH, SH]; samples outside a signal are zeros, which is the definition's "over all n where both exist".
//
// Four kernels per group of pairs, all FP64 after the samples' conversion:
//   align_spectra_kernel     one wave per transform: a 1024-point complex transform (the front end's three passes, from
//       dft16 / dft4 / rows_transpose4 of peaq_wave.h) carries reference block i in its real part and test window
//       i - S in its imaginary part; split by symmetry into the half-spectra R_i and T_i, bins 0 .. 511 with the
//       (real) bin 512 in bin 0's imaginary part, written to the scratch.  Also the block's share of sum r^2, sum t^2.
//   align_accumulate_kernel  one thread per bin, chunk of 128 blocks and group of 16 segments: the 16 products per
//       block accumulate in registers, the 16 test spectra a block meets sit in a register ring (one new spectrum per
//       block), so every spectrum is read once per chunk and segment group.  Partial sums per chunk, to the scratch.
//   align_inverse_kernel     one wave per segment: the chunks' partial sums added in chunk order, the Hermitian
//       spectrum rebuilt, one transform back, lags to the scratch.
//   align_pick_kernel        one workgroup per pair: norm, arg-max with the tie rule, runner-up.
// Every sum has a fixed order and every reduction across threads is a max or a min, so the record of a pair does
// not depend on the batch it is in, and is the same run to run.
//   align_cut_kernel         peaq_batch_cut: a strided copy, 16 bytes per lane where the alignment allows (copy_run,
//       peaq_host.h).
// The file also defines the steps the one-pair conveniences of every stage are built from (peaq_host.h).
#include "peaq_host.h"

namespace {

using peaq::cplx;
using peaq::cmul;

constexpr int kAlH = 512;                        // block length; transforms are 2H = 1024 points
constexpr int kAlBins = 512;                     // stored bins per half-spectrum (bin 512 rides in bin 0)
constexpr int kAlG = 16;                         // segments per group = products per thread and block
constexpr int kAlChunk = 128;                    // blocks per partial sum (a multiple of kAlG)
constexpr int kAlExch = 1088;                    // doubles of exchange buffer per wave (8.5 KiB)
constexpr uint32_t kAlMaxLag = 16384;
// Tie tolerance of the arg-max, in units of norm.  The rounding error of c[d] is a few times 2^-53 log2(1024) norm per
// transform it passes (three), some 1e-14 norm at worst; 1e-12 is two orders above that and three below
// the bound the header states for c.
constexpr double kAlTie = 1e-12;
constexpr size_t kAlScratchBudget = (size_t)1 << 30;   // pairs are taken in groups whose scratch stays below this

struct AlignArgs {
  const float* ref;             // first pair of the group
  const float* test;
  size_t stride;
  const uint32_t* n_ref;        // device, first pair of the group; nullptr: n_uniform
  const uint32_t* n_test;
  uint32_t n_uniform;
  int channels;
  uint32_t D;                   // max_lag
  uint32_t S;                   // segments each side: lags [-S H, S H]
  uint32_t NB, NT;              // reference blocks, test windows (= transforms) per pair
  uint32_t NSEG, NCH;           // segments computed (a multiple of kAlG, >= 2 S), chunks
  double2* rspec;               // [pair][NB][512]
  double2* tspec;               // [pair][NT][512]
  double2* part;                // [pair][NSEG][NCH][512]
  double* corr;                 // [pair][2 S H + 1]
  double* energy;               // [pair][NT][2]: sum r^2 of block i, sum t^2 of the first half of window i
  peaq_delay* out;              // first pair of the group
  const peaq::CommonTables* ct;
};

__device__ __forceinline__ int al_pad16(int i) { return i + (i >> 4); }
__device__ __forceinline__ cplx al_tw_lane(const peaq::CommonTables* __restrict__ ct, int e, int lane) {
  const double2 v = *reinterpret_cast<const double2*>(ct->tw_lane[e][lane]);
  return {v.x, v.y};
}
__device__ __forceinline__ cplx al_csqr(cplx a) { return {a.re * a.re - a.im * a.im, 2. * (a.re * a.im)}; }

template <typename WR, typename RD>
__device__ __forceinline__ void al_exchange16(cplx (&z)[16], double* buf, WR wr, RD rd) {
#pragma unroll
  for (int r = 0; r < 16; ++r) buf[al_pad16(wr(r))] = z[r].re;
  peaq::wave_lds_fence();
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r].re = buf[al_pad16(rd(r))];
  peaq::wave_lds_fence();
#pragma unroll
  for (int r = 0; r < 16; ++r) buf[al_pad16(wr(r))] = z[r].im;
  peaq::wave_lds_fence();
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r].im = buf[al_pad16(rd(r))];
  peaq::wave_lds_fence();
}

// 1024-point forward complex DFT of one wave, 16 x 16 x 4 Stockham: in z[r] = x[lane + 64 r], out z[q] = X[lane + 64 q]
// (the three passes of the front end's frame_power_spectrum; buf: kAlExch doubles of LDS of this wave's own)
__device__ __forceinline__ void al_fft1024(cplx (&z)[16], double* buf, int lane, const peaq::CommonTables* __restrict__ ct) {
  peaq::dft16(z);
  al_exchange16(z, buf, [&](int r) { return 16 * lane + r; }, [&](int r) { return lane + 64 * r; });
  {
    cplx w[9];
    w[1] = al_tw_lane(ct, 2, lane);                  // W_256^(lane & 15)
    w[2] = al_csqr(w[1]);
    w[4] = al_csqr(w[2]);
    w[8] = al_csqr(w[4]);
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
  peaq::dft16(z);
  // rows and registers trade places (see frame_power_spectrum): four 4 x 4 transposes and a renaming
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    peaq::rows_transpose4(z[4 * g].re, z[4 * g + 1].re, z[4 * g + 2].re, z[4 * g + 3].re);
    peaq::rows_transpose4(z[4 * g].im, z[4 * g + 1].im, z[4 * g + 2].im, z[4 * g + 3].im);
  }
#pragma unroll
  for (int a2 = 0; a2 < 4; ++a2)
#pragma unroll
    for (int g = a2 + 1; g < 4; ++g) {
      const cplx t = z[4 * a2 + g];
      z[4 * a2 + g] = z[4 * g + a2];
      z[4 * g + a2] = t;
    }
  {
    constexpr double c1 = 0.92387953251128673848, s1 = 0.38268343236508977173, c2 = 0.70710678118654752440;
    const cplx wb = al_tw_lane(ct, 1, lane);         // W_1024^lane
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const cplx w1 = m == 0 ? wb : m == 1 ? cmul(wb, {c1, -s1}) : m == 2 ? cmul(wb, {c2, -c2}) : cmul(wb, {s1, -c1});
      const cplx w2 = al_csqr(w1), w3 = cmul(w2, w1);
      z[m + 4] = cmul(z[m + 4], w1);
      z[m + 8] = cmul(z[m + 8], w2);
      z[m + 12] = cmul(z[m + 12], w3);
      peaq::dft4(z[m], z[m + 4], z[m + 8], z[m + 12]);
    }
  }
}

// mono sum of sample s, in double
__device__ __forceinline__ double al_mono(const float* __restrict__ x, long long s, int channels) {
  return channels == 2 ? (double)x[2 * s] + (double)x[2 * s + 1] : (double)x[s];
}

__global__ __launch_bounds__(256) void align_spectra_kernel(const AlignArgs a) {
  __shared__ double al_lds[4 * kAlExch];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned i = blockIdx.x * 4 + wave, pair = blockIdx.y;
  if (i >= a.NT) return;                             // (the whole wave; no workgroup barrier below)
  const long long n_ref = a.n_ref ? a.n_ref[pair] : a.n_uniform;
  const long long n_test = a.n_test ? a.n_test[pair] : a.n_uniform;
  const int C = a.channels;
  const float* ref = a.ref + (size_t)pair * a.stride * C;
  const float* test = a.test + (size_t)pair * a.stride * C;
  const long long r0 = (long long)i * kAlH, t0 = ((long long)i - (long long)a.S) * kAlH;
  cplx z[16];
  double er = 0., et = 0.;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = lane + 64 * r;
    double xr = 0., xt = 0.;
    if (r < 8 && r0 + n < n_ref) xr = al_mono(ref, r0 + n, C);
    if (t0 + n >= 0 && t0 + n < n_test) xt = al_mono(test, t0 + n, C);
    z[r] = {xr, xt};
    if (r < 8) {
      er = __builtin_fma(xr, xr, er);
      et = __builtin_fma(xt, xt, et);
    }
  }
  er = peaq::wave_sum(er);
  et = peaq::wave_sum(et);
  if (lane == 0) {
    double* e = a.energy + ((size_t)pair * a.NT + i) * 2;
    e[0] = er;
    e[1] = et;
  }
  al_fft1024(z, al_lds + wave * kAlExch, lane, a.ct);
  // Z = R + i T with R, T the spectra of two real signals: R[k] = (Z[k] + conj Z[1024 - k]) / 2,
  // T[k] = (Z[k] - conj Z[1024 - k]) / 2i.  Z[1024 - k], k = lane + 64 q, sits in lane 64 - lane, slot 15 - q
  // (lane 0: its own slot 16 - q).
  const int partner = (64 - lane) & 63;
  double2* R = a.rspec + ((size_t)pair * a.NB + i) * kAlBins;
  double2* T = a.tspec + ((size_t)pair * a.NT + i) * kAlBins;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int k = lane + 64 * q;
    cplx zm = {__shfl(z[15 - q].re, partner, 64), __shfl(z[15 - q].im, partner, 64)};
    if (lane == 0) zm = z[(16 - q) & 15];
    double2 rr = {0.5 * (z[q].re + zm.re), 0.5 * (z[q].im - zm.im)};
    double2 tt = {0.5 * (z[q].im + zm.im), 0.5 * (zm.re - z[q].re)};
    if (q == 0 && lane == 0) {                       // bins 0 and 512 are real: they share a slot
      rr = {z[0].re, z[8].re};
      tt = {z[0].im, z[8].im};
    }
    if (i < a.NB) R[k] = rr;
    T[k] = tt;
  }
}

__global__ __launch_bounds__(256) void align_accumulate_kernel(const AlignArgs a) {
  const unsigned k = (blockIdx.x & 1) * 256 + threadIdx.x;
  const unsigned chunk = blockIdx.x >> 1, pair = blockIdx.y, g = blockIdx.z;
  const double2* __restrict__ R = a.rspec + (size_t)pair * a.NB * kAlBins + k;
  const double2* __restrict__ T = a.tspec + ((size_t)pair * a.NT + (size_t)g * kAlG) * kAlBins + k;
  const unsigned j0 = chunk * kAlChunk, j1 = min(j0 + kAlChunk, a.NB);
  // segment u of the group meets, at block j, test window j + u (relative to the group's first): slot (j + u) mod G
  double2 t[kAlG], acc[kAlG];
#pragma unroll
  for (int u = 0; u < kAlG; ++u) acc[u] = {0., 0.};
#pragma unroll
  for (int u = 0; u < kAlG - 1; ++u) t[u] = T[(size_t)(j0 + u) * kAlBins];   // (j0 is a multiple of G)
  // bin 0 carries two real bins: its "product" is component by component
  const bool k0 = k == 0;
  const double m = k0 ? 0. : 1.;
  for (unsigned jb = j0; jb < j1; jb += kAlG) {
#pragma unroll
    for (int jj = 0; jj < kAlG; ++jj) {
      const unsigned j = jb + jj;
      if (j < j1) {
        t[(jj + kAlG - 1) % kAlG] = T[(size_t)(j + kAlG - 1) * kAlBins];
        const double2 r = R[(size_t)j * kAlBins];
        const double mry = m * r.y, p = k0 ? r.y : r.x;
#pragma unroll
        for (int u = 0; u < kAlG; ++u) {             // conj(r) t = (rx tx + ry ty, rx ty - ry tx)
          const double2 tt = t[(jj + u) % kAlG];
          acc[u].x = __builtin_fma(r.x, tt.x, acc[u].x);
          acc[u].x = __builtin_fma(mry, tt.y, acc[u].x);
          acc[u].y = __builtin_fma(p, tt.y, acc[u].y);
          acc[u].y = __builtin_fma(-mry, tt.x, acc[u].y);
        }
      }
    }
  }
  double2* P = a.part + (((size_t)pair * a.NSEG + (size_t)g * kAlG) * a.NCH + chunk) * kAlBins + k;
#pragma unroll
  for (int u = 0; u < kAlG; ++u) P[(size_t)u * a.NCH * kAlBins] = acc[u];
}

__global__ __launch_bounds__(256) void align_inverse_kernel(const AlignArgs a) {
  __shared__ double al_lds[4 * kAlExch];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned seg = blockIdx.x * 4 + wave, pair = blockIdx.y;
  if (seg >= 2 * a.S) return;                        // (the whole wave)
  const double2* __restrict__ P = a.part + ((size_t)pair * a.NSEG + seg) * a.NCH * kAlBins;
  // c[m] = (1 / N) sum_b A[b] W^(-b m) = (1 / N) Re sum_b conj(A[b]) W^(b m): the forward transform of conj A, with
  // A[1024 - b] = conj A[b] for the upper half
  cplx z[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = lane + 64 * r;
    const int b = (n < 512 ? n : 1024 - n) & 511;    // (bin 512 rides in bin 0)
    double sx = 0., sy = 0.;
    for (unsigned ch = 0; ch < a.NCH; ++ch) {        // chunk order
      const double2 v = P[(size_t)ch * kAlBins + b];
      sx += v.x;
      sy += v.y;
    }
    z[r] = n == 0 ? cplx{sx, 0.} : n == 512 ? cplx{sy, 0.} : n < 512 ? cplx{sx, -sy} : cplx{sx, sy};
  }
  al_fft1024(z, al_lds + wave * kAlExch, lane, a.ct);
  double* c = a.corr + (size_t)pair * (2 * (size_t)a.S * kAlH + 1) + (size_t)seg * kAlH;
#pragma unroll
  for (int q = 0; q < 8; ++q) c[lane + 64 * q] = z[q].re * (1. / 1024.);
  if (seg == 2 * a.S - 1 && lane == 0) c[kAlH] = z[8].re * (1. / 1024.);   // the lag S H itself
}

// workgroup reductions of align_pick_kernel (256 threads; sh: 256 entries)
template <typename T, typename OP>
__device__ __forceinline__ T al_block_reduce(T v, T* sh, OP op) {
  __syncthreads();                                   // (sh may still be read from the reduction before)
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] = op(sh[threadIdx.x], sh[threadIdx.x + w]);
    __syncthreads();
  }
  return sh[0];
}

__global__ __launch_bounds__(256) void align_pick_kernel(const AlignArgs a) {
  __shared__ double sh_d[256];
  __shared__ unsigned sh_u[256];
  const unsigned pair = blockIdx.x, tid = threadIdx.x;
  // energies: every thread its own blocks in index order, then a fixed tree
  double er = 0., et = 0.;
  const double* e = a.energy + (size_t)pair * a.NT * 2;
  for (unsigned i = tid; i < a.NT; i += 256) {
    er += e[2 * i];
    et += e[2 * i + 1];
  }
  const auto add = [](double x, double y) { return x + y; };
  er = al_block_reduce(er, sh_d, add);
  et = al_block_reduce(et, sh_d, add);
  peaq_delay rec;
  rec.lag = 0;
  rec.reserved = 0;
  rec.peak = rec.runner_up = rec.norm = 0.;
  const double e2 = er * et;
  if (!isfinite(e2)) {                               // (uniform) a NaN or Inf sample, or energies beyond FP64: no estimate
    rec.norm = __builtin_nan("");
  } else if (e2 > 0.) {
    const double norm = sqrt(e2);
    const int D = (int)a.D;
    const double* c = a.corr + (size_t)pair * (2 * (size_t)a.S * kAlH + 1) + (size_t)a.S * kAlH;   // c[d], d = -SH .. SH
    const auto fmx = [](double x, double y) { return fmax(x, y); };
    double best = 0.;
    for (int d = -D + (int)tid; d <= D; d += 256) best = fmax(best, fabs(c[d]));
    best = al_block_reduce(best, sh_d, fmx);
    // values within kAlTie norm of the largest are not told apart (the transforms' rounding gives the lags of an exact
    // tie different last bits): among them the smaller |d|, then the positive
    const double floor_ = best - kAlTie * norm;
    unsigned key = 0xFFFFFFFFu;                      // 2 |d| + (d < 0)
    for (int d = -D + (int)tid; d <= D; d += 256)
      if (fabs(c[d]) >= floor_) key = min(key, 2u * (unsigned)abs(d) + (d < 0 ? 1u : 0u));
    key = al_block_reduce(key, sh_u, [](unsigned x, unsigned y) { return min(x, y); });
    if (key == 0xFFFFFFFFu) {                        // (uniform) no lag selected: nothing of c is a number
      rec.norm = __builtin_nan("");
    } else {
      const int lag = (key & 1u) ? -(int)(key >> 1) : (int)(key >> 1);   // |lag| <= D by construction
      double second = 0.;
      for (int d = -D + (int)tid; d <= D; d += 256)
        if (d != lag) second = fmax(second, fabs(c[d]));
      second = al_block_reduce(second, sh_d, fmx);
      rec.lag = lag;
      rec.peak = c[lag];
      rec.runner_up = second;
      rec.norm = norm;
    }
  }
  if (tid == 0) a.out[pair] = rec;
}

struct CutArgs {
  const float* in;
  float* out;
  size_t in_stride, out_stride;  // samples per channel between pairs
  const uint32_t* skip;          // device [n_pairs]
  const uint32_t* n_keep;        // device [n_pairs]
  int channels;
};

// floats, not samples: a pair's run is n_keep x channels consecutive floats
__global__ __launch_bounds__(256) void align_cut_kernel(const CutArgs a) {
  const unsigned pair = blockIdx.y;
  const size_t count = (size_t)a.n_keep[pair] * a.channels;
  const float* __restrict__ src = a.in + ((size_t)pair * a.in_stride + a.skip[pair]) * a.channels;
  float* __restrict__ dst = a.out + (size_t)pair * a.out_stride * a.channels;
  copy_run(src, dst, count, (size_t)blockIdx.x * 256, blockIdx.x == 0, CopyBits());
}

// what one call's shape needs
struct AlignPlan {
  uint32_t S, NB, NT, NSEG, NCH;
  size_t rspec, tspec, part, corr, energy;           // bytes per pair
  size_t per_pair;
};

size_t round256(size_t v) { return (v + 255) & ~(size_t)255; }

AlignPlan align_plan(uint32_t n_max, uint32_t max_lag) {
  AlignPlan p;
  p.S = (max_lag + kAlH - 1) / kAlH;
  p.NB = std::max<uint32_t>(1, (uint32_t)(((uint64_t)n_max + kAlH - 1) / kAlH));
  p.NSEG = (2 * p.S + kAlG - 1) / kAlG * kAlG;
  p.NT = p.NB + p.NSEG - 1;
  p.NCH = (p.NB + kAlChunk - 1) / kAlChunk;
  p.rspec = round256((size_t)p.NB * kAlBins * sizeof(double2));
  p.tspec = round256((size_t)p.NT * kAlBins * sizeof(double2));
  p.part = round256((size_t)p.NSEG * p.NCH * kAlBins * sizeof(double2));
  p.corr = round256((2 * (size_t)p.S * kAlH + 1) * sizeof(double));
  p.energy = round256((size_t)p.NT * 2 * sizeof(double));
  p.per_pair = p.rspec + p.tspec + p.part + p.corr + p.energy;
  return p;
}

}  // namespace

int check_max_lag(const std::string& who, uint32_t max_lag) {
  if (max_lag < 1 || max_lag > kAlMaxLag)
    return fail(PEAQ_ERR_ARG, who + ": max_lag " + std::to_string(max_lag) + " is outside 1 .. " + std::to_string(kAlMaxLag));
  return PEAQ_OK;
}

struct AlignState {
  StageScratch scratch;
  LenStage lens;                // estimate: [n_ref | n_test]; cut: [skip | n_keep]
};

void align_release(peaq_ctx* c) { release_stage(c->al); }

extern "C" size_t peaq_align_workspace_bytes(int channels, int n_pairs, uint32_t n_max, uint32_t max_lag) {
  (void)channels;                                    // (the mono sum is taken while loading)
  if (n_pairs <= 0 || max_lag < 1 || max_lag > kAlMaxLag) return 0;
  return pair_groups(align_plan(n_max, max_lag).per_pair, n_pairs, kAlScratchBudget).bytes;
}

extern "C" void peaq_aligned_lengths(int32_t lag, uint32_t n_ref, uint32_t n_test, uint32_t* skip_ref,
                                     uint32_t* skip_test, uint32_t* n_common) {
  const uint64_t late = lag > 0 ? (uint64_t)lag : 0, early = lag < 0 ? (uint64_t)(-(int64_t)lag) : 0;
  const uint32_t sr = (uint32_t)std::min<uint64_t>(early, n_ref), st = (uint32_t)std::min<uint64_t>(late, n_test);
  if (skip_ref) *skip_ref = sr;
  if (skip_test) *skip_test = st;
  if (n_common) *n_common = std::min(n_ref - sr, n_test - st);
}

extern "C" int peaq_batch_estimate_delay(peaq_ctx* c, int channels, int n_pairs, const float* d_ref,
                                         const float* d_test, size_t pair_stride, const uint32_t* n_ref,
                                         const uint32_t* n_test, uint32_t n_uniform, uint32_t max_lag,
                                         peaq_delay* d_out, void* stream_) {
  const std::string who("peaq_batch_estimate_delay");
  // (what needs no context first)
  if (int rc = check_max_lag(who, max_lag)) return rc;
  if (int rc = check_shape(who, channels, n_pairs)) return rc;
  if (n_pairs > 0 && (!d_ref || !d_test || !d_out)) return fail(PEAQ_ERR_ARG, who + ": NULL buffer");
  if (!c) return fail(PEAQ_ERR_ARG, who + ": ctx is NULL");
  if (n_pairs == 0) return PEAQ_OK;
  if ((n_ref == nullptr) != (n_test == nullptr))
    return fail(PEAQ_ERR_ARG, who + ": n_ref and n_test must both be given or both be NULL");
  uint32_t nr_max = 0, nt_max = 0;
  if (int rc = check_lengths(who, n_pairs, n_ref, n_uniform, "n_ref", pair_stride, "pair_stride", &nr_max)) return rc;
  if (int rc = check_lengths(who, n_pairs, n_test, n_uniform, "n_test", pair_stride, "pair_stride", &nt_max)) return rc;
  const uint32_t n_max = std::max(nr_max, nt_max);
  std::vector<uint32_t> h;
  if (n_ref) {
    h.assign(n_ref, n_ref + n_pairs);
    h.insert(h.end(), n_test, n_test + n_pairs);
  }

  hipStream_t stream = static_cast<hipStream_t>(stream_);
  std::lock_guard<std::mutex> lock(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  if (!c->al) c->al = new AlignState;
  AlignState* st = c->al;
  const AlignPlan pl = align_plan(n_max, max_lag);
  const PairGroups pg = pair_groups(pl.per_pair, n_pairs, kAlScratchBudget);
  const int group = pg.group;
  if (int rc = st->scratch.acquire(pg.bytes, stream)) return rc;
  LenSlot* slot = nullptr;
  if (n_ref) {
    if (int rc = st->lens.upload(h.data(), h.size(), stream, &slot)) return rc;
  }
  char* base = st->scratch.buf.as<char>();
  AlignArgs a{};
  a.stride = pair_stride;
  a.n_uniform = n_uniform;
  a.channels = channels;
  a.D = max_lag;
  a.S = pl.S;
  a.NB = pl.NB;
  a.NT = pl.NT;
  a.NSEG = pl.NSEG;
  a.NCH = pl.NCH;
  a.ct = c->d_common;
  hipError_t launched = hipSuccess;
  for (int p0 = 0; p0 < n_pairs; p0 += group) {
    const unsigned np = (unsigned)std::min(group, n_pairs - p0);
    a.ref = d_ref + (size_t)p0 * pair_stride * channels;
    a.test = d_test + (size_t)p0 * pair_stride * channels;
    a.n_ref = slot ? slot->dev.as<uint32_t>() + p0 : nullptr;
    a.n_test = slot ? slot->dev.as<uint32_t>() + n_pairs + p0 : nullptr;
    a.out = d_out + p0;
    char* q = base;                                  // the group's arrays one after the other, each [np][...]
    a.rspec = reinterpret_cast<double2*>(q);
    q += (size_t)group * pl.rspec;
    a.tspec = reinterpret_cast<double2*>(q);
    q += (size_t)group * pl.tspec;
    a.part = reinterpret_cast<double2*>(q);
    q += (size_t)group * pl.part;
    a.corr = reinterpret_cast<double*>(q);
    q += (size_t)group * pl.corr;
    a.energy = reinterpret_cast<double*>(q);
    hipLaunchKernelGGL(align_spectra_kernel, dim3((pl.NT + 3) / 4, np), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(align_accumulate_kernel, dim3(2 * pl.NCH, np, pl.NSEG / kAlG), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(align_inverse_kernel, dim3((2 * pl.S + 3) / 4, np), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(align_pick_kernel, dim3(np), dim3(256), 0, stream, a);
    launched = hipGetLastError();
    if (launched != hipSuccess) break;
  }
  // (also after a failed launch: what was enqueued before it still reads the slot and the scratch)
  const hipError_t marked = st->scratch.mark(stream);
  const int sent = slot ? st->lens.sent(slot, stream) : PEAQ_OK;
  HIP_TRY(launched);
  HIP_TRY(marked);
  return sent;
}

extern "C" int peaq_batch_cut(peaq_ctx* c, int channels, int n_pairs, const float* d_in, size_t in_stride,
                              const uint32_t* skip, const uint32_t* n_keep, float* d_out, size_t out_stride,
                              void* stream_) {
  const std::string who("peaq_batch_cut");
  if (int rc = check_shape(who, channels, n_pairs)) return rc;
  if (n_pairs > 0 && (!skip || !n_keep)) return fail(PEAQ_ERR_ARG, who + ": NULL skip or n_keep");
  uint32_t keep_max = 0;
  if (int rc = check_cut_geometry(who, "pair", channels, n_pairs, n_pairs, d_in, in_stride, skip, n_keep, d_out, out_stride,
                                  &keep_max))
    return rc;
  if (!c) return fail(PEAQ_ERR_ARG, who + ": ctx is NULL");
  if (n_pairs == 0 || keep_max == 0) return PEAQ_OK;
  std::vector<uint32_t> h(skip, skip + n_pairs);
  h.insert(h.end(), n_keep, n_keep + n_pairs);

  hipStream_t stream = static_cast<hipStream_t>(stream_);
  std::lock_guard<std::mutex> lock(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  if (!c->al) c->al = new AlignState;
  LenSlot* slot = nullptr;
  if (int rc = c->al->lens.upload(h.data(), h.size(), stream, &slot)) return rc;
  CutArgs a{};
  a.in = d_in;
  a.out = d_out;
  a.in_stride = in_stride;
  a.out_stride = out_stride;
  a.skip = slot->dev.as<uint32_t>();
  a.n_keep = a.skip + n_pairs;
  a.channels = channels;
  const size_t vecs = ((size_t)keep_max * channels + 3) / 4;
  hipLaunchKernelGGL(align_cut_kernel, dim3((unsigned)((vecs + 255) / 256), (unsigned)n_pairs), dim3(256), 0, stream, a);
  const hipError_t launched = hipGetLastError();
  const int sent = c->al->lens.sent(slot, stream);   // (also after a failed launch: the copy into the slot is enqueued)
  HIP_TRY(launched);
  return sent;
}

// ---------------------------------------------------------------------------
// the steps of the one-pair conveniences (peaq_host.h)
// ---------------------------------------------------------------------------
int check_pair_args(const std::string& who, const peaq_ctx* c, int channels, uint32_t rate, const float* ref,
                    size_t n_ref, const float* test, size_t n_test, const void* out, bool need_out) {
  if (int rc = check_channels(who, channels)) return rc;
  if (rate != 48000 && !peaq_resample_supported(rate))
    return fail(PEAQ_ERR_ARG, who + ": rate " + std::to_string(rate) + " Hz is not supported on the device");
  if (!c) return fail(PEAQ_ERR_ARG, who + ": NULL argument: ctx is NULL");
  if (need_out && !out) return fail(PEAQ_ERR_ARG, who + ": NULL argument: out is NULL");
  if ((n_ref && !ref) || (n_test && !test)) return fail(PEAQ_ERR_ARG, who + ": NULL samples");
  if (n_ref > 0xFFFFFFFFu || n_test > 0xFFFFFFFFu) return fail(PEAQ_ERR_ARG, who + ": more than 2^32 samples");
  return PEAQ_OK;
}

int upload_pair_48k(peaq_ctx* c, int channels, uint32_t rate, const float* ref, size_t n_ref, const float* test,
                    size_t n_test, PairBuffers& pb) {
  const size_t n[2] = {n_ref, n_test};
  const float* src[2] = {ref, test};
  for (int i = 0; i < 2; ++i) {
    pb.len[i] = (uint32_t)n[i];
    if (rate != 48000) {
      pb.len[i] = peaq_resampled_length(n[i], rate);
      if (n[i] && !pb.len[i]) return PEAQ_ERR_ARG;   // (the message is peaq_resampled_length's)
    }
  }
  HIP_TRY(hipSetDevice(c->device));
  pb.stride = std::max<size_t>(std::max(pb.len[0], pb.len[1]), 2);
  pb.stride += pb.stride & 1;                        // 8-byte rows, as in peaq_run_pair
  const size_t bytes = pb.stride * channels * sizeof(float);
  for (int i = 0; i < 2; ++i) {
    HIP_TRY(pb.s48[i].reserve(bytes));
    HIP_TRY(hipMemset(pb.s48[i].p, 0, bytes));
    if (!n[i]) continue;
    if (rate == 48000) {
      HIP_TRY(hipMemcpy(pb.s48[i].p, src[i], n[i] * channels * sizeof(float), hipMemcpyHostToDevice));
      continue;
    }
    HIP_TRY(pb.raw[i].reserve(n[i] * channels * sizeof(float)));
    HIP_TRY(hipMemcpy(pb.raw[i].p, src[i], n[i] * channels * sizeof(float), hipMemcpyHostToDevice));
    if (int rc = peaq_batch_resample(c, channels, rate, 1, pb.raw[i].as<float>(), n[i], nullptr, (uint32_t)n[i],
                                     pb.s48[i].as<float>(), pb.stride, nullptr, nullptr))
      return rc;
  }
  HIP_TRY(hipDeviceSynchronize());
  return PEAQ_OK;
}

int estimate_one_delay(peaq_ctx* c, int channels, const PairBuffers& pb, uint32_t max_lag, peaq_delay* rec) {
  DevBuf d_rec;
  HIP_TRY(d_rec.reserve(sizeof(peaq_delay)));
  if (int rc = peaq_batch_estimate_delay(c, channels, 1, pb.d(0), pb.d(1), pb.stride, pb.len, pb.len + 1, 0, max_lag,
                                         d_rec.as<peaq_delay>(), nullptr))
    return rc;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(rec, d_rec.p, sizeof *rec, hipMemcpyDeviceToHost));
  return PEAQ_OK;
}

int score_one_pair(peaq_ctx* c, int advanced, int channels, double level_db, const float* d_ref, const float* d_test,
                   size_t stride, uint32_t len_ref, uint32_t len_test, peaq_result* out) {
  DevBuf d_res;
  HIP_TRY(d_res.reserve(sizeof(peaq_result)));
  if (int rc = peaq_batch_run(c, advanced, channels, level_db, 1, d_ref, d_test, stride, &len_ref, &len_test, 0,
                              d_res.as<peaq_result>(), nullptr))
    return rc;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, d_res.p, sizeof(peaq_result), hipMemcpyDeviceToHost));
  return PEAQ_OK;
}

int begin_delay_pair(const std::string& who, peaq_ctx* c, int channels, double level_db, uint32_t rate, uint32_t max_lag,
                     uint32_t window, int mode, double max_gain_db, const float* ref, size_t n_ref, const float* test,
                     size_t n_test, peaq_delay* delay, peaq_gain* gain, const void* out, PairBuffers& in, peaq_delay* rec,
                     uint32_t* W) {
  if (int rc = check_gain_mode(who, mode, max_gain_db)) return rc;
  if (int rc = check_max_lag(who, max_lag)) return rc;
  if (int rc = check_level(who, level_db)) return rc;
  if (int rc = check_pair_args(who, c, channels, rate, ref, n_ref, test, n_test, out, true)) return rc;
  if (gain) std::memset(gain, 0, sizeof *gain);
  // 1, 2: upload, rate conversion
  if (int rc = upload_pair_48k(c, channels, rate, ref, n_ref, test, n_test, in)) return rc;
  // 3: estimate
  if (int rc = estimate_one_delay(c, channels, in, max_lag, rec)) return rc;
  if (delay) *delay = *rec;
  if (!window) return PEAQ_OK;
  *W = peaq_drift_windows(rec->lag, in.len[0], in.len[1], window);
  if (*W > PEAQ_DRIFT_MAX_WINDOWS)
    return fail(PEAQ_ERR_ARG, who + ": " + std::to_string(*W) + " windows of " + std::to_string(window) + " samples are more than " +
                                  std::to_string(PEAQ_DRIFT_MAX_WINDOWS) + ": take a longer window");
  return PEAQ_OK;
}

int score_cut_pair(peaq_ctx* c, int advanced, int channels, double level_db, const PairBuffers& in, const uint32_t skip[2],
                   uint32_t keep, int mode, double max_gain_db, peaq_gain* gain,
                   const std::function<int(float* d_out, size_t out_stride)>& cut_test, peaq_result* out) {
  // 5, 6: plain cut of the reference, the stage's cut of the test signal
  DevBuf cut[2], matched, d_gain;
  size_t cstride = std::max<size_t>(keep, 2);
  cstride += cstride & 1;
  const size_t cbytes = cstride * channels * sizeof(float);
  for (int i = 0; i < 2; ++i) {
    HIP_TRY(cut[i].reserve(cbytes));
    HIP_TRY(hipMemset(cut[i].p, 0, cbytes));
  }
  if (int rc = peaq_batch_cut(c, channels, 1, in.d(0), in.stride, &skip[0], &keep, cut[0].as<float>(), cstride, nullptr)) return rc;
  if (int rc = cut_test(cut[1].as<float>(), cstride)) return rc;
  const float* scored = cut[1].as<float>();
  // 7: the gain of the CUT test signal, applied into a second buffer
  const bool match = (mode & 0xF) != PEAQ_GAIN_OFF;
  if (match) {
    const uint32_t zero = 0;
    HIP_TRY(d_gain.reserve(sizeof(peaq_gain)));
    HIP_TRY(matched.reserve(cbytes));
    HIP_TRY(hipMemset(matched.p, 0, cbytes));
    if (int rc = peaq_batch_measure_gain(c, channels, 1, cut[0].as<float>(), cstride, &zero, cut[1].as<float>(), cstride, &zero,
                                         &keep, mode, max_gain_db, d_gain.as<peaq_gain>(), nullptr))
      return rc;
    if (int rc = peaq_batch_cut_scaled(c, channels, 1, cut[1].as<float>(), cstride, &zero, &keep, d_gain.as<peaq_gain>(),
                                       matched.as<float>(), cstride, nullptr))
      return rc;
    scored = matched.as<float>();
  }
  HIP_TRY(hipDeviceSynchronize());
  if (match && gain) HIP_TRY(hipMemcpy(gain, d_gain.p, sizeof(peaq_gain), hipMemcpyDeviceToHost));
  // 8: the one-pair path
  return score_one_pair(c, advanced, channels, level_db, cut[0].as<float>(), scored, cstride, keep, keep, out);
}

// What peaq_run_pair_aligned, _matched and _trace score: the pair at 48 kHz as it is (neither max_lag nor a gain
// mode), or the two signals cut to their common part -- from the estimated lag with max_lag, from 0 without -- with
// the gain, where a mode other than PEAQ_GAIN_OFF asks for one, measured over that part of the uncut buffers and
// applied in the test signal's cut.  d[0], d[1]: `stride` samples per channel long, len[] their lengths.
struct ScoredPair {
  PairBuffers in;
  DevBuf cut[2], grec;
  const float* d[2] = {nullptr, nullptr};
  size_t stride = 0;
  uint32_t len[2] = {0, 0};
};
static int prepare_pair(peaq_ctx* c, int channels, uint32_t rate, uint32_t max_lag, int gain_mode, double max_gain_db,
                        const float* ref, size_t n_ref, const float* test, size_t n_test, peaq_delay* delay,
                        peaq_gain* gain, ScoredPair& sp) {
  const bool match = (gain_mode & 0xF) != PEAQ_GAIN_OFF;
  if (int rc = upload_pair_48k(c, channels, rate, ref, n_ref, test, n_test, sp.in)) return rc;
  const PairBuffers& in = sp.in;
  peaq_delay rec;
  std::memset(&rec, 0, sizeof rec);
  if (max_lag)
    if (int rc = estimate_one_delay(c, channels, in, max_lag, &rec)) return rc;
  if (delay) *delay = rec;
  if (!max_lag && !match) {                          // the signals as they are
    for (int i = 0; i < 2; ++i) {
      sp.d[i] = in.d(i);
      sp.len[i] = in.len[i];
    }
    sp.stride = in.stride;
    return PEAQ_OK;
  }
  uint32_t skip[2], common = 0;
  peaq_aligned_lengths(rec.lag, in.len[0], in.len[1], &skip[0], &skip[1], &common);
  size_t cstride = std::max<size_t>(common, 2);
  cstride += cstride & 1;
  const size_t cbytes = cstride * channels * sizeof(float);
  if (match) {
    HIP_TRY(sp.grec.reserve(sizeof(peaq_gain)));
    if (int rc = peaq_batch_measure_gain(c, channels, 1, in.d(0), in.stride, &skip[0], in.d(1), in.stride, &skip[1], &common,
                                         gain_mode, max_gain_db, sp.grec.as<peaq_gain>(), nullptr))
      return rc;
  }
  for (int i = 0; i < 2; ++i) {
    HIP_TRY(sp.cut[i].reserve(cbytes));
    HIP_TRY(hipMemset(sp.cut[i].p, 0, cbytes));
    if (int rc = match && i == 1
                     ? peaq_batch_cut_scaled(c, channels, 1, in.d(i), in.stride, &skip[i], &common, sp.grec.as<peaq_gain>(),
                                             sp.cut[i].as<float>(), cstride, nullptr)
                     : peaq_batch_cut(c, channels, 1, in.d(i), in.stride, &skip[i], &common, sp.cut[i].as<float>(), cstride,
                                      nullptr))
      return rc;
    sp.d[i] = sp.cut[i].as<float>();
    sp.len[i] = common;
  }
  HIP_TRY(hipDeviceSynchronize());
  if (match && gain) HIP_TRY(hipMemcpy(gain, sp.grec.p, sizeof(peaq_gain), hipMemcpyDeviceToHost));
  sp.stride = cstride;
  return PEAQ_OK;
}

extern "C" int peaq_run_pair_aligned(peaq_ctx* c, int advanced, int channels, double level_db, uint32_t rate,
                                     uint32_t max_lag, const float* ref, size_t n_ref, const float* test, size_t n_test,
                                     peaq_delay* delay, peaq_result* out) {
  const std::string who("peaq_run_pair_aligned");
  if (int rc = check_max_lag(who, max_lag)) return rc;
  if (int rc = check_level(who, level_db)) return rc;
  if (int rc = check_pair_args(who, c, channels, rate, ref, n_ref, test, n_test, out, true)) return rc;
  ScoredPair sp;
  if (int rc = prepare_pair(c, channels, rate, max_lag, PEAQ_GAIN_OFF, 0., ref, n_ref, test, n_test, delay, nullptr, sp))
    return rc;
  return score_one_pair(c, advanced, channels, level_db, sp.d[0], sp.d[1], sp.stride, sp.len[0], sp.len[1], out);
}

extern "C" int peaq_run_pair_matched(peaq_ctx* c, int advanced, int channels, double level_db, uint32_t rate,
                                     uint32_t max_lag, int mode, double max_gain_db, const float* ref, size_t n_ref,
                                     const float* test, size_t n_test, peaq_delay* delay, peaq_gain* gain, peaq_result* out) {
  const std::string who("peaq_run_pair_matched");
  if (int rc = check_gain_mode(who, mode, max_gain_db)) return rc;
  if (max_lag)
    if (int rc = check_max_lag(who, max_lag)) return rc;
  if (int rc = check_level(who, level_db)) return rc;
  if (int rc = check_pair_args(who, c, channels, rate, ref, n_ref, test, n_test, out, true)) return rc;
  if (gain) std::memset(gain, 0, sizeof *gain);
  ScoredPair sp;
  if (int rc = prepare_pair(c, channels, rate, max_lag, mode, max_gain_db, ref, n_ref, test, n_test, delay, gain, sp))
    return rc;
  return score_one_pair(c, advanced, channels, level_db, sp.d[0], sp.d[1], sp.stride, sp.len[0], sp.len[1], out);
}

// ---- the one-pair forms of the batch run's optional outputs ---------------------------------------------------------
// One array of such an output: a record per FFT frame, per filter-bank block or one per pair, `bytes` each, copied into
// the caller's `host` array of `cap` records (`cap_name` in the message when the pair has more); kNone: this run does
// not write the array.  run_pair_output fills in `n` and `dev`.
namespace {
struct PairRows {
  enum Per { kNone, kFrame, kBlock, kPair } per;
  size_t bytes;
  void* host;
  size_t cap;
  const char* cap_name;
  uint32_t* n_out;              // the count for the caller, or nullptr
  uint32_t n = 0;
  DevBuf dev;
};
}  // namespace

// What the six entries below share, after their own arguments: max_lag, the level and the pair are checked, the pair
// is prepared as peaq_run_pair_aligned's, each array's count is held against the caller's capacity, `run` -- the
// entry's batch call, with the pair and a device result -- fills the device arrays, and everything is copied back.
template <class Run>
static int run_pair_output(const std::string& w, peaq_ctx* c, int channels, double level_db, uint32_t rate,
                           uint32_t max_lag, const float* ref, size_t n_ref, const float* test, size_t n_test,
                           peaq_delay* delay, peaq_result* out, PairRows* rows, int n_rows, Run run) {
  if (max_lag)
    if (int rc = check_max_lag(w, max_lag)) return rc;
  if (int rc = check_level(w, level_db)) return rc;
  if (int rc = check_pair_args(w, c, channels, rate, ref, n_ref, test, n_test, out, false)) return rc;
  ScoredPair pp;
  if (int rc = prepare_pair(c, channels, rate, max_lag, PEAQ_GAIN_OFF, 0., ref, n_ref, test, n_test, delay, nullptr, pp))
    return rc;
  for (PairRows* r = rows; r < rows + n_rows; ++r) {
    const bool blocks = r->per == PairRows::kBlock;
    r->n = r->per == PairRows::kNone ? 0 : r->per == PairRows::kPair ? 1 : peaq_frame_count(pp.len[0], pp.len[1], blocks);
    if (r->n > r->cap)
      return fail(PEAQ_ERR_ARG, w + ": " + r->cap_name + " " + std::to_string(r->cap) + " is below the pair's " +
                                    std::to_string(r->n) + (blocks ? " blocks" : " frames"));
  }
  DevBuf d_res;
  HIP_TRY(d_res.reserve(sizeof(peaq_result)));
  for (PairRows* r = rows; r < rows + n_rows; ++r)
    if (r->per != PairRows::kNone) HIP_TRY(r->dev.reserve(std::max<size_t>(r->n, 1) * r->bytes));
  if (int rc = run(pp, d_res.as<peaq_result>())) return rc;
  HIP_TRY(hipDeviceSynchronize());
  for (PairRows* r = rows; r < rows + n_rows; ++r)
    if (r->n) HIP_TRY(hipMemcpy(r->host, r->dev.p, (size_t)r->n * r->bytes, hipMemcpyDeviceToHost));
  if (out) HIP_TRY(hipMemcpy(out, d_res.p, sizeof(peaq_result), hipMemcpyDeviceToHost));
  for (PairRows* r = rows; r < rows + n_rows; ++r)
    if (r->n_out) *r->n_out = r->n;
  return PEAQ_OK;
}

extern "C" int peaq_run_pair_trace(peaq_ctx* c, int advanced, int channels, double level_db, uint32_t rate,
                                   uint32_t max_lag, const float* ref, size_t n_ref, const float* test, size_t n_test,
                                   peaq_frame_trace* frames, size_t frame_cap, uint32_t* n_frames,
                                   peaq_block_trace* blocks, size_t block_cap, uint32_t* n_blocks, peaq_delay* delay,
                                   peaq_result* out) {
  const std::string w("peaq_run_pair_trace");
  if (!frames) return fail(PEAQ_ERR_ARG, w + ": frames is NULL");
  if (advanced && !blocks) return fail(PEAQ_ERR_ARG, w + ": blocks is NULL (the advanced version writes block records)");
  if (!advanced && blocks) return fail(PEAQ_ERR_ARG, w + ": blocks must be NULL in the basic version (it has no filter-bank blocks)");
  PairRows rows[2] = {
      {PairRows::kFrame, sizeof(peaq_frame_trace), frames, frame_cap, "frame_cap", n_frames},
      {advanced ? PairRows::kBlock : PairRows::kNone, sizeof(peaq_block_trace), blocks, block_cap, "block_cap", n_blocks}};
  return run_pair_output(w, c, channels, level_db, rate, max_lag, ref, n_ref, test, n_test, delay, out, rows, 2,
                         [&](const ScoredPair& pp, peaq_result* d_res) {
                           return peaq_batch_run_trace(c, advanced, channels, level_db, 1, pp.d[0], pp.d[1], pp.stride,
                                                       pp.len, pp.len + 1, 0, rows[0].dev.as<peaq_frame_trace>(),
                                                       rows[0].n, rows[1].dev.as<peaq_block_trace>(), rows[1].n, d_res,
                                                       nullptr);
                         });
}

extern "C" int peaq_run_pair_bands(peaq_ctx* c, int advanced, int channels, double level_db, uint32_t rate,
                                   uint32_t max_lag, const float* ref, size_t n_ref, const float* test, size_t n_test,
                                   uint32_t planes, double* bands, size_t frame_cap, uint32_t* n_frames,
                                   peaq_delay* delay, peaq_result* out) {
  const std::string w("peaq_run_pair_bands");
  if (int rc = check_band_planes(w, advanced, planes)) return rc;
  if (!bands) return fail(PEAQ_ERR_ARG, w + ": bands is NULL");
  const size_t frame_bytes = (size_t)channels * __builtin_popcount(planes) * peaq_band_row(advanced) * sizeof(double);
  PairRows rows[1] = {{PairRows::kFrame, frame_bytes, bands, frame_cap, "frame_cap", n_frames}};
  return run_pair_output(w, c, channels, level_db, rate, max_lag, ref, n_ref, test, n_test, delay, out, rows, 1,
                         [&](const ScoredPair& pp, peaq_result* d_res) {
                           return peaq_batch_run_bands(c, advanced, channels, level_db, 1, pp.d[0], pp.d[1], pp.stride,
                                                       pp.len, pp.len + 1, 0, planes, rows[0].dev.as<double>(),
                                                       rows[0].n, d_res, nullptr);
                         });
}

extern "C" int peaq_run_pair_fb_bands(peaq_ctx* c, int channels, double level_db, uint32_t rate, uint32_t max_lag,
                                      const float* ref, size_t n_ref, const float* test, size_t n_test, uint32_t planes,
                                      double* bands, size_t block_cap, uint32_t* n_blocks, peaq_delay* delay,
                                      peaq_result* out) {
  const std::string w("peaq_run_pair_fb_bands");
  if (int rc = check_fb_band_planes(w, planes)) return rc;
  if (!bands) return fail(PEAQ_ERR_ARG, w + ": bands is NULL");
  const size_t block_bytes = (size_t)channels * __builtin_popcount(planes) * peaq_fb_band_count() * sizeof(double);
  PairRows rows[1] = {{PairRows::kBlock, block_bytes, bands, block_cap, "block_cap", n_blocks}};
  return run_pair_output(w, c, channels, level_db, rate, max_lag, ref, n_ref, test, n_test, delay, out, rows, 1,
                         [&](const ScoredPair& pp, peaq_result* d_res) {
                           return peaq_batch_run_fb_bands(c, channels, level_db, 1, pp.d[0], pp.d[1], pp.stride, pp.len,
                                                          pp.len + 1, 0, planes, rows[0].dev.as<double>(), rows[0].n,
                                                          d_res, nullptr);
                         });
}

extern "C" int peaq_run_pair_pattern_bands(peaq_ctx* c, int channels, double level_db, uint32_t rate, uint32_t max_lag,
                                           const float* ref, size_t n_ref, const float* test, size_t n_test,
                                           uint32_t planes, double* bands, size_t frame_cap, uint32_t* n_frames,
                                           peaq_delay* delay, peaq_result* out) {
  const std::string w("peaq_run_pair_pattern_bands");
  if (int rc = check_pattern_band_planes(w, planes)) return rc;
  if (!bands) return fail(PEAQ_ERR_ARG, w + ": bands is NULL");
  const size_t frame_bytes = (size_t)channels * __builtin_popcount(planes) * peaq_band_row(0) * sizeof(double);
  PairRows rows[1] = {{PairRows::kFrame, frame_bytes, bands, frame_cap, "frame_cap", n_frames}};
  return run_pair_output(w, c, channels, level_db, rate, max_lag, ref, n_ref, test, n_test, delay, out, rows, 1,
                         [&](const ScoredPair& pp, peaq_result* d_res) {
                           return peaq_batch_run_pattern_bands(c, channels, level_db, 1, pp.d[0], pp.d[1], pp.stride,
                                                               pp.len, pp.len + 1, 0, planes, rows[0].dev.as<double>(),
                                                               rows[0].n, d_res, nullptr);
                         });
}

// (one record per pair: neither a count nor a capacity of the caller's)
extern "C" int peaq_run_pair_band_summary(peaq_ctx* c, int advanced, int channels, double level_db, uint32_t rate,
                                          uint32_t max_lag, const float* ref, size_t n_ref, const float* test,
                                          size_t n_test, double* summary, peaq_delay* delay, peaq_result* out) {
  const std::string w("peaq_run_pair_band_summary");
  if (!summary) return fail(PEAQ_ERR_ARG, w + ": summary is NULL");
  const size_t bytes =
      (size_t)channels * peaq_band_summary_rows(advanced) * peaq_band_row(advanced) * sizeof(double);
  PairRows rows[1] = {{PairRows::kPair, bytes, summary, 1, "", nullptr}};
  return run_pair_output(w, c, channels, level_db, rate, max_lag, ref, n_ref, test, n_test, delay, out, rows, 1,
                         [&](const ScoredPair& pp, peaq_result* d_res) {
                           return peaq_batch_run_band_summary(c, advanced, channels, level_db, 1, pp.d[0], pp.d[1],
                                                              pp.stride, pp.len, pp.len + 1, 0, rows[0].dev.as<double>(),
                                                              d_res, nullptr);
                         });
}

extern "C" int peaq_run_pair_fb_band_summary(peaq_ctx* c, int channels, double level_db, uint32_t rate, uint32_t max_lag,
                                             const float* ref, size_t n_ref, const float* test, size_t n_test,
                                             double* summary, peaq_delay* delay, peaq_result* out) {
  const std::string w("peaq_run_pair_fb_band_summary");
  if (!summary) return fail(PEAQ_ERR_ARG, w + ": summary is NULL");
  const size_t bytes = (size_t)channels * peaq_fb_band_summary_rows() * peaq_fb_band_summary_row() * sizeof(double);
  PairRows rows[1] = {{PairRows::kPair, bytes, summary, 1, "", nullptr}};
  return run_pair_output(w, c, channels, level_db, rate, max_lag, ref, n_ref, test, n_test, delay, out, rows, 1,
                         [&](const ScoredPair& pp, peaq_result* d_res) {
                           return peaq_batch_run_fb_band_summary(c, channels, level_db, 1, pp.d[0], pp.d[1], pp.stride,
                                                                 pp.len, pp.len + 1, 0, rows[0].dev.as<double>(), d_res,
                                                                 nullptr);
                         });
}

// (n_windows records per pair: neither a count nor a capacity of the caller's)
extern "C" int peaq_run_pair_windows(peaq_ctx* c, int channels, double level_db, uint32_t rate, uint32_t max_lag,
                                     const float* ref, size_t n_ref, const float* test, size_t n_test,
                                     const peaq_window* windows, int n_windows, peaq_result* out_windows,
                                     peaq_delay* delay, peaq_result* out) {
  const std::string w("peaq_run_pair_windows");
  if (int rc = check_span_list(w, "windows", "window", windows, n_windows, "out_windows", out_windows)) return rc;
  PairRows rows[1] = {{PairRows::kPair, (size_t)n_windows * sizeof(peaq_result), out_windows, 1, "", nullptr}};
  return run_pair_output(w, c, channels, level_db, rate, max_lag, ref, n_ref, test, n_test, delay, out, rows, 1,
                         [&](const ScoredPair& pp, peaq_result* d_res) {
                           return peaq_batch_run_windows(c, channels, level_db, 1, pp.d[0], pp.d[1], pp.stride, pp.len,
                                                         pp.len + 1, 0, windows, n_windows,
                                                         rows[0].dev.as<peaq_result>(), d_res, nullptr);
                         });
}

// (n_spans records per pair, as above; the advanced version)
extern "C" int peaq_run_pair_adv_spans(peaq_ctx* c, int channels, double level_db, uint32_t rate, uint32_t max_lag,
                                       const float* ref, size_t n_ref, const float* test, size_t n_test,
                                       const peaq_window* spans, int n_spans, peaq_result* out_spans, peaq_delay* delay,
                                       peaq_result* out) {
  const std::string w("peaq_run_pair_adv_spans");
  if (int rc = check_span_list(w, "spans", "span", spans, n_spans, "out_spans", out_spans)) return rc;
  PairRows rows[1] = {{PairRows::kPair, (size_t)n_spans * sizeof(peaq_result), out_spans, 1, "", nullptr}};
  return run_pair_output(w, c, channels, level_db, rate, max_lag, ref, n_ref, test, n_test, delay, out, rows, 1,
                         [&](const ScoredPair& pp, peaq_result* d_res) {
                           return peaq_batch_run_adv_spans(c, channels, level_db, 1, pp.d[0], pp.d[1], pp.stride, pp.len,
                                                           pp.len + 1, 0, spans, n_spans, rows[0].dev.as<peaq_result>(),
                                                           d_res, nullptr);
                         });
}

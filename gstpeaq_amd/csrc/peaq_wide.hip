// peaq_wide.hip -- delays of seconds, coarse to fine: both signals decimated by a power of two M, the aligner on the
// decimated copies, the cut by the coarse lag, the aligner again on the cut pair (peaq_wide_factor, peaq_wide_taps,
// peaq_batch_decimate, peaq_batch_estimate_delay_wide, peaq_wide_workspace_bytes, peaq_run_pair_wide;
// include/peaq_amd.h).
//
//   wide_decimate_kernel   peaq_batch_decimate: a workgroup owns PEAQ_WIDE_CHUNK = 248 consecutive outputs of one pair and
//       takes them in passes of P = 248, 124 or 62 (M <= 16, 32, 64): what fits 40 KB of LDS.  A pass stages the
//       (P + 16) M + 1 samples from (k - 8) M on, k the pass's first output, as FP64: the mono sum (its magnitude in
//       envelope mode) is formed on the way in, absent samples are zeros.  Loads are 16 bytes, four of them in flight
//       per lane, where the pair's row starts on 16 bytes and the pass lies inside the signal (two stereo samples, four
//       mono ones; the first staged sample is a multiple of 4), else dwords.  The tile is stored BY PHASE: staged sample t at tile[(t mod M) row + t / M], row = P + 17 (odd).  Lane o
//       owns output k + o and walks the taps in ascending order; tap j of it reads staged sample o M + j, which is
//       tile[(j mod M) row + j / M + o]: at every step the lanes of a wave read CONSECUTIVE doubles, and the tap is one
//       value for the whole wave (a scalar load).  One chain of fused multiply-adds per output, as the definition has
//       it; taps and samples are fetched four at a time, a block ahead of the multiply-adds that use them.  Waveform mode stores the float; envelope mode stores y in FP64 to the stage's scratch.
//   wide_center_kernel     envelope mode: one workgroup per pair sums the pair's y (a lane every 256th, then
//       block_sum4), divides by n_dec and stores (float) (y - m).
//   No other kernel: the estimate runs the aligner's kernels on the decimated copies and on the cut pair.
#include "peaq_host.h"

namespace {

constexpr int kWdChunk = PEAQ_WIDE_CHUNK;              // outputs per workgroup
constexpr int kWdHalf = 8;                             // the filter reaches 8 M samples each side
constexpr int kWdLds = 5056;                           // doubles: 64 rows of 62 + 17 (M = 64), 39.5 KB
constexpr int kWdBlock = 4;                            // taps fetched together, a block ahead of the multiply-adds that use them
constexpr size_t kWdRowsBudget = (size_t)256 << 20;    // envelope mode: pairs are taken in groups whose FP64 rows stay below this
constexpr size_t kWdStagingBudget = (size_t)1 << 30;   // estimate: ... whose cut and decimated copies stay below this
static_assert(kWdChunk % 4 == 0 && kWdChunk <= 256, "a pass starts on a multiple of 4 samples; a lane per output");

// outputs per pass: the whole chunk up to M = 16, a half at 32, a quarter at 64
constexpr int wide_pass(uint32_t M) { return M <= 16 ? kWdChunk : M == 32 ? kWdChunk / 2 : kWdChunk / 4; }
static_assert(16 * (wide_pass(16) + 17) <= kWdLds && 32 * (wide_pass(32) + 17) <= kWdLds &&
              64 * (wide_pass(64) + 17) <= kWdLds, "the tile of every factor fits");
static_assert(wide_pass(16) % 2 == 0 && wide_pass(32) % 2 == 0 && wide_pass(64) % 2 == 0, "rows of an odd length");
struct WideArgs {
  size_t in_stride, out_stride, y_stride;  // samples per channel (outputs) between pairs
  const uint32_t* n_in;         // device [n_pairs], or nullptr
  double* y;                    // envelope mode: device [n_pairs][y_stride]
  uint32_t n_uniform;
  uint32_t M, log_m, P, row;
  int channels;
};

__device__ __forceinline__ unsigned long long wide_n_dec(const WideArgs& a, unsigned pair) {
  const unsigned long long n = a.n_in ? a.n_in[pair] : a.n_uniform;
  return (n + a.M - 1) >> a.log_m;
}

// The sum of staged sample t, formed and stored by phase
template <int MODE, int C>
__device__ __forceinline__ void wide_store(const WideArgs& a, double* tile, int t, float l, float r) {
  double s = (double)l;
  if (C == 2) s += (double)r;
  if (MODE == PEAQ_WIDE_ENVELOPE) s = __builtin_fabs(s);
  tile[(t & ((int)a.M - 1)) * (int)a.row + (t >> a.log_m)] = s;
}

// A pass's samples into the tile, staged sample t being input sample b + t of the row.  A thread's 16-byte units are
// t0 = U (thread + 256 it), U = 2 stereo or 4 mono samples each.
// inside (uniform): the row lies on 16 bytes and every staged sample is in the signal -- every pass but a pair's first and
// last.  The loop is then free of branches and unrolled by four, so that four loads per lane are in flight (one at a time
// leaves the memory system idle).  Otherwise a sample at a time, absent samples as zeros.
template <int MODE, int C>
__device__ __forceinline__ void wide_stage(const WideArgs& a, const float* __restrict__ src, bool inside, long long n,
                                           long long b, int total, double* tile) {
  constexpr int U = 4 / C;                             // samples of 16 bytes
  if (inside) {
#pragma unroll 4
    for (int t0 = U * (int)threadIdx.x; t0 < total - 1; t0 += U * 256) {   // whole units: total - 1 is a multiple of 4
      const float4 x = *reinterpret_cast<const float4*>(src + (size_t)(b + t0) * C);
      const float f[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int e = 0; e < U; ++e) wide_store<MODE, C>(a, tile, t0 + e, f[C * e], f[C * e + C - 1]);
    }
    if (threadIdx.x == 0) {                            // ... and the last sample
      const float* last = src + (size_t)(b + total - 1) * C;
      wide_store<MODE, C>(a, tile, total - 1, last[0], last[C - 1]);
    }
    return;
  }
  for (int t = threadIdx.x; t < total; t += 256) {
    const long long i = b + t;
    float l = 0.f, r = 0.f;
    if (i >= 0 && i < n) {
      l = src[(size_t)i * C];
      if (C == 2) r = src[(size_t)i * C + 1];
    }
    wide_store<MODE, C>(a, tile, t, l, r);
  }
}

// (the buffers and the taps, device [16 M + 1], as parameters of their own, as frac_cut_kernel's: the taps are then scalar loads)
template <int MODE>
__global__ __launch_bounds__(256, 4) void wide_decimate_kernel(const WideArgs a, const float* __restrict__ a_in,
                                                              float* __restrict__ a_out, const double* __restrict__ h) {
  __shared__ __attribute__((aligned(16))) double tile[kWdLds];
  const unsigned pair = blockIdx.y;
  const long long n = a.n_in ? a.n_in[pair] : a.n_uniform;
  const unsigned long long n_dec = wide_n_dec(a, pair);
  const unsigned long long k0 = (unsigned long long)blockIdx.x * kWdChunk;
  if (k0 >= n_dec) return;                             // (the whole workgroup)
  const float* __restrict__ src = a_in + (size_t)pair * a.in_stride * a.channels;
  const bool vec = ((uintptr_t)src & 15) == 0;         // (uniform) every unit of the row lies on 16 bytes
  const int P = (int)a.P, M = (int)a.M;
  const int total = ((P + 2 * kWdHalf) << a.log_m) + 1;
  const int n_taps = 2 * kWdHalf * M;                  // ... and the last one
  for (int pass = 0; pass * P < kWdChunk; ++pass) {
    const unsigned long long kp = k0 + (unsigned long long)(pass * P);
    if (kp >= n_dec) break;                            // (uniform)
    const long long b = ((long long)kp - kWdHalf) * M; // the input sample under staged sample 0
    if (pass) __syncthreads();                         // the previous pass has read its tile
    const bool inside = vec && b >= 0 && b + total <= n;       // (uniform)
    if (a.channels == 2)
      wide_stage<MODE, 2>(a, src, inside, n, b, total, tile);
    else
      wide_stage<MODE, 1>(a, src, inside, n, b, total, tile);
    __syncthreads();
    const int o = threadIdx.x;
    if (o < P && kp + o < n_dec) {
      const double* col = tile + o;
      double acc = 0.;
      // j = -8M .. 8M - 1 of the definition, in that order, two blocks of kB taps in turn: while one's multiply-adds
      // run, the other's taps and samples are on their way (16 M is a multiple of 2 kB); the scheduling barriers keep
      // the compiler from sinking the fetches behind the multiply-adds
      constexpr int kB = kWdBlock;
      double ha[kB], ua[kB], hb[kB], ub[kB];
#pragma unroll
      for (int q = 0; q < kB; ++q) {
        ha[q] = h[q];
        ua[q] = col[(q & (M - 1)) * (int)a.row + (q >> a.log_m)];
      }
      for (int j0 = 0; j0 < n_taps; j0 += 2 * kB) {
        const int jb = j0 + kB;
#pragma unroll
        for (int q = 0; q < kB; ++q) {
          hb[q] = h[jb + q];
          ub[q] = col[((jb + q) & (M - 1)) * (int)a.row + ((jb + q) >> a.log_m)];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < kB; ++q) acc = __builtin_fma(ha[q], ua[q], acc);
        __builtin_amdgcn_sched_barrier(0);
        const int ja = j0 + 2 * kB < n_taps ? j0 + 2 * kB : 0;   // (behind the last block: fetched again, not used)
#pragma unroll
        for (int q = 0; q < kB; ++q) {
          ha[q] = h[ja + q];
          ua[q] = col[((ja + q) & (M - 1)) * (int)a.row + ((ja + q) >> a.log_m)];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < kB; ++q) acc = __builtin_fma(hb[q], ub[q], acc);
        __builtin_amdgcn_sched_barrier(0);
      }
      acc = __builtin_fma(h[n_taps], col[2 * kWdHalf], acc);
      if (MODE == PEAQ_WIDE_ENVELOPE)
        a.y[(size_t)pair * a.y_stride + kp + o] = acc;
      else
        a_out[(size_t)pair * a.out_stride + kp + o] = (float)acc;
    }
  }
}

__global__ __launch_bounds__(256, 4) void wide_center_kernel(const WideArgs a, float* __restrict__ a_out) {
  __shared__ double sh[4][1];
  const unsigned pair = blockIdx.x;
  const unsigned long long n_dec = wide_n_dec(a, pair);
  if (n_dec == 0) return;                              // (the whole workgroup)
  const double* __restrict__ y = a.y + (size_t)pair * a.y_stride;
  double s[1] = {0.};
  for (unsigned long long k = threadIdx.x; k < n_dec; k += 256) s[0] += y[k];
  block_sum4<1>(s, sh);
  const double m = s[0] / (double)n_dec;
  float* __restrict__ dst = a_out + (size_t)pair * a.out_stride;
  for (unsigned long long k = threadIdx.x; k < n_dec; k += 256) dst[k] = (float)(y[k] - m);
}

#pragma clang fp contract(off)                        // host arithmetic from here on: every operation rounded on its own

int wide_log2(uint32_t M) {                            // 1 .. 6 for a power of two in 2 .. 64, else 0
  for (int l = 1; l <= 6; ++l)
    if (M == (1u << l)) return l;
  return 0;
}

int check_wide_factor(const std::string& who, uint32_t M) {
  return wide_log2(M) ? PEAQ_OK : fail(PEAQ_ERR_ARG, who + ": M " + std::to_string(M) + " is not a power of two in 2 .. 64");
}
int check_wide_mode(const std::string& who, int mode) {
  return mode == PEAQ_WIDE_WAVEFORM || mode == PEAQ_WIDE_ENVELOPE
             ? PEAQ_OK
             : fail(PEAQ_ERR_ARG, who + ": mode " + std::to_string(mode) + " is neither PEAQ_WIDE_WAVEFORM (0) nor PEAQ_WIDE_ENVELOPE (1)");
}
int check_wide_offset(const std::string& who, uint32_t max_offset) {
  return peaq_wide_factor(max_offset)
             ? PEAQ_OK
             : fail(PEAQ_ERR_ARG, who + ": max_offset " + std::to_string(max_offset) + " is outside 1 .. " + std::to_string(PEAQ_WIDE_MAX_OFFSET));
}

double wide_i0(double x) {                             // sum_k ((x / 2)^2k / k!^2), ascending k
  const double q = 0.25 * x * x;
  double term = 1., sum = 1.;
  for (int k = 1; k < 200; ++k) {
    term = term * q / ((double)k * (double)k);
    const double next = sum + term;
    if (next == sum) break;
    sum = next;
  }
  return sum;
}

// sin (pi x) / (pi x) for x = num / den, den a power of two: the quotient is exact
double wide_sinc(long long num, long long den) {
  if (num == 0) return 1.;
  const double pi = 3.14159265358979323846;
  const long long two = 2 * den;
  long long r = num % two;                             // x mod 2, as a count of 1 / den: in (-2 den, 2 den)
  if (r > den) r -= two;
  if (r < -den) r += two;                              // [-den, den]: [-1, 1] half turns
  if (r > den / 2) r = den - r;                        // sin (pi (1 - x)) = sin (pi x)
  if (r < -den / 2) r = -den - r;
  return std::sin(pi * ((double)r / (double)den)) / (pi * ((double)num / (double)den));
}

void wide_taps(uint32_t M, std::vector<double>& h) {
  const long long m = M, K = kWdHalf * m;
  h.assign((size_t)(2 * K + 1), 0.);
  const double beta = 5.65, i0b = wide_i0(beta);
  for (long long j = 0; j <= K; ++j) {
    const double r = (double)j / (double)K;
    const double v = (0.75 / (double)m) * wide_sinc(3 * j, 4 * m) * wide_i0(beta * std::sqrt(1. - r * r)) / i0b;
    h[(size_t)(K + j)] = h[(size_t)(K - j)] = v;
  }
}

size_t even_stride(size_t n) {                         // 8-byte rows of at least two samples, as in peaq_run_pair
  n = std::max<size_t>(n, 2);
  return n + (n & 1);
}

// pairs of a group of the estimate, and the bytes of its staging: two cut buffers, two decimated ones, two records
struct WidePlan {
  size_t cut_stride, dec_stride;
  PairGroups pg;
};
WidePlan wide_plan(int channels, int n_pairs, uint32_t n_max, uint32_t M) {
  WidePlan pl;
  pl.cut_stride = even_stride(n_max);
  pl.dec_stride = even_stride(((size_t)n_max + M - 1) / M);
  const size_t per_pair = 2 * pl.cut_stride * channels * sizeof(float) + 2 * pl.dec_stride * sizeof(float) + 2 * sizeof(peaq_delay);
  pl.pg = pair_groups(per_pair, n_pairs, kWdStagingBudget);
  return pl;
}

}  // namespace

struct WideState {
  StageScratch scratch;         // envelope mode: [group][y_stride] doubles
  LenStage lens;                // [n_in]
  DevBuf taps[7];               // by log2 M, uploaded at the factor's first use
  bool have[7] = {false, false, false, false, false, false, false};
};

void wide_release(peaq_ctx* c) { release_stage(c->wd); }

extern "C" size_t peaq_wide_delay_size(void) { return sizeof(peaq_wide_delay); }

extern "C" uint32_t peaq_wide_factor(uint32_t max_offset) {
  if (max_offset < 1 || max_offset > PEAQ_WIDE_MAX_OFFSET) return 0;
  uint32_t M = 2;
  while ((max_offset + M - 1) / M > 16384) M *= 2;
  return M;
}

extern "C" int peaq_wide_taps(uint32_t M, double* h) {
  const std::string w("peaq_wide_taps");
  if (int rc = check_wide_factor(w, M)) return rc;
  if (!h) return fail(PEAQ_ERR_ARG, w + ": h is NULL");
  std::vector<double> t;
  wide_taps(M, t);
  std::memcpy(h, t.data(), t.size() * sizeof(double));
  return (int)t.size();
}

extern "C" int peaq_batch_decimate(peaq_ctx* c, int channels, int n_pairs, const float* d_in, size_t in_stride,
                                   const uint32_t* n_in, uint32_t n_uniform, uint32_t M, int mode, float* d_out,
                                   size_t out_stride, void* stream_) {
  const std::string w("peaq_batch_decimate");
  if (int rc = check_wide_factor(w, M)) return rc;
  if (int rc = check_wide_mode(w, mode)) return rc;
  if (int rc = check_shape(w, channels, n_pairs)) return rc;
  if (n_pairs > 0 && (!d_in || !d_out)) return fail(PEAQ_ERR_ARG, w + ": NULL buffer");
  uint32_t n_max = 0;
  if (int rc = check_lengths(w, n_pairs, n_in, n_uniform, "n_in", in_stride, "in_stride", &n_max)) return rc;
  const size_t dec_max = ((size_t)n_max + M - 1) / M;
  if (n_pairs > 0 && dec_max > out_stride)
    return fail(PEAQ_ERR_ARG, w + ": out_stride " + std::to_string(out_stride) + " is smaller than the longest n_dec (" +
                                  std::to_string(dec_max) + " samples)");
  if (n_pairs > 0) {
    const char* i0 = reinterpret_cast<const char*>(d_in);
    const char* o0 = reinterpret_cast<const char*>(d_out);
    const size_t ib = (size_t)n_pairs * in_stride * channels * sizeof(float);
    const size_t ob = (size_t)n_pairs * out_stride * sizeof(float);
    if (i0 < o0 + ob && o0 < i0 + ib) return fail(PEAQ_ERR_ARG, w + ": d_out overlaps d_in");
  }
  if (!c) return fail(PEAQ_ERR_ARG, w + ": ctx is NULL");
  if (n_pairs == 0 || dec_max == 0) return PEAQ_OK;

  hipStream_t stream = static_cast<hipStream_t>(stream_);
  std::lock_guard<std::mutex> lock(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  if (!c->wd) c->wd = new WideState;
  WideState* st = c->wd;
  const int lg = wide_log2(M);
  if (!st->have[lg]) {                                 // (blocking, once per context and factor)
    std::vector<double> t;
    wide_taps(M, t);
    HIP_TRY(st->taps[lg].reserve(t.size() * sizeof(double)));
    HIP_TRY(hipMemcpy(st->taps[lg].p, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
    st->have[lg] = true;
  }
  const bool envelope = mode == PEAQ_WIDE_ENVELOPE;
  PairGroups pg{0, n_pairs};
  if (envelope) {
    pg = pair_groups(dec_max * sizeof(double), n_pairs, kWdRowsBudget);
    if (int rc = st->scratch.acquire(pg.bytes, stream)) return rc;
  }
  LenSlot* slot = nullptr;
  if (n_in) {
    if (int rc = st->lens.upload(n_in, (size_t)n_pairs, stream, &slot)) return rc;
  }
  WideArgs a{};
  a.in_stride = in_stride;
  a.out_stride = out_stride;
  a.y_stride = dec_max;
  const double* taps = st->taps[lg].as<double>();
  a.y = envelope ? st->scratch.buf.as<double>() : nullptr;
  a.n_uniform = n_uniform;
  a.M = M;
  a.log_m = (uint32_t)lg;
  a.P = (uint32_t)wide_pass(M);
  a.row = a.P + 2 * kWdHalf + 1;
  a.channels = channels;
  const unsigned chunks = (unsigned)((dec_max + kWdChunk - 1) / kWdChunk);
  hipError_t launched = hipSuccess;
  for (int p0 = 0; p0 < n_pairs; p0 += pg.group) {
    const unsigned np = (unsigned)std::min(pg.group, n_pairs - p0);
    a.n_in = slot ? slot->dev.as<uint32_t>() + p0 : nullptr;
    const float* in = d_in + (size_t)p0 * in_stride * channels;
    float* out = d_out + (size_t)p0 * out_stride;
    if (envelope) {
      hipLaunchKernelGGL(wide_decimate_kernel<PEAQ_WIDE_ENVELOPE>, dim3(chunks, np), dim3(256), 0, stream, a, in, out, taps);
      hipLaunchKernelGGL(wide_center_kernel, dim3(np), dim3(256), 0, stream, a, out);
    } else {
      hipLaunchKernelGGL(wide_decimate_kernel<PEAQ_WIDE_WAVEFORM>, dim3(chunks, np), dim3(256), 0, stream, a, in, out, taps);
    }
    launched = hipGetLastError();
    if (launched != hipSuccess) break;
  }
  // (also after a failed launch: what was enqueued before it still reads the slot and the scratch)
  const hipError_t marked = envelope ? st->scratch.mark(stream) : hipSuccess;
  const int sent = slot ? st->lens.sent(slot, stream) : PEAQ_OK;
  HIP_TRY(launched);
  HIP_TRY(marked);
  return sent;
}

extern "C" size_t peaq_wide_workspace_bytes(int channels, int n_pairs, uint32_t n_max, uint32_t max_offset) {
  const uint32_t M = peaq_wide_factor(max_offset);
  if ((channels != 1 && channels != 2) || n_pairs <= 0 || n_pairs > 65535 || !M) return 0;
  return wide_plan(channels, n_pairs, n_max, M).pg.bytes;
}

extern "C" int peaq_batch_estimate_delay_wide(peaq_ctx* c, int channels, int n_pairs, const float* d_ref, const float* d_test,
                                              size_t pair_stride, const uint32_t* n_ref, const uint32_t* n_test,
                                              uint32_t n_uniform, uint32_t max_offset, int mode, uint32_t max_lag,
                                              peaq_wide_delay* out, void* stream_) {
  const std::string w("peaq_batch_estimate_delay_wide");
  if (int rc = check_wide_offset(w, max_offset)) return rc;
  if (int rc = check_wide_mode(w, mode)) return rc;
  if (int rc = check_max_lag(w, max_lag)) return rc;
  if (int rc = check_shape(w, channels, n_pairs)) return rc;
  if (n_pairs > 0 && (!d_ref || !d_test)) return fail(PEAQ_ERR_ARG, w + ": NULL buffer");
  if (n_pairs > 0 && !out) return fail(PEAQ_ERR_ARG, w + ": NULL out");
  if ((n_ref == nullptr) != (n_test == nullptr))
    return fail(PEAQ_ERR_ARG, w + ": n_ref and n_test must both be given or both be NULL");
  uint32_t nr_max = 0, nt_max = 0;
  if (int rc = check_lengths(w, n_pairs, n_ref, n_uniform, "n_ref", pair_stride, "pair_stride", &nr_max)) return rc;
  if (int rc = check_lengths(w, n_pairs, n_test, n_uniform, "n_test", pair_stride, "pair_stride", &nt_max)) return rc;
  if (!c) return fail(PEAQ_ERR_ARG, w + ": ctx is NULL");
  if (n_pairs == 0) return PEAQ_OK;

  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIP_TRY(hipSetDevice(c->device));
  const uint32_t M = peaq_wide_factor(max_offset);
  const uint32_t coarse_range = (max_offset + M - 1) / M;
  const WidePlan pl = wide_plan(channels, n_pairs, std::max(nr_max, nt_max), M);
  const int group = pl.pg.group;
  DevBuf cut[2], dec[2], d_rec;                         // (the call's own: the stages it calls take the context's lock)
  for (int i = 0; i < 2; ++i) {
    HIP_TRY(cut[i].reserve((size_t)group * pl.cut_stride * channels * sizeof(float)));
    HIP_TRY(dec[i].reserve((size_t)group * pl.dec_stride * sizeof(float)));
  }
  HIP_TRY(d_rec.reserve((size_t)group * 2 * sizeof(peaq_delay)));
  peaq_delay* d_coarse = d_rec.as<peaq_delay>();
  peaq_delay* d_fine = d_coarse + group;
  std::vector<uint32_t> len[2], n_dec[2], skip[2], common((size_t)group);
  for (int i = 0; i < 2; ++i) {
    len[i].resize((size_t)group);
    n_dec[i].resize((size_t)group);
    skip[i].resize((size_t)group);
  }
  std::vector<peaq_delay> coarse((size_t)group), fine((size_t)group);
  for (int p0 = 0; p0 < n_pairs; p0 += group) {
    const int g = std::min(group, n_pairs - p0);
    const float* in[2] = {d_ref + (size_t)p0 * pair_stride * channels, d_test + (size_t)p0 * pair_stride * channels};
    // 1, 2: the decimated copies, the coarse records
    for (int p = 0; p < g; ++p) {
      len[0][p] = n_ref ? n_ref[p0 + p] : n_uniform;
      len[1][p] = n_test ? n_test[p0 + p] : n_uniform;
      for (int i = 0; i < 2; ++i) n_dec[i][p] = (uint32_t)(((uint64_t)len[i][p] + M - 1) / M);
    }
    for (int i = 0; i < 2; ++i)
      if (int rc = peaq_batch_decimate(c, channels, g, in[i], pair_stride, len[i].data(), 0, M, mode, dec[i].as<float>(),
                                       pl.dec_stride, stream))
        return rc;
    if (int rc = peaq_batch_estimate_delay(c, 1, g, dec[0].as<float>(), dec[1].as<float>(), pl.dec_stride, n_dec[0].data(),
                                           n_dec[1].data(), 0, coarse_range, d_coarse, stream))
      return rc;
    HIP_TRY(hipMemcpyAsync(coarse.data(), d_coarse, (size_t)g * sizeof(peaq_delay), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    // 3, 4: the coarse lags, both signals cut by them
    for (int p = 0; p < g; ++p) {
      peaq_wide_delay& r = out[p0 + p];
      std::memset(&r, 0, sizeof r);
      r.factor = M;
      r.coarse = coarse[p];
      if (!(coarse[p].norm > 0.))
        r.flags = PEAQ_WIDE_F_NONE;
      else
        r.coarse_lag = coarse[p].lag * (int32_t)M;
      peaq_aligned_lengths(r.coarse_lag, len[0][p], len[1][p], &skip[0][p], &skip[1][p], &common[p]);
    }
    for (int i = 0; i < 2; ++i)
      if (int rc = peaq_batch_cut(c, channels, g, in[i], pair_stride, skip[i].data(), common.data(), cut[i].as<float>(),
                                  pl.cut_stride, stream))
        return rc;
    // 5, 6: the fine records
    if (int rc = peaq_batch_estimate_delay(c, channels, g, cut[0].as<float>(), cut[1].as<float>(), pl.cut_stride, common.data(),
                                           common.data(), 0, max_lag, d_fine, stream))
      return rc;
    HIP_TRY(hipMemcpyAsync(fine.data(), d_fine, (size_t)g * sizeof(peaq_delay), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));             // (the staging buffers are free again, too)
    for (int p = 0; p < g; ++p) {
      peaq_wide_delay& r = out[p0 + p];
      r.fine = fine[p];
      r.lag = r.coarse_lag + fine[p].lag;
      if (!(r.flags & PEAQ_WIDE_F_NONE) && (uint32_t)std::abs(coarse[p].lag) == coarse_range) r.flags |= PEAQ_WIDE_F_RANGE;
      if ((uint32_t)std::abs(fine[p].lag) == max_lag) r.flags |= PEAQ_WIDE_F_EDGE;
    }
  }
  return PEAQ_OK;
}

extern "C" int peaq_run_pair_wide(peaq_ctx* c, int advanced, int channels, double level_db, uint32_t rate,
                                  uint32_t max_offset, int mode, uint32_t max_lag, const float* ref, size_t n_ref,
                                  const float* test, size_t n_test, peaq_wide_delay* delay, peaq_result* out) {
  const std::string w("peaq_run_pair_wide");
  if (int rc = check_wide_offset(w, max_offset)) return rc;
  if (int rc = check_wide_mode(w, mode)) return rc;
  if (int rc = check_max_lag(w, max_lag)) return rc;
  if (int rc = check_level(w, level_db)) return rc;
  if (int rc = check_pair_args(w, c, channels, rate, ref, n_ref, test, n_test, out, true)) return rc;
  // 1, 2: upload, rate conversion
  PairBuffers in;
  if (int rc = upload_pair_48k(c, channels, rate, ref, n_ref, test, n_test, in)) return rc;
  // 3: the wide estimate
  peaq_wide_delay rec;
  if (int rc = peaq_batch_estimate_delay_wide(c, channels, 1, in.d(0), in.d(1), in.stride, in.len, in.len + 1, 0, max_offset,
                                              mode, max_lag, &rec, nullptr))
    return rc;
  if (delay) *delay = rec;
  // 4: both signals cut to their common part
  uint32_t skip[2], common = 0;
  peaq_aligned_lengths(rec.lag, in.len[0], in.len[1], &skip[0], &skip[1], &common);
  const size_t cstride = even_stride(common);
  const size_t cbytes = cstride * channels * sizeof(float);
  DevBuf cut[2];
  for (int i = 0; i < 2; ++i) {
    HIP_TRY(cut[i].reserve(cbytes));
    HIP_TRY(hipMemset(cut[i].p, 0, cbytes));
    if (int rc = peaq_batch_cut(c, channels, 1, in.d(i), in.stride, &skip[i], &common, cut[i].as<float>(), cstride, nullptr))
      return rc;
  }
  HIP_TRY(hipDeviceSynchronize());
  // 5: the one-pair path
  return score_one_pair(c, advanced, channels, level_db, cut[0].as<float>(), cut[1].as<float>(), cstride, common, common, out);
}

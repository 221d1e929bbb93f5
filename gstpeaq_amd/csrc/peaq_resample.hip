// peaq_resample.hip -- sample-rate conversion to 48 kHz for whole batches in device memory (peaq_batch_resample,
// peaq_run_pair_rate; include/peaq_amd.h).  The converter IS the CLI's resample_to_48k (gstpeaq_amd/cli/peaq.c, which
// stands in for the `audioresample` of peaq.c:154-209): the same Kaiser-windowed sinc, the same polyphase table built
// on the host in double, FP64 accumulation in the tap order, one rounding to FP32.
//
//   g = gcd(48000, rate), L = 48000 / g, M = rate / g;  output m: p = (m M) mod L, q = (m M) div L,
//   y[m] = sum_{j < 2K} h_p[j] x[q + floor(p / L - 1/8) - K + 1 + j], samples outside [0, n) taken as absent.
//
// Two kernels:
//   resample_tile_kernel   the fast one.  Outputs L' = c L apart (c: a small integer that makes L' a multiple of 4
//       and at least 32) have the same phase and sit M' = c M input samples apart, so with LANE = period the four tap
//       rows of four consecutive phases are wave-uniform: they come through scalar loads, 32 bytes per step, and each
//       sample a lane reads from LDS feeds four FP64 multiply-adds.  A workgroup owns 64 periods of one pair: it
//       stages their input samples in LDS once per channel (coalesced reads, every sample fetched from HBM once per
//       tile plus a halo of about M' + 2K), its eight waves walk the L' / 4 phase groups, and the results go through a
//       second LDS tile so that the stores to HBM are runs of L' consecutive samples.  Lanes read LDS M' floats apart
//       (odd M': conflict-free as it is; even M': every lane gets a row of its own, padded to an odd pitch) and write
//       the result tile L' | 1 floats apart.
//   resample_any_kernel    one thread per output sample, taps and samples from global memory: every supported rate
//       whose tiles do not fit LDS (L' > about 500: 11.025 kHz, odd ratios such as 1000 / 919).
#include "peaq_host.h"

#include <map>

namespace {

constexpr int kRsThreads = 512;                  // resample_tile_kernel: 8 waves
constexpr int kRsWaves = kRsThreads / 64;
constexpr int kRsGroup = 4;                      // phases per group = FP64 accumulators per lane
#ifndef PEAQ_RS_UNROLL
#define PEAQ_RS_UNROLL 4
#endif
constexpr unsigned kRsUnroll = PEAQ_RS_UNROLL;   // steps per trip of the tap loop; W is a multiple of it
constexpr int kRsPeriods = 64;                   // periods per tile = lanes
constexpr size_t kRsLdsMax = 160 * 1024;         // a CU's LDS; 44.1 kHz takes 79 KB: two workgroups per CU

struct RsTileArgs {
  size_t in_stride, out_stride; // of in [pair][in_stride][channels] and out [pair][out_stride][channels]
  const uint32_t* n_in;         // per-pair lengths (device) or nullptr: n_in_uniform / n_out_uniform
  const uint32_t* n_out;
  uint32_t n_in_uniform, n_out_uniform;
  int channels;
  uint32_t Lp, Mp;              // period: L' outputs, M' inputs
  uint32_t W;                   // taps per phase in the group tables (2K + the group's spread, rounded up to the loop's unroll)
  uint32_t G;                   // groups = L' / 4
  uint32_t pitch;               // floats between the LDS rows of consecutive lanes
  uint32_t rows, row_len;       // staging: rows x row_len floats (odd M': one row holding all 64 periods)
  uint32_t in_floats;           // size of the input tile
  uint32_t LP;                  // pitch of the result tile, L' | 1
  int off_min;                  // first staged sample relative to the first period's start
};                              // beside it: taps [G][W][4]; off [G], first sample of a group's window relative to its period's start

struct RsAnyArgs {
  const float* in;
  float* out;
  size_t in_stride, out_stride;
  const uint32_t* n_in;
  const uint32_t* n_out;
  uint32_t n_in_uniform, n_out_uniform;
  int channels;
  uint32_t L, M, K;
  const double* taps;           // [L][2K]
};

// (the buffers as parameters of their own: only a __restrict__ read-only PARAMETER lets the compiler fetch the taps with
// scalar loads; as members of the argument block they came through vector loads of a uniform address)
__global__ __launch_bounds__(kRsThreads) void resample_tile_kernel(const RsTileArgs a, const float* __restrict__ a_in,
                                                                    float* __restrict__ a_out,
                                                                    const double* __restrict__ a_taps,
                                                                    const int* __restrict__ a_off) {
  extern __shared__ __attribute__((aligned(16))) float rs_lds[];
  float* tin = rs_lds;
  float* tout = rs_lds + a.in_floats;
  const unsigned pair = blockIdx.y, tile = blockIdx.x;
  const uint32_t n_in = a.n_in ? a.n_in[pair] : a.n_in_uniform;
  const uint32_t n_out = a.n_out ? a.n_out[pair] : a.n_out_uniform;
  const unsigned long long m0 = (unsigned long long)tile * kRsPeriods * a.Lp;
  if (m0 >= n_out) return;                                         // (the whole workgroup)
  const long long s_base = (long long)tile * kRsPeriods * a.Mp + a.off_min;
  const unsigned tid = threadIdx.x, lane = tid & 63;
  const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int C = a.channels;
  const float* in = a_in + (size_t)pair * a.in_stride * C;
  float* out = a_out + (size_t)pair * a.out_stride * C;

  for (int c = 0; c < C; ++c) {
    // ---- stage the tile's input samples; absent samples are zeros (h x 0 leaves a sum as it is) ----
    if (a.rows == 1) {
      for (unsigned v = tid; v < a.row_len; v += kRsThreads) {
        const long long s = s_base + v;
        tin[v] = (s >= 0 && s < (long long)n_in) ? in[(size_t)s * C + c] : 0.f;
      }
    } else {
      for (unsigned i = wave; i < a.rows; i += kRsWaves) {
        const long long s_row = s_base + (long long)i * a.Mp;
        for (unsigned v = lane; v < a.row_len; v += 64) {
          const long long s = s_row + v;
          tin[i * a.pitch + v] = (s >= 0 && s < (long long)n_in) ? in[(size_t)s * C + c] : 0.f;
        }
      }
    }
    __syncthreads();
    // ---- four phases per wave and step: taps wave-uniform, lane = period ----
    for (unsigned g = wave; g < a.G; g += kRsWaves) {
      const float* x = tin + lane * a.pitch + (a_off[g] - a.off_min);
      const double* t = a_taps + (size_t)g * a.W * kRsGroup;
      double acc0 = 0., acc1 = 0., acc2 = 0., acc3 = 0.;
      for (unsigned w = 0; w < a.W; w += kRsUnroll) {
#pragma unroll
        for (unsigned u = 0; u < kRsUnroll; ++u) {
          const double xv = (double)x[w + u];
          acc0 = __builtin_fma(t[(w + u) * 4 + 0], xv, acc0);
          acc1 = __builtin_fma(t[(w + u) * 4 + 1], xv, acc1);
          acc2 = __builtin_fma(t[(w + u) * 4 + 2], xv, acc2);
          acc3 = __builtin_fma(t[(w + u) * 4 + 3], xv, acc3);
        }
      }
      float* y = tout + lane * a.LP + g * kRsGroup;
      y[0] = (float)acc0;
      y[1] = (float)acc1;
      y[2] = (float)acc2;
      y[3] = (float)acc3;
    }
    __syncthreads();
    // ---- runs of L' consecutive outputs per period ----
    for (unsigned i = wave; i < kRsPeriods; i += kRsWaves) {
      const unsigned long long m_row = m0 + (unsigned long long)i * a.Lp;
      for (unsigned j = lane; j < a.Lp; j += 64)
        if (m_row + j < n_out) out[(size_t)(m_row + j) * C + c] = tout[i * a.LP + j];
    }
    // (the next channel's staging overwrites tin only, and every wave is past its reads of it)
  }
}

__global__ __launch_bounds__(256) void resample_any_kernel(const RsAnyArgs a) {
  const unsigned pair = blockIdx.y;
  const uint32_t n_in = a.n_in ? a.n_in[pair] : a.n_in_uniform;
  const uint32_t n_out = a.n_out ? a.n_out[pair] : a.n_out_uniform;
  const unsigned long long m = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  if (m >= n_out) return;
  const int C = a.channels;
  const float* in = a.in + (size_t)pair * a.in_stride * C;
  const unsigned long long mm = m * a.M;
  const uint32_t p = (uint32_t)(mm % a.L);
  // floor(p / L - 1/8) is -1 below an eighth and 0 from there on (the host checks that against the double form)
  const long long n_first = (long long)(mm / a.L) + (8ull * p < a.L ? -1 : 0) - (long long)a.K + 1;
  const double* h = a.taps + (size_t)p * 2 * a.K;
  double acc0 = 0., acc1 = 0.;
  for (uint32_t j = 0; j < 2 * a.K; ++j) {
    const long long n = n_first + j;
    if (n < 0 || n >= (long long)n_in) continue;
    acc0 = __builtin_fma(h[j], (double)in[(size_t)n * C], acc0);
    if (C == 2) acc1 = __builtin_fma(h[j], (double)in[(size_t)n * C + 1], acc1);
  }
  float* out = a.out + ((size_t)pair * a.out_stride + m) * C;
  out[0] = (float)acc0;
  if (C == 2) out[1] = (float)acc1;
}

// ---------------------------------------------------------------------------
// the filter: gstpeaq_amd/cli/peaq.c bessel_i0 / rs_tap / resample_to_48k, formula for formula
// ---------------------------------------------------------------------------
double bessel_i0(double x) {
  double sum = 1., term = 1.;
  for (int k = 1; k < 60; k++) {
    term *= (x / (2. * k)) * (x / (2. * k));
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

struct RsFilter {
  double fc, half, beta, i0b;
};

double rs_tap(const RsFilter& k, double d) {
  const double u = d / k.half, arg = 2. * M_PI * k.fc * d;
  if (std::fabs(u) > 1.) return 0.;
  return 2. * k.fc * (std::fabs(arg) < 1e-12 ? 1. : std::sin(arg) / arg) * bessel_i0(k.beta * std::sqrt(1. - u * u)) / k.i0b;
}

uint32_t gcd_u32(uint32_t a, uint32_t b) {
  while (b) {
    const uint32_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

bool rate_supported(uint32_t rate) {
  if (rate < 8000 || rate > 384000 || rate == 48000) return false;
  return 48000u / gcd_u32(48000u, rate) <= 4096u;
}

// false = does not fit uint32_t (or rate 0)
bool resampled_length(uint64_t n, uint32_t rate, uint32_t* out) {
  *out = 0;
  if (rate == 0) return false;
  if (n == 0) return true;
  const double ratio = 48000. / rate;
  const double len = std::floor((double)(n - 1) * ratio) + 1.;
  if (!(len <= 4294967295.)) return false;
  *out = (uint32_t)len;
  return true;
}

// what one rate needs on the device
struct RsPlan {
  uint32_t L = 0, M = 0, K = 0;
  bool tiled = false;
  RsTileArgs tile{};            // geometry (pointers filled in per call)
  size_t lds_bytes = 0;
  uint32_t zero_taps = 0;       // tiled: W - 2K, taps evaluated beside the filter's own (all zero)
  DevBuf taps, off;
  DevBuf plain;                 // tiled: the plain [L][2K] table, for the range converter only (peaq_live_rate.hip)
};

// the filter of `rate` (the CLI's parameters) and its K
RsFilter rate_filter(uint32_t rate, long* K) {
  const double ratio = 48000. / rate;
  RsFilter k;
  if (ratio >= 1.) {
    k.fc = 0.94 * 0.5;
    k.half = 32.15;
    k.beta = 8.49;
  } else {
    k.fc = 0.921 * 0.5 * ratio;
    k.half = 4. * std::ceil(64. / ratio / 8.);
    k.beta = 8.41;
  }
  k.i0b = bessel_i0(k.beta);
  *K = (long)std::ceil(k.half) + 1;
  return k;
}

}  // namespace

struct RsState {
  std::map<uint32_t, std::unique_ptr<RsPlan>> plans;
  LenStage lens;                // per-pair lengths of one call, [n_in | n_out] (peaq_host.h)
};

void resample_release(peaq_ctx* c) {
  if (!c->rs) return;
  c->rs->lens.release();
  delete c->rs;                 // (the plans' tables and the slots' device buffers go with it)
  c->rs = nullptr;
}

static int check_rate(const char* who, uint32_t rate) {
  if (rate == 48000)
    return fail(PEAQ_ERR_ARG, std::string(who) + ": rate 48000 needs no conversion, pass the buffers straight on");
  if (!rate_supported(rate))
    return fail(PEAQ_ERR_ARG, std::string(who) + ": rate " + std::to_string(rate) +
                                  " Hz is not supported on the device (8000 .. 384000 Hz with 48000 / gcd(48000, rate) <= 4096)");
  return PEAQ_OK;
}

// The plan of `rate`, host only: filter, tile geometry, and the tables the kernels read (tiled: group tables and
// window offsets; otherwise the plain [L][2K] table).
// With h_plain, the plain table of a tiled rate goes there as well (otherwise h_taps is the plain table).
static int build_plan(uint32_t rate, RsPlan* pl, std::vector<double>* h_taps, std::vector<int>* h_off,
                      std::vector<double>* h_plain = nullptr) {
  const double delay = 0.125;
  long K = 0;
  const RsFilter k = rate_filter(rate, &K);
  const uint32_t g = gcd_u32(48000u, rate), L = 48000u / g, M = rate / g;
  pl->L = L;
  pl->M = M;
  pl->K = (uint32_t)K;
  std::vector<double> table((size_t)L * 2 * K);
  std::vector<int> fl(L);
  for (uint32_t p = 0; p < L; p++) {
    const double tf = (double)p / (double)L - delay, f = std::floor(tf), fr = tf - f;
    fl[p] = (int)f;
    if (fl[p] != (8ull * p < L ? -1 : 0)) return fail(PEAQ_ERR_ARG, "peaq_batch_resample: phase offset of rate " + std::to_string(rate));
    for (long j = 0; j < 2 * K; j++) table[(size_t)p * 2 * K + j] = rs_tap(k, fr + (double)(K - 1 - j));
  }
  // periods of L' = c L outputs: a multiple of the group of 4, at least 32 (eight waves x one group)
  uint32_t cmul = (32 + L - 1) / L;
  while ((cmul * L) % kRsGroup) ++cmul;
  const uint32_t Lp = cmul * L, Mp = cmul * M, G = Lp / kRsGroup;
  std::vector<long> nf(Lp);
  for (uint32_t r = 0; r < Lp; r++) {
    const unsigned long long mm = (unsigned long long)r * M;
    nf[r] = (long)(mm / L) + fl[mm % L] - K + 1;
  }
  std::vector<int> off(G);
  long spread = 0, off_min = 0, off_max = 0;
  for (uint32_t q = 0; q < G; q++) {
    long lo = nf[q * kRsGroup], hi = lo;
    for (int i = 1; i < kRsGroup; i++) {
      lo = std::min(lo, nf[q * kRsGroup + i]);
      hi = std::max(hi, nf[q * kRsGroup + i]);
    }
    off[q] = (int)lo;
    spread = std::max(spread, hi - lo);
    off_min = q ? std::min(off_min, lo) : lo;
    off_max = q ? std::max(off_max, lo) : lo;
  }
  const uint32_t W = (uint32_t)((2 * K + spread + kRsUnroll - 1) / kRsUnroll * kRsUnroll);
  const uint32_t V = (uint32_t)(off_max - off_min) + W;          // a lane's reach from its period's first staged sample
  RsTileArgs& t = pl->tile;
  t.Lp = Lp;
  t.Mp = Mp;
  t.W = W;
  t.G = G;
  t.LP = Lp | 1;
  t.off_min = (int)off_min;
  if (Mp & 1) {                                                   // lanes M' floats apart: conflict-free as it is
    t.pitch = Mp;
    t.rows = 1;
    t.row_len = (kRsPeriods - 1) * Mp + V;
  } else {                                                        // a row per lane, odd pitch
    t.pitch = V | 1;
    t.rows = kRsPeriods;
    t.row_len = V;
  }
  const unsigned long long in_floats =
      t.rows == 1 ? (unsigned long long)t.row_len : (unsigned long long)kRsPeriods * t.pitch;
  const unsigned long long lds = 4ull * (in_floats + (unsigned long long)kRsPeriods * t.LP);
  pl->tiled = lds <= kRsLdsMax;
  if (pl->tiled) {
    t.in_floats = (uint32_t)in_floats;
    pl->lds_bytes = (size_t)lds;
    pl->zero_taps = W - (uint32_t)(2 * K);
    std::vector<double>& gt = *h_taps;
    gt.assign((size_t)G * W * kRsGroup, 0.);
    for (uint32_t q = 0; q < G; q++)
      for (int i = 0; i < kRsGroup; i++) {
        const uint32_t r = q * kRsGroup + i;
        const uint32_t p = (uint32_t)(((unsigned long long)r * M) % L);
        const long shift = nf[r] - off[q];
        for (long j = 0; j < 2 * K; j++) gt[((size_t)q * W + (size_t)(shift + j)) * kRsGroup + i] = table[(size_t)p * 2 * K + j];
      }
    *h_off = off;
    if (h_plain) *h_plain = std::move(table);
  } else {
    *h_taps = std::move(table);
    h_off->clear();
  }
  return PEAQ_OK;
}

// builds the plan of `rate` and uploads its tables (once per context)
static int get_plan(peaq_ctx* c, uint32_t rate, RsPlan** out) {
  if (!c->rs) c->rs = new RsState;
  auto it = c->rs->plans.find(rate);
  if (it != c->rs->plans.end()) {
    *out = it->second.get();
    return PEAQ_OK;
  }
  std::unique_ptr<RsPlan> pl(new RsPlan);
  std::vector<double> h_taps;
  std::vector<int> h_off;
  if (int rc = build_plan(rate, pl.get(), &h_taps, &h_off)) return rc;
  HIP_TRY(pl->taps.reserve(h_taps.size() * sizeof(double)));
  HIP_TRY(hipMemcpy(pl->taps.p, h_taps.data(), h_taps.size() * sizeof(double), hipMemcpyHostToDevice));
  if (pl->tiled) {
    HIP_TRY(pl->off.reserve(h_off.size() * sizeof(int)));
    HIP_TRY(hipMemcpy(pl->off.p, h_off.data(), h_off.size() * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(resample_tile_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRsLdsMax));
  }
  *out = pl.get();
  c->rs->plans[rate] = std::move(pl);
  return PEAQ_OK;
}

// ---- for the range converter of live streams (peaq_live_rate.hip; declared in peaq_host.h) ----
int resample_geometry(const char* who, uint32_t rate, RateGeometry* out) {
  if (int rc = check_rate(who, rate)) return rc;
  long K = 0;
  (void)rate_filter(rate, &K);
  const uint32_t g = gcd_u32(48000u, rate);
  *out = RateGeometry{48000u / g, rate / g, (uint32_t)K};
  return PEAQ_OK;
}

uint64_t resampled_length_u64(uint64_t n, uint32_t rate) {
  return n ? (uint64_t)(std::floor((double)(n - 1) * (48000. / rate)) + 1.) : 0;   // (resampled_length, no limit)
}

int resample_plain_table(peaq_ctx* c, uint32_t rate, const double** taps, RateGeometry* geo, LenStage** lens) {
  RsPlan* pl = nullptr;
  if (int rc = get_plan(c, rate, &pl)) return rc;
  if (pl->tiled && !pl->plain.p) {                   // (once per rate and context, synchronously, as the plan's own tables)
    RsPlan again;
    std::vector<double> h_taps, h_plain;
    std::vector<int> h_off;
    if (int rc = build_plan(rate, &again, &h_taps, &h_off, &h_plain)) return rc;
    HIP_TRY(pl->plain.reserve(h_plain.size() * sizeof(double)));
    HIP_TRY(hipMemcpy(pl->plain.p, h_plain.data(), h_plain.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  *taps = pl->tiled ? pl->plain.as<double>() : pl->taps.as<double>();
  *geo = RateGeometry{pl->L, pl->M, pl->K};
  *lens = &c->rs->lens;
  return PEAQ_OK;
}

extern "C" int peaq_resample_plan_info(uint32_t rate, peaq_resample_plan* out) {
  if (!out) return fail(PEAQ_ERR_ARG, "peaq_resample_plan_info: NULL argument");
  std::memset(out, 0, sizeof *out);
  if (int rc = check_rate("peaq_resample_plan_info", rate)) return rc;
  RsPlan pl;
  std::vector<double> h_taps;
  std::vector<int> h_off;
  if (int rc = build_plan(rate, &pl, &h_taps, &h_off)) return rc;
  out->L = pl.L;
  out->M = pl.M;
  out->taps = 2 * pl.K;
  out->tiled = pl.tiled ? 1 : 0;
  out->period_out = pl.tile.Lp;
  out->period_in = pl.tile.Mp;
  out->zero_taps = pl.zero_taps;
  out->lds_bytes = (uint32_t)pl.lds_bytes;
  out->table_bytes = (uint64_t)h_taps.size() * sizeof(double);
  double sum_abs = 0.;                               // largest sum |h_p| over the phases (the tables' zeros add nothing)
  if (pl.tiled) {
    const size_t W = pl.tile.W;
    for (size_t q = 0; q < pl.tile.G; ++q)
      for (int i = 0; i < kRsGroup; ++i) {
        double a = 0.;
        for (size_t w = 0; w < W; ++w) a += std::fabs(h_taps[(q * W + w) * kRsGroup + i]);
        sum_abs = std::max(sum_abs, a);
      }
  } else {
    for (size_t p = 0; p < pl.L; ++p) {
      double a = 0.;
      for (size_t j = 0; j < 2 * (size_t)pl.K; ++j) a += std::fabs(h_taps[p * 2 * pl.K + j]);
      sum_abs = std::max(sum_abs, a);
    }
  }
  out->max_sum_abs_taps = sum_abs;
  return PEAQ_OK;
}

extern "C" int peaq_resample_supported(uint32_t rate) { return rate_supported(rate) ? 1 : 0; }

extern "C" uint32_t peaq_resampled_length(uint64_t n, uint32_t rate) {
  uint32_t len = 0;
  if (!resampled_length(n, rate, &len)) {
    fail(PEAQ_ERR_ARG, rate ? "peaq_resampled_length: " + std::to_string(n) + " samples at " + std::to_string(rate) +
                                  " Hz are more than 2^32 - 1 samples at 48 kHz"
                            : std::string("peaq_resampled_length: rate is 0"));
    return 0;
  }
  peaq_err_string().clear();
  return len;
}


extern "C" int peaq_batch_resample(peaq_ctx* c, int channels, uint32_t rate, int n_pairs, const float* d_in,
                                   size_t in_stride, const uint32_t* n_in, uint32_t n_uniform, float* d_out,
                                   size_t out_stride, uint32_t* n_out, void* stream_) {
  const std::string who("peaq_batch_resample");
  // (what needs no context first)
  if (int rc = check_rate("peaq_batch_resample", rate)) return rc;
  if (int rc = check_shape(who, channels, n_pairs)) return rc;
  if (!c) return fail(PEAQ_ERR_ARG, who + ": ctx is NULL");
  if (n_pairs == 0) return PEAQ_OK;
  if (!d_in || !d_out) return fail(PEAQ_ERR_ARG, who + ": NULL buffer");
  // lengths
  if (int rc = check_lengths(who, n_pairs, n_in, n_uniform, "n_in", in_stride, "in_stride")) return rc;
  std::vector<uint32_t> h;
  uint32_t len_uniform = 0, len_max = 0;
  if (n_in) {
    h.assign(n_in, n_in + n_pairs);
    h.resize(2 * (size_t)n_pairs);
    for (int p = 0; p < n_pairs; ++p) {
      if (!resampled_length(n_in[p], rate, &h[(size_t)n_pairs + p]))
        return fail(PEAQ_ERR_ARG, who + ": a converted length does not fit 32 bits");
      len_max = std::max(len_max, h[(size_t)n_pairs + p]);
    }
  } else {
    if (!resampled_length(n_uniform, rate, &len_uniform))
      return fail(PEAQ_ERR_ARG, who + ": the converted length does not fit 32 bits");
    len_max = len_uniform;
  }
  if (len_max > out_stride)
    return fail(PEAQ_ERR_ARG, "peaq_batch_resample: out_stride " + std::to_string(out_stride) +
                                  " is smaller than the longest converted signal (" + std::to_string(len_max) + " samples)");
  if (n_out)
    for (int p = 0; p < n_pairs; ++p) n_out[p] = n_in ? h[(size_t)n_pairs + p] : len_uniform;
  if (len_max == 0) return PEAQ_OK;

  hipStream_t stream = static_cast<hipStream_t>(stream_);
  std::lock_guard<std::mutex> lock(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  RsPlan* pl = nullptr;
  if (int rc = get_plan(c, rate, &pl)) return rc;
  const uint32_t* d_nin = nullptr;
  const uint32_t* d_nout = nullptr;
  LenSlot* slot = nullptr;
  if (n_in) {
    if (int rc = c->rs->lens.upload(h.data(), h.size(), stream, &slot)) return rc;
    d_nin = slot->dev.as<uint32_t>();
    d_nout = d_nin + n_pairs;
  }
  if (pl->tiled) {
    RsTileArgs a = pl->tile;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.n_in = d_nin;
    a.n_out = d_nout;
    a.n_in_uniform = n_uniform;
    a.n_out_uniform = len_uniform;
    a.channels = channels;
    const unsigned long long per_tile = (unsigned long long)kRsPeriods * a.Lp;
    const dim3 grid((unsigned)((len_max + per_tile - 1) / per_tile), (unsigned)n_pairs);
    hipLaunchKernelGGL(resample_tile_kernel, grid, dim3(kRsThreads), pl->lds_bytes, stream, a, d_in, d_out,
                       pl->taps.as<double>(), pl->off.as<int>());
  } else {
    RsAnyArgs a{};
    a.in = d_in;
    a.out = d_out;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.n_in = d_nin;
    a.n_out = d_nout;
    a.n_in_uniform = n_uniform;
    a.n_out_uniform = len_uniform;
    a.channels = channels;
    a.L = pl->L;
    a.M = pl->M;
    a.K = pl->K;
    a.taps = pl->taps.as<double>();
    const dim3 grid((unsigned)(((unsigned long long)len_max + 255) / 256), (unsigned)n_pairs);
    hipLaunchKernelGGL(resample_any_kernel, grid, dim3(256), 0, stream, a);
  }
  HIP_TRY(hipGetLastError());
  if (slot) return c->rs->lens.sent(slot, stream);
  return PEAQ_OK;
}

extern "C" int peaq_run_pair_rate(peaq_ctx* c, int advanced, int channels, double level_db, uint32_t rate,
                                  const float* ref, size_t n_ref, const float* test, size_t n_test, peaq_result* out) {
  if (rate == 48000) return peaq_run_pair(c, advanced, channels, level_db, ref, n_ref, test, n_test, out);
  if (int rc = check_rate("peaq_run_pair_rate", rate)) return rc;
  // (the playback level is not looked at here: peaq_run_pair, which a rate of 48000 goes to, does not either)
  if (int rc = check_pair_args("peaq_run_pair_rate", c, channels, rate, ref, n_ref, test, n_test, out, true)) return rc;
  PairBuffers in;
  if (int rc = upload_pair_48k(c, channels, rate, ref, n_ref, test, n_test, in)) return rc;
  return score_one_pair(c, advanced, channels, level_db, in.d(0), in.d(1), in.stride, in.len[0], in.len[1], out);
}

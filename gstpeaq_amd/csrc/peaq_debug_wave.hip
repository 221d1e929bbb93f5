// peaq_debug_wave.hip -- the primitives of peaq_wave.h on their own (include/peaq_amd.h, peaq_debug_wave): host
// arrays in, one small kernel that calls the very inline functions the product kernels are made of, host arrays
// out.  tests/test_gpu_wave_primitives.py compares what comes back with high-precision references.
//
// Every wave runs with all 64 lanes active (the arrays are padded to whole workgroups of four waves, so wave
// indices 1 .. 3 of a workgroup are exercised too), and nothing in the kernel branches on data: NaN and infinity
// are arguments like any other.
#include "peaq_host.h"
#include "peaq_wave.h"

using namespace peaq;

namespace {

constexpr int kWgThreads = 256;                      // four waves per workgroup

enum WaveOp : int {
  OP_LOG_POS, OP_LOG_POS_SK, OP_LOG_NONNEG, OP_LOG_NONNEG_SK, OP_LOG_TAB, OP_LOG_TAB_NONNEG,
  OP_EXP_FAST, OP_EXP_FAST_SK, OP_EXP_TAB, OP_SQRT_POS, OP_RSQRT_POS, OP_DIV_FAST, OP_POW_POS, OP_POW_TAB,
  OP_POW_LOGTAB, OP_LOG_NONNEG_N5, OP_EXP_FAST_N5,
  OP_WAVE_SUM, OP_WAVE_MAX, OP_WAVE_SUM2, OP_WAVE_SUM4, OP_WAVE_PREFIX_SUM, OP_WAVE_SUFFIX_GEOMETRIC,
  OP_WAVE_PREFIX_GEOMETRIC, OP_WAVE_PREFIX_GEOMETRIC_Z, OP_WAVE_PREFIX_GEOMETRIC_F32, OP_ROWS_TRANSPOSE4,
  OP_LANE_BELOW, OP_LANE_ABOVE, OP_READ_LANE_0, OP_READ_LANE_63, OP_DFT4, OP_DFT8, OP_DFT16, OP_COUNT
};

struct OpInfo {
  const char* name;
  int planes_in, planes_out, n_params;
};
// (in the order of WaveOp)
const OpInfo kOps[OP_COUNT] = {
    {"log_pos", 1, 1, 0},                 // log_pos<false>
    {"log_pos_sk", 1, 1, 0},              // log_pos<true>: the constants in scalar registers
    {"log_nonneg", 1, 1, 0},              // log_nonneg<false>
    {"log_nonneg_sk", 1, 1, 0},           // log_nonneg<true>
    {"log_tab", 1, 1, 0},
    {"log_tab_nonneg", 1, 1, 0},
    {"exp_fast", 1, 1, 0},                // exp_fast<false>
    {"exp_fast_sk", 1, 1, 0},             // exp_fast<true>
    {"exp_tab", 1, 1, 0},
    {"sqrt_pos", 1, 1, 0},
    {"rsqrt_pos", 1, 1, 0},
    {"div_fast", 2, 1, 0},                // in[0] / in[1]
    {"pow_pos", 2, 1, 0},                 // in[0] ^ in[1]
    {"pow_tab", 2, 1, 0},                 // exp_tab(y log_tab(x)): GlobalTabs::pow of peaq_backend.hip
    {"pow_logtab", 2, 1, 0},              // exp_fast(y log_tab(x)): LdsTabs::pow of peaq_backend.hip
    {"log_nonneg_n5", 5, 5, 0},           // log_nonneg_n<5>: plane k is element k of every lane's array
    {"exp_fast_n5", 5, 5, 0},
    {"wave_sum", 1, 1, 0},
    {"wave_max", 1, 1, 0},
    {"wave_sum2", 2, 2, 0},
    {"wave_sum4", 4, 4, 0},
    {"wave_prefix_sum", 1, 1, 0},
    {"wave_suffix_geometric", 1, 1, 1},   // params[0] = m
    {"wave_prefix_geometric", 1, 1, 1},   // the double overload without zero registers
    {"wave_prefix_geometric_z", 3, 3, 1}, // three scans in a row through the SAME z15 / z31
    {"wave_prefix_geometric_f32", 1, 1, 1},
    {"rows_transpose4", 4, 4, 0},
    {"lane_below", 1, 1, 0},
    {"lane_above", 1, 1, 0},
    {"read_lane_0", 1, 1, 0},             // read_lane<0>
    {"read_lane_63", 1, 1, 0},            // read_lane<63>
    {"dft4", 8, 8, 0},                    // planes 2 k, 2 k + 1: real and imaginary part of x[k]
    {"dft8", 16, 16, 0},
    {"dft16", 32, 32, 0},
};

// m^e by squaring and multiplying: the pow_m of fb_bank_kernel (peaq_fb.hip), which forms the scan's row weights
// decay_row = m^((lane & 15) + 1) with it
template <typename T>
__device__ __forceinline__ T pow_m(T m, int e) {
  T p = m, acc = 1;
  while (e) {
    if (e & 1) acc *= p;
    p *= p;
    e >>= 1;
  }
  return acc;
}

template <int OP, int N>
__device__ __forceinline__ void run_dft(const double* __restrict__ in, double* __restrict__ out, size_t n, size_t i) {
  cplx x[N];
#pragma unroll
  for (int k = 0; k < N; ++k) x[k] = {in[(2 * k) * n + i], in[(2 * k + 1) * n + i]};
  if constexpr (OP == OP_DFT4) dft4(x[0], x[1], x[2], x[3]);
  if constexpr (OP == OP_DFT8) dft8(x);
  if constexpr (OP == OP_DFT16) dft16(x);
#pragma unroll
  for (int k = 0; k < N; ++k) {
    out[(2 * k) * n + i] = x[k].re;
    out[(2 * k + 1) * n + i] = x[k].im;
  }
}

// in / out: planes of n doubles each, n a multiple of kWgThreads; element i of a plane belongs to lane i & 63 of
// wave i >> 6
template <int OP>
__global__ __launch_bounds__(kWgThreads) void debug_wave_kernel(const double* __restrict__ in, double* __restrict__ out,
                                                                size_t n, double m, const CommonTables* __restrict__ ct) {
  // the tables of log_tab / exp_tab in LDS, filled like fb_backend_kernel fills its own (peaq_backend_fb.inc);
  // log_tab reads an entry as one 16-byte double2
  __shared__ __attribute__((aligned(16))) double sh_ltab[2 * kLogTabEntries + 2];
  __shared__ double sh_etab[kExpTabEntries];
  for (int k = threadIdx.x; k < 2 * kLogTabEntries; k += blockDim.x) sh_ltab[k] = ct->log_tab[k >> 1][k & 1];
  if (threadIdx.x < kExpTabEntries) sh_etab[threadIdx.x] = ct->exp_tab[threadIdx.x];
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * kWgThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  auto X = [&](int p) { return in[(size_t)p * n + i]; };
  auto Y = [&](int p, double v) { out[(size_t)p * n + i] = v; };

  if constexpr (OP == OP_LOG_POS) Y(0, log_pos<false>(X(0)));
  if constexpr (OP == OP_LOG_POS_SK) Y(0, log_pos<true>(X(0)));
  if constexpr (OP == OP_LOG_NONNEG) Y(0, log_nonneg<false>(X(0)));
  if constexpr (OP == OP_LOG_NONNEG_SK) Y(0, log_nonneg<true>(X(0)));
  if constexpr (OP == OP_LOG_TAB) Y(0, log_tab(X(0), sh_ltab));
  if constexpr (OP == OP_LOG_TAB_NONNEG) Y(0, log_tab_nonneg(X(0), sh_ltab));
  if constexpr (OP == OP_EXP_FAST) Y(0, exp_fast<false>(X(0)));
  if constexpr (OP == OP_EXP_FAST_SK) Y(0, exp_fast<true>(X(0)));
  if constexpr (OP == OP_EXP_TAB) Y(0, exp_tab(X(0), sh_etab));
  if constexpr (OP == OP_SQRT_POS) Y(0, sqrt_pos(X(0)));
  if constexpr (OP == OP_RSQRT_POS) Y(0, rsqrt_pos(X(0)));
  if constexpr (OP == OP_DIV_FAST) Y(0, div_fast(X(0), X(1)));
  if constexpr (OP == OP_POW_POS) Y(0, pow_pos(X(0), X(1)));
  if constexpr (OP == OP_POW_TAB) Y(0, exp_tab(X(1) * log_tab(X(0), sh_ltab), sh_etab));
  if constexpr (OP == OP_POW_LOGTAB) Y(0, exp_fast(X(1) * log_tab(X(0), sh_ltab)));
  if constexpr (OP == OP_LOG_NONNEG_N5 || OP == OP_EXP_FAST_N5) {
    double x[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) x[k] = X(k);
    if constexpr (OP == OP_LOG_NONNEG_N5) log_nonneg_n<5>(x);
    if constexpr (OP == OP_EXP_FAST_N5) exp_fast_n<5>(x);
#pragma unroll
    for (int k = 0; k < 5; ++k) Y(k, x[k]);
  }
  if constexpr (OP == OP_WAVE_SUM) Y(0, wave_sum(X(0)));
  if constexpr (OP == OP_WAVE_MAX) Y(0, wave_max(X(0)));
  if constexpr (OP == OP_WAVE_SUM2) {
    double sa, sb;
    wave_sum2(X(0), X(1), sa, sb);
    Y(0, sa);
    Y(1, sb);
  }
  if constexpr (OP == OP_WAVE_SUM4) {
    double sa, sb, sc, sd;
    wave_sum4(X(0), X(1), X(2), X(3), sa, sb, sc, sd);
    Y(0, sa);
    Y(1, sb);
    Y(2, sc);
    Y(3, sd);
  }
  if constexpr (OP == OP_WAVE_PREFIX_SUM) Y(0, wave_prefix_sum(X(0), lane));
  if constexpr (OP == OP_WAVE_SUFFIX_GEOMETRIC) Y(0, wave_suffix_geometric(X(0), m, lane));
  if constexpr (OP == OP_WAVE_PREFIX_GEOMETRIC || OP == OP_WAVE_PREFIX_GEOMETRIC_Z) {
    // the weights as fb_bank_kernel forms them (peaq_fb.hip, kM1 .. kM16 and decay_row): the powers of two by
    // repeated squaring, the row weight m^((lane & 15) + 1) by pow_m
    const double wl = pow_m(m, (lane & 15) + 1);
    const double m1 = m, m2 = m1 * m1, m4 = m2 * m2, m8 = m4 * m4, m16 = m8 * m8;
    if constexpr (OP == OP_WAVE_PREFIX_GEOMETRIC) {
      Y(0, wave_prefix_geometric(X(0), m1, m2, m4, m8, m16, wl, lane));
    } else {
      double z15 = 0., z31 = 0.;
      const double v0 = wave_prefix_geometric(X(0), m1, m2, m4, m8, m16, wl, lane, z15, z31);
      const double v1 = wave_prefix_geometric(X(1), m1, m2, m4, m8, m16, wl, lane, z15, z31);
      const double v2 = wave_prefix_geometric(X(2), m1, m2, m4, m8, m16, wl, lane, z15, z31);
      Y(0, v0);
      Y(1, v1);
      Y(2, v2);
    }
  }
  if constexpr (OP == OP_WAVE_PREFIX_GEOMETRIC_F32) {
    // the FP32 overload: the same formation of the weights, in FP32 from (float)m; data rounded to FP32 on the way in
    const float mf = (float)m, wl = pow_m(mf, (lane & 15) + 1);
    const float m1 = mf, m2 = m1 * m1, m4 = m2 * m2, m8 = m4 * m4, m16 = m8 * m8;
    Y(0, (double)wave_prefix_geometric((float)X(0), m1, m2, m4, m8, m16, wl, lane));
  }
  if constexpr (OP == OP_ROWS_TRANSPOSE4) {
    double x0 = X(0), x1 = X(1), x2 = X(2), x3 = X(3);
    rows_transpose4(x0, x1, x2, x3);
    Y(0, x0);
    Y(1, x1);
    Y(2, x2);
    Y(3, x3);
  }
  if constexpr (OP == OP_LANE_BELOW) Y(0, lane_below(X(0)));
  if constexpr (OP == OP_LANE_ABOVE) Y(0, lane_above(X(0)));
  if constexpr (OP == OP_READ_LANE_0) Y(0, read_lane<0>(X(0)));
  if constexpr (OP == OP_READ_LANE_63) Y(0, read_lane<63>(X(0)));
  if constexpr (OP == OP_DFT4) run_dft<OP, 4>(in, out, n, i);
  if constexpr (OP == OP_DFT8) run_dft<OP, 8>(in, out, n, i);
  if constexpr (OP == OP_DFT16) run_dft<OP, 16>(in, out, n, i);
}

template <int OP>
hipError_t launch_one(int op, const double* in, double* out, size_t n, double m, const CommonTables* ct) {
  if (op == OP) {
    debug_wave_kernel<OP><<<dim3((unsigned)(n / kWgThreads)), dim3(kWgThreads)>>>(in, out, n, m, ct);
    return hipGetLastError();
  }
  if constexpr (OP + 1 < OP_COUNT) return launch_one<OP + 1>(op, in, out, n, m, ct);
  return hipErrorInvalidValue;
}

}  // namespace

extern "C" int peaq_debug_wave(peaq_ctx* c, const char* op, size_t n, int planes_in, const double* in, int n_params,
                               const double* params, int planes_out, double* out) {
  // everything that can be told without a device first
  if (!op) return fail(PEAQ_ERR_ARG, "peaq_debug_wave: NULL op");
  int which = -1;
  for (int k = 0; k < OP_COUNT; ++k)
    if (!std::strcmp(op, kOps[k].name)) which = k;
  if (which < 0) return fail(PEAQ_ERR_ARG, std::string("peaq_debug_wave: unknown op '") + op + "'");
  const OpInfo& info = kOps[which];
  if (planes_in != info.planes_in || planes_out != info.planes_out)
    return fail(PEAQ_ERR_ARG, std::string("peaq_debug_wave: ") + op + " takes " + std::to_string(info.planes_in) +
                                  " planes and returns " + std::to_string(info.planes_out));
  if (n_params != info.n_params || (n_params > 0 && !params))
    return fail(PEAQ_ERR_ARG, std::string("peaq_debug_wave: ") + op + " takes " + std::to_string(info.n_params) + " parameters");
  if (!c || !in || !out) return fail(PEAQ_ERR_ARG, "peaq_debug_wave: NULL argument");
  if (n > ((size_t)1 << 26)) return fail(PEAQ_ERR_ARG, "peaq_debug_wave: more than 2^26 elements per plane");
  if (n == 0) return PEAQ_OK;
  HIP_TRY(hipSetDevice(c->device));
  const size_t n_pad = (n + kWgThreads - 1) / kWgThreads * kWgThreads;   // whole workgroups: every lane of every wave active
  DevBuf d_in, d_out;
  HIP_TRY(d_in.reserve((size_t)planes_in * n_pad * sizeof(double)));
  HIP_TRY(d_out.reserve((size_t)planes_out * n_pad * sizeof(double)));
  HIP_TRY(hipMemset(d_in.p, 0, (size_t)planes_in * n_pad * sizeof(double)));    // the padding reads 0.
  HIP_TRY(hipMemset(d_out.p, 0, (size_t)planes_out * n_pad * sizeof(double)));
  for (int p = 0; p < planes_in; ++p)
    HIP_TRY(hipMemcpy(d_in.as<double>() + (size_t)p * n_pad, in + (size_t)p * n, n * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(launch_one<0>(which, d_in.as<double>(), d_out.as<double>(), n_pad, n_params ? params[0] : 0., c->d_common));
  HIP_TRY(hipDeviceSynchronize());
  for (int p = 0; p < planes_out; ++p)
    HIP_TRY(hipMemcpy(out + (size_t)p * n, d_out.as<double>() + (size_t)p * n_pad, n * sizeof(double), hipMemcpyDeviceToHost));
  return PEAQ_OK;
}

// host only: the tables log_tab / exp_tab read, as build_common_tables makes them for every context
extern "C" int peaq_debug_common_tables(double* log_tab, double* exp_tab) {
  if (!log_tab || !exp_tab) return fail(PEAQ_ERR_ARG, "peaq_debug_common_tables: NULL argument");
  auto ct = std::make_unique<CommonTables>();
  build_common_tables(*ct);
  std::memcpy(log_tab, ct->log_tab, sizeof ct->log_tab);
  std::memcpy(exp_tab, ct->exp_tab, sizeof ct->exp_tab);
  return PEAQ_OK;
}

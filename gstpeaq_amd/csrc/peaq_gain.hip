// peaq_gain.hip -- level and polarity matching between delay estimation and the cut (peaq_batch_measure_gain,
// peaq_batch_cut_scaled, peaq_gain_workspace_bytes; include/peaq_amd.h).
//
//   gain_measure_kernel      one workgroup per chunk of PEAQ_GAIN_CHUNK samples per channel of one pair: the three sums
//       sum r^2, sum t^2, sum r t per channel over the chunk, in FP64 (a product of two FP32 values is exact in FP64, so
//       only the additions round).  Both streams are read at their own offsets of the uncut buffers; whether a stream's
//       loads are 16 bytes wide or four dwords follows from its base, its stride and its skip, is decided per stream
//       and is the same for the whole workgroup.  The order of the additions is a matter of the index within the pair
//       alone -- never of an address -- so the phases change how the samples are loaded and nothing of what is added
//       to what: lane by lane over the vector units it owns (unit = thread + 256 j), then the wave (peaq::wave_sum),
//       then the four waves ((0 + 1) + (2 + 3)).  The last chunk's last, partial unit is its owner's, guarded.
//       One partial per sum and channel to the scratch; no atomics.
//   gain_finish_kernel       one workgroup per pair: thread t adds the partials of chunks t, t + 256, ... in chunk order,
//       then the same fixed tree; thread 0 derives the gain in FP64 and writes the record.
//   gain_cut_kernel          peaq_batch_cut_scaled: align_cut_kernel's copy (copy_run, peaq_host.h) with the pair's two
//       factors read from its record; a factor of exactly 1.0 moves the bits.
#include "peaq_host.h"

namespace {

constexpr uint32_t kGnChunk = PEAQ_GAIN_CHUNK;         // samples per channel per workgroup
constexpr size_t kGnPartial = 6 * sizeof(double);      // srr[2], stt[2], srt[2] of one chunk
constexpr size_t kGnScratchBudget = (size_t)256 << 20; // pairs are taken in groups whose partials stay below this
static_assert(kGnChunk % 1024 == 0, "a chunk is a whole number of vector units per thread, mono and stereo");

__host__ __device__ inline uint32_t gain_chunks(uint32_t n) { return (uint32_t)(((uint64_t)n + kGnChunk - 1) / kGnChunk); }

struct GainArgs {
  const float* ref;             // first pair of the group
  const float* test;
  size_t ref_stride, test_stride;
  const uint32_t* skip_ref;     // device, first pair of the group
  const uint32_t* skip_test;
  const uint32_t* n;
  int channels;
  int mode;                     // PEAQ_GAIN_* with PEAQ_GAIN_PER_CHANNEL or-ed in
  double g_lo, g_hi;            // 10^(-max_gain_db / 20), 10^(max_gain_db / 20)
  uint32_t nch_max;             // chunks of the call's longest pair: the partials' row length
  double* part;                 // [pair][nch_max][6]
  peaq_gain* out;               // first pair of the group
};

__device__ __forceinline__ float4 gn_load4(const float* __restrict__ s, bool vec) {
  if (vec) return *reinterpret_cast<const float4*>(s);
  return {s[0], s[1], s[2], s[3]};
}

template <int C>
__device__ __forceinline__ void gn_add(double (&s)[6], int e, float rf, float tf) {
  const int c = C == 2 ? (e & 1) : 0;                // (a unit starts at an even float of the pair)
  const double r = (double)rf, t = (double)tf;
  s[c] += r * r;
  s[2 + c] += t * t;
  s[4 + c] += r * t;
}

template <int C>
__device__ __forceinline__ void gn_measure(const GainArgs& a, double (*sh)[6]) {
  const unsigned pair = blockIdx.y, chunk = blockIdx.x;
  const size_t count = (size_t)a.n[pair] * C;        // floats of the pair
  const size_t f0 = (size_t)chunk * kGnChunk * C;    // the chunk's first
  if (f0 >= count) return;                           // (the whole workgroup; also a pair of no samples)
  const float* __restrict__ r = a.ref + ((size_t)pair * a.ref_stride + a.skip_ref[pair]) * C + f0;
  const float* __restrict__ t = a.test + ((size_t)pair * a.test_stride + a.skip_test[pair]) * C + f0;
  const size_t len = min(count - f0, (size_t)kGnChunk * C);
  const unsigned vecs = (unsigned)(len / 4), rest = (unsigned)(len & 3);
  const bool rvec = ((uintptr_t)r & 15) == 0, tvec = ((uintptr_t)t & 15) == 0;   // per stream, uniform
  double s[6] = {0., 0., 0., 0., 0., 0.};
  constexpr unsigned J = kGnChunk * C / 1024;        // units per thread in a whole chunk
  if (vecs == J * 256) {                             // (uniform) a whole chunk: every load issued before the sums
    float4 x[J], y[J];
#pragma unroll
    for (unsigned j = 0; j < J; ++j) {
      x[j] = gn_load4(r + 4 * (size_t)(threadIdx.x + 256 * j), rvec);
      y[j] = gn_load4(t + 4 * (size_t)(threadIdx.x + 256 * j), tvec);
    }
#pragma unroll
    for (unsigned j = 0; j < J; ++j) {
      gn_add<C>(s, 0, x[j].x, y[j].x);
      gn_add<C>(s, 1, x[j].y, y[j].y);
      gn_add<C>(s, 2, x[j].z, y[j].z);
      gn_add<C>(s, 3, x[j].w, y[j].w);
    }
  } else {                                           // the pair's last chunk: the same units in the same order
    for (unsigned v = threadIdx.x; v < vecs; v += 256) {
      const float4 x = gn_load4(r + 4 * (size_t)v, rvec), y = gn_load4(t + 4 * (size_t)v, tvec);
      gn_add<C>(s, 0, x.x, y.x);
      gn_add<C>(s, 1, x.y, y.y);
      gn_add<C>(s, 2, x.z, y.z);
      gn_add<C>(s, 3, x.w, y.w);
    }
    if (rest && threadIdx.x == (vecs & 255))         // the tail, at most 3 floats: the unit's owner, after its whole ones
      for (unsigned e = 0; e < rest; ++e) gn_add<C>(s, (int)e, r[4 * (size_t)vecs + e], t[4 * (size_t)vecs + e]);
  }
  block_sum4(s, sh);
  if (threadIdx.x == 0) {
    double* P = a.part + ((size_t)pair * a.nch_max + chunk) * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) P[k] = s[k];
  }
}

__global__ __launch_bounds__(256) void gain_measure_kernel(const GainArgs a) {
  __shared__ double sh[4][6];
  if (a.channels == 2)
    gn_measure<2>(a, sh);
  else
    gn_measure<1>(a, sh);
}

__device__ __forceinline__ uint32_t gn_derive(int base, double srr, double stt, double srt, bool empty, double lo, double hi,
                                              double* g_out) {
  double g = 1.;
  uint32_t fl = 0;
  if (!isfinite(srr) || !isfinite(stt) || !isfinite(srt)) {
    fl = PEAQ_GAIN_F_NONFINITE;
  } else if (empty || stt == 0.) {
    fl = PEAQ_GAIN_F_SILENT;
  } else if (base == PEAQ_GAIN_LSQ && srt == 0.) {
    fl = PEAQ_GAIN_F_ZERO;
  } else if (base != PEAQ_GAIN_OFF) {
    if (base == PEAQ_GAIN_LSQ)
      g = srt / stt;
    else if (base == PEAQ_GAIN_RMS)
      g = copysign(sqrt(srr / stt), srt < 0. ? -1. : 1.);
    else
      g = srt < 0. ? -1. : 1.;
    if (!(fabs(g) >= lo && fabs(g) <= hi)) {          // |20 log10 |g|| > max_gain_db; also a g of 0 or Inf
      fl = PEAQ_GAIN_F_RANGE;
      g = 1.;
    }
  }
  *g_out = g;
  return fl;
}

__global__ __launch_bounds__(256) void gain_finish_kernel(const GainArgs a) {
  __shared__ double sh[4][6];
  const unsigned pair = blockIdx.x;
  const uint32_t n = a.n[pair];
  const uint32_t nch = gain_chunks(n);
  const double* __restrict__ P = a.part + (size_t)pair * a.nch_max * 6;
  double s[6] = {0., 0., 0., 0., 0., 0.};
  for (uint32_t ch = threadIdx.x; ch < nch; ch += 256) {   // chunk order
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] += P[(size_t)ch * 6 + k];
  }
  block_sum4(s, sh);
  if (threadIdx.x != 0) return;
  peaq_gain rec;
  for (int c = 0; c < 2; ++c) {
    rec.srr[c] = s[c];
    rec.stt[c] = s[2 + c];
    rec.srt[c] = s[4 + c];
  }
  rec.n = n;
  rec.reserved = 0;
  const int base = a.mode & 0xF;
  if (a.channels == 2 && (a.mode & PEAQ_GAIN_PER_CHANNEL)) {
    for (int c = 0; c < 2; ++c) rec.flags[c] = gn_derive(base, s[c], s[2 + c], s[4 + c], n == 0, a.g_lo, a.g_hi, &rec.gain[c]);
  } else {                                           // one factor: channel 0's sums and channel 1's (zeros for mono), 0 first
    bool finite = true;
    for (int k = 0; k < 6; ++k) finite = finite && isfinite(s[k]);
    const double srr = s[0] + s[1], stt = s[2] + s[3], srt = s[4] + s[5];
    rec.flags[0] = gn_derive(base, finite ? srr : __builtin_nan(""), stt, srt, n == 0, a.g_lo, a.g_hi, &rec.gain[0]);
    rec.flags[1] = rec.flags[0];
    rec.gain[1] = rec.gain[0];
  }
  a.out[pair] = rec;
}

struct ScaledCutArgs {
  const float* in;
  float* out;
  size_t in_stride, out_stride;  // samples per channel between pairs
  const uint32_t* skip;          // device [n_pairs]
  const uint32_t* n_keep;        // device [n_pairs]
  const peaq_gain* gain;         // device [n_pairs]
  int channels;
};

// one rounding: the product in FP64, then to FP32; a factor of exactly 1.0 moves the bits
__device__ __forceinline__ float gn_scale(float x, double g) {
  const float y = (float)((double)x * g);
  return __uint_as_float(g == 1. ? __float_as_uint(x) : __float_as_uint(y));
}

// (both factors are read, then one is chosen: a choice between the two members themselves becomes an indexed read of
// the functor, which then does not dissolve into registers)
__device__ __forceinline__ double gn_pick(bool odd, double g_even, double g_odd) { return odd ? g_odd : g_even; }

// what copy_run stores: float i of a pair's run belongs to channel i mod channels
struct GnScale {
  double g0, g1;
  bool plain;                   // (uniform) an unmatched pair: peaq_batch_cut's copy
  __device__ __forceinline__ float4 operator()(float4 x, size_t i) const {
    if (plain) return x;
    const double ge = of(i), go = of(i + 1);           // of the unit's even and odd floats
    return {gn_scale(x.x, ge), gn_scale(x.y, go), gn_scale(x.z, ge), gn_scale(x.w, go)};
  }
  __device__ __forceinline__ float operator()(float x, size_t i) const { return plain ? x : gn_scale(x, of(i)); }
  __device__ __forceinline__ double of(size_t i) const { return gn_pick(i & 1, g0, g1); }
};

__global__ __launch_bounds__(256) void gain_cut_kernel(const ScaledCutArgs a) {
  const unsigned pair = blockIdx.y;
  const size_t count = (size_t)a.n_keep[pair] * a.channels;
  const float* __restrict__ src = a.in + ((size_t)pair * a.in_stride + a.skip[pair]) * a.channels;
  float* __restrict__ dst = a.out + (size_t)pair * a.out_stride * a.channels;
  const double g0 = a.gain[pair].gain[0], g1 = a.channels == 2 ? a.gain[pair].gain[1] : g0;
  copy_run(src, dst, count, (size_t)blockIdx.x * 256, blockIdx.x == 0, GnScale{g0, g1, g0 == 1. && g1 == 1.});
}

size_t gain_per_pair(uint32_t n_max) { return std::max<size_t>(gain_chunks(n_max), 1) * kGnPartial; }

}  // namespace

struct GainState {
  StageScratch scratch;         // the partials of a group of pairs
  LenStage lens;                // measure: [skip_ref | skip_test | n]; cut_scaled: [skip | n_keep]
};

void gain_release(peaq_ctx* c) { release_stage(c->gn); }

int check_gain_mode(const std::string& who, int mode, double max_gain_db) {
  if (mode < 0 || (mode & ~(0xF | PEAQ_GAIN_PER_CHANNEL)) || (mode & 0xF) > PEAQ_GAIN_POLARITY)
    return fail(PEAQ_ERR_ARG, who + ": mode " + std::to_string(mode) + " is not a PEAQ_GAIN_* mode with or without PEAQ_GAIN_PER_CHANNEL");
  if (!(max_gain_db > 0. && max_gain_db <= 120.))
    return fail(PEAQ_ERR_ARG, who + ": max_gain_db " + std::to_string(max_gain_db) + " is outside 0 < x <= 120");
  return PEAQ_OK;
}

extern "C" size_t peaq_gain_size(void) { return sizeof(peaq_gain); }

extern "C" size_t peaq_gain_workspace_bytes(int channels, int n_pairs, uint32_t n_max) {
  if (channels != 1 && channels != 2) return 0;
  return pair_groups(gain_per_pair(n_max), n_pairs, kGnScratchBudget).bytes;
}

extern "C" int peaq_batch_measure_gain(peaq_ctx* c, int channels, int n_pairs, const float* d_ref, size_t ref_stride,
                                       const uint32_t* skip_ref, const float* d_test, size_t test_stride,
                                       const uint32_t* skip_test, const uint32_t* n, int mode, double max_gain_db,
                                       peaq_gain* d_out, void* stream_) {
  const std::string w("peaq_batch_measure_gain");
  if (int rc = check_gain_mode(w, mode, max_gain_db)) return rc;
  if (int rc = check_shape(w, channels, n_pairs)) return rc;
  if (n_pairs > 0 && (!d_ref || !d_test || !d_out)) return fail(PEAQ_ERR_ARG, w + ": NULL buffer");
  if (n_pairs > 0 && (!skip_ref || !skip_test || !n)) return fail(PEAQ_ERR_ARG, w + ": NULL skip_ref, skip_test or n");
  const size_t np = (size_t)n_pairs;
  std::vector<uint32_t> h(3 * np);
  uint32_t n_max = 0;
  for (size_t p = 0; p < np; ++p) {
    if ((uint64_t)skip_ref[p] + n[p] > ref_stride)
      return fail(PEAQ_ERR_ARG, w + ": pair " + std::to_string(p) + ": skip_ref " + std::to_string(skip_ref[p]) + " + n " +
                                    std::to_string(n[p]) + " passes ref_stride " + std::to_string(ref_stride));
    if ((uint64_t)skip_test[p] + n[p] > test_stride)
      return fail(PEAQ_ERR_ARG, w + ": pair " + std::to_string(p) + ": skip_test " + std::to_string(skip_test[p]) + " + n " +
                                    std::to_string(n[p]) + " passes test_stride " + std::to_string(test_stride));
    h[p] = skip_ref[p];
    h[np + p] = skip_test[p];
    h[2 * np + p] = n[p];
    n_max = std::max(n_max, n[p]);
  }
  if (!c) return fail(PEAQ_ERR_ARG, w + ": ctx is NULL");
  if (n_pairs == 0) return PEAQ_OK;

  hipStream_t stream = static_cast<hipStream_t>(stream_);
  std::lock_guard<std::mutex> lock(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  if (!c->gn) c->gn = new GainState;
  GainState* st = c->gn;
  const uint32_t nch = std::max<uint32_t>(gain_chunks(n_max), 1);
  const PairGroups pg = pair_groups(gain_per_pair(n_max), n_pairs, kGnScratchBudget);
  const int group = pg.group;
  if (int rc = st->scratch.acquire(pg.bytes, stream)) return rc;
  LenSlot* slot = nullptr;
  if (int rc = st->lens.upload(h.data(), h.size(), stream, &slot)) return rc;
  GainArgs a{};
  a.ref_stride = ref_stride;
  a.test_stride = test_stride;
  a.channels = channels;
  a.mode = mode;
  a.g_lo = std::pow(10., -max_gain_db / 20.);
  a.g_hi = std::pow(10., max_gain_db / 20.);
  a.nch_max = nch;
  a.part = st->scratch.buf.as<double>();
  hipError_t launched = hipSuccess;
  for (int p0 = 0; p0 < n_pairs; p0 += group) {
    const unsigned g = (unsigned)std::min(group, n_pairs - p0);
    a.ref = d_ref + (size_t)p0 * ref_stride * channels;
    a.test = d_test + (size_t)p0 * test_stride * channels;
    a.skip_ref = slot->dev.as<uint32_t>() + p0;
    a.skip_test = a.skip_ref + np;
    a.n = a.skip_test + np;
    a.out = d_out + p0;
    if (n_max) hipLaunchKernelGGL(gain_measure_kernel, dim3(nch, g), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(gain_finish_kernel, dim3(g), dim3(256), 0, stream, a);
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

extern "C" int peaq_batch_cut_scaled(peaq_ctx* c, int channels, int n_pairs, const float* d_in, size_t in_stride,
                                     const uint32_t* skip, const uint32_t* n_keep, const peaq_gain* d_gain, float* d_out,
                                     size_t out_stride, void* stream_) {
  const std::string w("peaq_batch_cut_scaled");
  if (int rc = check_shape(w, channels, n_pairs)) return rc;
  if (n_pairs > 0 && !d_gain) return fail(PEAQ_ERR_ARG, w + ": NULL d_gain");
  if (n_pairs > 0 && (!skip || !n_keep)) return fail(PEAQ_ERR_ARG, w + ": NULL skip or n_keep");
  uint32_t keep_max = 0;
  if (int rc = check_cut_geometry(w, "pair", channels, n_pairs, n_pairs, d_in, in_stride, skip, n_keep, d_out, out_stride,
                                  &keep_max))
    return rc;
  if (!c) return fail(PEAQ_ERR_ARG, w + ": ctx is NULL");
  if (n_pairs == 0 || keep_max == 0) return PEAQ_OK;
  std::vector<uint32_t> h(skip, skip + n_pairs);
  h.insert(h.end(), n_keep, n_keep + n_pairs);

  hipStream_t stream = static_cast<hipStream_t>(stream_);
  std::lock_guard<std::mutex> lock(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  if (!c->gn) c->gn = new GainState;
  LenSlot* slot = nullptr;
  if (int rc = c->gn->lens.upload(h.data(), h.size(), stream, &slot)) return rc;
  ScaledCutArgs a{};
  a.in = d_in;
  a.out = d_out;
  a.in_stride = in_stride;
  a.out_stride = out_stride;
  a.skip = slot->dev.as<uint32_t>();
  a.n_keep = a.skip + n_pairs;
  a.gain = d_gain;
  a.channels = channels;
  const size_t vecs = ((size_t)keep_max * channels + 3) / 4;
  hipLaunchKernelGGL(gain_cut_kernel, dim3((unsigned)((vecs + 255) / 256), (unsigned)n_pairs), dim3(256), 0, stream, a);
  const hipError_t launched = hipGetLastError();
  const int sent = c->gn->lens.sent(slot, stream);   // (also after a failed launch: the copy into the slot is enqueued)
  HIP_TRY(launched);
  return sent;
}

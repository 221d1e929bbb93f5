// peaq_pcm.hip -- PCM from host memory (peaq_batch_decode_pcm, peaq_batch_run_host, peaq_feed_workspace_bytes;
// include/peaq_amd.h): the sample-format conversion as a kernel, and the feed that scores a list of host pairs chunk
// by chunk, the next chunk's packing and upload beside the running chunk's kernels.  At the end the
// same feed for tests that name shared references, each uploaded, decoded and converted once per chunk
// (peaq_batch_run_host_refs, peaq_feed_refs_workspace_bytes); it adds host code only.
//
//   pcm_decode_kernel<F>     one per format.  A thread turns 4 sb input bytes (sb = bytes per sample) into one aligned
//       16-byte store, from the first 16-byte aligned float of the pair's destination on.  Its input starts at byte
//       phase q = address & 3, the same for every thread of a pair (threads are 4 sb bytes apart): the sb aligned
//       dwords around it are loaded as ONE vector load (dwordx2 / x3 / x4; F64 two x4), one more dword when q != 0, and
//       funnel-shifted by q bytes (v_alignbyte_b32); no byte loads in the body.  A thread takes several such units, a
//       workgroup apart, loads first.  The unaligned head of the destination (at most 3 floats) and the tail (at most
//       3) are decoded sample by sample from bytes by the first workgroup.
//       No LDS; the arithmetic is exact in FP32 (U8, S16, S24: integer to float and a power of two), one conversion
//       with the hardware's round to nearest even (S32: v_cvt_f32_i32 and a power of two; F64: v_cvt_f32_f64), or a
//       copy of the bits (F32).
#include "peaq_host.h"

namespace {

constexpr int kPcmFormats = 6;
constexpr size_t kPcmBytes[kPcmFormats] = {1, 2, 3, 4, 4, 8};
constexpr uint32_t kFeedMaxLag = 16384;
constexpr size_t kFeedSlice = (size_t)1 << 20;       // host copies are dealt out to the threads in slices of 1 MiB

struct PcmArgs {
  const unsigned char* in;
  float* out;
  size_t in_stride, out_stride;  // samples per channel between pairs
  const uint32_t* n;             // device [n_pairs]; nullptr: n_uniform
  uint32_t n_uniform;
  int channels;
};

template <int N>
struct alignas(4) PcmWords {
  uint32_t w[N];
};

template <int F>
struct PcmTraits;
template <> struct PcmTraits<PEAQ_PCM_U8>  { static constexpr int SB = 1, U = 4; };
template <> struct PcmTraits<PEAQ_PCM_S16> { static constexpr int SB = 2, U = 4; };
template <> struct PcmTraits<PEAQ_PCM_S24> { static constexpr int SB = 3, U = 2; };
template <> struct PcmTraits<PEAQ_PCM_S32> { static constexpr int SB = 4, U = 2; };
template <> struct PcmTraits<PEAQ_PCM_F32> { static constexpr int SB = 4, U = 2; };
template <> struct PcmTraits<PEAQ_PCM_F64> { static constexpr int SB = 8, U = 1; };

__device__ __forceinline__ float pcm_bits(uint32_t u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ float pcm_f64(uint32_t lo, uint32_t hi) {
  return (float)__builtin_bit_cast(double, (unsigned long long)hi << 32 | lo);   // v_cvt_f32_f64: nearest even, +-Inf beyond
}
__device__ __forceinline__ float pcm_s24(uint32_t low24) { return (float)((int)(low24 << 8) >> 8) * 0x1p-23f; }

// four samples from the 4 SB bytes in d[0 .. SB)
template <int F>
__device__ __forceinline__ float4 pcm_convert4(const uint32_t* d) {
  if constexpr (F == PEAQ_PCM_U8) {
    return {((float)(d[0] & 255u) - 128.f) * 0x1p-7f, ((float)(d[0] >> 8 & 255u) - 128.f) * 0x1p-7f,
            ((float)(d[0] >> 16 & 255u) - 128.f) * 0x1p-7f, ((float)(d[0] >> 24) - 128.f) * 0x1p-7f};
  } else if constexpr (F == PEAQ_PCM_S16) {
    return {(float)((int)(d[0] << 16) >> 16) * 0x1p-15f, (float)((int)d[0] >> 16) * 0x1p-15f,
            (float)((int)(d[1] << 16) >> 16) * 0x1p-15f, (float)((int)d[1] >> 16) * 0x1p-15f};
  } else if constexpr (F == PEAQ_PCM_S24) {
    return {pcm_s24(d[0]), pcm_s24(__builtin_amdgcn_alignbyte(d[1], d[0], 3)),
            pcm_s24(__builtin_amdgcn_alignbyte(d[2], d[1], 2)), (float)((int)d[2] >> 8) * 0x1p-23f};
  } else if constexpr (F == PEAQ_PCM_S32) {          // v_cvt_f32_i32 rounds to nearest even; the scale is exact
    return {(float)(int)d[0] * 0x1p-31f, (float)(int)d[1] * 0x1p-31f, (float)(int)d[2] * 0x1p-31f,
            (float)(int)d[3] * 0x1p-31f};
  } else if constexpr (F == PEAQ_PCM_F32) {
    return {pcm_bits(d[0]), pcm_bits(d[1]), pcm_bits(d[2]), pcm_bits(d[3])};
  } else {
    return {pcm_f64(d[0], d[1]), pcm_f64(d[2], d[3]), pcm_f64(d[4], d[5]), pcm_f64(d[6], d[7])};
  }
}

// one sample from bytes (heads and tails)
template <int F>
__device__ __forceinline__ float pcm_convert1(const unsigned char* __restrict__ p) {
  constexpr int SB = PcmTraits<F>::SB;
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int i = 0; i < SB; ++i) {
    if (i < 4)
      lo |= (uint32_t)p[i] << (8 * i);
    else
      hi |= (uint32_t)p[i] << (8 * (i - 4));
  }
  if constexpr (F == PEAQ_PCM_U8) return ((float)lo - 128.f) * 0x1p-7f;
  if constexpr (F == PEAQ_PCM_S16) return (float)((int)(lo << 16) >> 16) * 0x1p-15f;
  if constexpr (F == PEAQ_PCM_S24) return pcm_s24(lo);
  if constexpr (F == PEAQ_PCM_S32) return (float)(int)lo * 0x1p-31f;
  if constexpr (F == PEAQ_PCM_F32) return pcm_bits(lo);
  return pcm_f64(lo, hi);
}

template <int F>
__global__ __launch_bounds__(256) void pcm_decode_kernel(const PcmArgs a) {
  constexpr int SB = PcmTraits<F>::SB, U = PcmTraits<F>::U;
  constexpr bool kPhased = SB < 4;                   // (wider samples sit on dwords: d_in is 4-byte aligned)
  const unsigned pair = blockIdx.y;
  const size_t count = (size_t)(a.n ? a.n[pair] : a.n_uniform) * a.channels;   // samples, all channels
  const unsigned char* __restrict__ src = a.in + (size_t)pair * a.in_stride * a.channels * SB;
  float* __restrict__ dst = a.out + (size_t)pair * a.out_stride * a.channels;
  const size_t head = min(count, (size_t)((16 - ((uintptr_t)dst & 15)) & 15) / sizeof(float));
  const size_t vecs = (count - head) / 4;
  const unsigned char* body = src + head * SB;
  const unsigned q = kPhased ? __builtin_amdgcn_readfirstlane((unsigned)((uintptr_t)body & 3)) : 0u;
  const uint32_t* __restrict__ words = reinterpret_cast<const uint32_t*>(body - q);
  uint32_t d[U][SB + 1];
#pragma unroll
  for (int j = 0; j < U; ++j) {
    const size_t v = ((size_t)blockIdx.x * U + j) * 256 + threadIdx.x;
    if (v < vecs) {
      const uint32_t* w = words + v * SB;
      if constexpr (SB == 8) {
        const PcmWords<4> x = *reinterpret_cast<const PcmWords<4>*>(w), y = *reinterpret_cast<const PcmWords<4>*>(w + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          d[j][i] = x.w[i];
          d[j][4 + i] = y.w[i];
        }
      } else {
        const PcmWords<SB> x = *reinterpret_cast<const PcmWords<SB>*>(w);
#pragma unroll
        for (int i = 0; i < SB; ++i) d[j][i] = x.w[i];
      }
      // (the dword behind holds bytes of this unit only when the phase is not 0: never a dword with no byte of the pair)
      d[j][SB] = kPhased && q ? w[SB] : 0u;
    }
  }
#pragma unroll
  for (int j = 0; j < U; ++j) {
    const size_t v = ((size_t)blockIdx.x * U + j) * 256 + threadIdx.x;
    if (v < vecs) {
      if constexpr (kPhased) {
#pragma unroll
        for (int i = 0; i < SB; ++i) d[j][i] = __builtin_amdgcn_alignbyte(d[j][i + 1], d[j][i], q);
      }
      *reinterpret_cast<float4*>(dst + head + 4 * v) = pcm_convert4<F>(d[j]);
    }
  }
  if (blockIdx.x == 0) {                             // the unaligned head and the tail: at most 3 samples each
    if (threadIdx.x < head) dst[threadIdx.x] = pcm_convert1<F>(src + (size_t)threadIdx.x * SB);
    const size_t tail = head + 4 * vecs + threadIdx.x;
    if (tail < count) dst[tail] = pcm_convert1<F>(src + tail * SB);
  }
}

template <int F>
void pcm_launch(const PcmArgs& a, uint32_t n_max, int n_pairs, hipStream_t stream) {
  const size_t per_block = (size_t)256 * PcmTraits<F>::U;
  const size_t vecs = ((size_t)n_max * a.channels + 3) / 4;
  const unsigned blocks = (unsigned)std::max<size_t>(1, (vecs + per_block - 1) / per_block);
  hipLaunchKernelGGL(pcm_decode_kernel<F>, dim3(blocks, (unsigned)n_pairs), dim3(256), 0, stream, a);
}

int check_format(const char* who, int format) {
  if (format < 0 || format >= kPcmFormats)
    return fail(PEAQ_ERR_ARG, std::string(who) + ": unknown sample format " + std::to_string(format) +
                                  " (PEAQ_PCM_U8 .. PEAQ_PCM_F64 = 0 .. 5)");
  return PEAQ_OK;
}

size_t even_stride(size_t n) {                       // 8-byte rows, as in peaq_run_pair
  n = std::max<size_t>(n, 2);
  return n + (n & 1);
}

// growable pinned host buffer
struct PinBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    release();
    const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
  template <typename T>
  T* as() const { return static_cast<T*>(p); }
};

struct FeedSet {
  PinBuf h_raw[2], h_res, h_del, h_gain;             // ref, test; the chunk's results, delay and gain records
  DevBuf d_raw[2];
  hipEvent_t uploaded = nullptr;                     // behind the copies out of h_raw into d_raw
  hipEvent_t raw_free = nullptr;                     // behind the decoder that read d_raw
  hipEvent_t res_done = nullptr;                     // behind the copy of the results into h_res
  bool upload_pending = false, raw_pending = false;
};

struct CopyJob {
  const char* src;
  char* dst;
  size_t bytes;
};

// the jobs, by `threads` host threads (the caller's among them)
void run_copies(const std::vector<CopyJob>& jobs, int threads) {
  std::atomic<size_t> next{0};
  const auto work = [&] {
    for (size_t i = next.fetch_add(1); i < jobs.size(); i = next.fetch_add(1)) std::memcpy(jobs[i].dst, jobs[i].src, jobs[i].bytes);
  };
  const int extra = (int)std::min<size_t>((size_t)std::max(threads, 1) - 1, jobs.size() > 1 ? jobs.size() - 1 : 0);
  std::vector<std::thread> pool;
  pool.reserve(extra);
  for (int t = 0; t < extra; ++t) pool.emplace_back(work);
  work();
  for (std::thread& t : pool) t.join();
}

// PEAQ_AMD_FEED_THREADS, strictly 1 .. 16
int feed_threads(int* out) {
  *out = PEAQ_FEED_DEFAULT_THREADS;
  const char* v = std::getenv("PEAQ_AMD_FEED_THREADS");
  if (!v) return PEAQ_OK;
  int n = 0;
  const size_t len = std::strlen(v);
  bool ok = len >= 1 && len <= 2;
  for (size_t i = 0; ok && i < len; ++i) {
    ok = v[i] >= '0' && v[i] <= '9';
    n = 10 * n + (v[i] - '0');
  }
  if (!ok || n < 1 || n > 16)
    return fail(PEAQ_ERR_ARG, std::string("peaq_batch_run_host: PEAQ_AMD_FEED_THREADS=\"") + v + "\" is not a number of 1 .. 16");
  *out = n;
  return PEAQ_OK;
}

// what peaq_batch_run_host and peaq_feed_workspace_bytes refuse in a feed (no device)
int check_feed(const char* who, const peaq_feed* f) {
  const std::string w(who);
  if (!f) return fail(PEAQ_ERR_ARG, w + ": feed is NULL");
  if (f->struct_size != sizeof(peaq_feed))
    return fail(PEAQ_ERR_ARG, w + ": struct_size " + std::to_string(f->struct_size) + " is not this library's sizeof (peaq_feed) = " +
                                  std::to_string(sizeof(peaq_feed)));
  if (int rc = check_format(who, f->format)) return rc;
  if (f->channels != 1 && f->channels != 2)
    return fail(PEAQ_ERR_ARG, w + ": channels must be 1 or 2, not " + std::to_string(f->channels));
  if (f->rate != 48000 && !peaq_resample_supported(f->rate))
    return fail(PEAQ_ERR_ARG, w + ": rate " + std::to_string(f->rate) + " Hz is not supported on the device");
  if (f->align_max_lag > kFeedMaxLag)
    return fail(PEAQ_ERR_ARG, w + ": align_max_lag " + std::to_string(f->align_max_lag) + " is outside 0 .. " + std::to_string(kFeedMaxLag));
  if (f->chunk_pairs > 65535)
    return fail(PEAQ_ERR_ARG, w + ": chunk_pairs " + std::to_string(f->chunk_pairs) + " is more than 65535");
  return PEAQ_OK;
}

// bytes of staging and device buffers one pair of a chunk takes when the chunk's longest signal has n samples per
// channel (n48 at 48 kHz): see PEAQ_FEED_BUDGET_BYTES in the header
size_t feed_pair_bytes(const peaq_feed& f, uint64_t n, uint64_t n48) {
  const size_t raw = (size_t)n * f.channels * kPcmBytes[f.format];
  const size_t f32 = sizeof(float) * f.channels;
  size_t b = 8 * raw + 2 * even_stride((size_t)n) * f32;
  if (f.rate != 48000) b += 2 * even_stride((size_t)n48) * f32;
  if (f.align_max_lag) b += 2 * even_stride((size_t)n48) * f32;
  return b + 2 * (sizeof(peaq_result) + sizeof(peaq_delay));
}

}  // namespace

struct FeedState {
  LenStage lens;                // peaq_batch_decode_pcm: [n_in] (under the context's lock)
  std::mutex run_mu;            // one peaq_batch_run_host at a time; everything below is its own
  FeedSet set[2];
  DevBuf f_dec[2], f_48[2], f_cut[2], d_res, d_del;
  DevBuf u_dec, u_48;           // peaq_batch_run_host_refs: a chunk's distinct references, decoded and at 48 kHz
  DevBuf d_gain;                // peaq_batch_run_host_matched: the chunk's gain records
  hipStream_t copy_s = nullptr, comp_s = nullptr;
  hipEvent_t del_done = nullptr;
};

void feed_release(peaq_ctx* c) {
  if (!c->feed) return;
  FeedState* st = c->feed;
  st->lens.release();
  for (FeedSet& s : st->set) {
    for (PinBuf& b : s.h_raw) b.release();
    s.h_res.release();
    s.h_del.release();
    s.h_gain.release();
    for (hipEvent_t e : {s.uploaded, s.raw_free, s.res_done})
      if (e) (void)hipEventDestroy(e);
  }
  if (st->del_done) (void)hipEventDestroy(st->del_done);
  if (st->copy_s) (void)hipStreamDestroy(st->copy_s);
  if (st->comp_s) (void)hipStreamDestroy(st->comp_s);
  delete st;                    // (the device buffers go with it)
  c->feed = nullptr;
}

extern "C" size_t peaq_pcm_sample_bytes(int format) { return format >= 0 && format < kPcmFormats ? kPcmBytes[format] : 0; }

extern "C" size_t peaq_feed_size(void) { return sizeof(peaq_feed); }

extern "C" int peaq_batch_decode_pcm(peaq_ctx* c, int format, int channels, int n_pairs, const void* d_in,
                                     size_t in_stride, const uint32_t* n_in, uint32_t n_uniform, float* d_out,
                                     size_t out_stride, void* stream_) {
  const char* who = "peaq_batch_decode_pcm";
  if (int rc = check_format(who, format)) return rc;
  if (channels != 1 && channels != 2)
    return fail(PEAQ_ERR_ARG, std::string(who) + ": channels must be 1 or 2, not " + std::to_string(channels));
  if (n_pairs < 0) return fail(PEAQ_ERR_ARG, std::string(who) + ": n_pairs " + std::to_string(n_pairs) + " < 0");
  if (n_pairs > 65535)
    return fail(PEAQ_ERR_ARG, std::string(who) + ": " + std::to_string(n_pairs) + " pairs are more than 65535 in one call");
  if (n_pairs > 0 && (!d_in || !d_out)) return fail(PEAQ_ERR_ARG, std::string(who) + ": NULL buffer");
  if ((uintptr_t)d_in & 3)
    return fail(PEAQ_ERR_ARG, std::string(who) + ": d_in is not 4-byte aligned (address mod 4 = " + std::to_string((uintptr_t)d_in & 3) + ")");
  uint32_t n_max = n_uniform;
  if (n_in) {
    n_max = 0;
    for (int p = 0; p < n_pairs; ++p) {
      if (n_in[p] > in_stride)
        return fail(PEAQ_ERR_ARG, std::string(who) + ": pair " + std::to_string(p) + " has " + std::to_string(n_in[p]) +
                                      " samples, more than in_stride " + std::to_string(in_stride));
      n_max = std::max(n_max, n_in[p]);
    }
  } else if (n_uniform > in_stride) {
    return fail(PEAQ_ERR_ARG, std::string(who) + ": n_uniform " + std::to_string(n_uniform) + " is more than in_stride " + std::to_string(in_stride));
  }
  if (n_pairs > 0 && n_max > out_stride)
    return fail(PEAQ_ERR_ARG, std::string(who) + ": out_stride " + std::to_string(out_stride) +
                                  " is smaller than the longest pair (" + std::to_string(n_max) + " samples)");
  if (!c) return fail(PEAQ_ERR_ARG, std::string(who) + ": ctx is NULL");
  if (n_pairs == 0 || n_max == 0) return PEAQ_OK;

  hipStream_t stream = static_cast<hipStream_t>(stream_);
  std::lock_guard<std::mutex> lock(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  if (!c->feed) c->feed = new FeedState;
  LenSlot* slot = nullptr;
  if (n_in) {
    if (int rc = c->feed->lens.upload(n_in, (size_t)n_pairs, stream, &slot)) return rc;
  }
  PcmArgs a{};
  a.in = static_cast<const unsigned char*>(d_in);
  a.out = d_out;
  a.in_stride = in_stride;
  a.out_stride = out_stride;
  a.n = slot ? slot->dev.as<uint32_t>() : nullptr;
  a.n_uniform = n_uniform;
  a.channels = channels;
  switch (format) {
    case PEAQ_PCM_U8: pcm_launch<PEAQ_PCM_U8>(a, n_max, n_pairs, stream); break;
    case PEAQ_PCM_S16: pcm_launch<PEAQ_PCM_S16>(a, n_max, n_pairs, stream); break;
    case PEAQ_PCM_S24: pcm_launch<PEAQ_PCM_S24>(a, n_max, n_pairs, stream); break;
    case PEAQ_PCM_S32: pcm_launch<PEAQ_PCM_S32>(a, n_max, n_pairs, stream); break;
    case PEAQ_PCM_F32: pcm_launch<PEAQ_PCM_F32>(a, n_max, n_pairs, stream); break;
    default: pcm_launch<PEAQ_PCM_F64>(a, n_max, n_pairs, stream); break;
  }
  const hipError_t launched = hipGetLastError();
  const int sent = slot ? c->feed->lens.sent(slot, stream) : PEAQ_OK;   // (also after a failed launch: the copy is enqueued)
  HIP_TRY(launched);
  return sent;
}

// ---------------------------------------------------------------------------
// host-fed batch
// ---------------------------------------------------------------------------
namespace {

// pairs per chunk: first pair of every chunk, and one entry behind the last
int plan_chunks(const peaq_feed& f, size_t n_pairs, const peaq_host_pair* pairs, const std::vector<uint32_t>& n48,
                std::vector<size_t>* starts) {
  starts->clear();
  size_t p = 0;
  while (p < n_pairs) {
    starts->push_back(p);
    if (f.chunk_pairs) {
      p = std::min(n_pairs, p + f.chunk_pairs);
      continue;
    }
    uint64_t longest = 0, longest48 = 0;
    size_t np = 0;
    while (p + np < n_pairs && np < 65535) {
      const uint64_t l = std::max(longest, std::max(pairs[p + np].n_ref, pairs[p + np].n_test));
      const uint64_t l48 = std::max<uint64_t>(longest48, std::max(n48[2 * (p + np)], n48[2 * (p + np) + 1]));
      if (np && (np + 1) * feed_pair_bytes(f, l, l48) > PEAQ_FEED_BUDGET_BYTES) break;   // (a pair beyond the budget: a chunk of one)
      longest = l;
      longest48 = l48;
      ++np;
    }
    p += np;
  }
  starts->push_back(n_pairs);
  return PEAQ_OK;
}

struct FeedRun {
  peaq_ctx* c;
  FeedState* st;
  peaq_feed f;
  int advanced, threads;
  double level_db;
  const peaq_host_pair* pairs;
  const std::vector<uint32_t>* n48;                   // [pair][ref, test] lengths at 48 kHz
  const std::vector<size_t>* starts;
  peaq_result* results;
  peaq_delay* delays;

  size_t first(size_t k) const { return (*starts)[k]; }
  size_t count(size_t k) const { return (*starts)[k + 1] - (*starts)[k]; }
  size_t raw_stride(size_t k) const {                // samples per channel: the chunk's longest signal
    uint64_t l = 0;
    for (size_t p = first(k); p < first(k) + count(k); ++p) l = std::max(l, std::max(pairs[p].n_ref, pairs[p].n_test));
    return (size_t)l;
  }

  // chunk k's raw bytes into its staging set at the chunk's stride, then to the device on the copy stream
  int stage(size_t k) {
    FeedSet& s = st->set[k & 1];
    const size_t np = count(k), pair_bytes = raw_stride(k) * f.channels * kPcmBytes[f.format];
    const size_t bytes = std::max<size_t>(np * pair_bytes, 16);
    if (s.upload_pending) {                            // chunk k - 2's copies still read the pinned buffers
      HIP_TRY(hipEventSynchronize(s.uploaded));
      s.upload_pending = false;
    }
    std::vector<CopyJob> jobs;
    for (int i = 0; i < 2; ++i) {
      HIP_TRY(s.h_raw[i].reserve(bytes));
      for (size_t q = 0; q < np; ++q) {
        const peaq_host_pair& pr = pairs[first(k) + q];
        const char* src = static_cast<const char*>(i ? pr.test : pr.ref);
        const size_t len = (size_t)(i ? pr.n_test : pr.n_ref) * f.channels * kPcmBytes[f.format];
        char* dst = s.h_raw[i].as<char>() + q * pair_bytes;
        for (size_t o = 0; o < len; o += kFeedSlice) jobs.push_back({src + o, dst + o, std::min(kFeedSlice, len - o)});
      }
    }
    run_copies(jobs, threads);
    if (s.raw_pending) {                               // chunk k - 2's decoder still reads the device buffers
      HIP_TRY(hipStreamWaitEvent(st->copy_s, s.raw_free, 0));
      s.raw_pending = false;
    }
    for (int i = 0; i < 2; ++i) {
      if (bytes > s.d_raw[i].cap) HIP_TRY(hipDeviceSynchronize());   // (growing frees the old buffer)
      HIP_TRY(s.d_raw[i].reserve(bytes));
      if (np * pair_bytes)
        HIP_TRY(hipMemcpyAsync(s.d_raw[i].p, s.h_raw[i].p, np * pair_bytes, hipMemcpyHostToDevice, st->copy_s));
    }
    HIP_TRY(hipEventRecord(s.uploaded, st->copy_s));
    s.upload_pending = true;
    return PEAQ_OK;
  }

  int reserve2(DevBuf (&b)[2], size_t bytes) {
    for (DevBuf& d : b) {
      if (bytes > d.cap) HIP_TRY(hipDeviceSynchronize());            // (growing frees the old buffer)
      HIP_TRY(d.reserve(std::max<size_t>(bytes, 16)));
    }
    return PEAQ_OK;
  }

  // decode through score for chunk k on the compute stream; the results travel to the set's pinned buffer
  int compute(size_t k) {
    FeedSet& s = st->set[k & 1];
    const size_t p0 = first(k), np = count(k), rs = raw_stride(k), C = (size_t)f.channels;
    hipStream_t cs = st->comp_s;
    std::vector<uint32_t> n[2], m[2];                  // lengths as uploaded, and as they stand after each stage
    for (int i = 0; i < 2; ++i) {
      n[i].resize(np);
      for (size_t q = 0; q < np; ++q) n[i][q] = (uint32_t)(i ? pairs[p0 + q].n_test : pairs[p0 + q].n_ref);
      m[i] = n[i];
    }
    HIP_TRY(hipStreamWaitEvent(cs, s.uploaded, 0));
    size_t stride = even_stride(rs);
    if (int rc = reserve2(st->f_dec, np * stride * C * sizeof(float))) return rc;
    float* cur[2] = {st->f_dec[0].as<float>(), st->f_dec[1].as<float>()};
    for (int i = 0; i < 2; ++i)
      if (int rc = peaq_batch_decode_pcm(c, f.format, f.channels, (int)np, s.d_raw[i].p, rs, n[i].data(), 0, cur[i], stride, cs))
        return rc;
    HIP_TRY(hipEventRecord(s.raw_free, cs));
    s.raw_pending = true;
    if (f.rate != 48000) {
      uint32_t longest = 0;
      for (size_t q = 0; q < np; ++q) longest = std::max(longest, std::max((*n48)[2 * (p0 + q)], (*n48)[2 * (p0 + q) + 1]));
      const size_t s48 = even_stride(longest);
      if (int rc = reserve2(st->f_48, np * s48 * C * sizeof(float))) return rc;
      for (int i = 0; i < 2; ++i) {
        if (int rc = peaq_batch_resample(c, f.channels, f.rate, (int)np, cur[i], stride, n[i].data(), 0,
                                         st->f_48[i].as<float>(), s48, m[i].data(), cs))
          return rc;
        cur[i] = st->f_48[i].as<float>();
      }
      stride = s48;
    }
    if (f.align_max_lag) {
      if (np * sizeof(peaq_delay) > st->d_del.cap) HIP_TRY(hipDeviceSynchronize());
      HIP_TRY(st->d_del.reserve(np * sizeof(peaq_delay)));
      HIP_TRY(s.h_del.reserve(np * sizeof(peaq_delay)));
      if (int rc = peaq_batch_estimate_delay(c, f.channels, (int)np, cur[0], cur[1], stride, m[0].data(), m[1].data(), 0,
                                             f.align_max_lag, st->d_del.as<peaq_delay>(), cs))
        return rc;
      HIP_TRY(hipMemcpyAsync(s.h_del.p, st->d_del.p, np * sizeof(peaq_delay), hipMemcpyDeviceToHost, cs));
      HIP_TRY(hipEventRecord(st->del_done, cs));
      HIP_TRY(hipEventSynchronize(st->del_done));    // the cut needs the lags on the host
      std::vector<uint32_t> skip[2], common(np);
      skip[0].resize(np);
      skip[1].resize(np);
      uint32_t longest = 0;
      for (size_t q = 0; q < np; ++q) {
        const peaq_delay& rec = s.h_del.as<peaq_delay>()[q];
        if (delays) delays[p0 + q] = rec;
        peaq_aligned_lengths(rec.lag, m[0][q], m[1][q], &skip[0][q], &skip[1][q], &common[q]);
        longest = std::max(longest, common[q]);
      }
      const size_t sc = even_stride(longest);
      if (int rc = reserve2(st->f_cut, np * sc * C * sizeof(float))) return rc;
      for (int i = 0; i < 2; ++i) {
        if (int rc = peaq_batch_cut(c, f.channels, (int)np, cur[i], stride, skip[i].data(), common.data(),
                                    st->f_cut[i].as<float>(), sc, cs))
          return rc;
        cur[i] = st->f_cut[i].as<float>();
        m[i] = common;
      }
      stride = sc;
    }
    if (np * sizeof(peaq_result) > st->d_res.cap) HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(st->d_res.reserve(np * sizeof(peaq_result)));
    HIP_TRY(s.h_res.reserve(np * sizeof(peaq_result)));
    if (int rc = peaq_batch_run(c, advanced, f.channels, level_db, (int)np, cur[0], cur[1], stride, m[0].data(), m[1].data(),
                                0, st->d_res.as<peaq_result>(), cs))
      return rc;
    HIP_TRY(hipMemcpyAsync(s.h_res.p, st->d_res.p, np * sizeof(peaq_result), hipMemcpyDeviceToHost, cs));
    HIP_TRY(hipEventRecord(s.res_done, cs));
    return PEAQ_OK;
  }

  int collect(size_t k) {
    FeedSet& s = st->set[k & 1];
    HIP_TRY(hipEventSynchronize(s.res_done));
    std::memcpy(results + first(k), s.h_res.p, count(k) * sizeof(peaq_result));
    return PEAQ_OK;
  }

  int run() {
    const size_t n_chunks = starts->size() - 1;
    if (int rc = stage(0)) return rc;
    for (size_t k = 0; k < n_chunks; ++k) {
      if (int rc = compute(k)) return rc;
      if (k + 1 < n_chunks)                            // packing and upload beside chunk k's kernels
        if (int rc = stage(k + 1)) return rc;
      if (k)
        if (int rc = collect(k - 1)) return rc;
    }
    return collect(n_chunks - 1);
  }
};

}  // namespace

extern "C" size_t peaq_feed_workspace_bytes(const peaq_feed* feed, int advanced, size_t n_pairs, uint64_t n_max) {
  if (check_feed("peaq_feed_workspace_bytes", feed) != PEAQ_OK || n_pairs == 0 || n_max > 0xFFFFFFFFull) return 0;
  uint64_t n48 = n_max;
  if (feed->rate != 48000) {
    n48 = peaq_resampled_length(n_max, feed->rate);
    if (n_max && !n48) return 0;
  }
  const size_t per_pair = feed_pair_bytes(*feed, n_max, n48);
  size_t chunk = feed->chunk_pairs ? feed->chunk_pairs : std::max<size_t>(1, PEAQ_FEED_BUDGET_BYTES / per_pair);
  chunk = std::min<size_t>(std::min<size_t>(chunk, n_pairs), 65535);
  size_t b = chunk * per_pair + peaq_batch_workspace_bytes(advanced, feed->channels, (int)chunk, (uint32_t)n48);
  if (feed->align_max_lag) b += peaq_align_workspace_bytes(feed->channels, (int)chunk, (uint32_t)n48, feed->align_max_lag);
  return b;
}

extern "C" int peaq_batch_run_host(peaq_ctx* c, int advanced, double level_db, const peaq_feed* feed, size_t n_pairs,
                                   const peaq_host_pair* pairs, peaq_result* results, peaq_delay* delays) {
  const char* who = "peaq_batch_run_host";
  const std::string w(who);
  if (int rc = check_feed(who, feed)) return rc;
  if (int rc = check_level(w, level_db)) return rc;
  int threads = 0;
  if (int rc = feed_threads(&threads)) return rc;
  if (n_pairs && (!pairs || !results)) return fail(PEAQ_ERR_ARG, w + ": NULL pairs or results");
  std::vector<uint32_t> n48(2 * n_pairs);
  for (size_t p = 0; p < n_pairs; ++p) {
    const uint64_t n[2] = {pairs[p].n_ref, pairs[p].n_test};
    const void* src[2] = {pairs[p].ref, pairs[p].test};
    for (int i = 0; i < 2; ++i) {
      if (n[i] && !src[i])
        return fail(PEAQ_ERR_ARG, w + ": pair " + std::to_string(p) + " has " + std::to_string(n[i]) + " samples and a NULL buffer");
      if (n[i] > 0xFFFFFFFFull)
        return fail(PEAQ_ERR_ARG, w + ": pair " + std::to_string(p) + " has " + std::to_string(n[i]) + " samples, more than 2^32 - 1");
      n48[2 * p + i] = (uint32_t)n[i];
      if (feed->rate != 48000) {
        n48[2 * p + i] = peaq_resampled_length(n[i], feed->rate);
        if (n[i] && !n48[2 * p + i]) return PEAQ_ERR_ARG;   // (the message is peaq_resampled_length's)
      }
    }
  }
  if (!c) return fail(PEAQ_ERR_ARG, w + ": ctx is NULL");
  if (n_pairs == 0) return PEAQ_OK;
  if (delays && !feed->align_max_lag) std::memset(delays, 0, n_pairs * sizeof(peaq_delay));

  FeedState* st;
  {
    std::lock_guard<std::mutex> lock(c->mu);
    if (!c->feed) c->feed = new FeedState;
    st = c->feed;
  }
  std::lock_guard<std::mutex> run_lock(st->run_mu);
  HIP_TRY(hipSetDevice(c->device));
  if (!st->copy_s) HIP_TRY(hipStreamCreateWithFlags(&st->copy_s, hipStreamNonBlocking));
  if (!st->comp_s) HIP_TRY(hipStreamCreateWithFlags(&st->comp_s, hipStreamNonBlocking));
  if (!st->del_done) HIP_TRY(hipEventCreateWithFlags(&st->del_done, hipEventDisableTiming));
  for (FeedSet& s : st->set)
    for (hipEvent_t* e : {&s.uploaded, &s.raw_free, &s.res_done})
      if (!*e) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
  std::vector<size_t> starts;
  plan_chunks(*feed, n_pairs, pairs, n48, &starts);
  FeedRun run{c, st, *feed, advanced ? 1 : 0, threads, level_db, pairs, &n48, &starts, results, delays};
  const int rc = run.run();
  if (rc != PEAQ_OK) {                               // stop: nothing more is started, what runs drains before the buffers are reused
    const std::string msg = peaq_err_string();
    (void)hipDeviceSynchronize();
    for (FeedSet& s : st->set) s.upload_pending = s.raw_pending = false;
    return fail(rc, msg);
  }
  // (every chunk's results have been collected: both streams are idle, the staging sets free)
  for (FeedSet& s : st->set) s.upload_pending = s.raw_pending = false;
  return PEAQ_OK;
}

// ---------------------------------------------------------------------------
// host-fed batch, references shared: tests[t] is scored against refs[tests[t].ref]
// ---------------------------------------------------------------------------
namespace {

// what one distinct reference of a chunk takes: its raw bytes in two pinned sets and two device buffers, decoded once
// and, if rate != 48000, converted once
size_t feed_ref_bytes(const peaq_feed& f, uint64_t n, uint64_t n48) {
  const size_t f32 = sizeof(float) * f.channels;
  size_t b = 4 * (size_t)n * f.channels * kPcmBytes[f.format] + even_stride((size_t)n) * f32;
  if (f.rate != 48000) b += even_stride((size_t)n48) * f32;
  return b;
}

// ... and one test: a pair of peaq_batch_run_host (the reference's copy in the pair layout among it) less the
// reference's four raw signals
size_t feed_test_bytes(const peaq_feed& f, uint64_t n, uint64_t n48) {
  return feed_pair_bytes(f, n, n48) - 4 * (size_t)n * f.channels * kPcmBytes[f.format];
}

struct RefsPlan {
  std::vector<size_t> starts;    // first test of every chunk, and one entry behind the last
  std::vector<size_t> ustarts;   // the same into uniq
  std::vector<uint32_t> uniq;    // per chunk: the references its tests name, each once, in the order they first appear
  std::vector<uint32_t> row;     // [n_tests]: where the test's reference stands among its chunk's
};

void plan_ref_chunks(const peaq_feed& f, size_t n_refs, const peaq_host_signal* refs, size_t n_tests,
                     const peaq_host_test* tests, const std::vector<uint32_t>& r48, const std::vector<uint32_t>& t48,
                     RefsPlan* pl) {
  std::vector<size_t> stamp(n_refs, (size_t)-1);     // the chunk that listed the reference last
  std::vector<uint32_t> row_of(n_refs, 0);
  pl->row.resize(n_tests);
  const size_t most = f.chunk_pairs ? f.chunk_pairs : 65535;
  size_t p = 0;
  for (size_t k = 0; p < n_tests; ++k) {
    pl->starts.push_back(p);
    pl->ustarts.push_back(pl->uniq.size());
    uint64_t longest = 0, longest48 = 0;
    size_t np = 0, nu = 0;
    while (p + np < n_tests && np < most) {
      const peaq_host_test& t = tests[p + np];
      const bool fresh = stamp[t.ref] != k;
      const uint64_t l = std::max(longest, std::max(t.n, refs[t.ref].n));
      const uint64_t l48 = std::max<uint64_t>(longest48, std::max(t48[p + np], r48[t.ref]));
      if (!f.chunk_pairs && np &&                      // (a test beyond the budget: a chunk of one)
          (np + 1) * feed_test_bytes(f, l, l48) + (nu + fresh) * feed_ref_bytes(f, l, l48) > PEAQ_FEED_BUDGET_BYTES)
        break;
      if (fresh) {
        stamp[t.ref] = k;
        row_of[t.ref] = (uint32_t)nu++;
        pl->uniq.push_back(t.ref);
      }
      pl->row[p + np] = row_of[t.ref];
      longest = l;
      longest48 = l48;
      ++np;
    }
    p += np;
  }
  pl->starts.push_back(n_tests);
  pl->ustarts.push_back(pl->uniq.size());
}

int reserve_dev(DevBuf& d, size_t bytes) {
  if (bytes > d.cap) HIP_TRY(hipDeviceSynchronize());                // (growing frees the old buffer)
  HIP_TRY(d.reserve(std::max<size_t>(bytes, 16)));
  return PEAQ_OK;
}

// FeedRun with side 0 of a staging set holding the chunk's distinct references instead of one reference per pair
struct RefsRun {
  peaq_ctx* c;
  FeedState* st;
  peaq_feed f;
  int advanced, threads;
  double level_db;
  const peaq_host_signal* refs;
  const peaq_host_test* tests;
  const std::vector<uint32_t>* r48;                   // [n_refs], [n_tests]: lengths at 48 kHz
  const std::vector<uint32_t>* t48;
  const RefsPlan* pl;
  peaq_result* results;
  peaq_delay* delays;
  int gain_mode = PEAQ_GAIN_OFF;                     // peaq_batch_run_host_matched: the stage between estimate and cut
  double max_gain_db = 40.;
  peaq_gain* gains = nullptr;
  bool match() const { return (gain_mode & 0xF) != PEAQ_GAIN_OFF; }

  size_t first(size_t k) const { return pl->starts[k]; }
  size_t count(size_t k) const { return pl->starts[k + 1] - pl->starts[k]; }
  const uint32_t* uniq(size_t k) const { return pl->uniq.data() + pl->ustarts[k]; }
  size_t ucount(size_t k) const { return pl->ustarts[k + 1] - pl->ustarts[k]; }
  // samples per channel: the chunk's longest reference (side 0) or test (side 1)
  size_t raw_stride(size_t k, int side) const {
    uint64_t l = 0;
    if (side)
      for (size_t p = first(k); p < first(k) + count(k); ++p) l = std::max(l, tests[p].n);
    else
      for (size_t u = 0; u < ucount(k); ++u) l = std::max(l, refs[uniq(k)[u]].n);
    return (size_t)l;
  }

  // chunk k's raw bytes into its staging set, each side at its own stride, then to the device on the copy stream
  int stage(size_t k) {
    FeedSet& s = st->set[k & 1];
    const size_t unit = f.channels * kPcmBytes[f.format], cnt[2] = {ucount(k), count(k)};
    const size_t row_bytes[2] = {raw_stride(k, 0) * unit, raw_stride(k, 1) * unit};
    if (s.upload_pending) {                            // chunk k - 2's copies still read the pinned buffers
      HIP_TRY(hipEventSynchronize(s.uploaded));
      s.upload_pending = false;
    }
    std::vector<CopyJob> jobs;
    for (int i = 0; i < 2; ++i) {
      HIP_TRY(s.h_raw[i].reserve(std::max<size_t>(cnt[i] * row_bytes[i], 16)));
      for (size_t q = 0; q < cnt[i]; ++q) {
        const char* src = static_cast<const char*>(i ? tests[first(k) + q].data : refs[uniq(k)[q]].data);
        const size_t len = (size_t)(i ? tests[first(k) + q].n : refs[uniq(k)[q]].n) * unit;
        char* dst = s.h_raw[i].as<char>() + q * row_bytes[i];
        for (size_t o = 0; o < len; o += kFeedSlice) jobs.push_back({src + o, dst + o, std::min(kFeedSlice, len - o)});
      }
    }
    run_copies(jobs, threads);
    if (s.raw_pending) {                               // chunk k - 2's decoder still reads the device buffers
      HIP_TRY(hipStreamWaitEvent(st->copy_s, s.raw_free, 0));
      s.raw_pending = false;
    }
    for (int i = 0; i < 2; ++i) {
      if (int rc = reserve_dev(s.d_raw[i], cnt[i] * row_bytes[i])) return rc;
      if (cnt[i] * row_bytes[i])
        HIP_TRY(hipMemcpyAsync(s.d_raw[i].p, s.h_raw[i].p, cnt[i] * row_bytes[i], hipMemcpyHostToDevice, st->copy_s));
    }
    HIP_TRY(hipEventRecord(s.uploaded, st->copy_s));
    s.upload_pending = true;
    return PEAQ_OK;
  }

  // decode through score for chunk k on the compute stream; the results travel to the set's pinned buffer
  int compute(size_t k) {
    FeedSet& s = st->set[k & 1];
    const size_t p0 = first(k), np = count(k), nu = ucount(k), C = (size_t)f.channels;
    const size_t rs_ref = raw_stride(k, 0), rs_test = raw_stride(k, 1);
    const uint32_t* row = pl->row.data() + p0;
    hipStream_t cs = st->comp_s;
    std::vector<uint32_t> n_u(nu), m_u(nu), n_t(np), m[2];   // lengths as uploaded, and as they stand after each stage
    for (size_t u = 0; u < nu; ++u) n_u[u] = (uint32_t)refs[uniq(k)[u]].n;
    for (size_t q = 0; q < np; ++q) n_t[q] = (uint32_t)tests[p0 + q].n;
    m_u = n_u;
    m[1] = n_t;
    HIP_TRY(hipStreamWaitEvent(cs, s.uploaded, 0));
    size_t stride = even_stride(std::max(rs_ref, rs_test)), ustride = even_stride(rs_ref);   // pairs; the distinct references
    if (int rc = reserve_dev(st->f_dec[1], np * stride * C * sizeof(float))) return rc;
    if (int rc = reserve_dev(st->u_dec, nu * ustride * C * sizeof(float))) return rc;
    const float* cur_u = st->u_dec.as<float>();
    float* cur[2] = {nullptr, st->f_dec[1].as<float>()};
    if (int rc = peaq_batch_decode_pcm(c, f.format, f.channels, (int)np, s.d_raw[1].p, rs_test, n_t.data(), 0, cur[1], stride, cs))
      return rc;
    if (int rc = peaq_batch_decode_pcm(c, f.format, f.channels, (int)nu, s.d_raw[0].p, rs_ref, n_u.data(), 0, st->u_dec.as<float>(),
                                       ustride, cs))
      return rc;
    HIP_TRY(hipEventRecord(s.raw_free, cs));
    s.raw_pending = true;
    DevBuf* paired = &st->f_dec[0];                    // where the references stand in the pair layout
    if (f.rate != 48000) {
      uint32_t longest = 0, ulongest = 0;
      for (size_t u = 0; u < nu; ++u) ulongest = std::max(ulongest, (*r48)[uniq(k)[u]]);
      for (size_t q = 0; q < np; ++q) longest = std::max(longest, (*t48)[p0 + q]);
      const size_t s48 = even_stride(std::max(longest, ulongest)), us48 = even_stride(ulongest);
      if (int rc = reserve_dev(st->f_48[1], np * s48 * C * sizeof(float))) return rc;
      if (int rc = reserve_dev(st->u_48, nu * us48 * C * sizeof(float))) return rc;
      if (int rc = peaq_batch_resample(c, f.channels, f.rate, (int)np, cur[1], stride, n_t.data(), 0, st->f_48[1].as<float>(),
                                       s48, m[1].data(), cs))
        return rc;
      if (int rc = peaq_batch_resample(c, f.channels, f.rate, (int)nu, cur_u, ustride, n_u.data(), 0, st->u_48.as<float>(), us48,
                                       m_u.data(), cs))
        return rc;
      cur[1] = st->f_48[1].as<float>();
      cur_u = st->u_48.as<float>();
      stride = s48;
      ustride = us48;
      paired = &st->f_48[0];
    }
    // every test's reference from the distinct rows into the pair layout
    std::vector<uint32_t> src(row, row + np), none(np, 0);
    m[0].resize(np);
    for (size_t q = 0; q < np; ++q) m[0][q] = m_u[row[q]];
    if (int rc = reserve_dev(*paired, np * stride * C * sizeof(float))) return rc;
    cur[0] = paired->as<float>();
    if (int rc = peaq_batch_gather(c, f.channels, (int)nu, (int)np, cur_u, ustride, src.data(), none.data(), m[0].data(), cur[0],
                                   stride, cs))
      return rc;
    if (f.align_max_lag || match()) {
      std::vector<uint32_t> skip[2], common(np);
      skip[0].assign(np, 0);
      skip[1].assign(np, 0);
      uint32_t longest = 0;
      if (f.align_max_lag) {
        if (np * sizeof(peaq_delay) > st->d_del.cap) HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(st->d_del.reserve(np * sizeof(peaq_delay)));
        HIP_TRY(s.h_del.reserve(np * sizeof(peaq_delay)));
        if (int rc = peaq_batch_estimate_delay(c, f.channels, (int)np, cur[0], cur[1], stride, m[0].data(), m[1].data(), 0,
                                               f.align_max_lag, st->d_del.as<peaq_delay>(), cs))
          return rc;
        HIP_TRY(hipMemcpyAsync(s.h_del.p, st->d_del.p, np * sizeof(peaq_delay), hipMemcpyDeviceToHost, cs));
        HIP_TRY(hipEventRecord(st->del_done, cs));
        HIP_TRY(hipEventSynchronize(st->del_done));    // the cut needs the lags on the host
      }
      for (size_t q = 0; q < np; ++q) {
        int32_t lag = 0;
        if (f.align_max_lag) {
          const peaq_delay& rec = s.h_del.as<peaq_delay>()[q];
          if (delays) delays[p0 + q] = rec;
          lag = rec.lag;
        }
        peaq_aligned_lengths(lag, m[0][q], m[1][q], &skip[0][q], &skip[1][q], &common[q]);
        longest = std::max(longest, common[q]);
      }
      const size_t sc = even_stride(longest);
      for (DevBuf& d : st->f_cut)
        if (int rc = reserve_dev(d, np * sc * C * sizeof(float))) return rc;
      if (match()) {                                   // over the common part of the uncut buffers; the records stay on the device
        if (int rc = reserve_dev(st->d_gain, np * sizeof(peaq_gain))) return rc;
        HIP_TRY(s.h_gain.reserve(np * sizeof(peaq_gain)));
        if (int rc = peaq_batch_measure_gain(c, f.channels, (int)np, cur[0], stride, skip[0].data(), cur[1], stride,
                                             skip[1].data(), common.data(), gain_mode, max_gain_db, st->d_gain.as<peaq_gain>(), cs))
          return rc;
        HIP_TRY(hipMemcpyAsync(s.h_gain.p, st->d_gain.p, np * sizeof(peaq_gain), hipMemcpyDeviceToHost, cs));
      }
      // the reference's cut: again from the distinct rows, each test's own skip
      if (int rc = peaq_batch_gather(c, f.channels, (int)nu, (int)np, cur_u, ustride, src.data(), skip[0].data(), common.data(),
                                     st->f_cut[0].as<float>(), sc, cs))
        return rc;
      if (int rc = match() ? peaq_batch_cut_scaled(c, f.channels, (int)np, cur[1], stride, skip[1].data(), common.data(),
                                                   st->d_gain.as<peaq_gain>(), st->f_cut[1].as<float>(), sc, cs)
                           : peaq_batch_cut(c, f.channels, (int)np, cur[1], stride, skip[1].data(), common.data(),
                                            st->f_cut[1].as<float>(), sc, cs))
        return rc;
      for (int i = 0; i < 2; ++i) {
        cur[i] = st->f_cut[i].as<float>();
        m[i] = common;
      }
      stride = sc;
    }
    if (np * sizeof(peaq_result) > st->d_res.cap) HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(st->d_res.reserve(np * sizeof(peaq_result)));
    HIP_TRY(s.h_res.reserve(np * sizeof(peaq_result)));
    if (int rc = peaq_batch_run(c, advanced, f.channels, level_db, (int)np, cur[0], cur[1], stride, m[0].data(), m[1].data(),
                                0, st->d_res.as<peaq_result>(), cs))
      return rc;
    HIP_TRY(hipMemcpyAsync(s.h_res.p, st->d_res.p, np * sizeof(peaq_result), hipMemcpyDeviceToHost, cs));
    HIP_TRY(hipEventRecord(s.res_done, cs));
    return PEAQ_OK;
  }

  int collect(size_t k) {
    FeedSet& s = st->set[k & 1];
    HIP_TRY(hipEventSynchronize(s.res_done));
    std::memcpy(results + first(k), s.h_res.p, count(k) * sizeof(peaq_result));
    if (match() && gains) std::memcpy(gains + first(k), s.h_gain.p, count(k) * sizeof(peaq_gain));   // (copied before the results)
    return PEAQ_OK;
  }

  int run() {
    const size_t n_chunks = pl->starts.size() - 1;
    if (int rc = stage(0)) return rc;
    for (size_t k = 0; k < n_chunks; ++k) {
      if (int rc = compute(k)) return rc;
      if (k + 1 < n_chunks)                            // packing and upload beside chunk k's kernels
        if (int rc = stage(k + 1)) return rc;
      if (k)
        if (int rc = collect(k - 1)) return rc;
    }
    return collect(n_chunks - 1);
  }
};

}  // namespace

extern "C" size_t peaq_feed_refs_workspace_bytes(const peaq_feed* feed, int advanced, size_t n_refs, size_t n_tests,
                                                 uint64_t n_max) {
  if (check_feed("peaq_feed_refs_workspace_bytes", feed) != PEAQ_OK || n_refs == 0 || n_tests == 0 || n_max > 0xFFFFFFFFull)
    return 0;
  uint64_t n48 = n_max;
  if (feed->rate != 48000) {
    n48 = peaq_resampled_length(n_max, feed->rate);
    if (n_max && !n48) return 0;
  }
  const size_t per_test = feed_test_bytes(*feed, n_max, n48), per_ref = feed_ref_bytes(*feed, n_max, n48);
  // the most distinct references a chunk of `chunk` tests can name is min (chunk, n_refs)
  size_t chunk = feed->chunk_pairs;
  if (!chunk) {
    chunk = PEAQ_FEED_BUDGET_BYTES / (per_test + per_ref);
    if (chunk > n_refs) chunk = std::max(n_refs, (PEAQ_FEED_BUDGET_BYTES - std::min(PEAQ_FEED_BUDGET_BYTES, n_refs * per_ref)) / per_test);
    chunk = std::max<size_t>(chunk, 1);
  }
  chunk = std::min<size_t>(std::min<size_t>(chunk, n_tests), 65535);
  size_t b = chunk * per_test + std::min(chunk, n_refs) * per_ref +
             peaq_batch_workspace_bytes(advanced, feed->channels, (int)chunk, (uint32_t)n48);
  if (feed->align_max_lag) b += peaq_align_workspace_bytes(feed->channels, (int)chunk, (uint32_t)n48, feed->align_max_lag);
  return b;
}

// peaq_batch_run_host_refs and, with a gain mode, peaq_batch_run_host_matched
static int run_host_refs(const char* who, peaq_ctx* c, int advanced, double level_db, const peaq_feed* feed, int gain_mode,
                         double max_gain_db, size_t n_refs, const peaq_host_signal* refs, size_t n_tests,
                         const peaq_host_test* tests, peaq_result* results, peaq_delay* delays, peaq_gain* gains) {
  const std::string w(who);
  if (int rc = check_feed(who, feed)) return rc;
  if (int rc = check_level(w, level_db)) return rc;
  int threads = 0;
  if (int rc = feed_threads(&threads)) return rc;
  if (n_tests && (!tests || !results)) return fail(PEAQ_ERR_ARG, w + ": NULL tests or results");
  if (n_tests && n_refs && !refs) return fail(PEAQ_ERR_ARG, w + ": NULL refs");
  std::vector<uint32_t> r48(n_refs, 0), t48(n_tests);
  std::vector<char> named(n_refs, 0);
  const auto length48 = [&](const char* what, size_t i, uint64_t n, const void* data, uint32_t* out) {
    if (n && !data)
      return fail(PEAQ_ERR_ARG, w + ": " + what + " " + std::to_string(i) + " has " + std::to_string(n) + " samples and a NULL buffer");
    if (n > 0xFFFFFFFFull)
      return fail(PEAQ_ERR_ARG, w + ": " + what + " " + std::to_string(i) + " has " + std::to_string(n) + " samples, more than 2^32 - 1");
    *out = (uint32_t)n;
    if (feed->rate != 48000) {
      *out = peaq_resampled_length(n, feed->rate);
      if (n && !*out) return (int)PEAQ_ERR_ARG;          // (the message is peaq_resampled_length's)
    }
    return (int)PEAQ_OK;
  };
  for (size_t t = 0; t < n_tests; ++t) {
    if (tests[t].ref >= n_refs)
      return fail(PEAQ_ERR_ARG, w + ": test " + std::to_string(t) + " names reference " + std::to_string(tests[t].ref) + " of " +
                                    std::to_string(n_refs));
    if (int rc = length48("test", t, tests[t].n, tests[t].data, &t48[t])) return rc;
    named[tests[t].ref] = 1;
  }
  for (size_t r = 0; r < n_refs; ++r)                   // (a reference nobody names is not looked at)
    if (named[r])
      if (int rc = length48("reference", r, refs[r].n, refs[r].data, &r48[r])) return rc;
  if (!c) return fail(PEAQ_ERR_ARG, w + ": ctx is NULL");
  if (n_tests == 0) return PEAQ_OK;
  if (delays && !feed->align_max_lag) std::memset(delays, 0, n_tests * sizeof(peaq_delay));
  if (gains) std::memset(gains, 0, n_tests * sizeof(peaq_gain));

  FeedState* st;
  {
    std::lock_guard<std::mutex> lock(c->mu);
    if (!c->feed) c->feed = new FeedState;
    st = c->feed;
  }
  std::lock_guard<std::mutex> run_lock(st->run_mu);   // (the lock, streams, events and staging sets of peaq_batch_run_host)
  HIP_TRY(hipSetDevice(c->device));
  if (!st->copy_s) HIP_TRY(hipStreamCreateWithFlags(&st->copy_s, hipStreamNonBlocking));
  if (!st->comp_s) HIP_TRY(hipStreamCreateWithFlags(&st->comp_s, hipStreamNonBlocking));
  if (!st->del_done) HIP_TRY(hipEventCreateWithFlags(&st->del_done, hipEventDisableTiming));
  for (FeedSet& s : st->set)
    for (hipEvent_t* e : {&s.uploaded, &s.raw_free, &s.res_done})
      if (!*e) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
  RefsPlan plan;
  peaq_feed budget = *feed;                          // the cut buffers count as with alignment (feed_pair_bytes)
  if ((gain_mode & 0xF) != PEAQ_GAIN_OFF && !budget.align_max_lag) budget.align_max_lag = 1;
  plan_ref_chunks(budget, n_refs, refs, n_tests, tests, r48, t48, &plan);
  RefsRun run{c, st, *feed, advanced ? 1 : 0, threads, level_db, refs, tests, &r48, &t48, &plan, results, delays};
  run.gain_mode = gain_mode;
  run.max_gain_db = max_gain_db;
  run.gains = gains;
  const int rc = run.run();
  const std::string msg = rc != PEAQ_OK ? peaq_err_string() : std::string();
  if (rc != PEAQ_OK) (void)hipDeviceSynchronize();    // stop: nothing more is started, what runs drains before the buffers are reused
  for (FeedSet& s : st->set) s.upload_pending = s.raw_pending = false;
  return rc != PEAQ_OK ? fail(rc, msg) : PEAQ_OK;
}

extern "C" int peaq_batch_run_host_refs(peaq_ctx* c, int advanced, double level_db, const peaq_feed* feed, size_t n_refs,
                                        const peaq_host_signal* refs, size_t n_tests, const peaq_host_test* tests,
                                        peaq_result* results, peaq_delay* delays) {
  return run_host_refs("peaq_batch_run_host_refs", c, advanced, level_db, feed, PEAQ_GAIN_OFF, 40., n_refs, refs, n_tests, tests,
                       results, delays, nullptr);
}

extern "C" int peaq_batch_run_host_matched(peaq_ctx* c, int advanced, double level_db, const peaq_feed* feed, int mode,
                                           double max_gain_db, size_t n_refs, const peaq_host_signal* refs, size_t n_tests,
                                           const peaq_host_test* tests, peaq_result* results, peaq_delay* delays,
                                           peaq_gain* gains) {
  if (int rc = check_gain_mode("peaq_batch_run_host_matched", mode, max_gain_db)) return rc;
  return run_host_refs("peaq_batch_run_host_matched", c, advanced, level_db, feed, mode, max_gain_db, n_refs, refs, n_tests,
                       tests, results, delays, gains);
}

extern "C" size_t peaq_feed_matched_workspace_bytes(const peaq_feed* feed, int advanced, int mode, size_t n_refs, size_t n_tests,
                                                    uint64_t n_max) {
  if (mode < 0 || (mode & ~(0xF | PEAQ_GAIN_PER_CHANNEL)) || (mode & 0xF) > PEAQ_GAIN_POLARITY) return 0;
  if ((mode & 0xF) == PEAQ_GAIN_OFF) return peaq_feed_refs_workspace_bytes(feed, advanced, n_refs, n_tests, n_max);
  if (check_feed("peaq_feed_matched_workspace_bytes", feed) != PEAQ_OK) return 0;
  const peaq_feed& f = *feed;
  size_t b = peaq_feed_refs_workspace_bytes(feed, advanced, n_refs, n_tests, n_max);
  if (!b) return 0;
  uint64_t n48 = n_max;
  if (f.rate != 48000) n48 = peaq_resampled_length(n_max, f.rate);
  size_t chunk = f.chunk_pairs ? f.chunk_pairs : std::max<size_t>(1, PEAQ_FEED_BUDGET_BYTES / feed_test_bytes(f, n_max, n48));
  chunk = std::min<size_t>(std::min<size_t>(chunk, n_tests), 65535);
  if (!f.align_max_lag) b += 2 * chunk * even_stride((size_t)n48) * sizeof(float) * f.channels;   // the cut buffers
  // per test: the record on the device and in both pinned sets; the partials of the largest chunk there can be
  return b + 3 * chunk * sizeof(peaq_gain) + peaq_gain_workspace_bytes(f.channels, (int)chunk, (uint32_t)n48);
}

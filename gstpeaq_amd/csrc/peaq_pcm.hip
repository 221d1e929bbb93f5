// peaq_pcm.hip -- PCM from host memory (peaq_batch_decode_pcm, peaq_batch_run_host, peaq_feed_workspace_bytes;
// include/peaq_amd.h): the sample-format conversion as a kernel, and the feed that scores a list of host pairs chunk
// by chunk, the next chunk's packing and upload beside the running chunk's kernels.
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
  PinBuf h_raw[2], h_res, h_del;                     // ref, test; the chunk's results and delay records
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

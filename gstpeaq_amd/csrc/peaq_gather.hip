// peaq_gather.hip -- peaq_batch_gather (include/peaq_amd.h): peaq_batch_cut with a source index, what puts each
// reference of a corpus, uploaded and decoded once, in front of every test that names it (peaq_batch_run_host_refs,
// peaq_pcm.hip).
//
//   gather_kernel            a strided copy, out[p] = in[src[p]] from skip[p] on: 16-byte stores from the first aligned
//       float of the destination on, 16-byte loads where the source has the same phase, four dwords otherwise; the
//       phase follows from src, skip and the destination's base, so it differs from output to output and is the same
//       for every thread of a workgroup.  Head and tail (at most 3 floats each) are the first workgroup's.  The grid is
//       (vector units, outputs): blockIdx.y walks the outputs sorted by source row, and the x extent is a multiple of
//       8, so that the outputs of one row run one after the other and the same part of the row is read by workgroups
//       that the dispatcher deals to one XCD (it deals linear workgroup ids round robin over the eight): the later
//       readers find the lines in that XCD's L2.  Placement is a matter of speed only; nothing depends on it.
#include "peaq_host.h"

namespace {

struct GatherArgs {
  const float* in;
  float* out;
  size_t in_stride, out_stride;  // samples per channel between rows / outputs
  const uint32_t* order;         // device [n_out]: the outputs sorted by source row
  const uint32_t* src;           // device [n_out]
  const uint32_t* skip;          // device [n_out]
  const uint32_t* n_keep;        // device [n_out]
  int channels;
};

// floats, not samples: an output's run is n_keep x channels consecutive floats (as align_cut_kernel, peaq_align.hip)
__global__ __launch_bounds__(256) void gather_kernel(const GatherArgs a) {
  const unsigned p = a.order[blockIdx.y];
  const size_t count = (size_t)a.n_keep[p] * a.channels;
  const float* __restrict__ src = a.in + ((size_t)a.src[p] * a.in_stride + a.skip[p]) * a.channels;
  float* __restrict__ dst = a.out + (size_t)p * a.out_stride * a.channels;
  const size_t head = min(count, (size_t)((16 - ((uintptr_t)dst & 15)) & 15) / sizeof(float));
  const size_t vecs = (count - head) / 4;
  const bool same_phase = ((uintptr_t)(src + head) & 15) == 0;   // of the whole output: units are 16 bytes apart
  const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (v < vecs) {
    const float* s = src + head + 4 * v;
    float4 x;
    if (same_phase)
      x = *reinterpret_cast<const float4*>(s);
    else
      x = {s[0], s[1], s[2], s[3]};
    *reinterpret_cast<float4*>(dst + head + 4 * v) = x;
  }
  if (blockIdx.x == 0) {                             // the unaligned head and the tail: at most 3 floats each
    if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
    const size_t tail0 = head + 4 * vecs;
    if (tail0 + threadIdx.x < count) dst[tail0 + threadIdx.x] = src[tail0 + threadIdx.x];
  }
}

}  // namespace

struct GatherState {
  LenStage lens;                // [order, src, skip, n_keep][n_out] (under the context's lock)
};

void gather_release(peaq_ctx* c) {
  if (!c->ga) return;
  c->ga->lens.release();
  delete c->ga;
  c->ga = nullptr;
}

extern "C" int peaq_batch_gather(peaq_ctx* c, int channels, int n_rows, int n_out, const float* d_in, size_t in_stride,
                                 const uint32_t* src, const uint32_t* skip, const uint32_t* n_keep, float* d_out,
                                 size_t out_stride, void* stream_) {
  const std::string w("peaq_batch_gather");
  if (channels != 1 && channels != 2) return fail(PEAQ_ERR_ARG, w + ": channels must be 1 or 2, not " + std::to_string(channels));
  if (n_rows < 0 || n_out < 0)
    return fail(PEAQ_ERR_ARG, w + ": n_rows " + std::to_string(n_rows) + " or n_out " + std::to_string(n_out) + " < 0");
  if (n_rows > 65535) return fail(PEAQ_ERR_ARG, w + ": " + std::to_string(n_rows) + " rows are more than 65535 in one call");
  if (n_out > 65535) return fail(PEAQ_ERR_ARG, w + ": " + std::to_string(n_out) + " outputs are more than 65535 in one call");
  if (n_out > 0 && (!d_in || !d_out)) return fail(PEAQ_ERR_ARG, w + ": NULL buffer");
  if (n_out > 0 && (!src || !skip || !n_keep)) return fail(PEAQ_ERR_ARG, w + ": NULL src, skip or n_keep");
  const size_t no = (size_t)std::max(n_out, 0);
  std::vector<uint32_t> h(4 * no);                     // order, src, skip, n_keep
  uint32_t keep_max = 0;
  for (size_t p = 0; p < no; ++p) {
    if (src[p] >= (uint32_t)n_rows)
      return fail(PEAQ_ERR_ARG, w + ": output " + std::to_string(p) + " names row " + std::to_string(src[p]) + " of " +
                                    std::to_string(n_rows));
    if ((uint64_t)skip[p] + n_keep[p] > in_stride)
      return fail(PEAQ_ERR_ARG, w + ": output " + std::to_string(p) + ": skip " + std::to_string(skip[p]) + " + n_keep " +
                                    std::to_string(n_keep[p]) + " passes in_stride " + std::to_string(in_stride));
    h[p] = (uint32_t)p;
    h[no + p] = src[p];
    h[2 * no + p] = skip[p];
    h[3 * no + p] = n_keep[p];
    keep_max = std::max(keep_max, n_keep[p]);
  }
  if (keep_max > out_stride)
    return fail(PEAQ_ERR_ARG, w + ": out_stride " + std::to_string(out_stride) + " is smaller than the longest n_keep (" +
                                  std::to_string(keep_max) + " samples)");
  if (n_out > 0) {
    const char* i0 = reinterpret_cast<const char*>(d_in);
    const char* o0 = reinterpret_cast<const char*>(d_out);
    const size_t ib = (size_t)n_rows * in_stride * channels * sizeof(float);
    const size_t ob = no * out_stride * channels * sizeof(float);
    if (i0 < o0 + ob && o0 < i0 + ib) return fail(PEAQ_ERR_ARG, w + ": d_out overlaps d_in");
  }
  if (!c) return fail(PEAQ_ERR_ARG, w + ": ctx is NULL");
  if (n_out == 0 || keep_max == 0) return PEAQ_OK;
  // outputs of one row next to each other, in the caller's order among themselves
  std::stable_sort(h.begin(), h.begin() + no, [&](uint32_t x, uint32_t y) { return src[x] < src[y]; });

  hipStream_t stream = static_cast<hipStream_t>(stream_);
  std::lock_guard<std::mutex> lock(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  if (!c->ga) c->ga = new GatherState;
  LenSlot* slot = nullptr;
  if (int rc = c->ga->lens.upload(h.data(), h.size(), stream, &slot)) return rc;
  GatherArgs a{};
  a.in = d_in;
  a.out = d_out;
  a.in_stride = in_stride;
  a.out_stride = out_stride;
  a.order = slot->dev.as<uint32_t>();
  a.src = a.order + no;
  a.skip = a.src + no;
  a.n_keep = a.skip + no;
  a.channels = channels;
  const size_t vecs = ((size_t)keep_max * channels + 3) / 4;
  const size_t blocks = ((vecs + 255) / 256 + 7) & ~(size_t)7;   // a multiple of 8: column x of every output on one XCD
  hipLaunchKernelGGL(gather_kernel, dim3((unsigned)blocks, (unsigned)n_out), dim3(256), 0, stream, a);
  const hipError_t launched = hipGetLastError();
  const int sent = c->ga->lens.sent(slot, stream);     // (also after a failed launch: the copy into the slot is enqueued)
  HIP_TRY(launched);
  return sent;
}

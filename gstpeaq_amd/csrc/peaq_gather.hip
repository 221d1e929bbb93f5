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

// floats, not samples: an output's run is n_keep x channels consecutive floats (copy_run, peaq_host.h)
__global__ __launch_bounds__(256) void gather_kernel(const GatherArgs a) {
  const unsigned p = a.order[blockIdx.y];
  const size_t count = (size_t)a.n_keep[p] * a.channels;
  const float* __restrict__ src = a.in + ((size_t)a.src[p] * a.in_stride + a.skip[p]) * a.channels;
  float* __restrict__ dst = a.out + (size_t)p * a.out_stride * a.channels;
  copy_run(src, dst, count, (size_t)blockIdx.x * 256, blockIdx.x == 0, CopyBits());
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
  if (int rc = check_channels(w, channels)) return rc;
  if (int rc = check_count(w, n_rows, "n_rows", "rows")) return rc;
  if (int rc = check_count(w, n_out, "n_out", "outputs")) return rc;
  if (n_out > 0 && (!src || !skip || !n_keep)) return fail(PEAQ_ERR_ARG, w + ": NULL src, skip or n_keep");
  const size_t no = (size_t)n_out;
  for (size_t p = 0; p < no; ++p)
    if (src[p] >= (uint32_t)n_rows)
      return fail(PEAQ_ERR_ARG, w + ": output " + std::to_string(p) + " names row " + std::to_string(src[p]) + " of " +
                                    std::to_string(n_rows));
  uint32_t keep_max = 0;
  if (int rc = check_cut_geometry(w, "output", channels, n_rows, n_out, d_in, in_stride, skip, n_keep, d_out, out_stride,
                                  &keep_max))
    return rc;
  std::vector<uint32_t> h(4 * no);                     // order, src, skip, n_keep
  for (size_t p = 0; p < no; ++p) h[p] = (uint32_t)p;
  std::copy(src, src + no, h.begin() + no);
  std::copy(skip, skip + no, h.begin() + 2 * no);
  std::copy(n_keep, n_keep + no, h.begin() + 3 * no);
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

// peaq_delay_cut.h -- what the cuts of a test signal along its delay share: the shifted cut of peaq_frac.hip (one grid
// point per pair), the drift cut of peaq_drift.hip (one line), the track cut of peaq_track.hip (a line per window) and
// the pieces cut of peaq_steps.hip (lines that jump).  DESIGN.md 17.
//   device   the tile's constants; the copy a pair without a delay takes instead of the filter (cut_tile_copied); the
//            ONE pass of the three cuts along lines (delay_cut_pass).  No kernel is defined here: the kernels, their
//            argument blocks, their spreads and the arithmetic that proves those stay in the stages' files.
//   host     one call of such a cut from its checks to the event behind its launch (DelayCutCall); the window check of
//            the stages that estimate per window (check_delay_window).
#pragma once
#include "peaq_host.h"

// ---------------------------------------------------------------------------
// DEVICE SIDE (256 threads per workgroup)
// ---------------------------------------------------------------------------
constexpr int kCutK = PEAQ_SUB_HALF;                   // taps each side
constexpr int kCutTaps = 2 * kCutK + 1;                // 65
constexpr int kCutSteps = PEAQ_SUB_STEPS;              // rows of the shift table
constexpr int kCutTile = 1024;                         // outputs per workgroup
constexpr int kCutPer = 4;                             // ... per lane
static_assert(kCutTile == 256 * kCutPer, "a lane's share");
static_assert(kCutSteps == 256, "peaq_drift_index: 256 phases per sample");
// samples a pass stages when m_i - m_lo stays below `spread` over its outputs
constexpr int delay_cut_stage(int spread) { return kCutTile + 2 * kCutK + spread; }

// What every cut kernel starts with.  True: the workgroup is done -- its tile lies past the pair's n_keep, or `plain`
// (uniform) says that the pair has no delay, and the tile's floats were copied as peaq_batch_cut copies them: their
// bits are moved.  `plain` is a VALUE, made from the pair's own scalars (q; a and e; a count) that the kernel reads
// beside n_keep in front of this call: all of a pair's scalar loads are then asked for together and waited for once,
// not n_keep, its test, and the pair's own behind that.
__device__ __forceinline__ bool cut_tile_copied(const float* __restrict__ in, float* __restrict__ out, size_t in_stride,
                                                size_t out_stride, const uint32_t* __restrict__ skip, uint32_t n_keep,
                                                int channels, bool plain) {
  const unsigned pair = blockIdx.y;
  const bool past = (unsigned long long)blockIdx.x * kCutTile >= n_keep;   // (the whole workgroup)
  if (past || !plain) return past;
  const size_t count = (size_t)n_keep * channels;
  const float* __restrict__ src = in + ((size_t)pair * in_stride + skip[pair]) * channels;
  float* __restrict__ dst = out + (size_t)pair * out_stride * channels;
  for (int sub = 0; sub < channels; ++sub)               // a tile is `channels` units of 256 x 4 floats
    copy_run(src, dst, count, ((size_t)blockIdx.x * channels + sub) * 256, blockIdx.x == 0 && sub == 0, CopyBits());
  return true;
}

// both channels of an output as the store writes them: a native vector, so that the store is ONE of 8 bytes (as an
// assignment to a float2 the pieces cut's came out as two of 4 with a branch between them: DESIGN.md 17)
typedef float CutPair __attribute__((ext_vector_type(2)));

// One pass of a cut along lines: the outputs first .. last of the tile that starts at i0 (lane l owns outputs i0 + l +
// 256 j).  index(i, &m, &phi) gives output i's place on its line, drift_index of the (a, e) it follows -- the index and
// not the line, so that this header needs nothing of peaq_drift_math.h, which turns contraction off for whatever
// follows it (peaq_frac.hip's estimate must not see that); the stages include their arithmetic in front of this header,
// and the pass is rounded as that is.  src, dst: the pair's rows; pairs8: both channels go out in one aligned store.
// m_lo: the smallest m of the pass's outputs, which the caller knows from the outputs
// where m can turn; m_i - m_lo stays below SPREAD, and n_stage <= delay_cut_stage(SPREAD) samples are staged in LDS from
// input sample skip + first + m_lo - 32 on, the channels of a sample side by side (absent samples as zeros).
// Neighbouring lanes read neighbouring samples: one LDS read per tap fetches both channels, no bank conflicts.  The tap
// row is per output: each lane loads its taps from the table in device memory with vector loads (DESIGN.md 17 says why
// not through LDS).  SKIP_IDLE_WAVES: a wave none of whose outputs lies in first .. last leaves after the staging.
template <int C, int SPREAD, bool SKIP_IDLE_WAVES, typename Index>
__device__ __forceinline__ void delay_cut_pass(const float* __restrict__ src, float* __restrict__ dst, bool pairs8,
                                               long long n_in, long long skip, long long i0, long long first, long long last,
                                               long long m_lo, int n_stage, Index index, const double* __restrict__ tab,
                                               float* lds) {
  const long long s0 = skip + first + m_lo - kCutK;                // input sample under staged position 0
  // ---- stage: consecutive lanes read consecutive floats; staged sample v, channel c at lds[C v + c] ----
  for (int f = threadIdx.x; f < n_stage * C; f += 256) {
    const long long s = s0 + (C == 2 ? f >> 1 : f);
    lds[f] = (s >= 0 && s < n_in) ? src[(size_t)s * C + (C == 2 ? f & 1 : 0)] : 0.f;
  }
  __syncthreads();
  // ---- output j of the lane: i = i0 + l + 256 j; tap o of it meets staged position i - first + (m_i - m_lo) + o ----
  const double* __restrict__ row[kCutPer];
  const float* x[kCutPer];
  bool mine[kCutPer], any = false;
#pragma unroll
  for (int j = 0; j < kCutPer; ++j) {
    const long long own = i0 + (long long)threadIdx.x + 256 * j;
    mine[j] = own >= first && own <= last;
    any = any || mine[j];
    const long long i = min(max(own, first), last);                // (an output outside the pass: computed, not stored)
    long long m;
    int phi;
    index(i, &m, &phi);
    const int dm = max(0, min((int)(m - m_lo), SPREAD - 1));       // (below SPREAD by the caller's bound: the clamp never acts)
    row[j] = tab + (size_t)(phi + kCutSteps / 2) * kCutTaps;
    x[j] = lds + C * ((int)(i - first) + dm);
  }
  if (SKIP_IDLE_WAVES && __builtin_amdgcn_ballot_w64(any) == 0) return;   // (per wave)
  double acc[C][kCutPer];
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int j = 0; j < kCutPer; ++j) acc[c][j] = 0.;
#pragma unroll 5
  for (int o = 0; o < kCutTaps; ++o) {                             // o = -32 .. 32 of the definition, in that order
#pragma unroll
    for (int j = 0; j < kCutPer; ++j) {
      const double h = row[j][o];
      if (C == 2) {
        const float2 v = *reinterpret_cast<const float2*>(x[j] + 2 * o);
        acc[0][j] = __builtin_fma(h, (double)v.x, acc[0][j]);
        acc[C - 1][j] = __builtin_fma(h, (double)v.y, acc[C - 1][j]);
      } else {
        acc[0][j] = __builtin_fma(h, (double)x[j][o], acc[0][j]);
      }
    }
  }
  // ---- consecutive lanes store consecutive samples ----
#pragma unroll
  for (int j = 0; j < kCutPer; ++j) {
    if (!mine[j]) continue;
    const long long i = i0 + (long long)threadIdx.x + 256 * j;
    if (pairs8) {
      reinterpret_cast<CutPair*>(dst)[i] = CutPair{(float)acc[0][j], (float)acc[C - 1][j]};
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) dst[(size_t)i * C + c] = (float)acc[c][j];
    }
  }
}

// ---------------------------------------------------------------------------
// HOST SIDE
// ---------------------------------------------------------------------------
// the window of the stages that estimate a delay per window
inline int check_delay_window(const std::string& who, uint32_t window) {
  if (window < PEAQ_DRIFT_MIN_WINDOW || window > PEAQ_DRIFT_MAX_WINDOW)
    return fail(PEAQ_ERR_ARG, who + ": window " + std::to_string(window) + " is outside 4096 .. 1048576");
  return PEAQ_OK;
}

// One call of peaq_batch_cut_shifted, _cut_drift, _cut_track or _cut_pieces, in the order of its members: the checks
// all four make, the call's host arrays packed into one vector of words, its upload into a length slot of the
// sub-sample stage, and -- the launch itself being the entry point's -- what follows the launch.  The words:
//   [cols][n_pairs] uint32     n_in | skip | n_keep | whatever the stage adds per pair
//   [2][lines] double          a | e of every line, behind an 8-byte boundary (a pad word where cols n_pairs is odd)
//   [lines] uint32             b, where the lines have one
struct DelayCutCall {
  const std::string& who;
  peaq_ctx* c;
  int channels, n_pairs;
  const float* d_in;
  size_t in_stride;
  const uint32_t *n_in, *skip, *n_keep;
  float* d_out;
  size_t out_stride;
  hipStream_t stream;

  size_t np = 0, words = 0, lines = 0, next_line = 0;
  uint32_t keep_max = 0;
  std::vector<uint32_t> h;
  std::unique_lock<std::mutex> lock;                   // the context's, from upload() on
  const double* tab = nullptr;                         // the shift table on the device
  LenStage* lens = nullptr;
  LenSlot* slot = nullptr;                             // (none after upload(): no pair keeps a sample, nothing to launch)

  // shape, the NULL check of the per-pair arrays (`others`: the stage's own are there; `names`: how the message goes
  // on behind "n_keep"), the cut geometry, n_in
  int check(bool others, const char* names) {
    if (int rc = check_shape(who, channels, n_pairs)) return rc;
    if (n_pairs > 0 && (!n_in || !skip || !n_keep || !others)) return fail(PEAQ_ERR_ARG, who + ": NULL n_in, skip, n_keep" + names);
    if (int rc = check_cut_geometry(who, "pair", channels, n_pairs, n_pairs, d_in, in_stride, skip, n_keep, d_out, out_stride,
                                    &keep_max))
      return rc;
    np = (size_t)std::max(n_pairs, 0);
    return check_lengths(who, n_pairs, n_in, 0, "n_in", in_stride, "in_stride");
  }
  // the words: n_cols columns per pair, the first three filled here (the others: col(), the entry's); n_lines lines
  // in all, with or without b
  void pack(size_t n_cols, size_t n_lines, bool with_b) {
    lines = n_lines;
    words = n_cols * np + (lines ? (n_cols * np) & 1 : 0);
    h.assign(words + (with_b ? 5 : 4) * lines, 0);
    for (size_t p = 0; p < np; ++p) {
      h[p] = n_in[p];
      h[np + p] = skip[p];
      h[2 * np + p] = n_keep[p];
    }
  }
  uint32_t& col(size_t k, size_t p) { return h[k * np + p]; }
  // The next n lines, pair p's, from line next_line on: a and e of each against their ranges (e: |e| <= max_e, which
  // the message calls e_range), then the stage's own check more(k, where) of line k.  where() makes "<who>: pair p" or,
  // with a noun, "<who>: pair p, <noun> k": a refusal calls it, a line that passes builds no string.  *plain: all of
  // the lines are (0, 0) -- the pair's bits are moved.
  template <typename More>
  int add_lines(size_t p, const char* noun, uint32_t n, const double* a, const double* e, const uint32_t* b, double max_e,
                const char* e_range, bool* plain, More more) {
    *plain = true;
    for (uint32_t k = 0; k < n; ++k) {
      const auto where = [&] {
        return who + ": pair " + std::to_string(p) + (noun ? std::string(", ") + noun + " " + std::to_string(k) : "");
      };
      if (!(std::fabs(a[k]) <= PEAQ_DRIFT_MAX_A))
        return fail(PEAQ_ERR_ARG, where() + ": a " + std::to_string(a[k]) + " is outside -1048576 .. 1048576");
      if (!(std::fabs(e[k]) <= max_e)) return fail(PEAQ_ERR_ARG, where() + ": e " + std::to_string(e[k]) + " is outside " + e_range);
      if (int rc = more(k, where)) return rc;
      *plain = *plain && a[k] == 0. && e[k] == 0.;
      std::memcpy(&h[words + 2 * (next_line + k)], &a[k], sizeof(double));
      std::memcpy(&h[words + 2 * lines + 2 * (next_line + k)], &e[k], sizeof(double));
      if (b) h[words + 4 * lines + next_line + k] = b[k];
    }
    next_line += n;
    return PEAQ_OK;
  }
  // the context, last of the checks; then its lock, the device, the table, the words on their way to the slot
  int upload() {
    if (!c) return fail(PEAQ_ERR_ARG, who + ": ctx is NULL");
    if (n_pairs == 0 || keep_max == 0) return PEAQ_OK;
    lock = std::unique_lock<std::mutex>(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = frac_shift_table(c, &tab, &lens)) return rc;
    return lens->upload(h.data(), h.size(), stream, &slot);
  }
  // where the words are on the device
  const uint32_t* dev_col(size_t k) const { return slot->dev.as<uint32_t>() + k * np; }
  const double* dev_a() const { return reinterpret_cast<const double*>(slot->dev.as<uint32_t>() + words); }
  const double* dev_e() const { return dev_a() + lines; }
  const uint32_t* dev_b() const { return reinterpret_cast<const uint32_t*>(dev_e() + lines); }
  unsigned tiles() const { return (unsigned)(((uint64_t)keep_max + kCutTile - 1) / kCutTile); }   // of the longest pair
  // behind the launch
  int launched() {
    const hipError_t e = hipGetLastError();
    const int sent = lens->sent(slot, stream);         // (also after a failed launch: the copy into the slot is enqueued)
    HIP_TRY(e);
    return sent;
  }
};

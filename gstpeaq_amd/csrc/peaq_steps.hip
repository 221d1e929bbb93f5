// peaq_steps.hip -- steps of a pair's delay: where inside two windows the delay jumps from one integer value to another
// (device), a track rebuilt as pieces that jump there (host), and the test signal's cut along such pieces
// (peaq_batch_locate_steps, peaq_steps_candidates, peaq_steps_fit, peaq_pieces_index, peaq_pieces_lengths,
// peaq_batch_estimate_steps, peaq_batch_cut_pieces, peaq_run_pair_steps; include/peaq_amd.h).
//
//   steps_chunk_kernel   one workgroup per chunk of 4096 positions of one candidate's interval.  Lane l owns the 16
//       consecutive positions from 16 l on: h = r (tA - tB) for each in registers, its running sums, and beside them the
//       lane's terms of the three sums polarity and norm need.  The lanes' totals are scanned in LDS in a fixed order (a
//       wave's lanes one after the other, then the four waves), which gives every position its sum from the chunk's
//       start; the chunk keeps the largest and the smallest of them with their first positions (the polarity is not
//       known yet), its total and the three side sums: 8 doubles to the scratch.  No atomics.
//   steps_pick_kernel    one workgroup per candidate: the chunks' totals added in chunk order, the side sums likewise,
//       the polarity, then the largest s H over the chunks' extremes, ties to the smaller position; the record.
//   pieces_cut_kernel    peaq_batch_cut_pieces: 1024 outputs of one pair per workgroup, made in one pass of the cuts'
//       shared body (delay_cut_pass, peaq_delay_cut.h) PER PIECE that meets the tile.  The piece of the tile's first
//       output comes from a binary search over b that is uniform over the workgroup; then a loop, uniform too, over the
//       pieces that meet the tile -- almost always one.  A pass stages ITS piece's span in LDS (m is monotone along one
//       line, so the smallest m is at one of the pass's two end outputs; kPcSpread has the arithmetic) and computes the
//       tile's outputs inside the piece -- a wave that owns none of them skips the sum --, so lines need not meet and a
//       jump may be of any size.  Pairs whose pieces are all (0, 0) take align_cut_kernel's copy (cut_tile_copied):
//       their bits are moved.
#include "peaq_host.h"
#include "peaq_steps_math.h"
#include "peaq_delay_cut.h"   // (behind the arithmetic: its pass is rounded as that is)

namespace {

// ---------------------------------------------------------------------------
// locate
// ---------------------------------------------------------------------------
constexpr uint32_t kStChunk = 4096;                    // positions per workgroup of steps_chunk_kernel
constexpr int kStOwn = 16;                             // ... per lane
constexpr int kStRow = 8;                              // doubles a chunk leaves: T, P, R2, D2, max, its offset, min, its offset
constexpr int kStCandWords = 8;                        // pair, lo, hi, LA, LB, skip_ref, skip_test, n_test
constexpr size_t kStScratchBudget = (size_t)256 << 20; // candidates are taken in groups whose rows stay below this
constexpr int32_t kStMaxL = (1 << 20) + 16384;
static_assert(kStChunk == 256 * kStOwn, "a lane's share");
static_assert(PEAQ_STEP_MAX_SPAN / kStChunk == 1024, "steps_pick_kernel holds a candidate's chunks in LDS");
constexpr uint32_t kStMaxChunks = PEAQ_STEP_MAX_SPAN / kStChunk;

struct LocateArgs {
  const float* ref;
  const float* test;
  size_t stride;
  const uint32_t* cand;         // device [n][kStCandWords], first candidate of the group
  int channels;
  uint32_t nch_max;             // chunks of the call's longest searched interval; a candidate's scratch is [nch_max][8]
  double* part;
  peaq_step* out;               // first candidate of the group
};

__host__ __device__ inline uint32_t steps_chunks(uint32_t span) { return (span + kStChunk - 1) / kStChunk; }

template <int C>
__device__ __forceinline__ double st_mono(const float* __restrict__ x, long long s) {
  if (C == 2) return (double)x[2 * s] + (double)x[2 * s + 1];
  return (double)x[s];
}

// the better of two (value, offset): the larger value (LARGER) or the smaller, then the smaller offset
template <bool LARGER>
__device__ __forceinline__ void st_better(double& v, uint32_t& at, double v2, uint32_t at2) {
  const bool take = LARGER ? (v2 > v || (v2 == v && at2 < at)) : (v2 < v || (v2 == v && at2 < at));
  if (take) {
    v = v2;
    at = at2;
  }
}

template <int C>
__device__ __forceinline__ void st_chunk(const LocateArgs& a, double* sh_s, double* sh_w, double (*sh3)[3], double* sh_v,
                                         uint32_t* sh_at) {
  const unsigned q = blockIdx.y, chunk = blockIdx.x;
  const uint32_t* __restrict__ cd = a.cand + (size_t)q * kStCandWords;
  const uint32_t lo = cd[1], hi = cd[2];
  if (hi - lo > PEAQ_STEP_MAX_SPAN) return;            // (the whole workgroup) nothing is searched
  const long long i0 = (long long)lo + (long long)chunk * kStChunk;
  if (i0 >= (long long)hi) return;                     // (the whole workgroup)
  const uint32_t pair = cd[0];
  const long long LA = (int32_t)cd[3], LB = (int32_t)cd[4], skip_ref = cd[5], skip_test = cd[6], n_test = cd[7];
  const float* __restrict__ ref = a.ref + (size_t)pair * a.stride * C;
  const float* __restrict__ test = a.test + (size_t)pair * a.stride * C;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // ---- the lane's 16 positions: h in registers, the running sum, the side sums ----
  double h[kStOwn];
  double run = 0., side[3] = {0., 0., 0.};             // r (tA + tB), r r, (tA - tB)^2
  const long long m0 = i0 + (long long)kStOwn * tid;
#pragma unroll
  for (int u = 0; u < kStOwn; ++u) {
    const long long i = m0 + u;
    double r = 0., tA = 0., tB = 0.;
    if (i < (long long)hi) {
      r = st_mono<C>(ref, skip_ref + i);               // (inside the reference: hi <= n_common)
      const long long ja = skip_test + i + LA, jb = skip_test + i + LB;
      if (ja >= 0 && ja < n_test) tA = st_mono<C>(test, ja);
      if (jb >= 0 && jb < n_test) tB = st_mono<C>(test, jb);
    }
    const double d = __dsub_rn(tA, tB);
    h[u] = __dmul_rn(r, d);
    run = __dadd_rn(run, h[u]);
    side[0] = __builtin_fma(r, __dadd_rn(tA, tB), side[0]);
    side[1] = __builtin_fma(r, r, side[1]);
    side[2] = __builtin_fma(d, d, side[2]);
  }
  // ---- the sum in front of the lane: its wave's earlier lanes one after the other, then the earlier waves ----
  sh_s[tid] = run;
  __syncthreads();
  double before = 0.;
  for (int l = 0; l < lane; ++l) before = __dadd_rn(before, sh_s[64 * wave + l]);
  if (lane == 63) sh_w[wave] = __dadd_rn(before, run);
  __syncthreads();
  double waves = 0.;
  for (int w = 0; w < wave; ++w) waves = __dadd_rn(waves, sh_w[w]);
  const double total = __dadd_rn(__dadd_rn(__dadd_rn(sh_w[0], sh_w[1]), sh_w[2]), sh_w[3]);
  // ---- the lane's extremes of H = waves + (before + (h_0 + .. + h_u)) at offset 16 l + u + 1, the first of equals; the
  //      chunk's last one is `total` to the bit ----
  double vmax = -INFINITY, vmin = INFINITY;
  uint32_t amax = 0xFFFFFFFFu, amin = 0xFFFFFFFFu;
  run = 0.;
#pragma unroll
  for (int u = 0; u < kStOwn; ++u) {
    run = __dadd_rn(run, h[u]);
    const double H = __dadd_rn(waves, __dadd_rn(before, run));
    const uint32_t off = (uint32_t)(kStOwn * tid + u + 1);
    if (m0 + u < (long long)hi) {
      st_better<true>(vmax, amax, H, off);
      st_better<false>(vmin, amin, H, off);
    }
  }
  // ---- the workgroup's: a tree over the 256 lanes in LDS, once for the largest, once for the smallest ----
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    __syncthreads();
    sh_v[tid] = pass ? vmin : vmax;
    sh_at[tid] = pass ? amin : amax;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
      if (tid < half) {
        double v = sh_v[tid];
        uint32_t at = sh_at[tid];
        if (pass)
          st_better<false>(v, at, sh_v[tid + half], sh_at[tid + half]);
        else
          st_better<true>(v, at, sh_v[tid + half], sh_at[tid + half]);
        sh_v[tid] = v;
        sh_at[tid] = at;
      }
      __syncthreads();
    }
    if (pass) {
      vmin = sh_v[0];
      amin = sh_at[0];
    } else {
      vmax = sh_v[0];
      amax = sh_at[0];
    }
  }
  block_sum4(side, sh3);
  if (tid == 0) {
    double* row = a.part + ((size_t)q * a.nch_max + chunk) * kStRow;
    row[0] = total;
    row[1] = side[0];
    row[2] = side[1];
    row[3] = side[2];
    row[4] = vmax;
    row[5] = (double)amax;
    row[6] = vmin;
    row[7] = (double)amin;
  }
}

__global__ __launch_bounds__(256, 4) void steps_chunk_kernel(const LocateArgs a) {
  __shared__ double sh_s[256];
  __shared__ double sh_w[4];
  __shared__ double sh3[4][3];
  __shared__ double sh_v[256];
  __shared__ uint32_t sh_at[256];
  if (a.channels == 2)
    st_chunk<2>(a, sh_s, sh_w, sh3, sh_v, sh_at);
  else
    st_chunk<1>(a, sh_s, sh_w, sh3, sh_v, sh_at);
}

__global__ __launch_bounds__(256, 4) void steps_pick_kernel(const LocateArgs a) {
  __shared__ double sh_c[kStMaxChunks + 1];            // the sum in front of chunk j; [nch]: H[hi]
  __shared__ double sh_side[3];
  __shared__ double sh_v[256];
  __shared__ uint32_t sh_at[256];
  const unsigned q = blockIdx.x;
  const int tid = threadIdx.x;
  const uint32_t* __restrict__ cd = a.cand + (size_t)q * kStCandWords;
  const uint32_t lo = cd[1], hi = cd[2];
  peaq_step rec;
  rec.pair = cd[0];
  rec.c = lo;
  rec.LA = (int32_t)cd[3];
  rec.LB = (int32_t)cd[4];
  rec.flags = 0;
  rec.reserved = 0;
  rec.gain_left = rec.gain_right = rec.norm = 0.;
  if (hi - lo > PEAQ_STEP_MAX_SPAN) {                  // (uniform)
    rec.flags = PEAQ_STEP_F_SPAN;
    if (tid == 0) a.out[q] = rec;
    return;
  }
  const uint32_t nch = steps_chunks(hi - lo);
  const double* __restrict__ P = a.part + (size_t)q * a.nch_max * kStRow;
  // ---- four sums in chunk order, each by one lane of a wave of its own ----
  if ((tid & 63) == 0) {
    const int which = tid >> 6;                        // 0: the totals, with every sum on the way; 1 .. 3: the side sums
    double s = 0.;
    for (uint32_t j = 0; j < nch; ++j) {
      if (which == 0) sh_c[j] = s;
      s = __dadd_rn(s, P[(size_t)j * kStRow + which]);
    }
    if (which == 0)
      sh_c[nch] = s;
    else
      sh_side[which - 1] = s;
  }
  __syncthreads();
  const double pol = sh_side[0] < 0. ? -1. : 1.;       // (+ for 0, and for a NaN: the norm catches that one)
  const double norm = sqrt(__dmul_rn(sh_side[1], sh_side[2]));
  rec.norm = norm;
  if (!(norm > 0.) || !isfinite(norm)) {               // (uniform)
    rec.flags = PEAQ_STEP_F_NONE;
    if (tid == 0) a.out[q] = rec;
    return;
  }
  // ---- the largest s H: c = lo (H = 0) first, then the chunks' extremes; lane t takes chunks t, t + 256, ... ----
  double best = 0.;
  uint32_t at = 0;                                     // offsets from lo
  for (uint32_t j = tid; j < nch; j += 256) {
    const double ext = P[(size_t)j * kStRow + (pol > 0. ? 4 : 6)];
    const uint32_t off = (uint32_t)P[(size_t)j * kStRow + (pol > 0. ? 5 : 7)];
    const double v = __dmul_rn(pol, __dadd_rn(sh_c[j], ext));
    st_better<true>(best, at, v, j * kStChunk + off);
  }
  sh_v[tid] = best;
  sh_at[tid] = at;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if (tid < half) {
      double v = sh_v[tid];
      uint32_t o = sh_at[tid];
      st_better<true>(v, o, sh_v[tid + half], sh_at[tid + half]);
      sh_v[tid] = v;
      sh_at[tid] = o;
    }
    __syncthreads();
  }
  if (tid == 0) {
    best = sh_v[0];
    rec.c = lo + sh_at[0];
    rec.gain_left = best;
    rec.gain_right = __dmul_rn(pol, __dsub_rn(__dmul_rn(pol, best), sh_c[nch]));
    a.out[q] = rec;
  }
}

// ---------------------------------------------------------------------------
// cut
// ---------------------------------------------------------------------------
// m_i - m_lo within one pass stays below this.  A pass follows ONE line: in grid steps of 1/256 sample, g = rint (256 (a
// + e i)) moves over the pass's outputs by at most 256 |e| per output (4096 in all at 1/64 over a whole tile) and one
// more for each of the two roundings at its ends: 4098 at the outside.  m = floor ((g + 128) / 256) then moves by at
// most 4098 / 256 + 1 = 17.  The same span as track_cut_kernel's, so the same LDS.
constexpr int kPcSpread = 20;
constexpr int kPcStage = delay_cut_stage(kPcSpread);   // staged samples
static_assert(kCutTile * PEAQ_TRACK_MAX_E * kCutSteps + 2 <= (kPcSpread - 2) * kCutSteps, "the spread of m over a pass");

struct PiecesArgs {
  size_t in_stride, out_stride; // samples per channel between pairs
  const uint32_t* n_in;         // device [n_pairs]
  const uint32_t* skip;
  const uint32_t* n_keep;
  const uint32_t* n_pieces;     // 0: every piece of the pair is (0, 0), its bits are moved
  const uint32_t* off;          // the pair's first piece in a, e and b
  const double* a;              // device [sum of n_pieces]
  const double* e;
  const uint32_t* b;
  int channels;
};

template <int C>
__device__ __forceinline__ void pc_cut(const PiecesArgs& args, const float* __restrict__ in, float* __restrict__ out,
                                       const double* __restrict__ tab, float* lds, uint32_t n_pieces) {
  const unsigned pair = blockIdx.y;
  const long long n_in = args.n_in[pair], n_keep = args.n_keep[pair];
  const long long i0 = (long long)blockIdx.x * kCutTile;           // the tile's first output (below n_keep)
  const long long i_last = min(i0 + kCutTile, n_keep) - 1;         // ... and its last
  const uint32_t* __restrict__ pb = args.b + args.off[pair];
  const double* __restrict__ pa = args.a + args.off[pair];
  const double* __restrict__ pe = args.e + args.off[pair];
  const float* __restrict__ src = in + (size_t)pair * args.in_stride * C;
  float* __restrict__ dst = out + (size_t)pair * args.out_stride * C;
  const bool pairs8 = C == 2 && ((uintptr_t)dst & 7) == 0;         // (uniform) both channels in one store
  // ---- the pieces that meet the tile (uniform): from that of i0 on, while they start at or before i_last ----
  bool staged = false;
  for (uint32_t piece = pieces_find(pb, n_pieces, i0); piece < n_pieces; ++piece) {
    const long long first = max((long long)pb[piece], i0);         // the pass's outputs: first .. last
    if (first > i_last) break;
    const long long last = piece + 1 < n_pieces ? min((long long)pb[piece + 1] - 1, i_last) : i_last;
    const double a = pa[piece], e = pe[piece];
    long long m_a, m_b;
    int phi;
    drift_index(a, e, first, &m_a, &phi);
    drift_index(a, e, last, &m_b, &phi);
    const long long m_lo = min(m_a, m_b);
    const int n_stage = (int)(last - first) + 1 + 2 * kCutK + kPcSpread;     // (at most kPcStage)
    if (staged) __syncthreads();                                   // (uniform) the pass before this one still reads
    staged = true;
    delay_cut_pass<C, kPcSpread, true>(src, dst, pairs8, n_in, args.skip[pair], i0, first, last, m_lo, n_stage,
                                       [=](long long i, long long* m, int* ph) { drift_index(a, e, i, m, ph); },
                                       tab, lds);
  }
}

// (the buffers and the table as parameters of their own, as track_cut_kernel's)
__global__ __launch_bounds__(256, 4) void pieces_cut_kernel(const PiecesArgs args, const float* __restrict__ a_in,
                                                         float* __restrict__ a_out, const double* __restrict__ shift_tab) {
  __shared__ __attribute__((aligned(16))) float lds[2 * kPcStage];
  const unsigned pair = blockIdx.y;
  const uint32_t n_pieces = args.n_pieces[pair];
  if (cut_tile_copied(a_in, a_out, args.in_stride, args.out_stride, args.skip, args.n_keep[pair], args.channels, n_pieces == 0))
    return;
  if (args.channels == 2)
    pc_cut<2>(args, a_in, a_out, shift_tab, lds, n_pieces);
  else
    pc_cut<1>(args, a_in, a_out, shift_tab, lds, n_pieces);
}

#pragma clang fp contract(off)                        // host arithmetic from here on: every operation rounded on its own

size_t steps_per_cand(uint32_t span_max) {
  return (size_t)std::max<uint32_t>(steps_chunks(std::min<uint32_t>(span_max, PEAQ_STEP_MAX_SPAN)), 1) * kStRow * sizeof(double);
}

int check_steps_knots(const std::string& w, uint32_t n_windows, uint32_t window, uint32_t n_common) {
  if (int rc = check_delay_window(w, window)) return rc;
  if (n_windows > PEAQ_DRIFT_MAX_WINDOWS)
    return fail(PEAQ_ERR_ARG, w + ": " + std::to_string(n_windows) + " windows are more than " + std::to_string(PEAQ_DRIFT_MAX_WINDOWS));
  if ((uint64_t)n_windows * window > n_common)
    return fail(PEAQ_ERR_ARG, w + ": " + std::to_string(n_windows) + " windows of " + std::to_string(window) +
                                  " samples pass n_common " + std::to_string(n_common));
  return PEAQ_OK;
}
int check_steps_params(const std::string& w, double min_step, double ratio, double min_gain, double max_e) {
  if (!(min_step >= 0.) || !std::isfinite(min_step))
    return fail(PEAQ_ERR_ARG, w + ": min_step " + std::to_string(min_step) + " is negative or not finite");
  if (!(ratio >= 0.) || !std::isfinite(ratio))
    return fail(PEAQ_ERR_ARG, w + ": ratio " + std::to_string(ratio) + " is negative or not finite");
  if (!(min_gain >= 0.) || !std::isfinite(min_gain))
    return fail(PEAQ_ERR_ARG, w + ": min_gain " + std::to_string(min_gain) + " is negative or not finite");
  if (!(max_e > 0. && max_e <= PEAQ_TRACK_MAX_E))
    return fail(PEAQ_ERR_ARG, w + ": max_e " + std::to_string(max_e) + " is outside (0, 0.015625]");
  return PEAQ_OK;
}

// the candidates of one pair, as the public record
uint32_t pair_candidates(const double* knots, uint32_t W, uint32_t window, uint32_t n_common, uint32_t pair, double min_step,
                         double ratio, peaq_step_candidate* out) {
  std::vector<StepCandidate> cd(std::max<uint32_t>(W, 2) - 1);
  const uint32_t n = steps_candidates(knots, W, window, n_common, min_step, ratio, cd.data());
  for (uint32_t j = 0; j < n; ++j) out[j] = {pair, cd[j].lo, cd[j].hi, cd[j].LA, cd[j].LB};
  return n;
}

// peaq_steps_fit behind its checks of the arrays and parameters
int pair_fit(const std::string& w, const double* knots, uint32_t W, uint32_t window, uint32_t n_common, double min_step,
             double ratio, double min_gain, double max_e, peaq_step* steps, uint32_t n_steps, peaq_pieces* out, uint32_t* b,
             double* a, double* e) {
  std::vector<StepCandidate> cd(std::max<uint32_t>(W, 2) - 1);
  const uint32_t n = steps_candidates(knots, W, window, n_common, min_step, ratio, cd.data());
  if (n != n_steps)
    return fail(PEAQ_ERR_ARG, w + ": n_steps " + std::to_string(n_steps) + " is not the number of candidates, " + std::to_string(n));
  std::vector<StepFound> found(n);
  for (uint32_t j = 0; j < n; ++j) {
    if (steps[j].LA != cd[j].LA || steps[j].LB != cd[j].LB)
      return fail(PEAQ_ERR_ARG, w + ": record " + std::to_string(j) + ": LA " + std::to_string(steps[j].LA) + ", LB " +
                                    std::to_string(steps[j].LB) + " are not the candidate's " + std::to_string(cd[j].LA) + ", " +
                                    std::to_string(cd[j].LB));
    found[j] = {steps[j].c, steps[j].flags, steps[j].LA, steps[j].LB, steps[j].gain_left, steps[j].gain_right, steps[j].norm};
  }
  PiecesSummary s;
  steps_fit(knots, W, window, cd.data(), found.data(), n, min_gain, max_e, b, a, e, &s);
  for (uint32_t j = 0; j < n; ++j) steps[j].flags = found[j].flags;
  std::memset(out, 0, sizeof *out);
  out->flags = s.flags;
  out->n_candidates = s.n_candidates;
  out->n_accepted = s.n_accepted;
  out->n_pieces = s.n_pieces;
  out->max_abs_e = s.max_abs_e;
  return PEAQ_OK;
}

}  // namespace

static_assert(kStepNone == PEAQ_STEP_F_NONE && kStepSpan == PEAQ_STEP_F_SPAN && kStepWeak == PEAQ_STEP_F_WEAK &&
                  kPiecesRange == PEAQ_PIECES_F_RANGE, "peaq_steps_math.h's flags");
static_assert(kStMaxL == PEAQ_STEP_MAX_L, "the largest |LA|, |LB|");
static_assert(sizeof(peaq_step_candidate) == 20 && sizeof(peaq_step) == 48 && sizeof(peaq_pieces) == 24, "the records");

struct StepsState {
  StageScratch scratch;         // the chunks' rows of a group of candidates
  LenStage lens;                // locate: [n_cand][8]
};

void steps_release(peaq_ctx* c) { release_stage(c->sp); }

extern "C" size_t peaq_step_candidate_size(void) { return sizeof(peaq_step_candidate); }
extern "C" size_t peaq_step_size(void) { return sizeof(peaq_step); }
extern "C" size_t peaq_pieces_size(void) { return sizeof(peaq_pieces); }

extern "C" size_t peaq_steps_workspace_bytes(int n_cand, uint32_t span_max) {
  return pair_groups(steps_per_cand(span_max), n_cand, kStScratchBudget).bytes;
}

extern "C" int peaq_batch_locate_steps(peaq_ctx* c, int channels, int n_pairs, const float* d_ref, const float* d_test,
                                       size_t pair_stride, const uint32_t* n_ref, const uint32_t* n_test, uint32_t n_uniform,
                                       const int32_t* lag0, int n_cand, const peaq_step_candidate* cand, peaq_step* d_out,
                                       void* stream_) {
  const std::string w("peaq_batch_locate_steps");
  if (int rc = check_shape(w, channels, n_pairs)) return rc;
  if (int rc = check_count(w, n_cand, "n_cand", "candidates")) return rc;
  if (n_pairs > 0 && (!d_ref || !d_test)) return fail(PEAQ_ERR_ARG, w + ": NULL buffer");
  if (n_pairs > 0 && !lag0) return fail(PEAQ_ERR_ARG, w + ": NULL lag0");
  if (n_cand > 0 && (!cand || !d_out)) return fail(PEAQ_ERR_ARG, w + ": NULL cand or d_out");
  if ((n_ref == nullptr) != (n_test == nullptr))
    return fail(PEAQ_ERR_ARG, w + ": n_ref and n_test must both be given or both be NULL");
  if (int rc = check_lengths(w, n_pairs, n_ref, n_uniform, "n_ref", pair_stride, "pair_stride")) return rc;
  if (int rc = check_lengths(w, n_pairs, n_test, n_uniform, "n_test", pair_stride, "pair_stride")) return rc;
  const size_t nc = (size_t)std::max(n_cand, 0);
  std::vector<uint32_t> h(nc * kStCandWords);
  uint32_t span_max = 0;
  for (size_t q = 0; q < nc; ++q) {
    const peaq_step_candidate& cd = cand[q];
    const std::string where = w + ": candidate " + std::to_string(q);
    if (cd.pair >= (uint32_t)std::max(n_pairs, 0))
      return fail(PEAQ_ERR_ARG, where + ": pair " + std::to_string(cd.pair) + " is not below n_pairs " + std::to_string(n_pairs));
    const uint32_t nr = n_ref ? n_ref[cd.pair] : n_uniform, nt = n_test ? n_test[cd.pair] : n_uniform;
    uint32_t sr, st, common;
    peaq_aligned_lengths(lag0[cd.pair], nr, nt, &sr, &st, &common);
    if (cd.lo >= cd.hi)
      return fail(PEAQ_ERR_ARG, where + ": lo " + std::to_string(cd.lo) + " is not below hi " + std::to_string(cd.hi));
    if (cd.hi > common)
      return fail(PEAQ_ERR_ARG, where + ": hi " + std::to_string(cd.hi) + " passes the pair's n_common " + std::to_string(common));
    if (cd.LA == cd.LB) return fail(PEAQ_ERR_ARG, where + ": LA and LB are both " + std::to_string(cd.LA));
    for (int32_t L : {cd.LA, cd.LB})
      if (L > kStMaxL || L < -kStMaxL)
        return fail(PEAQ_ERR_ARG, where + ": a delay of " + std::to_string(L) + " is outside -1064960 .. 1064960");
    uint32_t* row = &h[q * kStCandWords];
    row[0] = cd.pair;
    row[1] = cd.lo;
    row[2] = cd.hi;
    std::memcpy(&row[3], &cd.LA, sizeof(uint32_t));
    std::memcpy(&row[4], &cd.LB, sizeof(uint32_t));
    row[5] = sr;
    row[6] = st;
    row[7] = nt;
    if (cd.hi - cd.lo <= PEAQ_STEP_MAX_SPAN) span_max = std::max(span_max, cd.hi - cd.lo);
  }
  if (!c) return fail(PEAQ_ERR_ARG, w + ": ctx is NULL");
  if (n_cand == 0) return PEAQ_OK;

  hipStream_t stream = static_cast<hipStream_t>(stream_);
  std::lock_guard<std::mutex> lock(c->mu);
  HIP_TRY(hipSetDevice(c->device));
  if (!c->sp) c->sp = new StepsState;
  StepsState* st = c->sp;
  const uint32_t nch = std::max<uint32_t>(steps_chunks(span_max), 1);
  const PairGroups pg = pair_groups(steps_per_cand(span_max), n_cand, kStScratchBudget);
  const int group = pg.group;
  if (int rc = st->scratch.acquire(pg.bytes, stream)) return rc;
  LenSlot* slot = nullptr;
  if (int rc = st->lens.upload(h.data(), h.size(), stream, &slot)) return rc;
  LocateArgs a{};
  a.ref = d_ref;
  a.test = d_test;
  a.stride = pair_stride;
  a.channels = channels;
  a.nch_max = nch;
  a.part = st->scratch.buf.as<double>();
  hipError_t launched = hipSuccess;
  for (int q0 = 0; q0 < n_cand; q0 += group) {
    const unsigned g = (unsigned)std::min(group, n_cand - q0);
    a.cand = slot->dev.as<uint32_t>() + (size_t)q0 * kStCandWords;
    a.out = d_out + q0;
    if (span_max) hipLaunchKernelGGL(steps_chunk_kernel, dim3(nch, g), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(steps_pick_kernel, dim3(g), dim3(256), 0, stream, a);
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

extern "C" int peaq_steps_candidates(const double* knots, uint32_t n_windows, uint32_t window, uint32_t n_common, uint32_t pair,
                                     double min_step, double ratio, peaq_step_candidate* out, uint32_t* n) {
  const std::string w("peaq_steps_candidates");
  if (!out || !n || (n_windows && !knots)) return fail(PEAQ_ERR_ARG, w + ": knots, out or n is NULL");
  if (int rc = check_steps_knots(w, n_windows, window, n_common)) return rc;
  if (int rc = check_steps_params(w, min_step, ratio, 0., PEAQ_TRACK_MAX_E)) return rc;
  *n = pair_candidates(knots, n_windows, window, n_common, pair, min_step, ratio, out);
  return PEAQ_OK;
}

extern "C" int peaq_steps_fit(const double* knots, uint32_t n_windows, uint32_t window, uint32_t n_common, double min_step,
                              double ratio, double min_gain, double max_e, peaq_step* steps, uint32_t n_steps, peaq_pieces* out,
                              uint32_t* b, double* a, double* e) {
  const std::string w("peaq_steps_fit");
  if (!out || !b || !a || !e) return fail(PEAQ_ERR_ARG, w + ": out, b, a or e is NULL");
  if ((n_windows && !knots) || (n_steps && !steps)) return fail(PEAQ_ERR_ARG, w + ": knots or steps is NULL");
  if (int rc = check_steps_knots(w, n_windows, window, n_common)) return rc;
  if (int rc = check_steps_params(w, min_step, ratio, min_gain, max_e)) return rc;
  return pair_fit(w, knots, n_windows, window, n_common, min_step, ratio, min_gain, max_e, steps, n_steps, out, b, a, e);
}

extern "C" void peaq_pieces_index(uint32_t n_pieces, const uint32_t* b, const double* a, const double* e, int64_t i, int64_t* m,
                                  int32_t* phi) {
  long long mm = 0;
  int pp = 0;
  if (n_pieces && b && a && e && i >= 0) pieces_index(n_pieces, b, a, e, i, &mm, &pp);
  if (m) *m = mm;
  if (phi) *phi = pp;
}

extern "C" void peaq_pieces_lengths(int32_t lag0, uint32_t n_pieces, const uint32_t* b, const double* a, const double* e,
                                    uint32_t n_ref, uint32_t n_test, uint32_t* skip_ref, uint32_t* skip_test, uint32_t* n_keep) {
  uint32_t sr, st, common;
  peaq_aligned_lengths(lag0, n_ref, n_test, &sr, &st, &common);
  if (skip_ref) *skip_ref = sr;
  if (skip_test) *skip_test = st;
  if (!n_keep) return;
  const double zero = 0.;
  const uint32_t b0 = 0;
  const bool none = !n_pieces || !b || !a || !e;       // (no pieces: the plain cut's lengths)
  *n_keep = pieces_keep(none ? 1 : n_pieces, none ? &b0 : b, none ? &zero : a, none ? &zero : e, st, common, n_test);
}

extern "C" int peaq_batch_estimate_steps(peaq_ctx* c, int channels, int n_pairs, const float* d_ref, const float* d_test,
                                         size_t pair_stride, const uint32_t* n_ref, const uint32_t* n_test, uint32_t n_uniform,
                                         const int32_t* lag0, uint32_t window, uint32_t R, double min_corr, double max_e,
                                         double min_step, double ratio, double min_gain, uint32_t w_max,
                                         peaq_delay* d_win_delay, peaq_subdelay* d_win_sub, peaq_drift* drift, peaq_track* track,
                                         double* knots, uint32_t steps_stride, peaq_step* steps, peaq_pieces* pieces,
                                         uint32_t piece_stride, uint32_t* b, double* a, double* e, void* stream_) {
  const std::string w("peaq_batch_estimate_steps");
  if (int rc = check_steps_params(w, min_step, ratio, min_gain, max_e)) return rc;
  const uint32_t seg_stride = std::max<uint32_t>(w_max, 2) - 1;
  if (steps_stride < seg_stride)
    return fail(PEAQ_ERR_ARG, w + ": steps_stride " + std::to_string(steps_stride) + " is below max (w_max - 1, 1) for w_max " +
                                  std::to_string(w_max));
  if ((uint64_t)piece_stride < 2 * (uint64_t)seg_stride)
    return fail(PEAQ_ERR_ARG, w + ": piece_stride " + std::to_string(piece_stride) + " is below 2 max (w_max - 1, 1) for w_max " +
                                  std::to_string(w_max));
  if (n_pairs > 0 && (!steps || !pieces || !b || !a || !e)) return fail(PEAQ_ERR_ARG, w + ": NULL steps, pieces, b, a or e");
  const size_t np = (size_t)std::max(n_pairs, 0);
  // 1: the track (its own segments stay here: the pieces are built from the knots)
  std::vector<double> sa(np * seg_stride), se(np * seg_stride);
  if (int rc = peaq_batch_estimate_track(c, channels, n_pairs, d_ref, d_test, pair_stride, n_ref, n_test, n_uniform, lag0, window,
                                         R, min_corr, max_e, w_max, d_win_delay, d_win_sub, drift, track, knots, seg_stride,
                                         sa.data(), se.data(), stream_))
    return rc;
  if (n_pairs == 0) return PEAQ_OK;
  // 2: every pair's candidates
  std::vector<peaq_step_candidate> cand;
  std::vector<uint32_t> first(np + 1, 0), common(np);
  std::vector<peaq_step_candidate> row(seg_stride);
  for (size_t p = 0; p < np; ++p) {
    const uint32_t nr = n_ref ? n_ref[p] : n_uniform, nt = n_test ? n_test[p] : n_uniform;
    peaq_aligned_lengths(lag0[p], nr, nt, nullptr, nullptr, &common[p]);
    const uint32_t n = pair_candidates(knots + p * w_max, track[p].n_windows, window, common[p], (uint32_t)p, min_step, ratio,
                                       row.data());
    cand.insert(cand.end(), row.begin(), row.begin() + n);
    first[p + 1] = (uint32_t)cand.size();
  }
  if (cand.size() > 65535)
    return fail(PEAQ_ERR_ARG, w + ": " + std::to_string(cand.size()) + " candidates are more than 65535 in one call");
  // 3: locate, read back
  std::vector<peaq_step> found(cand.size());
  if (!cand.empty()) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_TRY(hipSetDevice(c->device));
    DevBuf d_found;
    HIP_TRY(d_found.reserve(found.size() * sizeof(peaq_step)));
    if (int rc = peaq_batch_locate_steps(c, channels, n_pairs, d_ref, d_test, pair_stride, n_ref, n_test, n_uniform, lag0,
                                         (int)cand.size(), cand.data(), d_found.as<peaq_step>(), stream_))
      return rc;
    HIP_TRY(hipMemcpyAsync(found.data(), d_found.p, found.size() * sizeof(peaq_step), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
  }
  // 4: the fit per pair
  for (size_t p = 0; p < np; ++p) {
    peaq_step* ps = steps + p * steps_stride;
    uint32_t* pb = b + p * piece_stride;
    double* pa = a + p * piece_stride;
    double* pe = e + p * piece_stride;
    std::memset(ps, 0, (size_t)steps_stride * sizeof(peaq_step));
    std::fill(pb, pb + piece_stride, 0u);
    std::fill(pa, pa + piece_stride, 0.);
    std::fill(pe, pe + piece_stride, 0.);
    const uint32_t n = first[p + 1] - first[p];
    std::copy(found.begin() + first[p], found.begin() + first[p + 1], ps);
    if (int rc = pair_fit(w, knots + p * w_max, track[p].n_windows, window, common[p], min_step, ratio, min_gain, max_e, ps, n,
                          &pieces[p], pb, pa, pe))
      return rc;
  }
  return PEAQ_OK;
}

extern "C" int peaq_batch_cut_pieces(peaq_ctx* c, int channels, int n_pairs, const float* d_in, size_t in_stride,
                                     const uint32_t* n_in, const uint32_t* skip, const uint32_t* n_keep, const uint32_t* n_pieces,
                                     uint32_t piece_stride, const uint32_t* b, const double* a, const double* e, float* d_out,
                                     size_t out_stride, void* stream_) {
  const std::string w("peaq_batch_cut_pieces");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  DelayCutCall k{w, c, channels, n_pairs, d_in, in_stride, n_in, skip, n_keep, d_out, out_stride, stream};
  if (int rc = k.check(n_pieces && b && a && e, ", n_pieces, b, a or e")) return rc;
  uint64_t total = 0;
  for (size_t p = 0; p < k.np; ++p) {
    if (n_pieces[p] < 1 || n_pieces[p] > piece_stride || n_pieces[p] > PEAQ_PIECES_MAX_PER_PAIR)
      return fail(PEAQ_ERR_ARG, w + ": pair " + std::to_string(p) + ": n_pieces " + std::to_string(n_pieces[p]) +
                                    " is outside 1 .. min (piece_stride " + std::to_string(piece_stride) + ", " +
                                    std::to_string(PEAQ_PIECES_MAX_PER_PAIR) + ")");
    total += n_pieces[p];
  }
  if (total > PEAQ_PIECES_MAX_PER_CALL)
    return fail(PEAQ_ERR_ARG, w + ": " + std::to_string(total) + " pieces are more than " + std::to_string(PEAQ_PIECES_MAX_PER_CALL) +
                                  " in one call");
  k.pack(5, (size_t)total, true);
  for (size_t p = 0; p < k.np; ++p) {
    const uint32_t* pb = b + p * piece_stride;
    const size_t first = k.next_line;
    bool plain;
    if (int rc = k.add_lines(p, "piece", n_pieces[p], a + p * piece_stride, e + p * piece_stride, pb, PEAQ_TRACK_MAX_E,
                             "-0.015625 .. 0.015625", &plain, [&](uint32_t s, const auto& where) {
                               if (s == 0 && pb[0] != 0) return fail(PEAQ_ERR_ARG, where() + ": b " + std::to_string(pb[0]) + " is not 0");
                               if (s && pb[s] <= pb[s - 1])
                                 return fail(PEAQ_ERR_ARG, where() + ": b " + std::to_string(pb[s]) +
                                                               " is not above the piece before it at " + std::to_string(pb[s - 1]));
                               return (int)PEAQ_OK;
                             }))
      return rc;
    k.col(3, p) = plain ? 0 : n_pieces[p];             // (0: every piece is (0, 0), the pair's bits are moved)
    k.col(4, p) = (uint32_t)first;
  }
  if (int rc = k.upload()) return rc;
  if (!k.slot) return PEAQ_OK;
  PiecesArgs args{};
  args.in_stride = in_stride;
  args.out_stride = out_stride;
  args.n_in = k.dev_col(0);
  args.skip = k.dev_col(1);
  args.n_keep = k.dev_col(2);
  args.n_pieces = k.dev_col(3);
  args.off = k.dev_col(4);
  args.a = k.dev_a();
  args.e = k.dev_e();
  args.b = k.dev_b();
  args.channels = channels;
  hipLaunchKernelGGL(pieces_cut_kernel, dim3(k.tiles(), (unsigned)n_pairs), dim3(256), 0, stream, args, d_in, d_out, k.tab);
  return k.launched();
}

extern "C" int peaq_run_pair_steps(peaq_ctx* c, int advanced, int channels, double level_db, uint32_t rate, uint32_t max_lag,
                                   uint32_t window, int mode, double max_gain_db, const float* ref, size_t n_ref,
                                   const float* test, size_t n_test, peaq_delay* delay, peaq_track* track, peaq_pieces* pieces,
                                   peaq_step* steps, uint32_t max_steps, peaq_gain* gain, peaq_result* out) {
  const std::string w("peaq_run_pair_steps");
  if (int rc = check_delay_window(w, window)) return rc;
  const uint32_t R = std::min<uint32_t>(window / 4, 1024);
  // 1 .. 3: upload, rate conversion, estimate
  PairBuffers in;
  peaq_delay rec;
  uint32_t W = 0;
  if (int rc = begin_delay_pair(w, c, channels, level_db, rate, max_lag, window, mode, max_gain_db, ref, n_ref, test, n_test,
                                delay, gain, out, in, &rec, &W))
    return rc;
  const uint32_t* len = in.len;
  const size_t stride = in.stride;
  // 4: the track, its steps
  DevBuf d_dl, d_sb;
  const uint32_t n_seg = std::max<uint32_t>(W, 2) - 1, stride_p = 2 * n_seg;
  std::vector<double> knots(std::max<uint32_t>(W, 1)), pa(stride_p, 0.), pe(stride_p, 0.);
  std::vector<uint32_t> pb(stride_p, 0);
  std::vector<peaq_step> found(n_seg);
  std::memset(found.data(), 0, found.size() * sizeof(peaq_step));
  peaq_track tr;
  std::memset(&tr, 0, sizeof tr);
  tr.lag0 = rec.lag;
  tr.flags = PEAQ_TRACK_F_NONE;
  tr.n_segments = n_seg;
  peaq_pieces pc;
  std::memset(&pc, 0, sizeof pc);
  pc.n_pieces = 1;
  if (W >= 1) {                                        // (none: no track whatever, one piece (0, 0))
    HIP_TRY(d_dl.reserve((size_t)W * sizeof(peaq_delay)));
    HIP_TRY(d_sb.reserve((size_t)W * sizeof(peaq_subdelay)));
    if (int rc = peaq_batch_estimate_steps(c, channels, 1, in.d(0), in.d(1), stride, len, len + 1, 0, &rec.lag, window, R, 0.5,
                                           PEAQ_TRACK_MAX_E, PEAQ_STEP_MIN_STEP, PEAQ_STEP_RATIO, PEAQ_STEP_MIN_GAIN, W,
                                           d_dl.as<peaq_delay>(), d_sb.as<peaq_subdelay>(), nullptr, &tr, knots.data(), n_seg,
                                           found.data(), &pc, stride_p, pb.data(), pa.data(), pe.data(), nullptr))
      return rc;
  }
  if (track) *track = tr;
  if (pieces) *pieces = pc;
  if (steps) std::copy(found.begin(), found.begin() + std::min(max_steps, pc.n_candidates), steps);
  // 5 .. 8: both signals cut to the pieces' lengths, the test signal along the pieces; the gain; the score
  uint32_t skip[2], keep = 0;
  peaq_pieces_lengths(rec.lag, pc.n_pieces, pb.data(), pa.data(), pe.data(), len[0], len[1], &skip[0], &skip[1], &keep);
  return score_cut_pair(c, advanced, channels, level_db, in, skip, keep, mode, max_gain_db, gain,
                        [&](float* d_out, size_t out_stride) {
                          return peaq_batch_cut_pieces(c, channels, 1, in.d(1), stride, &len[1], &skip[1], &keep, &pc.n_pieces,
                                                       stride_p, pb.data(), pa.data(), pe.data(), d_out, out_stride, nullptr);
                        },
                        out);
}

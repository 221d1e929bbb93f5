// peaq_meter_bands.hip -- per-band rows of the meter's readings (peaq_session_set_meter_bands,
// peaq_session_meter_read_bands, peaq_broker_set_meter_bands, peaq_broker_meter_read_bands in include/peaq_amd.h, "meter:
// band rows"): rows 0 .. 3 of the band summary -- sum and maximum of the noise-to-mask ratio, its count of
// frames above 1.5 dB, sum of the reference excitation -- of every window of the meter, reduced over the window's
// counted frames behind the launches of a running session or a broker's ticks.
//
// The counted frames of window k are the first .. the last of its frames [k H, k H + W) that have kTraceAbove, the
// frames in between included: what accumulators that start fresh at the window's first frame count (movaccum.c:317-362),
// and the rule of the batch side's band summary (backend_summary_kernel) with the window's frames for the pair's.
//
// With the band meter on, a stream's FFT back end is the live-band instantiation (backend_liveband_kernel): beside the
// trace records of peaq_meter.hip it leaves the planes NMR and EXC_REF of every frame at the frame's index within the
// launch.  Behind the meter's own kernel of the launch one more:
//
//   meter_bands_kernel<NB>   the launch's frames into the rows of the windows that are open in them
//
//   The grid is (streams of the launch, K, channels): one wave per stream, slot of open windows and channel.  Lane
//   l < band_row / 2 owns entries 2 l and 2 l + 1 of all four rows -- NB is odd, so the lane of band NB - 1 owns the
//   rows' last entry, the count of counted frames, as its second --, and reads a frame's two planes and its rows as
//   consecutive 16-byte pieces.  The wave walks the launch's frames with the slot's current window exactly as the FFT
//   path of meter_replay (peaq_meter.hip) does, and delivers at exactly its points: a window's last frame and, in the
//   launch that ends a stream whose end is known, the oldest window that the end cuts short.  A frame's flags come from
//   its trace record and are wave-uniform.  The status follows the accumulators': kInit until the window's first frame
//   above the boundary (nothing is counted before it), from a frame below it kTentative -- the running rows are copied
//   to the saved rows at that turn -- until the next one above; every frame after the first counted one is added to the
//   running rows, and a window that ends tentative delivers its saved rows.  The delivered rows go to a ring of
//   ring_depth sets at k % ring_depth, beside the score ring, so that the host's count of delivered windows covers
//   both.  Between launches the running rows, the saved rows and the status sit in the snapshot [stream][slot][channel]
//   (the status per channel: no wave reads a word that another writes), loaded at entry and stored at exit.
//   No atomics, no LDS, no cross-lane traffic, no scratch: sixteen doubles of rows per lane.  In a broker's launch
//   every stream has its own frames and slot (MeterArgs::s_*), the rows the tick uploads anyway.
#include <hip/hip_runtime.h>

#include "peaq_device.h"
#include "peaq_kernels.h"

namespace peaq {

template <int NB>
__global__ __launch_bounds__(64) void meter_bands_kernel(MeterArgs m, MeterBandArgs mb, int channels) {
#pragma clang fp contract(off)
  constexpr int R = kMeterBandRows, ROW = band_row(NB), SNAP = meter_band_snap(NB);
  const int lane = threadIdx.x & 63;
  const unsigned strm = blockIdx.x;
  const uint32_t r = blockIdx.y;                     // the slot of open windows this wave serves (< K: the grid's)
  const unsigned ch = blockIdx.z;                    // (< channels: the grid's)
  const uint32_t W = m.window, H = m.hop, K = m.k_open;
  // the stream's frames of this launch and where its snapshots are: its own (a broker's launch) or the uniform ones
  uint32_t u0 = m.unit0, n_units = m.n_units, sidx = strm;
  if (m.s_unit0) {
    u0 = m.s_unit0[strm];
    n_units = m.s_nunits[strm];
    sidx = m.s_slot[strm];
  }
  if (n_units > (uint32_t)m.frame_stride) n_units = (uint32_t)m.frame_stride;   // (the scratch holds no more)
  const uint32_t T = m.s_total_frames ? m.s_total_frames[strm] : m.total_frames;
  const uint32_t total_units = m.s_total_units ? m.s_total_units[strm] : m.total_units;
  const uint32_t u1 = u0 + n_units;
  const bool known = T != UINT_MAX;                  // the stream's end is known: this is (part of) its flush
  const bool last = known && u1 == total_units;      // ... and this launch ends the stream's frames
  const bool own = 2 * lane < NB;                    // lanes 0 .. ROW / 2 - 1
  const bool cnt = 2 * lane + 1 == NB;               // ... the last of them: its second entry is the count
  const int e0 = own ? 2 * lane : 0;                 // (the other lanes read entry 0 and store nothing)

  // window k (the FFT path of meter_replay): is there one, its first frame, the frame after its last one
  auto exists = [&](uint32_t k) { return !known || (uint64_t)k * H < T; };
  uint32_t k = r;
  if (u0 > 0) {
    const uint64_t q = (u0 - 1) / H;                 // the largest k whose first frame is before this launch
    if (q >= r) k = (uint32_t)(q - (q - r) % K);
    while (!exists(k) && k >= K) k -= K;
  }
  uint32_t fk = k * H, ek = k * H + W;
  uint32_t nf = exists(k + K) ? (k + K) * H : UINT_MAX;

  double* __restrict__ snap = mb.open + (((size_t)sidx * K + r) * channels + ch) * SNAP;
  double* __restrict__ ring = mb.ring + (size_t)sidx * m.ring_depth * channels * (R * ROW);
  double run[R][2], sav[R][2];                       // (plain doubles: the rows stay in registers)
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const double2 a = *reinterpret_cast<const double2*>(snap + j * ROW + e0);
    const double2 b = *reinterpret_cast<const double2*>(snap + (R + j) * ROW + e0);
    run[j][0] = a.x;
    run[j][1] = a.y;
    sav[j][0] = b.x;
    sav[j][1] = b.y;
  }
  int status = __builtin_amdgcn_readfirstlane(*reinterpret_cast<const int*>(snap + 2 * R * ROW));
  auto fresh = [&]() {
#pragma unroll
    for (int j = 0; j < R; ++j) run[j][0] = run[j][1] = sav[j][0] = sav[j][1] = 0.;
    status = kInit;
  };
  // a finished window's rows into the delivered ring: the saved ones if it ends tentative (nothing after its last frame
  // above the boundary counts); a window without a counted frame has zeros in both
  auto deliver = [&](uint32_t kk) {
    double* __restrict__ rp = ring + ((size_t)(kk % m.ring_depth) * channels + ch) * (R * ROW);
    if (!own) return;
    const bool tent = status == kTentative;
#pragma unroll
    for (int j = 0; j < R; ++j)
      *reinterpret_cast<double2*>(rp + j * ROW + e0) =
          make_double2(tent ? sav[j][0] : run[j][0], tent ? sav[j][1] : run[j][1]);
  };

  if (u0 < u1) {
    const FrameTrace* __restrict__ trace = m.frames + (size_t)strm * m.frame_stride;
    const double* __restrict__ planes = mb.planes + (size_t)strm * m.frame_stride * channels * (2 * ROW);
    struct Raw {
      double2 nmr, exc;
      uint32_t flags;
    };
    auto load_of = [&](uint32_t unit) {
      const double* __restrict__ p = planes + ((size_t)(unit - u0) * channels + ch) * (2 * ROW) + e0;
      Raw v;
      v.nmr = *reinterpret_cast<const double2*>(p);
      v.exc = *reinterpret_cast<const double2*>(p + ROW);
      v.flags = trace[unit - u0].flags;
      return v;
    };
    Raw cur = load_of(u0);
    for (uint32_t unit = u0; unit < u1; ++unit) {
      // (the next frame's loads before this frame's adds; the last frame reads itself again)
      const Raw nxt = load_of(unit + 1 < u1 ? unit + 1 : unit);
      if (unit >= nf) {                              // the slot's next window begins
        k += K;
        fk = nf;
        ek = k * H + W;
        nf = exists(k + K) ? (k + K) * H : UINT_MAX;
      }
      if (unit == fk) fresh();
      if (unit >= fk && unit < ek) {
        const bool above = (__builtin_amdgcn_readfirstlane((int)cur.flags) & (int)kTraceAbove) != 0;
        if (above) {
          status = kNormal;
        } else if (status == kNormal) {
#pragma unroll
          for (int j = 0; j < R; ++j) {
            sav[j][0] = run[j][0];
            sav[j][1] = run[j][1];
          }
          status = kTentative;
        }
        if (status != kInit) {
          const double n0 = cur.nmr.x, n1 = cur.nmr.y;
          run[kSumNmrSum][0] += n0;
          run[kSumNmrSum][1] += cnt ? 1. : n1;
          if (n0 > run[kSumNmrMax][0]) run[kSumNmrMax][0] = n0;
          if (cnt)
            run[kSumNmrMax][1] += 1.;
          else if (n1 > run[kSumNmrMax][1])
            run[kSumNmrMax][1] = n1;
          run[kSumNmrDisturbed][0] += n0 > 1.41253754462275 ? 1. : 0.;
          run[kSumNmrDisturbed][1] += cnt || n1 > 1.41253754462275 ? 1. : 0.;
          run[kSumExcRef][0] += cur.exc.x;
          run[kSumExcRef][1] += cnt ? 1. : cur.exc.y;
        }
        if (unit + 1 == ek) deliver(k);
      }
      cur = nxt;
    }
  }
  if (last) {
    // every window of the slot has begun by now (the FFT path has a frame for each that exists)
    if (exists(k + K)) {
      k += K;
      fk = k * H;
      fresh();
    } else if (exists(k) && fk >= u1) {
      fresh();
    }
    if (exists(k)) {
      const uint64_t b = (uint64_t)k * H + W;
      const uint32_t k_old = T >= W ? (T - W) / H + 1 : 0;   // the oldest window that the stream's end cuts short
      // (a window with b == T was stored at its last frame, above)
      if (b > T && k == k_old) deliver(k);
    }
  }
  if (own) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      *reinterpret_cast<double2*>(snap + j * ROW + e0) = make_double2(run[j][0], run[j][1]);
      *reinterpret_cast<double2*>(snap + (R + j) * ROW + e0) = make_double2(sav[j][0], sav[j][1]);
    }
  }
  if (lane == 0) *reinterpret_cast<int*>(snap + 2 * R * ROW) = status;
}

hipError_t launch_meter_bands(const MeterArgs& m, const MeterBandArgs& mb, bool advanced, int channels, unsigned n_streams,
                              hipStream_t stream) {
  if (n_streams == 0) return hipSuccess;
  const bool per = m.s_unit0 != nullptr;             // a broker's launch: every stream at its own position
  if (!mb.planes || !mb.open || !mb.ring || !m.frames || !m.frame_stride || m.window < 1 || m.hop < 1 ||
      m.k_open != (m.window + m.hop - 1) / m.hop || m.k_open > kMeterBandsMaxOpen || m.ring_depth < 1 ||
      m.ring_depth > kMeterBandsMaxDepth + 2 || (channels != 1 && channels != 2) ||
      (!per && m.n_units > m.frame_stride) || (per && (!m.s_nunits || !m.s_slot || !m.s_total_frames || !m.s_total_units)))
    return hipErrorInvalidValue;
  const dim3 grid(n_streams, m.k_open, channels);
  if (advanced)
    hipLaunchKernelGGL(meter_bands_kernel<55>, grid, dim3(64), 0, stream, m, mb, channels);
  else
    hipLaunchKernelGGL(meter_bands_kernel<109>, grid, dim3(64), 0, stream, m, mb, channels);
  return hipGetLastError();
}

}  // namespace peaq

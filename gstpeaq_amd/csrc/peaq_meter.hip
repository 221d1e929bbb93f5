// peaq_meter.hip -- sliding-window scores of a live stream (peaq_session_set_meter, peaq_session_meter_read,
// peaq_broker_set_meter, peaq_broker_meter_read in include/peaq_amd.h): the reading of the batch side's
// windows and spans (peaq_replay.hip), continuously, behind the launches of a running session or a broker's ticks.
//
// Window k of a stream covers FFT frames [k H, k H + W), W the window and H the hop in frames, and in the advanced
// version the filter-bank blocks [start_k / 192, e_k / 192), start_k = k ? 1024 (k H + 1) : 0, e_k = 1024 (k H + W + 1);
// a window that takes the stream's last frame takes the blocks to the last, the flush block included.  Its reading is
// the read-out of accumulators reset just before its first unit and then given what the stream's own accumulators are
// given in its units.  K = ceil (W / H) windows are open at once; window k lives in slot k % K, and the windows of one
// slot are disjoint in time because K H >= W.
//
// A metered session's back ends are the live instantiations (backend_live_kernel, fb_backend_live_kernel), which leave
// every unit's MOV-layer values and gate flags at the unit's index within the launch.  Behind each of them one kernel:
//
//   meter_basic_kernel     the launch's frames into all eleven accumulators of the basic version
//   meter_adv_fft_kernel   the launch's frames into SegmentalNMR, EHS and the energies of the advanced version
//   meter_adv_fb_kernel    the launch's blocks into RmsModDiff, RmsNoiseLoudAsym and AvgLinDist
//
//   The grid is (streams of the launch, ceil (K / slots)); the lane layout and the feeds are span_replay's
//   (peaq_replay_feed.h): lane l owns accumulator l % L of channel (l / L) & 1 of slot l / (2 L).  A lane walks the
//   launch's units with the window k of its slot that is current: it moves on to window k + K at that window's first
//   unit, sets its twelve fields to what launch_points_init leaves at a window's first unit, feeds the units of the
//   window, and after the window's last unit stores the fields into the delivered ring at k % ring_depth.  Between
//   launches the fields sit in the slot's snapshot [stream][slot], loaded at entry and stored at exit.  A launch that
//   knows the stream's end (total_frames, total_units: the flush) stores, after the stream's last unit of its path, the
//   window that ends on the last frame and the OLDEST window that the end cuts short; younger cut windows are dropped.
//   Such a launch may have no unit at all: a stream whose blocks were all whole ones has no flush block, and the windows
//   that run to the last block end there all the same.
//   No atomics, no LDS, no cross-lane traffic: every lane stores what it owns, the head lane of a slot the counts and
//   the energies.  The two kernels of the advanced version write disjoint words of the same snapshots; each may be
//   windows ahead of the other between a session's launches, and both are at the same window (the filter-bank path at
//   most one ahead) whenever a push or the flush returns; the broker's ticks keep a metered session's blocks at the
//   frames' sample horizon for the same end, and the tick of a flush frame may leave the FFT path two windows ahead
//   for a tick -- which is why the ring has two slots more than the depth the caller asked for, and why the host counts
//   as delivered only what both paths have finished.  In a broker's launch every stream has its own units and slot
//   (MeterArgs::s_*): the rows and windows the tick uploads for its back ends.
#include <hip/hip_runtime.h>

#include "peaq_device.h"
#include "peaq_kernels.h"
#include "peaq_replay_feed.h"

namespace peaq {

namespace {

template <class Feed>
__device__ __forceinline__ void meter_replay(const MeterArgs& m, const double* __restrict__ records, int channels) {
#pragma clang fp contract(off)
  constexpr int L = Feed::kLanes, kSlots = 64 / (2 * L);
  constexpr bool FFT = Feed::kFft;
  const int lane = threadIdx.x & 63;
  const int a = lane % L, ch = (lane / L) & 1, slot = lane / (2 * L);
  const unsigned strm = blockIdx.x;
  const uint32_t r = kSlots * blockIdx.y + slot;     // the slot of open windows this lane serves
  const uint32_t W = m.window, H = m.hop, K = m.k_open;
  // the stream's units of this launch and where its snapshots are: its own (a broker's launch) or the uniform ones
  uint32_t u0 = m.unit0, n_units = m.n_units, sidx = strm;
  if (!FFT && m.s_win) {
    const FbPairWindow w = m.s_win[strm];
    u0 = w.block0;
    n_units = w.n_blocks;
    sidx = w.slot;
  } else if (FFT && m.s_unit0) {
    u0 = m.s_unit0[strm];
    n_units = m.s_nunits[strm];
    sidx = m.s_slot[strm];
  }
  {
    const uint32_t most = (uint32_t)(FFT ? m.frame_stride : m.block_stride);   // (the trace scratch holds no more)
    if (n_units > most) n_units = most;
  }
  const uint32_t T = m.s_total_frames ? m.s_total_frames[strm] : m.total_frames;
  const uint32_t total_units = m.s_total_units ? m.s_total_units[strm] : m.total_units;
  const uint32_t u1 = u0 + n_units;
  const bool known = T != UINT_MAX;                  // the stream's end is known: this is (part of) its flush
  const bool last = known && u1 == total_units;      // ... and this launch ends the units of this path
  const bool used = a < Feed::kUsed;
  const bool own = r < K && used && ch < channels;
  const bool head_lane = own && a == 0 && ch == 0;   // the slot's counts and energies
  const int lane_a = used ? a : 0, lane_ch = ch < channels ? ch : 0;
  const int acc = Feed::acc(lane_a), mode = Feed::mode(lane_a);

  // window k: is there one (its first frame lies in the stream), its first unit, and the unit after its last one --
  // UINT_MAX for a window of the filter-bank path that runs to the stream's end (stored after the walk, below)
  auto exists = [&](uint32_t k) { return !known || (uint64_t)k * H < T; };
  auto first_unit = [&](uint32_t k) -> uint32_t {
    if (FFT) return k * H;
    return k ? (uint32_t)(1024ull * ((uint64_t)k * H + 1) / 192u) : 0u;
  };
  auto end_unit = [&](uint32_t k) -> uint32_t {
    const uint64_t b = (uint64_t)k * H + W;
    if (FFT) return (uint32_t)b;
    return known && b >= T ? UINT_MAX : (uint32_t)(1024ull * (b + 1) / 192u);
  };

  // the slot's current window at entry: the last one whose first unit is before this launch, else the slot's first
  uint32_t k = r;
  if (u0 > 0) {
    const uint32_t up = u0 - 1;
    uint64_t q;                                      // the largest k with first_unit (k) <= up
    if (FFT) {
      q = up / H;
    } else {
      const uint64_t fr = (192ull * up + 191u) / 1024u;
      q = fr >= 1 ? (fr - 1) / H : 0;
    }
    if (q >= r) k = (uint32_t)(q - (q - r) % K);
    while (!exists(k) && k >= K) k -= K;
  }
  uint32_t fk = first_unit(k), ek = end_unit(k);
  uint32_t nf = exists(k + K) ? first_unit(k + K) : UINT_MAX;

  PointSnap* __restrict__ op = m.open + (size_t)sidx * K + (r < K ? r : 0);   // (touched by `own` lanes only)
  PointSnap* __restrict__ ring = m.ring + (size_t)sidx * m.ring_depth;
  double f[kAccFields];
  int status = kInit;
  double sig_e = 0., noise_e = 0.;
  if (own) {
#pragma unroll
    for (int i = 0; i < kAccFields; ++i) f[i] = op->acc[ch][acc][i];
    status = op->status[acc];
  } else {
#pragma unroll
    for (int i = 0; i < kAccFields; ++i) f[i] = 0.;
  }
  if (FFT && head_lane) {
    sig_e = op->sig_energy;
    noise_e = op->noise_energy;
  }
  // what launch_points_init leaves: zeros, the AVG_WINDOW history at its NaN sentinels (movaccum.c:293), status initial
  auto fresh = [&]() {
#pragma unroll
    for (int i = 0; i < kAccFields; ++i) f[i] = i >= F_P0 && i <= F_P2 ? __builtin_nan("") : 0.;
    status = kInit;
    sig_e = 0.;
    noise_e = 0.;
  };
  // a finished window's fields into the delivered ring; `count` its units of this path
  auto deliver = [&](uint32_t kk, uint32_t count) {
    PointSnap* __restrict__ rp = ring + kk % m.ring_depth;
    if (own) {
#pragma unroll
      for (int i = 0; i < kAccFields; ++i) rp->acc[ch][acc][i] = f[i];
      if (ch == 0) rp->status[acc] = status;
    }
    if (head_lane) {
      if (FFT) {
        rp->frames = count;
        rp->sig_energy = sig_e;
        rp->noise_energy = noise_e;
      } else {
        rp->fb_blocks = count;
      }
    }
  };

  if (u0 < u1) {
    const LaneSrc src = Feed::source(lane_a, lane_ch);
    const char* __restrict__ trace =
        FFT ? reinterpret_cast<const char*>(m.frames + (size_t)strm * m.frame_stride)
            : reinterpret_cast<const char*>(m.blocks + (size_t)strm * m.block_stride);
    constexpr size_t kTraceBytes = FFT ? sizeof(FrameTrace) : sizeof(BlockTrace);
    const double* __restrict__ recs = FFT ? records + (size_t)strm * m.rec_stride * channels * kRecDoubles : nullptr;
    auto load_of = [&](uint32_t unit) {
      return Feed::load(trace + (size_t)(unit - u0) * kTraceBytes,
                        FFT ? recs + (size_t)(unit - u0) * channels * kRecDoubles : nullptr, channels, lane_ch, src);
    };
    Given cur = Feed::feed(load_of(u0), lane_a, lane_ch);
    for (uint32_t unit = u0; unit < u1; ++unit) {
      // (the next unit's loads before this unit's adds; the last unit reads itself again)
      const Raw nxt = load_of(unit + 1 < u1 ? unit + 1 : unit);
      if (unit >= nf) {                              // the slot's next window begins
        k += K;
        fk = nf;
        ek = end_unit(k);
        nf = exists(k + K) ? first_unit(k + K) : UINT_MAX;
      }
      if (unit == fk) fresh();
      if (unit >= fk && unit < ek) {
        if (own) replay_accumulate<Feed>(f, status, sig_e, noise_e, cur, mode, head_lane);
        if (unit + 1 == ek) deliver(k, unit + 1 - fk);
      }
      cur = Feed::feed(nxt, lane_a, lane_ch);
    }
  }
  if (last) {
    // every window of the slot has begun by now, but one that has no unit of this path (its blocks would start where a
    // stream without a flush block ends): it reads as fresh
    if (exists(k + K)) {
      k += K;
      fk = first_unit(k);
      fresh();
    } else if (exists(k) && fk >= u1) {
      fresh();
    }
    if (exists(k)) {
      const uint64_t b = (uint64_t)k * H + W;
      const uint32_t k_old = T >= W ? (T - W) / H + 1 : 0;   // the oldest window that the stream's end cuts short
      // (the FFT path has stored a window with b == T at its last frame, above)
      const bool at_end = FFT ? b > T : b >= T;
      if (at_end && (b == T || k == k_old)) deliver(k, u1 > fk ? u1 - fk : 0u);
    }
  }
  if (own) {
#pragma unroll
    for (int i = 0; i < kAccFields; ++i) op->acc[ch][acc][i] = f[i];
    if (ch == 0) op->status[acc] = status;
  }
  if (FFT && head_lane) {
    op->sig_energy = sig_e;
    op->noise_energy = noise_e;
  }
}

}  // namespace

__global__ __launch_bounds__(64) void meter_basic_kernel(MeterArgs m, const double* __restrict__ records, int channels) {
  meter_replay<BasicFftFeed>(m, records, channels);
}

__global__ __launch_bounds__(64) void meter_adv_fft_kernel(MeterArgs m, const double* __restrict__ records,
                                                           int channels) {
  meter_replay<AdvFftFeed>(m, records, channels);
}

__global__ __launch_bounds__(64) void meter_adv_fb_kernel(MeterArgs m, int channels) {
  meter_replay<AdvFbFeed>(m, nullptr, channels);
}

// what both launches hold
static bool meter_args_ok(const MeterArgs& m, int channels) {
  return m.open && m.ring && m.window >= 1 && m.hop >= 1 && m.k_open == (m.window + m.hop - 1) / m.hop &&
         m.k_open <= kMeterMaxOpen && m.ring_depth >= 1 && (channels == 1 || channels == 2);
}

hipError_t launch_meter_fft(const MeterArgs& m, bool advanced, const double* records, int channels, unsigned n_streams,
                            hipStream_t stream) {
  if (n_streams == 0) return hipSuccess;
  const bool per = m.s_unit0 != nullptr;             // a broker's launch: every stream at its own position
  if (!meter_args_ok(m, channels) || ((m.n_units || per) && (!records || !m.frames || !m.frame_stride)) ||
      (!per && m.n_units > m.frame_stride) || (per && (!m.s_nunits || !m.s_slot || !m.s_total_frames || !m.s_total_units)))
    return hipErrorInvalidValue;
  const unsigned slots = advanced ? 8 : 2;           // open windows per wave: 64 / (2 kLanes) of the feed
  const auto kernel = advanced ? meter_adv_fft_kernel : meter_basic_kernel;
  hipLaunchKernelGGL(kernel, dim3(n_streams, (m.k_open + slots - 1) / slots), dim3(64), 0, stream, m, records, channels);
  return hipGetLastError();
}

hipError_t launch_meter_fb(const MeterArgs& m, int channels, unsigned n_streams, hipStream_t stream) {
  if (n_streams == 0) return hipSuccess;
  const bool per = m.s_win != nullptr;
  if (!meter_args_ok(m, channels) || ((m.n_units || per) && (!m.blocks || !m.block_stride)) ||
      (!per && m.n_units > m.block_stride) || (per && (!m.s_total_frames || !m.s_total_units)))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(meter_adv_fb_kernel, dim3(n_streams, (m.k_open + 7) / 8), dim3(64), 0, stream, m, channels);
  return hipGetLastError();
}

}  // namespace peaq

// peaq_backend_fb.inc -- body of the filter-bank back end, included by fb_backend_kernel<DBG> (PTS = TRC = BND = FSUM =
// false), fb_backend_points_kernel (PTS = true), fb_backend_trace_kernel (TRC = true), fb_backend_bands_kernel (BND =
// true) and fb_band_summary_kernel (FSUM = true) in peaq_backend.hip, and by fb_backend_live_kernel (TRC = LIVE = true;
// LIVE is false in all the others): one text, six kernels of their own names.
  __shared__ FbBackendShared sh;
  __shared__ __attribute__((aligned(16))) double sh_ltab[2 * kLogTabEntries + 2];
  __shared__ double sh_etab[kExpTabEntries];
  constexpr int NB = kFbBands, SLOTS = 1;
  const int lane = threadIdx.x & 63;
  const int chan = threadIdx.x >> 6;
  const int channels = a.channels;
  const unsigned pair = blockIdx.x;
  for (int i = threadIdx.x; i < 2 * kLogTabEntries; i += blockDim.x) sh_ltab[i] = a.common->log_tab[i >> 1][i & 1];
  if (threadIdx.x < kExpTabEntries) sh_etab[threadIdx.x] = a.common->exp_tab[threadIdx.x];
  __syncthreads();
  GlobalTabs bt{a.bands, sh_ltab, sh_etab};
  const BandLane<NB, SLOTS> bl{lane};
  unsigned b_begin, b_end, slot = pair;
  if (a.windows) {                                   // broker launch: this session's own window and state
    const FbPairWindow w = a.windows[pair];
    b_begin = w.block0;
    b_end = w.block0 + w.n_blocks;
    slot = w.slot;
  } else {
    const unsigned n_blocks = a.n_blocks ? a.n_blocks[pair] : a.n_blocks_uniform;
    b_begin = a.block0;
    b_end = a.block0 + a.blocks_per_launch;
    if (b_end > n_blocks) b_end = n_blocks;
  }
  if (b_begin >= b_end) return;
  PairState* __restrict__ ps = a.state + slot;
  ChannelState* __restrict__ cs = &ps->ch[chan];

  const int bb = lane < kBandStride ? lane : 0;
  double la[6][SLOTS], mdr[3][SLOTS], mdt[3][SLOTS];
#pragma unroll
  for (int v = 0; v < 6; ++v) la[v][0] = cs->vec[kLaFiltRef + v][bb];
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    mdr[v][0] = cs->vec[kModPrevRef + v][bb];
    mdt[v][0] = cs->vec[kModPrevTest + v][bb];
  }
  LaneAcc acc;
  {
    const int i = lane < kMaxAcc ? lane : 0;
    acc.load(&sh.acc[chan][0][lane < kAccLdsStride ? lane : kAccLdsStride - 1], cs->acc[i], acc_mode(true, i),
             ps->status[i]);
  }
  if (lane < kPaPad) sh.pa[chan][0][lane] = sh.pa[chan][1][lane] = 0.;
  wave_lds_fence();
  const bool owns = lane == MA_RMSMOD || lane == MA_NLASYM || lane == MA_LINDIST;
  unsigned loud_reached = ps->loudness_reached;
  __shared__ PointWalk<true> sh_pw[2];                  // (points instantiation only)
  PointWalk<true>& pw = sh_pw[wave_uniform(chan)];
  if (PTS) pw.init(pts, pair, b_begin);
  // (trace instantiation only) this block's values as they come up, one row per channel.  Value k of channel c sits at
  // [c][c + k]: BlockTrace::ch[1] starts on an odd double, so the pairs of doubles that share a 16-byte store in the
  // record share one here too.  Lane 0 writes them, lane 0 stores the record at the end of the block.
  __shared__ __attribute__((aligned(16))) double sh_trc[2][8];
  unsigned trc_full = 0;                             // full blocks of the pair: the one after them is the flush block
  if (TRC) {
    const uint32_t nr = trc.n_ref ? trc.n_ref[pair] : trc.n_uniform, nt = trc.n_test ? trc.n_test[pair] : trc.n_uniform;
    trc_full = PointWalk<true>::count(nr < nt ? nr : nt);
  }
  // (summary instantiation only) the running rows of both channels: loaded from the caller's array here, stored back
  // after the launch's last block.  Lane = entry: bands 0 .. 39, the denominator, the zero behind it.  The rows follow
  // the status of the RmsModDiff accumulator (movaccum.c:317-362; the path's three accumulators see the same
  // set_tentative) as a scalar: kInit until the first block above the data boundary, kTentative from a block below it
  // to the next one above.
  __shared__ double sh_fsum[FSUM ? 2 * kFbSumRows * kFbSumRow : 1];
  const bool fsum_own = FSUM && lane < kFbSumRow;
  auto fsum_row = [&](int k) -> double* {
    unsigned off = (unsigned)lane * 8u;
    asm volatile("" : "+v"(off));                    // (made where it is used, not kept across the block loop)
    return reinterpret_cast<double*>(reinterpret_cast<char*>(sh_fsum + (wave_uniform(chan) * kFbSumRows + k) * kFbSumRow) +
                                     off);
  };
  auto fsum_cell = [&](double* base) -> double* {
    unsigned off = (unsigned)lane * 8u;
    asm volatile("" : "+v"(off));
    return reinterpret_cast<double*>(
        reinterpret_cast<char*>(base + ((size_t)pair * channels + wave_uniform(chan)) * (kFbSumRows * kFbSumRow)) + off);
  };
  int fsum_st = kInit;
  if (FSUM) {
    fsum_st = __builtin_amdgcn_readfirstlane(ps->status[MA_RMSMOD]);
    fb_summary_copy(fsum_row(0), fsum_cell(fsum.rows), fsum_own);
  }

  // the block's values are requested one block ahead: the walk is a chain of dependent transcendental
  // arithmetic, a record load per block would add its full memory latency 320 times per launch
  const int lb = lane < NB ? lane : 0;
  struct BlockIn {
    double ur, ut, er, et, f0, f1;
  };
  auto fetch = [&](unsigned blk) {
    const double* __restrict__ rec0 =
        a.records + ((size_t)(pair * a.blocks_per_launch + (blk - b_begin)) * channels) * kFbRecDoubles;
    const double* __restrict__ rec = rec0 + (size_t)chan * kFbRecDoubles;
    BlockIn in;
    in.ur = rec[kFbRecUnsmRef + lb];
    in.ut = rec[kFbRecUnsmTest + lb];
    in.er = rec[kFbRecExcRef + lb];
    in.et = rec[kFbRecExcTest + lb];
    in.f0 = rec0[kFbRecFlags];
    in.f1 = channels == 2 ? rec0[kFbRecDoubles + kFbRecFlags] : 0.;
    return in;
  };
  // (the trace and bands instantiations load each block as they come to it: the twelve registers of the block held
  // ahead are what they need to keep every block's values without scratch)
  constexpr bool ALL = TRC || BND;                   // the block's MOV values for every block, whatever the gates
  BlockIn nxt = ALL ? BlockIn{} : fetch(b_begin);
  // (bands instantiation only) the row of plane slot 0 of (pair, block 0, this wave's channel): uniform, like the plane
  // tests on the kernel argument; a block's rows lie channels * n_planes rows further on
  const unsigned bnd_planes = BND ? (unsigned)__builtin_popcount(bnd.planes) : 0u;
  const size_t bnd_cell0 = BND ? ((size_t)pair * bnd.block_stride * channels + wave_uniform(chan)) * bnd_planes : 0;
  for (unsigned blk = b_begin; blk < b_end; ++blk) {
    const BlockIn cur = ALL ? fetch(blk) : nxt;
    // (... and re-read the per-band constants from the tables in every block: held across the loop they are the ten
    // registers the other instantiations keep in scratch.  The summary instantiation re-reads them too, but keeps the
    // block held ahead: holding the constants as well it spills 16 registers where the plain kernel spills 10; so, 8)
    if (ALL || FSUM) asm volatile("" : "+s"(bt.p));
    if (!ALL && blk + 1 < b_end) nxt = fetch(blk + 1);
    const size_t bnd_row = BND ? bnd_cell0 + (size_t)blk * channels * bnd_planes : 0;
    // boundary detector on the 192-sample block, any reference channel (gstpeaq.c:971-979)
    const bool above = cur.f0 != 0. || cur.f1 != 0.;
    if (owns) acc.set_tentative(!above);
    // (summary instantiation only) the rows take the same turns: the copy a pair that ends tentative gets back
    // (summary_restore_kernel) is taken where the accumulators take theirs -- wave-uniform and rare
    bool fsum_cnt = false;
    if (FSUM) {
      if (__builtin_amdgcn_readfirstlane((int)above)) {
        fsum_st = kNormal;
      } else if (fsum_st == kNormal) {
        fb_summary_copy(fsum_cell(fsum.saved), fsum_row(0), fsum_own);
        fsum_st = kTentative;
      }
      fsum_st = __builtin_amdgcn_readfirstlane(fsum_st);
      fsum_cnt = fsum_st != kInit;
    }

    double ur[SLOTS], ut[SLOTS], er[SLOTS], et[SLOTS], lr[SLOTS], lt[SLOTS];
    ur[0] = cur.ur;
    ut[0] = cur.ut;
    er[0] = cur.er;
    et[0] = cur.et;
    if (FSUM && fsum_cnt) {
      fb_summary_add(fsum_row(kFbSumExcRef), fsum_own, fb_summary_pick(lane, er[0], 1.));
      fb_summary_add(fsum_row(kFbSumExcTest), fsum_own, fb_summary_pick(lane, et[0], 1.));
    }
    if (BND) {
      fb_band_store(bnd, kFbBandUnsmRef, bnd_row, lane, ur[0]);
      fb_band_store(bnd, kFbBandUnsmTest, bnd_row, lane, ut[0]);
      fb_band_store(bnd, kFbBandExcRef, bnd_row, lane, er[0]);
      fb_band_store(bnd, kFbBandExcTest, bnd_row, lane, et[0]);
    }
    lr[0] = bt.pow(ur[0], 0.3);                      // modpatt.c:235
    lt[0] = bt.pow(ut[0], 0.3);
    double ad_ref[SLOTS], ad_test[SLOTS], mr[SLOTS], mt[SLOTS];
    level_adapt<NB, SLOTS>(bl, bt, er, et, la, &sh.pa[chan][0][0], ad_ref, ad_test);
    modulation<NB, SLOTS>(bl, bt, lr, mdr, mr);
    modulation<NB, SLOTS>(bl, bt, lt, mdt, mt);
    if (BND) {
      fb_band_store(bnd, kFbBandAdaptRef, bnd_row, lane, ad_ref[0]);
      fb_band_store(bnd, kFbBandAdaptTest, bnd_row, lane, ad_test[0]);
      fb_band_store(bnd, kFbBandModRef, bnd_row, lane, mr[0]);
      fb_band_store(bnd, kFbBandModTest, bnd_row, lane, mt[0]);
    }
    double* __restrict__ dbg =
        DBG ? a.debug + ((size_t)(pair * a.blocks_per_launch + (blk - b_begin)) * channels + chan) * kDbgFbDoubles : nullptr;
    if (loud_reached == UINT_MAX) {                  // workgroup-uniform
      double n_ref, n_test;
      wave_sum2(total_loudness_part<NB, SLOTS>(bl, bt, er), total_loudness_part<NB, SLOTS>(bl, bt, et), n_ref, n_test);
      n_ref *= 24. / NB;
      n_test *= 24. / NB;
      if (lane == 0) sh.gate[chan] = (n_ref > 0.1 && n_test > 0.1);
      if (DBG && lane == 0) {
        dbg[5] = n_ref;
        dbg[6] = n_test;
      }
      __syncthreads();
      const int g = sh.gate[0] | (channels == 2 ? sh.gate[1] : 0);
      __syncthreads();
      if (g) loud_reached = blk;
    }
    double v0 = 0., w0 = 1.;
    bool hit = false;
    if (DBG || ALL || blk >= 125) {                  // gstpeaq.c:988-993
      double d1, d2, wt;
      mod_difference<NB, SLOTS>(bl, bt, 1., mr, mt, mdr[1], d1, d2, wt);
      if (BND) {                                     // the lane's terms of d1 and wt, as mod_difference forms them
        fb_band_store(bnd, kFbBandModDiff, bnd_row, lane, div_fast(fabs(mr[0] - mt[0]), 1. + mr[0]));
        fb_band_store(bnd, kFbBandModWt, bnd_row, lane, div_fast(mdr[1][0], mdr[1][0] + 1. * bt.noise_pow03(bl.band(0))));
      }
      if (FSUM && fsum_cnt && blk >= 125) {          // the lane's term of d1 as mod_difference forms it, weighted as the
        const double t = div_fast(fabs(mr[0] - mt[0]), 1. + mr[0]);   // accumulator weights the block: W and W^2 D
        const double w2 = wt * wt;
        fb_summary_add(fsum_row(kFbSumModDiffW), fsum_own, fb_summary_pick(lane, wt * t, wt));
        fb_summary_add(fsum_row(kFbSumModDiffSq), fsum_own, fb_summary_pick(lane, w2 * (d1 * t), w2));
      }
      d1 *= 100. / sqrt((double)NB);                 // MODE_RMS variant, movs.c:243-244
      if (blk >= 125 && lane == MA_RMSMOD) {
        v0 = d1;
        w0 = wt;
        hit = true;
      }
      if (DBG && lane == 0) {
        dbg[0] = d1;
        dbg[1] = wt;
      }
      if (TRC && lane == 0) {
        sh_trc[chan][chan + 0] = d1;
        sh_trc[chan][chan + 1] = wt;
      }
    }
    if (DBG || ALL || (blk >= 125 && blk - 13 >= loud_reached)) {    // gstpeaq.c:996-1007
      // movs.c:551-577; SWAP_MOD_PATTS_FOR_NOISE_LOUDNESS_MOVS (shipped: 1) exchanges the modulation
      // patterns of the missing-components term ...
      const bool swap = a.cfg.swap_mod_patts != 0;   // workgroup-uniform
      const double nl_p = noise_loudness_part<NB, SLOTS>(bl, bt, 2.5, 0.3, 1., mr, mt, ad_ref, ad_test);
      double lead[SLOTS] = {};                       // (ethres / stest)^0.23: the same stest in both calls below
      const double mc_p = noise_loudness_part<NB, SLOTS, GlobalTabs, LEAD_KEEP>(bl, bt, 1.5, 0.15, 1., swap ? mt : mr,
                                                                                swap ? mr : mt, ad_test, ad_ref, lead);
      // ... and (movs.c:679-706) takes the reference modulation twice; unadapted FB excitation
      const double ld_p = noise_loudness_part<NB, SLOTS, GlobalTabs, LEAD_USE>(bl, bt, 1.5, 0.15, 1., mr, swap ? mr : mt,
                                                                               ad_ref, er, lead);
      if (BND) {
        fb_band_store(bnd, kFbBandNoiseLoud, bnd_row, lane, nl_p);
        fb_band_store(bnd, kFbBandMissing, bnd_row, lane, mc_p);
        fb_band_store(bnd, kFbBandLinDist, bnd_row, lane, ld_p);
      }
      double nl, mc, ld, none;                       // the three sums over the bands in one reduction
      wave_sum4(nl_p, mc_p, ld_p, 0., nl, mc, ld, none);
      nl = noise_loudness_total<NB>(nl, 0.1);
      mc = noise_loudness_total<NB>(mc, 0.);
      ld = noise_loudness_total<NB>(ld, 0.);
      const bool open = blk >= 125 && blk - 13 >= loud_reached;
      if (FSUM && fsum_cnt && open) {                // the band's share of the squares RmsNoiseLoudAsym averages
        fb_summary_add(fsum_row(kFbSumNoiseLoudSq), fsum_own, fb_summary_pick(lane, nl * nl_p, 1.));
        fb_summary_add(fsum_row(kFbSumMissingSq), fsum_own, fb_summary_pick(lane, mc * mc_p, 1.));
        fb_summary_add(fsum_row(kFbSumLinDist), fsum_own, fb_summary_pick(lane, ld_p, 1.));
      }
      if (open && lane == MA_NLASYM) {
        v0 = nl;
        w0 = mc;
        hit = true;
      }
      if (open && lane == MA_LINDIST) {
        v0 = ld;
        w0 = 1.;
        hit = true;
      }
      if (DBG && lane == 0) {
        dbg[2] = nl;
        dbg[3] = mc;
        dbg[4] = ld;
      }
      if (TRC && lane == 0) {
        sh_trc[chan][chan + 2] = nl;
        sh_trc[chan][chan + 3] = mc;
        sh_trc[chan][chan + 4] = ld;
      }
    }
    if (hit) acc.add(v0, w0);
    // ---- trace: lane 0 of each channel's wave stores that channel's five values, channel 0's also the block's own
    // fields (and a mono pair's zero ch[1]), at the pair's absolute block index.  Doubles 0-3 and 6-9 of the record and
    // the flags go out as 16-byte stores; doubles 4 and 5, the two that straddle the channels, as single ones.
    // (LIVE, fb_backend_live_kernel: at the block's index within the launch, block_stride the most blocks of a launch)
    if (TRC && lane == 0) {
      double* __restrict__ od =
          reinterpret_cast<double*>(trc.blocks + (size_t)pair * trc.block_stride + (LIVE ? blk - b_begin : blk));
      double2* __restrict__ o = reinterpret_cast<double2*>(od);
      const double2* __restrict__ s = reinterpret_cast<const double2*>(sh_trc[chan]);
      if (chan == 0) {
        // gstpeaq.c:988 and :996-997 (unsigned compare with the UINT_MAX sentinel)
        const uint32_t fl = (above ? kTraceAbove : 0u) | (blk >= 125 ? kTraceModOpen : 0u) |
                            (blk >= 125 && blk - 13 >= loud_reached ? kTraceLoudOpen : 0u) |
                            (blk >= trc_full ? kTraceFlush : 0u);
        o[0] = s[0];
        o[1] = s[1];
        od[4] = sh_trc[0][4];
        if (channels == 1) {
          od[5] = 0.;
          o[3] = o[4] = make_double2(0., 0.);
        }
        o[5] = make_double2(__hiloint2double((int)blk, (int)fl), 0.);
      } else {
        od[5] = sh_trc[1][1];
        o[3] = s[1];
        o[4] = s[2];
      }
    }
    if (PTS) {                                       // reading points after this block (see backend_kernel)
      while (PointSnap* __restrict__ sp = pw.take(blk + 1)) {
        if (owns) {
#pragma unroll 1
          for (int k = 0; k < kAccFields; ++k) sp->acc[chan][lane][k] = acc.at(k);
          if (chan == 0) sp->status[lane] = acc.status;
        }
        if (chan == 0 && lane == 0) sp->fb_blocks = blk + 1;
      }
    }
  }

  if (FSUM) fb_summary_copy(fsum_cell(fsum.rows), fsum_row(0), fsum_own);
  if (lane < kBandStride) {
#pragma unroll
    for (int v = 0; v < 6; ++v) cs->vec[kLaFiltRef + v][lane] = la[v][0];
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      cs->vec[kModPrevRef + v][lane] = mdr[v][0];
      cs->vec[kModPrevTest + v][lane] = mdt[v][0];
    }
  }
  if (owns) {
    acc.store(cs->acc[lane]);
    if (chan == 0) ps->status[lane] = acc.status;
  }
  if (chan == 0 && lane == 0) {
    ps->fb_counter = b_end;
    ps->loudness_reached = loud_reached;
  }

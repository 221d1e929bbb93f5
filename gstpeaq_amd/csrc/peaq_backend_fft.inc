// peaq_backend_fft.inc -- body of the FFT-model back end, included by backend_kernel<NB, ADV, DBG> (PTS = TRC = BND =
// PBD = SUM = false), backend_points_kernel<NB, ADV> (PTS = true), backend_trace_kernel<NB, ADV> (TRC = true),
// backend_bands_kernel<NB, ADV> (BND = true), backend_pattern_bands_kernel<NB, false> (PBD = true) and
// backend_summary_kernel<NB, ADV> (SUM = true) in peaq_backend.hip, and by backend_live_kernel<NB, ADV> (TRC = LIVE =
// true) and backend_liveband_kernel<NB, ADV> (TRC = LIVE = BND = true; LIVE is false in all the others): one text, eight
// kernels of their own names.
  __shared__ BackendShared sh;
  __shared__ double sh_tab[T_COUNT * kBandStride];
  __shared__ __attribute__((aligned(16))) double sh_ltab[2 * kLogTabEntries + 2];
  constexpr int SLOTS = 2;
  const int lane = threadIdx.x & 63;
  const int chan = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: keep it scalar
  const int channels = a.channels;                  // == blockDim.x / 64
  const unsigned pair = blockIdx.x;
  const BandLane<NB, SLOTS> bl{lane};
  {
    const BandTables* __restrict__ g = a.bands;
    const double* const src[T_COUNT] = {g->adapt_tc, g->ear_tc, g->threshold, g->loud_factor, g->exc_threshold,
                                        g->internal_noise, g->noise_pow03, g->mask_diff, g->inv_spread_norm,
                                        g->inv_spread_norm_pow03, g->ln_internal_noise, g->inv_window_count};
#pragma unroll
    for (int t = 0; t < T_COUNT; ++t)
      for (int i = threadIdx.x; i < kBandStride; i += blockDim.x) sh_tab[t * kBandStride + i] = src[t][i];
    for (int i = threadIdx.x; i < 2 * kLogTabEntries; i += blockDim.x) sh_ltab[i] = a.common->log_tab[i >> 1][i & 1];
  }
  LdsTabs bt{sh_tab, 0, a.bands->deriv_factor, sh_ltab};
  PairState* __restrict__ ps = a.state + (a.pair_slot ? a.pair_slot[pair] : pair);
  ChannelState* __restrict__ cs = &ps->ch[chan];

  unsigned f_begin, f_end;
  if (a.pair_frame0) {                               // broker launch: this pair's own window
    f_begin = a.pair_frame0[pair];
    f_end = f_begin + a.pair_nframes[pair];
  } else {
    const unsigned n_frames = a.n_frames ? a.n_frames[pair] : a.n_frames_uniform;
    f_begin = a.frame0;
    f_end = a.frame0 + a.frames_per_launch;
    if (f_end > n_frames) f_end = n_frames;
  }
  if (f_begin >= f_end) return;
  const bool clk_wave = a.clk && blockIdx.x == 0 && chan == 0;   // wave-uniform
  unsigned long long clk_s0 = 0, clk_w0 = 0;
  if (clk_wave) {
    clk_w0 = wall_clock64();
    clk_s0 = __builtin_readcyclecounter();
  }
  if (lane < kPaPad) sh.pa[chan][0][lane] = sh.pa[chan][1][lane] = 0.;
  __syncthreads();                                   // the table copy is complete

  // (summary instantiation only) the channel's running rows in LDS, this lane's two entries of each: loaded from the
  // caller's array, where they sit between the launches of a run, and stored back at the end (here, before the band
  // state comes into its registers, and there after it has left them).  sum_st follows the
  // accumulators' status (movaccum.c:317-362) as a scalar: kInit until the first frame above the data boundary (nothing
  // is counted before it), kTentative from a frame below it to the next one above.
  constexpr int SUM_R = band_summary_rows(ADV), SUM_ROW = band_row(NB);
  __shared__ __attribute__((aligned(16))) double sh_sum[SUM ? 2 * SUM_R * SUM_ROW : 2];
  const bool sum_own = SUM && 2 * lane < NB;           // (the last of them owns band NB - 1 and the denominators)
  const bool sum_last = SUM && 2 * lane + 1 == NB;
  // (a uniform row address and the lane's 32-bit byte offset, made where it is used: no lane address lives through the
  // frame loop -- band_store's way)
  auto sum_at = [&](double* base) -> double* {
    unsigned off = (unsigned)lane * 16u;
    asm volatile("" : "+v"(off));
    return reinterpret_cast<double*>(reinterpret_cast<char*>(base) + off);
  };
  auto sum_row = [&](int k) -> double* { return sum_at(sh_sum + (SUM ? (chan * SUM_R + k) * SUM_ROW : 0)); };
  auto sum_cell = [&](double* base) -> double* {
    return sum_at(base + ((size_t)pair * channels + chan) * (SUM_R * SUM_ROW));
  };
  int sum_st = kInit;
  if (SUM) {
    sum_st = __builtin_amdgcn_readfirstlane(ps->status[ADV ? (int)MA_SEGNMR : (int)MB_NMR]);
    summary_copy<SUM_R, SUM_ROW>(sum_row(0), sum_cell(sum.rows), sum_own);
  }

  // ---- recurrent state -> registers -----------------------------------------------
  double sm[2][SLOTS];                               // smeared excitation filters (ref, test)
  double la[6][SLOTS];
  double mdr[3][SLOTS], mdt[3][SLOTS];
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int b = bl.band(s);
    sm[0][s] = cs->vec[kSmearRef][b < kBandStride ? b : 0];
    // (the 55-band path never changes the test filter; its bands kernel leaves that state in memory: the band stores
    // take the four registers it would sit in through the frame loop)
    sm[1][s] = (BND || SUM) && ADV ? 0. : cs->vec[kSmearTest][b < kBandStride ? b : 0];
#pragma unroll
    for (int v = 0; v < 6; ++v) la[v][s] = cs->vec[kLaFiltRef + v][b < kBandStride ? b : 0];
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      mdr[v][s] = cs->vec[kModPrevRef + v][b < kBandStride ? b : 0];
      mdt[v][s] = cs->vec[kModPrevTest + v][b < kBandStride ? b : 0];
    }
  }
  // (summary instantiation, basic version) the test side's modulation state -- used once a frame, in modulation<> --
  // lives in LDS between its uses: the twelve registers it would sit in through the frame loop are what the running
  // rows' updates need to keep the plain kernel's waves per SIMD.  The same values go through the same arithmetic.
  constexpr bool MDT_LDS = SUM && !ADV;
  __shared__ __attribute__((aligned(16))) double sh_mdt[MDT_LDS ? 2 * 3 * kLdsBands : 2];
  auto mdt_at = [&](int v) -> double2* {
    return reinterpret_cast<double2*>(sum_at(sh_mdt + (MDT_LDS ? (chan * 3 + v) * kLdsBands : 0)));
  };
  if (MDT_LDS) {
#pragma unroll
    for (int v = 0; v < 3; ++v) *mdt_at(v) = make_double2(mdt[v][0], mdt[v][1]);
    asm volatile("" ::: "memory");
  }
  LaneAcc acc;
  {
    const int i = lane < kMaxAcc ? lane : 0;
    acc.load(&sh.acc[chan][0][lane < kAccLdsStride ? lane : kAccLdsStride - 1], cs->acc[i], acc_mode(ADV, i),
             ps->status[i]);   // lanes beyond the 11 accumulators work on dummy slots
  }
  unsigned loud_reached = ps->loudness_reached;
  __shared__ PointWalk<false> sh_pw[2];                  // (points instantiation only)
  PointWalk<false>& pw = sh_pw[chan];
  if (PTS) pw.init(pts, pair, f_begin);
  // (trace instantiation only) this frame's values as they come up, one row per channel: the six of FrameTrace::ch,
  // then p_detect and steps (channel 0's row) -- lane 0 writes them, lane 0 stores the record at the end of the frame
  __shared__ __attribute__((aligned(16))) double sh_trc[2][8];
  unsigned trc_full = 0;                             // full frames of the pair: the one after them is the flush frame
  if (TRC) {
    const uint32_t nr = trc.n_ref ? trc.n_ref[pair] : trc.n_uniform, nt = trc.n_test ? trc.n_test[pair] : trc.n_uniform;
    trc_full = PointWalk<false>::count(nr < nt ? nr : nt);
    if (ADV && lane == 0) {                          // the 55-band path has two values; the rest of the row stays zero
#pragma unroll
      for (int k = 2; k < 8; ++k) sh_trc[chan][k] = 0.;
    }
  }
  // totalsnr: the two running energies live in channel 0's registers through the frame loop (wave-uniform values);
  // they go to memory where a reading point takes them and where the state is stored behind the loop
  double e_sig = 0., e_noise = 0.;
  if (chan == 0) {
    e_sig = ps->sig_energy;
    e_noise = ps->noise_energy;
  }
  for (unsigned frame = f_begin; frame < f_end; ++frame) {
    asm volatile("" : "+v"(bt.off));                 // the tables are re-read from LDS where they are used
    const double* __restrict__ rec0 =
        a.records + ((size_t)(pair * a.frames_per_launch + (frame - f_begin)) * channels) * kRecDoubles;
    const double* __restrict__ rec = rec0 + (size_t)chan * kRecDoubles;

    // ---- everything the frame reads of its record(s), requested back to back and waited for once: the three band
    // vectors and ONE gather of the scalars -- lanes 0 .. 6 hold channel 0's kRecScalars + lane, lanes 8 .. 14
    // channel 1's (a mono pair has none: the slot behind its record is the next frame's), every other lane 0.  The
    // scalars are handed out by lane reads below: wave-uniform, so they sit in scalar registers.
    const int bb = bl.band(0) < kBandStride ? bl.band(0) : 0;
    const double2 v_root_ref = *reinterpret_cast<const double2*>(rec + kRecRootRef + bb);
    const double2 v_root_test = *reinterpret_cast<const double2*>(rec + kRecRootTest + bb);
    const double2 v_noise = *reinterpret_cast<const double2*>(rec + kRecNoise + bb);
    double sc = 0.;
    if (lane < kRecScalarsUsed || (channels == 2 && lane >= 8 && lane < 8 + kRecScalarsUsed))
      sc = rec0[(lane < 8 ? kRecScalars : kRecDoubles + kRecScalars - 8) + lane];
    // ---- ... and behind them the next frame's record(s) are asked into L2: the front end's launch wrote them long
    // ago, so the first touch of a record comes from HBM, and the frames of a pair follow each other in order.  One
    // dword per 128-byte line, 22 lines a record, by channel 0's wave; the value is never used.  Behind the frame's own
    // loads, because the wait for those counts in issue order.  frame + 1 < f_end: the next frame of THIS launch,
    // whose records lie behind this frame's in every launch kind -- nothing beyond the pair's last record is read.
    // The guard chooses the ADDRESS, not whether to load (every other lane, channel 1's wave and a launch's last frame
    // re-read the first word of this frame's record): behind a branch the compiler could no longer count the touch,
    // and the frame's wait would be for everything outstanding, the touch's trip to HBM included.
    unsigned warm_keep = 0;
    if (WARM) {
      const bool warm = chan == 0 && frame + 1 < f_end && lane < (kRecDoubles * 8 / 128) * channels;
      const char* next = reinterpret_cast<const char*>(rec0 + channels * kRecDoubles) + (unsigned)lane * 128u;
      warm_keep = *reinterpret_cast<const unsigned*>(warm ? next : reinterpret_cast<const char*>(rec0));
    }

    // ---- frame flags over all channels (gstpeaq.c:858-862, movs.c:1374-1381) -----
    const int sc_i = (int)sc;                         // (the flag words' conversion, in their lanes)
    const int fl_ref = __builtin_amdgcn_readlane(sc_i, kRecFlagsRef - kRecScalars) |
                       __builtin_amdgcn_readlane(sc_i, 8 + kRecFlagsRef - kRecScalars);
    const int fl_test = __builtin_amdgcn_readlane(sc_i, kRecFlagsTest - kRecScalars) |
                        __builtin_amdgcn_readlane(sc_i, 8 + kRecFlagsTest - kRecScalars);
    // this channel's bandwidths and EHS, used far below; totalsnr (gstpeaq.c:913-918): channel 0 + channel 1, added
    // to the running sums here, where the gather's register ends
    const double bw_ref = lane_value_d(sc, 8 * chan + kRecBwRef - kRecScalars);
    const double bw_test = lane_value_d(sc, 8 * chan + kRecBwTest - kRecScalars);
    const double ehs = lane_value_d(sc, 8 * chan + kRecEhs - kRecScalars);
    if (chan == 0) {
      e_sig += read_lane<kRecSigE - kRecScalars>(sc) + read_lane<8 + kRecSigE - kRecScalars>(sc);
      e_noise += read_lane<kRecNoiseE - kRecScalars>(sc) + read_lane<8 + kRecNoiseE - kRecScalars>(sc);
    }
    const bool above = fl_ref & 1;
    const bool ehs_valid = ((fl_ref | fl_test) & 2) != 0;
    if (!ADV || lane == MA_SEGNMR || lane == MA_EHS) acc.set_tentative(!above);
    // (summary instantiation only) the rows take the same turns: the copy a pair that ends tentative gets back
    // (summary_restore_kernel) is taken where the accumulators take theirs -- wave-uniform and rare
    bool sum_cnt = false;
    if (SUM) {
      if (__builtin_amdgcn_readfirstlane((int)above)) {
        sum_st = kNormal;
      } else if (sum_st == kNormal) {
        summary_copy<SUM_R, SUM_ROW>(sum_cell(sum.saved), sum_row(0), sum_own);
        sum_st = kTentative;
      }
      sum_st = __builtin_amdgcn_readfirstlane(sum_st);
      sum_cnt = sum_st != kInit;
    }

    // ---- this frame's patterns -------------------------------------------------------
    double ur[SLOTS], ut[SLOTS], lr[SLOTS], lt[SLOTS], nz[SLOTS];
    {
      const double2 v0 = v_root_ref, v1 = v_root_test, v4 = v_noise;
      // unsmeared excitation (fftearmodel.c:593-597) and its 0.3rd power (modpatt.c:235) from the roots
      const double n0 = bt.at(T_ISN, bb), n1 = bt.at(T_ISN, bb + 1);
      const double m0 = bt.at(T_ISN03, bb), m1 = bt.at(T_ISN03, bb + 1);
      excitation_from_root(v0.x, n0, m0, ur[0], lr[0]);
      excitation_from_root(v0.y, n1, m1, ur[1], lr[1]);
      excitation_from_root(v1.x, n0, m0, ut[0], lt[0]);
      excitation_from_root(v1.y, n1, m1, ut[1], lt[1]);
      nz[0] = v4.x; nz[1] = v4.y;
    }
    // (pattern-bands instantiation: the noise pattern is read again where the ratio needs it, below -- the four
    // registers it would sit in through the pattern layer are what the term stores need)
    if (PBD || (SUM && !ADV)) nz[0] = nz[1] = 0.;
    // (pattern-bands instantiation only) the row cell of this (pair, frame, channel); the unsmeared excitations go out
    // here, every other plane where it comes up
    const size_t pbd_cell = PBD ? ((size_t)pair * pbd.frame_stride + frame) * channels + chan : 0;
    if (PBD) {
      band_store<NB>(pbd, kPatBandUnsmRef, pbd_cell, lane, ur[0], bl.valid(1) ? ur[1] : 0.);
      band_store<NB>(pbd, kPatBandUnsmTest, pbd_cell, lane, ut[0], bl.valid(1) ? ut[1] : 0.);
    }
    double nl_part = 0.;                               // basic version: the lane's part of the noise loudness, summed with the NMR's
    bool nl_open = false;
    // time smearing, fftearmodel.c:496-504
    double er[SLOTS], et[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int b = bl.band(s) < kBandStride ? bl.band(s) : 0;
      const double ac = bt.ear_tc(b);
      // (summary instantiation, basic version: the two filters spelt out as the compiler contracts them in the plain
      // instantiation -- the reference's rounds (1 - a) u and fuses a s, the test's rounds a s and fuses (1 - a) u.  Left
      // to itself it fuses a s in both here, and the results would not be peaq_batch_run's to the bit.  The live-band
      // instantiation spells them out as well: a session's scores must not depend on its band meter.)
      constexpr bool SPELT = SUM || (BND && LIVE);
      if (SPELT && !ADV)
        sm[0][s] = __builtin_fma(ac, sm[0][s], (1. - ac) * ur[s]);
      else
        sm[0][s] = ac * sm[0][s] + (1. - ac) * ur[s];
      er[s] = sm[0][s] > ur[s] ? sm[0][s] : ur[s];
      if (!ADV) {
        if (SPELT)
          sm[1][s] = __builtin_fma(1. - ac, ut[s], ac * sm[1][s]);
        else
          sm[1][s] = ac * sm[1][s] + (1. - ac) * ut[s];
        et[s] = sm[1][s] > ut[s] ? sm[1][s] : ut[s];
      } else {
        et[s] = 0.;
      }
    }

    // (bands instantiations only) the row cell of this (pair, frame, channel) -- LIVE: of the frame's index within the
    // launch, as the trace record's --; the smeared excitations go out here
    const size_t bnd_cell =
        BND ? ((size_t)pair * bnd.frame_stride + (LIVE ? frame - f_begin : frame)) * channels + chan : 0;
    if (BND) {
      band_store<NB>(bnd, kBandExcRef, bnd_cell, lane, er[0], bl.valid(1) ? er[1] : 0.);
      if (!ADV) band_store<NB>(bnd, kBandExcTest, bnd_cell, lane, et[0], bl.valid(1) ? et[1] : 0.);
    }
    if (PBD) {
      band_store<NB>(pbd, kPatBandExcRef, pbd_cell, lane, er[0], bl.valid(1) ? er[1] : 0.);
      band_store<NB>(pbd, kPatBandExcTest, pbd_cell, lane, et[0], bl.valid(1) ? et[1] : 0.);
    }
    if (SUM && sum_cnt) {
      summary_add(sum_row(kSumExcRef), sum_own, er[0], sum_last ? 1. : er[1]);
      if (!ADV) summary_add(sum_row(kSumExcTest), sum_own, et[0], sum_last ? 1. : et[1]);
    }

    // lane i owns accumulator i: every MOV value of the frame is routed to its owner as soon as
    // it exists (two selects) instead of being kept in a per-lane table
    double my_v = 0., my_w = 1.;
    bool my_hit = false;
    auto route = [&](int idx, double v, double w) {
      if (lane == idx) {
        my_v = v;
        my_w = w;
        my_hit = true;
      }
    };

    if (!ADV) {
      // ---- pattern processing (gstpeaq.c:834-845) ------------------------------------
      double ad_ref[SLOTS], ad_test[SLOTS], mr[SLOTS], mt[SLOTS];
      level_adapt<NB, SLOTS>(bl, bt, er, et, la, &sh.pa[chan][0][0], ad_ref, ad_test);
      modulation<NB, SLOTS>(bl, bt, lr, mdr, mr);
      if (MDT_LDS) {
        double m[3][SLOTS];
#pragma unroll
        for (int v = 0; v < 3; ++v) {
          const double2 t = *mdt_at(v);
          m[v][0] = t.x;
          m[v][1] = t.y;
        }
        modulation<NB, SLOTS, LdsTabs, true>(bl, bt, lt, m, mt);
#pragma unroll
        for (int v = 0; v < 3; ++v) *mdt_at(v) = make_double2(m[v][0], m[v][1]);
      } else {
        modulation<NB, SLOTS>(bl, bt, lt, mdt, mt);
      }
      if (PBD) {                                     // (the helpers leave 0 in the slot beyond the last band)
        band_store<NB>(pbd, kPatBandAdaptRef, pbd_cell, lane, ad_ref[0], ad_ref[1]);
        band_store<NB>(pbd, kPatBandAdaptTest, pbd_cell, lane, ad_test[0], ad_test[1]);
        band_store<NB>(pbd, kPatBandModRef, pbd_cell, lane, mr[0], mr[1]);
        band_store<NB>(pbd, kPatBandModTest, pbd_cell, lane, mt[0], mt[1]);
        band_store<NB>(pbd, kPatBandAvgLoudRef, pbd_cell, lane, mdr[1][0], bl.valid(1) ? mdr[1][1] : 0.);
      }
      if (DBG) {
        double* __restrict__ d =
            a.debug + ((size_t)(pair * a.frames_per_launch + (frame - f_begin)) * channels + chan) * kDbgDoubles;
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
          if (bl.valid(s)) {
            const int b = bl.band(s);
            d[kDbgExcRef + b] = er[s];
            d[kDbgExcTest + b] = et[s];
            d[kDbgAdaptRef + b] = ad_ref[s];
            d[kDbgAdaptTest + b] = ad_test[s];
            d[kDbgModRef + b] = mr[s];
            d[kDbgModTest + b] = mt[s];
            d[kDbgAvgLoudRef + b] = mdr[1][s];
            d[kDbgAvgLoudTest + b] = mdt[1][s];
          }
        }
      }
      if (loud_reached == UINT_MAX) {                // wave-uniform
        double n_ref, n_test;
        wave_sum2(total_loudness_part<NB, SLOTS>(bl, bt, er), total_loudness_part<NB, SLOTS>(bl, bt, et), n_ref, n_test);
        n_ref *= 24. / NB;
        n_test *= 24. / NB;
        if (lane == 0) sh.gate[chan] = (n_ref > 0.1 && n_test > 0.1);
        if (DBG && lane == 0) {
          double* __restrict__ d =
              a.debug + ((size_t)(pair * a.frames_per_launch + (frame - f_begin)) * channels + chan) * kDbgDoubles;
          d[kDbgLoudnessRef] = n_ref;
          d[kDbgLoudnessTest] = n_test;
        }
      }
      // ---- detection probability, per channel part (movs.c:1239-1262) -----------------
      double bnd_x[SLOTS], bnd_q[SLOTS];             // (bands instantiation only: dead otherwise)
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        double pc = 0., qc = 0.;
        if (bl.valid(s)) {
          const double er_db = (10. * kInvLn10) * bt.log(er[s]);      // 10 log10: excitations are > 0
          const double et_db = (10. * kInvLn10) * bt.log(et[s]);
          const double l = 0.3 * fmax(er_db, et_db) + 0.7 * et_db;
          const double l2 = l * l;
          // (6.39468 / l)^1.71332 = exp(1.71332 (ln 6.39468 - ln l)); one reciprocal of s for both quotients
          const double sd = l > 0. ? 5.95072 * bt.exp(1.71332 * (1.8554663946857675 - bt.log(l))) + 9.01033e-11 * l2 * l2 +
                                         5.05622e-6 * l2 * l - 0.00102438 * l * l + 0.0550197 * l - 0.198719
                                   : 1e30;
          const double inv_sd = div_fast(1., sd);
          const double e = er_db - et_db;
          const double x = e * inv_sd, x2 = x * x;
          const double xb = er_db > et_db ? x2 * x2 : x2 * x2 * x2;   // (e/s)^b, b = 4 or 6
          // The channel's detection probability is pc = 1 - 0.5^xb (movs.c:1253); what the frame needs of it is
          // prod_b (1 - max_c pc) = 0.5^(sum_b max_c xb) (pc grows with xb, so the maxima agree): the EXPONENTS are
          // exchanged and summed, and the one exponential of the frame is taken after the reduction -- an exponential
          // per band, channel and frame less, and the product's own reduction rides in the free slot of the sums'.
          pc = xb;
          qc = fabs(a.cfg.floor_steps ? floor(e) : trunc(e)) * inv_sd;        // movs.c:1256-1260
        }
        sh.pc[chan][bl.band(s)] = pc;
        sh.qc[chan][bl.band(s)] = qc;
        bnd_x[s] = pc;
        bnd_q[s] = qc;
      }
      if (BND) {
        band_store<NB>(bnd, kBandDetect, bnd_cell, lane, bnd_x[0], bnd_x[1]);
        band_store<NB>(bnd, kBandSteps, bnd_cell, lane, bnd_q[0], bnd_q[1]);
      }
      __syncthreads();
      if (loud_reached == UINT_MAX) {
        const int g = sh.gate[0] | (channels == 2 ? sh.gate[1] : 0);
        if (g) loud_reached = frame;
      }
      double* __restrict__ dmov =                    // debug instantiation: this (frame, channel)'s MOV values
          DBG ? a.debug + ((size_t)(pair * a.frames_per_launch + (frame - f_begin)) * channels + chan) * kDbgDoubles + kDbgMov
              : nullptr;
      // ---- modulation difference (gstpeaq.c:871-877) --------------------------------
      if (DBG || TRC || PBD || frame >= 24) {
        double d1, d2, wt;
        if (PBD) {                                   // the terms the three sums add, per slot
          double md_t[3][SLOTS];
          mod_difference<NB, SLOTS, LdsTabs, true>(bl, bt, 100., mr, mt, mdr[1], d1, d2, wt, md_t);
          band_store<NB>(pbd, kPatBandModDiff1, pbd_cell, lane, md_t[0][0], md_t[0][1]);
          band_store<NB>(pbd, kPatBandModDiff2, pbd_cell, lane, md_t[1][0], md_t[1][1]);
          band_store<NB>(pbd, kPatBandModWt, pbd_cell, lane, md_t[2][0], md_t[2][1]);
        } else if (SUM) {                            // (frame >= 24 here) the frame's weight times the terms, per slot
          double md_t[3][SLOTS];
          mod_difference<NB, SLOTS, LdsTabs, true>(bl, bt, 100., mr, mt, mdr[1], d1, d2, wt, md_t);
          if (sum_cnt) {
            summary_add(sum_row(kSumModDiff1), sum_own, wt * md_t[0][0], sum_last ? wt : wt * md_t[0][1]);
            summary_add(sum_row(kSumModDiff2), sum_own, wt * md_t[1][0], sum_last ? wt : wt * md_t[1][1]);
          }
        } else {
          mod_difference<NB, SLOTS>(bl, bt, 100., mr, mt, mdr[1], d1, d2, wt);
        }
        d1 *= 100. / NB;
        d2 *= 100. / NB;
        if (frame >= 24) {
          route(MB_AVGMOD1, d1, wt);
          route(MB_AVGMOD2, d2, wt);
          route(MB_WINMOD, d1, 1.);
        }
        if (DBG && lane == 0) {
          dmov[0] = d1;
          dmov[1] = d2;
          dmov[2] = wt;
        }
        if (TRC && lane == 0) {
          sh_trc[chan][0] = d1;
          sh_trc[chan][1] = d2;
          sh_trc[chan][2] = wt;
        }
      }
      // ---- noise loudness (gstpeaq.c:880-886; unsigned compare with UINT_MAX sentinel)
      // (its sum over the bands goes through the reduction of the noise-to-mask ratio below)
      nl_open = DBG || TRC || PBD || (frame >= 24 && frame - 3 >= loud_reached);
      if (PBD) {                                     // the terms the sum adds, per slot
        double nl_t[SLOTS];
        nl_part = noise_loudness_part<NB, SLOTS, LdsTabs, LEAD_OWN, true>(bl, bt, 1.5, 0.15, 0.5, mr, mt, ad_ref, ad_test,
                                                                          nullptr, nl_t);
        band_store<NB>(pbd, kPatBandNoiseLoud, pbd_cell, lane, nl_t[0], nl_t[1]);
      } else if (SUM && nl_open) {                   // (the gate is open here: nothing is evaluated behind a closed one)
        double nl_t[SLOTS];
        nl_part = noise_loudness_part<NB, SLOTS, LdsTabs, LEAD_OWN, true>(bl, bt, 1.5, 0.15, 0.5, mr, mt, ad_ref, ad_test,
                                                                          nullptr, nl_t);
        if (sum_cnt) summary_add(sum_row(kSumNoiseLoud), sum_own, nl_t[0], sum_last ? 1. : nl_t[1]);
      } else if (nl_open) {
        nl_part = noise_loudness_part<NB, SLOTS>(bl, bt, 1.5, 0.15, 0.5, mr, mt, ad_ref, ad_test);
      }
      // ---- bandwidth (movs.c:797-807) ------------------------------------------------------
      if (bw_ref > 346.) {
        route(MB_BW_REF, bw_ref, 1.);
        route(MB_BW_TEST, bw_test, 1.);
      }
    }
    // ---- noise-to-mask ratio (movs.c:1002-1022), detection probability's binaural part (movs.c:1263-1275): the
    // lanes' parts first, then ONE reduction for the three sums of this place (with the noise loudness's from above) ----
    {
      double nsum = 0., nmax = 0.;
      double bnd_r[SLOTS] = {0., 0.};                  // (bands instantiation only: dead otherwise)
      if (PBD || (SUM && !ADV)) {
        const int b0 = bl.band(0);
        const double2 v4 = *reinterpret_cast<const double2*>(rec + kRecNoise + (b0 < kBandStride ? b0 : 0));
        nz[0] = v4.x; nz[1] = v4.y;
      }
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        if (bl.valid(s)) {
          const double r = div_fast(nz[s] * bt.mask_diff(bl.band(s)), er[s]);   // noise / (excitation / mask)
          nsum += r;
          if (r > nmax) nmax = r;
          bnd_r[s] = r;
        }
      }
      if (BND) band_store<NB>(bnd, kBandNmr, bnd_cell, lane, bnd_r[0], bnd_r[1]);
      if (SUM && sum_cnt) {
        summary_add(sum_row(kSumNmrSum), sum_own, bnd_r[0], sum_last ? 1. : bnd_r[1]);
        summary_max(sum_row(kSumNmrMax), sum_own, sum_last, bnd_r[0], bnd_r[1]);
        summary_add(sum_row(kSumNmrDisturbed), sum_own, bnd_r[0] > 1.41253754462275 ? 1. : 0.,
                    sum_last || bnd_r[1] > 1.41253754462275 ? 1. : 0.);
      }
      double xsum = 0., qsum = 0.;                    // sum of the bands' exponents (pc above), of the steps
      if (!ADV && chan == 0) {
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
          if (bl.valid(s)) {
            const int b = bl.band(s);
            double x = fmax(sh.pc[0][b], 0.), q = sh.qc[0][b];      // (fmax: a NaN exponent counts as 0, like `pc > p`)
            if (channels == 2) {
              if (sh.pc[1][b] > x) x = sh.pc[1][b];
              if (sh.qc[1][b] > q) q = sh.qc[1][b];
            }
            xsum += x;
            qsum += q;
          }
        }
      }
      double nl_sum;
      if (!ADV)
        wave_sum4(nsum, nl_part, qsum, xsum, nsum, nl_sum, qsum, xsum);
      else
        nsum = wave_sum(nsum);
      nsum /= NB;
      // RelDistFrames asks whether ANY band's ratio is above 1.5 dB: a vote, not a maximum (the debug build reports the value)
      const bool disturbed = __any(nmax > 1.41253754462275);
      if (DBG || TRC) nmax = wave_max(nmax);
      if (!ADV && nl_open) {
        const double nl = noise_loudness_total<NB>(nl_sum, 0.);
        if (frame >= 24 && frame - 3 >= loud_reached) route(MB_NOISELOUD, nl, 1.);
        if (DBG && lane == 0)
          a.debug[((size_t)(pair * a.frames_per_launch + (frame - f_begin)) * channels + chan) * kDbgDoubles + kDbgMov + 3] = nl;
        if (TRC && lane == 0) sh_trc[chan][3] = nl;
      }
      if (DBG && lane == 0) {
        double* __restrict__ d =
            a.debug + ((size_t)(pair * a.frames_per_launch + (frame - f_begin)) * channels + chan) * kDbgDoubles + kDbgMov;
        d[4] = nsum;
        d[5] = nmax;
      }
      if (TRC && !ADV && lane == 0) {
        sh_trc[chan][4] = nsum;
        sh_trc[chan][5] = nmax;
      }
      if (!ADV) {
        route(MB_NMR, nsum, 1.);                                    // MODE_AVG_LOG
        route(MB_RELDIST, disturbed ? 1. : 0., 1.);
      } else {
        const double seg = (10. * kInvLn10) * log_pos(nsum);        // 10 log10, MODE_AVG; nsum > 0 (floored bands)
        route(MA_SEGNMR, seg, 1.);
        if (DBG && lane == 0)
          a.debug[((size_t)(pair * a.frames_per_launch + (frame - f_begin)) * channels + chan) * kDbgDoubles + kDbgMov + 3] = seg;
        if (TRC && lane == 0) {
          sh_trc[chan][0] = seg;
          sh_trc[chan][1] = nsum;
        }
      }
      if (!ADV && chan == 0) {
        const double p_bin = 1. - bt.exp(-kLn2 * xsum);             // 1 - prod_b 0.5^xb (movs.c:1263-1270)
        if (DBG && lane == 0) {
          double* __restrict__ d =
              a.debug + ((size_t)(pair * a.frames_per_launch + (frame - f_begin)) * channels) * kDbgDoubles + kDbgMov;
          d[6] = p_bin;
          d[7] = qsum;
        }
        if (TRC && lane == 0) {
          sh_trc[0][6] = p_bin;
          sh_trc[0][7] = qsum;
        }
        if (p_bin > 0.5) route(MB_ADB, qsum, 1.);
        route(MB_MFPD, p_bin, 1.);
      }
    }
    // ---- error harmonic structure (movs.c:1374-1381,1442) ------------------------------
    if (ehs_valid) {
      route(ADV ? MA_EHS : MB_EHS, 1000. * ehs, 1.);
    }
    // ---- accumulate: lane i owns accumulator i --------------------------------------------------
    if (my_hit) acc.add(my_v, my_w);
    // ---- reading points after this frame: every lane stores what it wrote itself (its accumulator's LDS slot,
    // lane 0 of channel 0 the energies), so no barrier -----------------------------------------------------------
    if (PTS) {
      while (PointSnap* __restrict__ sp = pw.take(frame + 1)) {
        if (lane < kMaxAcc && (!ADV || lane == MA_SEGNMR || lane == MA_EHS)) {
#pragma unroll
          for (int k = 0; k < kAccFields; ++k) sp->acc[chan][lane][k] = acc.at(k);
          if (chan == 0) sp->status[lane] = acc.status;
        }
        if (chan == 0 && lane == 0) {
          sp->frames = frame + 1;
          sp->sig_energy = e_sig;
          sp->noise_energy = e_noise;
        }
      }
    }
    // ---- trace: lane 0 of each channel's wave stores that channel's six values, channel 0's also the frame's own
    // fields (and a mono pair's zero ch[1]) -- eight 16-byte stores per record, at the pair's absolute frame index
    // (LIVE, backend_live_kernel: at the frame's index within the launch, frame_stride the most frames of a launch)
    if (TRC && lane == 0) {
      const double2* __restrict__ s = reinterpret_cast<const double2*>(sh_trc[chan]);
      double2* __restrict__ o =
          reinterpret_cast<double2*>(trc.frames + (size_t)pair * trc.frame_stride + (LIVE ? frame - f_begin : frame));
#pragma unroll
      for (int k = 0; k < 3; ++k) o[3 * chan + k] = s[k];
      if (chan == 0) {
        // gstpeaq.c:871 and :880-881 (unsigned compare with the UINT_MAX sentinel); the 55-band path has neither gate
        const uint32_t fl = (above ? kTraceAbove : 0u) | (!ADV && frame >= 24 ? kTraceModOpen : 0u) |
                            (!ADV && frame >= 24 && frame - 3 >= loud_reached ? kTraceLoudOpen : 0u) |
                            (frame >= trc_full ? kTraceFlush : 0u);
        if (channels == 1) {
#pragma unroll
          for (int k = 3; k < 6; ++k) o[k] = make_double2(0., 0.);
        }
        o[6] = s[3];
        o[7] = make_double2(__hiloint2double((int)frame, (int)fl), 0.);
      }
    }
    if (WARM) asm volatile("" ::"v"(warm_keep));       // the touch's register: asked for above, never read
    if (!ADV) __syncthreads();                       // sh.pc/qc/gate are rewritten next frame
  }

  // ---- registers -> recurrent state -------------------------------------------------------
  if (MDT_LDS) {
    asm volatile("" ::: "memory");
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      const double2 t = *mdt_at(v);
      mdt[v][0] = t.x;
      mdt[v][1] = t.y;
    }
  }
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int b = bl.band(s);
    if (b < kBandStride) {
      cs->vec[kSmearRef][b] = sm[0][s];
      if (!((BND || SUM) && ADV)) cs->vec[kSmearTest][b] = sm[1][s];
      if (!ADV) {                                    // advanced: these belong to the filter-bank back end
#pragma unroll
        for (int v = 0; v < 6; ++v) cs->vec[kLaFiltRef + v][b] = la[v][s];
#pragma unroll
        for (int v = 0; v < 3; ++v) {
          cs->vec[kModPrevRef + v][b] = mdr[v][s];
          cs->vec[kModPrevTest + v][b] = mdt[v][s];
        }
      }
    }
  }
  if (lane < kMaxAcc) {
    if (!ADV || lane == MA_SEGNMR || lane == MA_EHS) {
      acc.store(cs->acc[lane]);
      if (chan == 0) ps->status[lane] = acc.status;
    }
  }
  if (chan == 0 && lane == 0) {
    ps->frame_counter = f_end;
    if (!ADV) ps->loudness_reached = loud_reached;
    ps->sig_energy = e_sig;
    ps->noise_energy = e_noise;
  }
  if (clk_wave && lane == 0) {                       // launches of one batch follow each other on one stream: one writer
    a.clk[0] += __builtin_readcyclecounter() - clk_s0;
    a.clk[1] += wall_clock64() - clk_w0;
  }
  // (last: the band state's registers are free by now)
  if (SUM) summary_copy<SUM_R, SUM_ROW>(sum_cell(sum.rows), sum_row(0), sum_own);

// The persistent backward's prologue and step loop, as text: included by gru_bwd_seq_kernel and by the
// backward phase of gru_fb_one_kernel (gru_seq.hip); see gru_seq_fwd_body.h for why text.
// In scope at the include: the arguments `a` (SeqBwdArgs or derived), the LDS arrays part, srow, sgT, red,
// bwL, idsL, constexpr NKW3, NTW, NTP, TAIL.  GK_FB_ONE defined: the flag lines lie `foff` words behind
// a.cnt, the W_hh^T slice comes from `wpre`, the exchange protocol from `loc_f`, and nothing is zeroed.
// Leaves the accumulators accW, accP, dbh, dbi (and row, col, lane, w, ... of the item map).
#ifdef GK_FB_ONE
  unsigned* const cnt0 = a.cnt + (size_t)foff;
#else
  unsigned* const cnt0 = a.cnt;
#endif
  // H = 1024 (NKW3 = 12): scalar wave index and scalar-offset exchange loads (below); the smaller
  // variants measured slower with them (h512 step 0.2257 -> 0.2327 ms, profiles/r2_bwd_soffset_ab.json)
  constexpr bool kScalarX = NKW3 >= 12;
  const int tid = threadIdx.x, lane = tid & 63, w = kScalarX ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;
  const int H = a.H, H3 = 3 * a.H, Bp = a.Bp, T = a.T;
  const int nrb = Bp / 32, ut = seq_unit_tile(nrb);
  const int j0 = ut * 16, rbk = seq_row_block(nrb), b0 = rbk * 32;
  const int lr = lane & 15, lk = 8 * (lane >> 4);
  const int k0 = w * NKW3 * 32;
  const unsigned nunit = (unsigned)(H / 16);

  // this wave's K-slice of W_hh^T rows j0..j0+15 (dh = dGh · W_hh), resident all sequence: in
  // VGPRs, or -- for the variants with fused weight gradients, whose accumulators take the
  // register file -- lane-linear in LDS (each lane re-reads only its own 16-B slots: conflict-free,
  // and program order suffices, no barrier)
  // (also at H = 1024, NKW3 = 12, where the 48-VGPR slice measured 342 -> 327 us per layer in LDS)
  constexpr bool kBwLds = NTW > 0 || NTP > 0 || NKW3 >= 12;
  bf16x8 bw[kBwLds ? 1 : NKW3];
#pragma unroll
  for (int kk = 0; kk < NKW3; ++kk) {
#ifdef GK_FB_ONE
    const bf16x8 v = wpre[kk];   // loaded ahead of the hand-over wait
#else
    const bf16x8 v = ld8(a.WhhT + (size_t)(j0 + lr) * H3 + k0 + kk * 32 + lk);
#endif
    if constexpr (kBwLds) bwL[kk][tid] = v; else bw[kk] = v;
  }

  const int rb = tid >> 8, reg = (tid >> 6) & 3, ln = tid & 63;
  const int row = rb * 16 + (ln >> 4) * 4 + reg, col = ln & 15;
  const int b = b0 + row, j = j0 + col;
  float carry = 0.f;
  float dbh[3] = {0.f, 0.f, 0.f}, dbi = 0.f;   // dbi: only the n gate differs from dbh
  f32x4 accW[3][NTW > 0 ? NTW : 1];
  f32x4 accP[3][NTP > 0 ? NTP : 1];
  zero_acc(accW);
  zero_acc(accP);
  // exchange ring (SeqBwdArgs::xring, gru_seq16.hip): the slot of step t is reused at step t - xr
  const int xr = a.xring >= 2 ? a.xring : T;
  const rsrc_t rX = make_rsrc(a.xbuf, (unsigned)((size_t)T * Bp * H3 * 2));
  const unsigned xlane = (unsigned)(((lk >> 4) * 3 * 512 + lr * 16 + (lk & 15)) * 2);   // exchange lane offset
#ifdef GK_FB_ONE
  const bool loc = loc_f;   // the forward phase's census holds: same workgroup, same row block
#else
  zero_next_flags(a.zero_next, a.zero_words);
  const bool loc = a.allow_local && row_block_local(cnt0 + (size_t)rbk * nunit * kFlagStride, ut, (int)nunit, a.err);
#endif
  // the saves of step t-1 are loaded during step t, right after its hand-off: in front of the
  // next poll they would delay it (vmcnt retires in order), and they have a whole step to land
  float sv[6];
  int svid = 0;
  // the step's 32 row ids for the fused dP one-hot: staged through LDS by the epilogue threads of
  // unit column 0 and read back right before use (8 ids held in registers across the barriers and
  // the publish pushed the register file over the limit)
  auto load_saves = [&](int t) {
    const size_t o = ((size_t)t * Bp + b) * H + j;
    sv[0] = a.dy[o];
    if (TAIL || a.s16) ld_save16_raw(a.s16 + o * 4, sv[1], sv[2]);   // unpacked at use
    else { sv[1] = a.sr[o]; sv[2] = a.sz[o]; sv[3] = a.sn[o]; sv[4] = a.sghn[o]; }
    sv[5] = a.HSf[o];   // HS[t] = h_{t-1}
    if constexpr (NTP > 0) svid = a.ids[(size_t)t * Bp + b];   // this thread's row id (fused dP)
  };
  load_saves(T - 1);

  for (int t = T - 1; t >= 0; --t) {
    const int s = T - 1 - t;
    stamp(a.dbg, s, 0);
    f32x4 acc[2];
    acc[0] = f32x4{0.f, 0.f, 0.f, 0.f};
    acc[1] = acc[0];
    if (s > 0) {
      // wave w's columns [k0, k0 + 32*NKW3) of dGh (3 gates x H) come from unit tiles ((k0+16p) mod H)/16
      bf16x8 af[NKW3][2];
      // dGh_{t+1} column c = k0 + 32kk + lk (gate c/H, unit c%H) lives in producer tile (c%H)/16 of
      // slot t+1 at column (c/H)*16 + c%16
      // 32-column k-steps never straddle a gate (H % 32 == 0): gate c0 / H and producer tile
      // (c0 % H) / 16 are wave-uniform (scalar offset); the lane part is fixed for the launch
      const size_t slot = ((size_t)((t + 1) % xr) * nrb + rbk) * nunit;
      wave_wait_load<NKW3>(cnt0 + (size_t)rbk * nunit * kFlagStride, lane < 2 * NKW3,
                           ((k0 + 16 * lane) % H) / 16, (unsigned)s, a.err, [&](int kk) {
        if constexpr (kScalarX) {
          const int c0 = k0 + kk * 32;
          const int so = (int)((((slot + (size_t)((c0 % H) / 16)) * 3 + (size_t)(c0 / H)) * 512) * 2);
#pragma unroll
          for (int r = 0; r < 2; ++r) af[kk][r] = ld8_sc1s(rX, xlane + (unsigned)(r * 16 * 16 * 2), so);
        } else {
          const int c = k0 + kk * 32 + lk, u = c % H;
          const unsigned tb = (unsigned)(((slot + u / 16) * 3 + c / H) * 512 + lr * 16 + (u & 15)) * 2;
#pragma unroll
          for (int r = 0; r < 2; ++r) af[kk][r] = ld8_sc1(rX, tb + (unsigned)(r * 16 * 16 * 2));
        }
      });
      stamp(a.dbg, s, 1);
#pragma unroll
      for (int kk = 0; kk < NKW3; ++kk) {
        bf16x8 bk;
        if constexpr (kBwLds) bk = bwL[kk][tid]; else bk = bw[kk];
#pragma unroll
        for (int r = 0; r < 2; ++r) acc[r] = mfma16(af[kk][r], bk, acc[r]);
      }
    }
    const int idc = svid;
    float sr = sv[1], sz = sv[2], sn = sv[3], sghn = sv[4];
    const float dy = sv[0], hprev = sv[5];
    if (t > 0) load_saves(t - 1);
    if (TAIL || a.s16) unpack_save16(sr, sz, sr, sz, sn, sghn);
    // operands of the fused weight-gradient MFMAs (independent of other workgroups): issued after
    // the hand-off so the poll above does not wait behind them; first used after the publish
    bf16x8 hB[NTW > 0 ? NTW : 1];
    if constexpr (NTW > 0) {
      if (TAIL || a.HF) {   // whole 1-KB fragment blocks (8 lines each) instead of 16 rows x 64 B
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt)
          hB[nt] = ld8(a.HF + (((size_t)t * nunit + w * NTW + nt) * nrb + rbk) * 512 + lane * 8);
      } else {
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt)
          hB[nt] = ld8(a.HT + (size_t)(w * NTW * 16 + nt * 16 + lr) * a.ldT + (size_t)t * Bp + b0 + lk);
      }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i) part[w][r][i * 64 + lane] = acc[r][i];
    __syncthreads();
    stamp(a.dbg, s, 2);
    float dh = dy + carry;
#pragma unroll
    for (int ww = 0; ww < 8; ++ww) dh += part[ww][rb][reg * 64 + ln];
    const float dn = dh * (1.f - sz);
    const float dz = dh * (hprev - sn);
    const float dan = dn * (1.f - sn * sn);
    const float dar = dan * sghn * sr * (1.f - sr);
    const float daz = dz * sz * (1.f - sz);
    const float dhn = dan * sr;
    carry = sz * dh;
    dbh[0] += dar; dbh[1] += daz; dbh[2] += dhn; dbi += dan;
    const u16 br = f2bf(dar), bz = f2bf(daz), bn = f2bf(dhn), bi = f2bf(dan);
    srow[0][row][col] = br; srow[1][row][col] = bz; srow[2][row][col] = bn;
    sgT[0][col][row] = br; sgT[1][col][row] = bz; sgT[2][col][row] = bn; sgT[3][col][row] = bi;
    if constexpr (NTP > 0) {
      if (col == 0) idsL[row] = idc;
    }
    __syncthreads();
    stamp(a.dbg, s, 3);
    // fused weight-gradient MFMAs (A = this step's dG^T tile from LDS), off the exchange: every wave
    // runs them after the publish / transposed copies.  (Deferred into the next step's exchange-load window they delayed its
    // recurrent MFMAs: 0.2199 -> 0.2291 ms, profiles/r2_rejected_ab.jsonl)
    auto fused_mma = [&]() {
      if constexpr (NTW > 0 || NTP > 0) {
        bf16x8 ga[3];
#pragma unroll
        for (int g = 0; g < 3; ++g) ga[g] = *reinterpret_cast<const bf16x8*>(&sgT[g][lr][lk]);
        if constexpr (NTW > 0) {
#pragma unroll
          for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) accW[g][nt] = mfma16(ga[g], hB[nt], accW[g][nt]);
        }
        if constexpr (NTP > 0) {
          ga[2] = *reinterpret_cast<const bf16x8*>(&sgT[3][lr][lk]);   // dGi: n gate without r
          int idv[8];
          const int4 i0 = *reinterpret_cast<const int4*>(&idsL[lk]), i1 = *reinterpret_cast<const int4*>(&idsL[lk + 4]);
          idv[0] = i0.x; idv[1] = i0.y; idv[2] = i0.z; idv[3] = i0.w;
          idv[4] = i1.x; idv[5] = i1.y; idv[6] = i1.z; idv[7] = i1.w;
#pragma unroll
          for (int nt = 0; nt < NTP; ++nt) {
            const int v = (w * NTP + nt) * 16 + lr;
            bf16x8 oh;
#pragma unroll
            for (int e = 0; e < 8; ++e) oh[e] = (__bf16)(idv[e] == v ? 1.0f : 0.0f);
#pragma unroll
            for (int g = 0; g < 3; ++g) accP[g][nt] = mfma16(ga[g], oh, accP[g][nt]);
          }
        }
      }
    };
    if (w == 0) {
      // publish the dGh_t tile as 3 gate blocks of [32 rows][16 units] (1 KB each, whole lines of its
      // own): a consumer's 16-row fragment of one gate is then 512 contiguous bytes per producer
      // (8 full lines per load instruction instead of 16-row x 96-B strided pieces)
      const size_t tile = (((size_t)(t % xr) * nrb + rbk) * nunit + ut) * (3 * 32 * 16);
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(&srow[g][lane >> 1][(lane & 1) * 8]);
        if (loc) st16_plain(rX, (unsigned)((tile + g * 512 + lane * 8) * 2), v);
        else st16_sc1(rX, (unsigned)((tile + g * 512 + lane * 8) * 2), v);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      unsigned* fl = cnt0 + ((size_t)rbk * nunit + ut) * kFlagStride;
      if (lane == 0) {
        if (loc) signal_flag_local(fl, (unsigned)(s + 1));
        else signal_flag(fl, (unsigned)(s + 1));
      }
      stamp(a.dbg, s, 4);
    } else if (!TAIL && w <= 4 && a.dghT) {
      // transposed copies for the (non-fused) weight-gradient GEMMs: 16 units x 32 rows per gate
      const int g = w - 1;          // 0..3 : dGh r, z, n and dGi n
      const u32x4 v = *reinterpret_cast<const u32x4*>(&sgT[g][lane >> 2][(lane & 3) * 8]);
      const size_t c0 = (size_t)t * Bp + b0 + (lane & 3) * 8;
      const int gg = g < 3 ? g : 2;
      const size_t rowsel = (size_t)(gg * H + j0 + (lane >> 2)) * a.ldG + c0;
      if (g < 3) *reinterpret_cast<u32x4*>(a.dghT + rowsel) = v;
      if (g != 2) *reinterpret_cast<u32x4*>(a.dgiT + rowsel) = v;
    }
    if (!TAIL && a.dgi) {   // row-major dGi for the layer below, after the publish (not in wave 0's drain)
      const size_t og = ((size_t)t * Bp + b) * H3 + j;
      a.dgi[og] = br; a.dgi[og + H] = bz; a.dgi[og + 2 * H] = bi;
    }
    stamp(a.dbg, s, 5);
    fused_mma();
    stamp(a.dbg, s, 6);
  }

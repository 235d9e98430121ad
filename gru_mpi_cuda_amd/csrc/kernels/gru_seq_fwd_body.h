// The persistent forward's prologue and step loop, as text: included by gru_fwd_seq_kernel and by the forward
// phase of gru_fb_one_kernel (gru_seq.hip), so that both run ONE code path and the stand-alone kernels keep
// the ISA they were measured with (as a device function taking the arguments by reference the step loop
// came out 498 -> 556 instructions long; docs/DESIGN.md section 6.11).
// In scope at the include: SeqFwdArgs `a`, the FC arguments `fc`, `unsigned char* smem` (the LDS union),
// constexpr NKW, RS, FC, TAIL.  GK_FB_ONE defined: the flag lines lie `foff` words behind a.cnt (the
// launch's flag set) and nothing is zeroed here.  Leaves `loc` (the row block's exchange protocol).
#ifdef GK_FB_ONE
  unsigned* const cnt0 = a.cnt + (size_t)foff;
#else
  unsigned* const cnt0 = a.cnt;
#endif
  auto& part = *reinterpret_cast<float(*)[8][6][256]>(smem);
  // padded rows (48 B / 80 B, still 16-B aligned for the vector reads): the epilogue's per-item
  // u16 writes -- rows 4 apart within a wave -- land in distinct banks (unpadded: 2-way / 4-way)
  auto& stg = *reinterpret_cast<u16(*)[32][24]>(smem + sizeof(float) * 8 * 6 * 256);
  auto& stgT = *reinterpret_cast<u16(*)[16][40]>(smem + sizeof(float) * 8 * 6 * 256 + sizeof(u16) * 32 * 24);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int H = a.H, Bp = a.Bp, T = a.T;
  const int nrb = Bp / 32;
  const unsigned nunit = (unsigned)(H / 16);
  if constexpr (FC) {
    const int nrec = (int)nunit * nrb;
    if ((int)blockIdx.x >= nrec) {
      zero_next_flags(a.zero_next, a.zero_words);
      if constexpr (NKW * 128 == 512 && RS == 2) fwd_fc_consumer<512>(a, fc, smem, (int)blockIdx.x - nrec);
      return;
    }
  }
  // flag lines per row block: its H/16 producers (+ its FC consumers)
  const size_t rb_lines = nunit + (FC ? kFcCons : 0);
  // (FC: the grid also holds the consumers, so the block -> tile map takes the recurrence's own count)
  const int ut = FC ? seq_unit_tile_n(nrb, (int)nunit * nrb) : seq_unit_tile(nrb);
  const int j0 = ut * 16, rbk = FC ? seq_row_block_n(nrb, (int)nunit * nrb) : seq_row_block(nrb), b0 = rbk * 32;
  const int lr = lane & 15, lk = 8 * (lane >> 4);
  constexpr int NR = RS == 2 ? 1 : 2;           // row tiles per wave
  const int rt = RS == 2 ? (w >> 2) : 0;        // first row tile of this wave
  const int k0 = (RS == 2 ? (w & 3) : w) * NKW * 32;

  bf16x8 bw[NKW][3];   // this wave's K-slice of W_h{r,z,n} for the 16 units, resident all sequence
#pragma unroll
  for (int kk = 0; kk < NKW; ++kk)
#pragma unroll
    for (int g = 0; g < 3; ++g) bw[kk][g] = ld8(a.Whh + (size_t)(g * H + j0 + lr) * H + k0 + kk * 32 + lk);

  // this thread's epilogue item (row, unit) -- one per thread with 512 threads
  const int rb = tid >> 8, reg = (tid >> 6) & 3, ln = tid & 63;
  const int row = rb * 16 + (ln >> 4) * 4 + reg, col = ln & 15;
  const int b = b0 + row, j = j0 + col;
  float bh[3];
#pragma unroll
  for (int g = 0; g < 3; ++g) bh[g] = a.bhh[g * H + j];
  float hp = a.h0 ? a.h0[(size_t)b * H + j] : 0.f;
  const rsrc_t rH = make_rsrc(a.HSb, (unsigned)((size_t)(T + 1) * Bp * H * 2));
  const rsrc_t rX = make_rsrc(a.xch, (unsigned)((size_t)T * Bp * H * 2));
  // exchange ring: the slot of step t is reused at step t + xr.  Safe for xr >= 2: a producer writes
  // step t only after every producer of its row block published step t - 1, i.e. finished reading
  // the tiles of step t - 2 -- the ones the write replaces when xr = 2.
  const int xr = a.xring >= 2 ? a.xring : T;
  const unsigned sv_bytes = (unsigned)((size_t)T * Bp * H * 4);   // < 4 GB: checked on the host
  const rsrc_t rHSf = make_rsrc(a.HSf, sv_bytes + (unsigned)(Bp * H * 4));
  const rsrc_t rSr = make_rsrc(a.sr, a.sr ? sv_bytes : 0u), rSz = make_rsrc(a.sz, a.sz ? sv_bytes : 0u);
  const rsrc_t rSn = make_rsrc(a.sn, a.sn ? sv_bytes : 0u), rSg = make_rsrc(a.sghn, a.sghn ? sv_bytes : 0u);
  const rsrc_t rS16 = make_rsrc(a.s16, a.s16 ? 2u * sv_bytes : 0u);   // < 4 GB: checked on the host
  const unsigned sv_lane = (unsigned)((b * H + j) * 4);
  stamp(a.dbg, T + 1, 0);   // prologue stamps in the (unused) step slot T + 1
#ifndef GK_FB_ONE
  zero_next_flags(a.zero_next, a.zero_words);
#endif
  // (probe 3: consumers leave before the census, which then covers the producers only)
  int cens = (int)rb_lines;
  if constexpr (FC) {
    if ((fc.probe & 7) == 3) cens = (int)nunit;
    if (fc.probe & 8) __builtin_amdgcn_s_setprio(2);
  }
  const bool loc = a.allow_local && row_block_local(cnt0 + (size_t)rbk * rb_lines * kFlagStride, ut, cens, a.err);
  stamp(a.dbg, T + 1, 4);

  // the input projection of step t, gathered one step ahead, after the publish (its latency off
  // the critical path; issued before wave 0's drain it would be part of it: vmcnt retires in order).
  // The char id it needs is loaded one step earlier still, so the gather never waits on an id load.
  int idn = a.ids ? a.ids[b] : 0;   // id of the step whose row load_gi gathers next
  auto load_gi = [&](int t, float (&gi)[3]) {
    if (t >= T) return;
    const float* src = a.ids ? a.P + (size_t)idn * 3 * H : a.Gi + ((size_t)t * Bp + b) * 3 * H;
#pragma unroll
    for (int g = 0; g < 3; ++g) gi[g] = src[g * H + j];
    if (a.ids && t + 1 < T) idn = a.ids[(size_t)(t + 1) * Bp + b];
  };
  float gin[3] = {0.f, 0.f, 0.f};
  load_gi(0, gin);
  for (int t = 0; t < T; ++t) {
    stamp(a.dbg, t, 0);
    const float gi[3] = {gin[0], gin[1], gin[2]};
    f32x4 acc[NR][3];
    zero_acc(acc);
    if (t > 0 || a.h0) {
      // wave w's K-slice [k0, k0 + 32*NKW) is produced by unit tiles k0/16 .. k0/16 + 2*NKW - 1
      bf16x8 af[NKW][NR];
      if (t > 0) {
        // h_t from the producers' exchange tiles (written at step t-1); unit u = k0 + 32kk + lk
        // lives in tile u/16 at column u%16
        const size_t slot = ((size_t)((t - 1) % xr) * nrb + rbk) * nunit;
        wave_wait_load<NKW>(cnt0 + (size_t)rbk * rb_lines * kFlagStride, lane < 2 * NKW, k0 / 16 + lane,
                            (unsigned)t, a.err, [&](int kk) {
          const int u = k0 + kk * 32 + lk;
          const unsigned tb = (unsigned)(((slot + u / 16) * 32 + lr) * 16 + (u & 15)) * 2;
#pragma unroll
          for (int r = 0; r < NR; ++r) af[kk][r] = ld8_sc1(rX, tb + (unsigned)((rt + r) * 16 * 16 * 2));
        });
      } else {   // h_init, row-major HS[0] (written before the launch)
        const unsigned base = (unsigned)((((size_t)b0 + rt * 16 + lr) * H + k0 + lk) * 2);
#pragma unroll
        for (int kk = 0; kk < NKW; ++kk)
#pragma unroll
          for (int r = 0; r < NR; ++r) af[kk][r] = ld8_sc1(rH, base + (unsigned)(r * 16 * H * 2 + kk * 64));
      }
      stamp(a.dbg, t, 1);
#pragma unroll
      for (int kk = 0; kk < NKW; ++kk)
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
          for (int g = 0; g < 3; ++g) acc[r][g] = mfma16(af[kk][r], bw[kk][g], acc[r][g]);
    }
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
      for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i) part[w][r * 3 + g][i * 64 + lane] = acc[r][g][i];
    // FC consumers read wave 2's HF block of step t - 1 once wave 0 signals t + 1: drain it before
    // the barrier wave 0 passes first (its exchange loads retired, so this waits on nothing else)
    if constexpr (FC) {
      if (w == 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    stamp(a.dbg, t, 2);
    float gh[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      float s = 0.f;
      if constexpr (RS == 2) {
#pragma unroll
        for (int ww = 0; ww < 4; ++ww) s += part[rb * 4 + ww][g][reg * 64 + ln];
      } else {
#pragma unroll
        for (int ww = 0; ww < 8; ++ww) s += part[ww][rb * 3 + g][reg * 64 + ln];
      }
      gh[g] = s + bh[g];
    }
    const float r = sigmoidf_(gi[0] + gh[0]);
    const float z = sigmoidf_(gi[1] + gh[1]);
    const float n = tanhf_(gi[2] + r * gh[2]);
    const float h = n + z * (hp - n);
    hp = h;
    const u16 hb = f2bf(h);
    stg[row][col] = hb;
    stgT[col][row] = hb;
    __syncthreads();
    stamp(a.dbg, t, 3);
    if (w == 0) {
      // publish: the 32x16 bf16 tile (1 KB, whole lines of its own), 16 B per lane, write-through;
      // drain; one signal.  Then the row-major copy for the GEMMs that read HS later.
      const u32x4 v = *reinterpret_cast<const u32x4*>(&stg[lane >> 1][(lane & 1) * 8]);
      const unsigned xo = (unsigned)((((size_t)(t % xr) * nrb + rbk) * nunit + ut) * 512 + lane * 8) * 2;
      unsigned* fl = cnt0 + ((size_t)rbk * rb_lines + ut) * kFlagStride;
      if (loc) {
        st16_plain(rX, xo, v);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) signal_flag_local(fl, (unsigned)(t + 1));
      } else {
        st16_sc1(rX, xo, v);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) signal_flag(fl, (unsigned)(t + 1));
      }
      stamp(a.dbg, t, 4);
      const size_t hs = ((size_t)(t + 1) * Bp + b0 + (lane >> 1)) * H + j0 + (lane & 1) * 8;
      if (FC && !loc) st16_sc1(rH, (unsigned)(hs * 2), v);   // write-through: FC consumers on other XCDs
      else if (TAIL && !loc) {
        // write-through for tail blocks on other XCDs: four agent-scope dword stores (sc1) at the plain
        // store's address.  (As one sc1 buffer store through rH the branch cost the step loop ~80
        // v_readlane / v_writelane per step -- scalars parked in VGPR lanes -- against the plain kernel's 17.)
        unsigned* hp = reinterpret_cast<unsigned*>(a.HSb + hs);
#pragma unroll
        for (int i = 0; i < 4; ++i) __hip_atomic_store(hp + i, v[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else *reinterpret_cast<u32x4*>(a.HSb + hs) = v;
      stamp(a.dbg, t, 5);
    } else if (w == 1 && a.HT) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(&stgT[lane >> 2][(lane & 3) * 8]);
      *reinterpret_cast<u32x4*>(a.HT + (size_t)(j0 + (lane >> 2)) * a.ldT + (size_t)(t + 1) * Bp + b0 + (lane & 3) * 8) = v;
    } else if (w == 2 && a.HF) {   // the backward's dW_hh operand: one whole 1-KB block
      const u32x4 v = *reinterpret_cast<const u32x4*>(&stgT[lane & 15][8 * (lane >> 4)]);
      const size_t hf = (((size_t)(t + 1) * nunit + ut) * nrb + rbk) * 512 + lane * 8;
      if (FC && !loc) st16_sc1(make_rsrc(a.HF, (unsigned)((size_t)(T + 1) * Bp * H * 2)), (unsigned)(hf * 2), v);
      else *reinterpret_cast<u32x4*>(a.HF + hf) = v;
    }
    // the next gather, then the saves for the backward pass, AFTER the publish (not part of wave
    // 0's drain).  Saves as buffer stores: one per-lane offset for the launch, the step in the
    // scalar offset -- with 64-bit VGPR address math the compiler reused the in-flight gather's
    // destination as a temporary and waited for it (+0.3 us per step at H = 512).
    load_gi(t + 1, gin);
    const int sstep = __builtin_amdgcn_readfirstlane(t * Bp * H * 4);   // uniform: no waterfall loop
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(h), rHSf, sv_lane, sstep + Bp * H * 4, 0);
    // (TAIL: built for the packed saves only -- without the four fp32 save descriptors the step loop
    // keeps every scalar in SGPRs: no v_readlane / v_writelane at all, 381 instructions per step against
    // the plain kernel's 414 with 17 of them)
    if (TAIL || a.s16) {   // packed bf16 (r, z, n, gh_n): one 8-B store at twice the fp32 offsets
      typedef unsigned u32x2_ __attribute__((ext_vector_type(2)));
      const u32x2_ pv = {(unsigned)f2bf(r) | ((unsigned)f2bf(z) << 16), (unsigned)f2bf(n) | ((unsigned)f2bf(gh[2]) << 16)};
      __builtin_amdgcn_raw_buffer_store_b64(pv, rS16, sv_lane * 2u, sstep * 2, 0);
    } else if (a.sr) {
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(r), rSr, sv_lane, sstep, 0);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(z), rSz, sv_lane, sstep, 0);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(n), rSn, sv_lane, sstep, 0);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(gh[2]), rSg, sv_lane, sstep, 0);
    }
    stamp(a.dbg, t, 6);
  }
  if constexpr (FC) {   // h of the last step complete in HSb / HF -> epoch T + 1 for the consumers
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      unsigned* fl = cnt0 + ((size_t)rbk * rb_lines + ut) * kFlagStride;
      if (loc) signal_flag_local(fl, (unsigned)(T + 1));
      else signal_flag(fl, (unsigned)(T + 1));
    }
  }

// Teacher-forced scoring of small batches as ONE persistent launch (docs/DESIGN.md §4a, "Inside a persistent
// launch"; the rule: cpu_ref.score; the recorded graph it replaces: Generator::record_score).
//
// The grid, the residency and the weight layout are gen_persist_kernel's (gen_persist_kernel.h): 256
// workgroups x 512 threads, workgroup b owns U = H / 256 units of every recurrent matrix and VR = V / 256
// FC rows, the fp32 MFMA A-fragments stay in VGPRs for the launch, the 8 wave partials meet in LDS and
// are summed in wave order.  The schedule is not that kernel's.  Under teacher forcing nothing feeds back
// from the logits: layer l at step t needs h_l(t-1) and h_{l-1}(t) only, so the layers run as a WAVEFRONT
// inside the launch --
//   * phase p = 0 .. T + L - 1 (T = the longest row's token count): layer l runs step p - l, the FC rows
//     step p - L.  Everything a phase multiplies was published in phase p - 1: state h_s(p - 1 - s) of layer
//     s is loaded once and feeds W_hh_s (layer s, next step) and W_ih_(s+1) (layer s + 1, same step), or the
//     FC rows for the top layer.  The 2L products of a phase issue back to back into their own LDS partial
//     slots red[product][name tile]; one barrier later every (layer, name, unit) gate is ONE thread that
//     sums its six rows' wave partials itself (in wave order), computes the gate, keeps the carry in LDS
//     and stores its unit write-through; the FC rows' threads sum and store their logits beside them.  A
//     second barrier, then ONE flag per workgroup carrying the phase number: one hand-off per phase, where
//     generation pays L + 1 per char.  The logits have a flag kind of their own that no product waits for.
//   * red holds TP name tiles per product (TP = 4, 2, 1, 1 for L = 1 .. 4: 64, 64, 48, 64 KiB); more names
//     than 16 TP take several passes of a phase, each with its own barrier pair, before the one flag.
//   * The prologue reads the caller's rows [n][ML + 1] in every workgroup and derives n_tok, the input ids
//     and the targets by score_prep's rule into LDS; layer 0's gi is a gather from the resident table slice.
//   * One name: the products run on the VALU (gen_persist_kernel's one-name form).
//   * The tail: workgroup n < N scores name n, its 8 waves taking steps w, w + 8, ...: wait for the 256
//     logits flags of the step, then score_logprob_f32's arithmetic on the row (fixed-order DPP helpers,
//     readlane for the target, ballot popcounts for the rank).  One lane sums the name in step order and
//     workgroup n alone writes name n's outputs: no atomics, two launches are bitwise equal.
// Every hand-off uses flags (the workspace needs no fill).  Spins are bounded (error bit 32, then every
// wait returns at once and the grid drains; no address is formed from anything read out of the exchange);
// the last workgroup out zeroes the flags.  Out of scope: controls, constraints, soft terms, bf16.
#include "gen_persist_kernel.h"

namespace gk {

namespace {
constexpr int kSML = 64;   // steps per row
constexpr int kSRL = 68;   // bytes of a row in LDS (max_len + 1 <= 65)
}

// PER = V / 64 logits per lane in the tail
template <int KJ, int L, int PER>
__global__ void __launch_bounds__(512, 1) gen_persist_score_kernel(GenPersistScoreArgs a) {
  constexpr int U = KJ / 8, H = 32 * KJ, KW = H / 8, NT = 2 * L - 1, R3 = 3 * U;
  constexpr int V = 64 * PER, VR = V / kG;
  constexpr int NP = 2 * L, SFC = NP - 1;             // products of a phase; the FC rows' slot
  constexpr int TP = L == 1 ? 4 : L == 2 ? 2 : 1;     // name tiles per pass
  constexpr int GI = TP * 16 * U;                     // gate threads per layer and pass
  static_assert(L * GI + TP * 16 * VR <= 512, "a pass's gates and logits are one thread each");
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, q4 = lane >> 4;
  const int N = a.N, Np = (N + 15) & ~15, nnt = Np / 16, ML = a.ML;

  __shared__ float sP[V * R3];                   // P[v][g H + b U + u] -> sP[v][g U + u]
  __shared__ float red[NP][TP][8][256];          // wave partials: slot s < L: W_hh_s, L + s: W_ih_(s+1), SFC: the FC rows
  __shared__ float sh[L][kNmax][U];              // own units' hidden states (the carry)
  __shared__ float sbh[L][16], sbi[L][16], sbf[16];
  __shared__ __attribute__((aligned(16))) float sWf[VR][H];   // this workgroup's FC rows
  __shared__ unsigned short sid[kSML][kNmax];    // step t's input id of name n (masked steps, pad names: SOS)
  __shared__ unsigned char srow[kNmax][kSRL];    // the caller's rows; after the parse the clamped targets
  __shared__ int sntok[kNmax];
  __shared__ float stok[kSML];                   // the tail: this workgroup's name
  __shared__ int srank[kSML];
  __shared__ int s_last, s_T;

  // one slot per step: X_l[t][name][H], then LG[t][name][V]
  const size_t ws_floats = ((size_t)L * kNmax * H + (size_t)kNmax * V) * ML;
  const prsrc_t xr = prsrc(a.ws, (unsigned)(ws_floats * 4));
  const unsigned lg0 = (unsigned)((size_t)L * ML * kNmax * H * 4);
  auto xoff = [&](int l, int t, int n, int col) -> unsigned {
    return (unsigned)((((size_t)(l * ML + t) * kNmax + n) * H + col) * 4);
  };
  auto lgoff = [&](int t, int n, int v) -> unsigned { return lg0 + (unsigned)(((size_t)t * kNmax + n) * V + v) * 4; };
  unsigned* flags = a.sync;   // kind 0: phases (value p + 1), kind 1: logits (value t + 1)
  unsigned* done = a.sync + (size_t)2 * kG * kFS;

  // ---- resident weights: tile ti < L: W_hh_ti; L <= ti < 2L-1: W_ih_(ti-L+1); the FC rows in LDS
  float Wr[NT][KJ];
#pragma unroll
  for (int ti = 0; ti < NT; ++ti) {
    const float* M = ti < L ? a.Whh[ti] : a.Wih[ti - L + 1];
    const bool valid = fr < R3;
    const int row = (fr / U) * H + b * U + fr % U;
    const float* src = M + (size_t)(valid ? row : 0) * H + w * KW + q4 * KJ;
#pragma unroll
    for (int j = 0; j < KJ; j += 4) {
      float4 v = valid ? *reinterpret_cast<const float4*>(src + j) : make_float4(0.f, 0.f, 0.f, 0.f);
      Wr[ti][j] = v.x; Wr[ti][j + 1] = v.y; Wr[ti][j + 2] = v.z; Wr[ti][j + 3] = v.w;
    }
  }
  for (int i = tid; i < VR * H; i += 512) sWf[i / H][i % H] = a.Wfc[(size_t)(b * VR + i / H) * H + i % H];
  for (int i = tid; i < V * R3; i += 512) {
    const int v = i / R3, c = i % R3;
    sP[i] = a.P[(size_t)v * 3 * H + (c / U) * H + b * U + c % U];
  }
  if (tid < 16) {
#pragma unroll
    for (int l = 0; l < L; ++l) {
      sbh[l][tid] = tid < R3 ? a.bhh[l][(tid / U) * H + b * U + tid % U] : 0.f;
      sbi[l][tid] = (l > 0 && tid < R3) ? a.bih[l][(tid / U) * H + b * U + tid % U] : 0.f;
    }
    sbf[tid] = tid < VR ? a.bfc[b * VR + tid] : 0.f;
  }
  // ---- the rows: n_tok, input ids and targets by score_prep's rule, in every workgroup
  for (int i = tid; i < N * (ML + 1); i += 512) srow[i / (ML + 1)][i % (ML + 1)] = a.rows[i];
  for (int i = tid; i < kSML * kNmax; i += 512) (&sid[0][0])[i] = (unsigned short)a.sos;
  __syncthreads();
  if (tid < kNmax) {   // (wave 0)
    int nt = 0;
    if (tid < N) {
      nt = ML;
      for (int l = 0; l < ML; ++l)
        if (srow[tid][l] == a.eos) { nt = l + 1; break; }
      bool bad = false;
      int prev = a.sos;
      for (int l = 0; l < nt; ++l) {
        int c = srow[tid][l];
        if (c >= V) { bad = true; c = 0; srow[tid][l] = 0; }   // caller error: clamp, flag (score_prep's bit)
        sid[l][tid] = (unsigned short)prev;
        prev = c;
      }
      if (bad && b == tid) __hip_atomic_fetch_or(a.err, 16u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    sntok[tid] = nt;
    int m = nt;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
    if (tid == 0) s_T = m;
  }
  __syncthreads();
  const int T = s_T;   // 1 <= T <= ML: later phases are skipped, not computed

  const bool one = N == 1;
  const int kw0 = w * KW + q4 * KJ;
  auto stash = [&](int slot, int tl, const f32x4& acc) {
#pragma unroll
    for (int r = 0; r < 4; ++r) red[slot][tl][w][(4 * q4 + r) * 16 + fr] = acc[r];
  };
  // the 8 wave partials of element e, in wave order (reduce_el's sum)
  auto wsum = [&](int slot, int tl, int e) -> float {
    float s = red[slot][tl][0][e];
#pragma unroll
    for (int k = 1; k < 8; ++k) s += red[slot][tl][k][e];
    return s;
  };

  for (int p = 0; p < T + L; ++p) {
    // every state of phase p - 1, from the 32 producers of this wave's K-slice
    if (p > 0) pwait(flags, 0, w * 32, 32, (unsigned)p, a.err);
    for (int nt0 = 0; nt0 < nnt; nt0 += TP) {
      // ---- the products of this pass, back to back: x = h_s(p - 1 - s) times W_hh_s and W_ih_(s+1) / the FC rows
      if (p > 0) {
        static_for<0, L>([&](auto st) {
          constexpr int s = decltype(st)::value;
          const int ts = p - 1 - s;
          if (ts < 0 || ts >= T) return;
#pragma unroll
          for (int tl = 0; tl < TP; ++tl) {
            if (nt0 + tl < nnt) {
              const int n = one ? 0 : (nt0 + tl) * 16 + fr;   // one name: every lane takes name 0's x
              float x[KJ];
              load_x<KJ>(xr, xoff(s, ts, n, kw0), one || n < N, x);
              if constexpr (s == L - 1) {
                // the VR <= 2 FC rows on the VALU, from the LDS copy; the quarters and waves are summed by the logits' thread
                auto dot = [&](const float* wr) -> float {
                  float pr = 0.f;
#pragma unroll
                  for (int j = 0; j < KJ; j += 4) {
                    const float4 u = *reinterpret_cast<const float4*>(wr + j);
                    pr = fmaf(u.x, x[j], pr); pr = fmaf(u.y, x[j + 1], pr);
                    pr = fmaf(u.z, x[j + 2], pr); pr = fmaf(u.w, x[j + 3], pr);
                  }
                  return pr;
                };
#pragma unroll
                for (int r = 0; r < VR; ++r) red[SFC][tl][w][(4 * q4 + r) * 16 + fr] = dot(&sWf[r][kw0]);
              }
              if (one) {
                // KJ VALU FMAs per lane (row fr, quarter q4 of the K-slice), summed over the quarters, into column 0
                auto vdot = [&](auto ti_tag) -> float {
                  constexpr int TI = decltype(ti_tag)::value;
                  float pr = 0.f;
#pragma unroll
                  for (int j = 0; j < KJ; ++j) pr = fmaf(Wr[TI][j], x[j], pr);
                  pr += __shfl_xor(pr, 16, 64);
                  pr += __shfl_xor(pr, 32, 64);
                  return pr;
                };
                const float p0 = vdot(ic<s>{});
                if (q4 == 0) red[s][0][w][fr * 16] = p0;
                if constexpr (s < L - 1) {
                  const float p1 = vdot(ic<L + s>{});
                  if (q4 == 0) red[L + s][0][w][fr * 16] = p1;
                }
              } else {
                auto whh = [&](int j) { return Wr[s][j]; };
                f32x4 o0, o1;
                if constexpr (s < L - 1) {
                  auto wih = [&](int j) { return Wr[L + s][j]; };
                  tile_mm2<KJ, true>(whh, wih, x, o0, o1, false, xr, 0u, false);
                  stash(L + s, tl, o1);
                } else {
                  tile_mm2<KJ, false>(whh, whh, x, o0, o1, false, xr, 0u, false);
                }
                stash(s, tl, o0);
              }
            }
          }
        });
      }
      lds_barrier();
      // ---- the gates: thread (l, name of the pass, unit) sums its rows' partials, gates, keeps and stores its unit
      {
        const int l = tid / GI, rr = tid % GI, nl = rr / U, u = rr % U;
        const int n = nt0 * 16 + nl, t = p - l;
        if (l < L && n < N && t >= 0 && t < T) {
          const int tl = nl >> 4, col = nl & 15;
          float gi[3], gh[3];
#pragma unroll
          for (int g = 0; g < 3; ++g) {
            const int row = g * U + u, e = row * 16 + col;
            gh[g] = t > 0 ? wsum(l, tl, e) + sbh[l][row] : sbh[l][row];   // h(-1) = 0: the bias
            gi[g] = l == 0 ? sP[(int)sid[t][n] * R3 + row] : wsum(L + l - 1, tl, e) + sbi[l][row];
          }
          const float r = sig_ieee(gi[0] + gh[0]);
          const float z = sig_ieee(gi[1] + gh[1]);
          const float nn = tanhf(gi[2] + r * gh[2]);
          const float hv = (1.f - z) * nn + z * (t > 0 ? sh[l][n][u] : 0.f);
          sh[l][n][u] = hv;
          st_sc1(xr, xoff(l, t, n, b * U + u), hv);
        }
        // ---- the logits of step p - L: the threads from the top, one per (FC row, name of the pass)
        const int j = 511 - tid, r = j / (TP * 16), ml = j % (TP * 16);
        const int m = nt0 * 16 + ml, tf = p - L;
        if (r < VR && m < N && tf >= 0) {
          const int tl = ml >> 4, col = ml & 15;
          float s = 0.f;
#pragma unroll
          for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q) s += red[SFC][tl][k][(4 * q + r) * 16 + col];
          st_sc1(xr, lgoff(tf, m, b * VR + r), s + sbf[r]);
        }
      }
      // every store of the pass has left before the barrier, the flag comes after it
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    if (tid == 0) {
      if (p < T + L - 1)
        __hip_atomic_store(flags + (size_t)b * kFS, (unsigned)(p + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (p >= L)
        __hip_atomic_store(flags + (size_t)(kG + b) * kFS, (unsigned)(p - L + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }

  // ---- the tail: workgroup n scores name n, a wave per step (score_logprob_f32's arithmetic), one writer
  if (b < N) {
    const int nt = sntok[b];
    for (int t = w; t < nt; t += 8) {
      pwait(flags, 1, 0, kG, (unsigned)(t + 1), a.err);
      const int sl = lane_now();
      const int tg = __builtin_amdgcn_readfirstlane((int)srow[b][t]);   // < V: clamped by the parse
      float xv[PER];
#pragma unroll
      for (int e = 0; e < PER; e += 4) {
        const pu32x4 v = __builtin_amdgcn_raw_buffer_load_b128(xr, lgoff(t, b, sl * PER + e), 0, 0);
        xv[e] = __uint_as_float(v.x); xv[e + 1] = __uint_as_float(v.y);
        xv[e + 2] = __uint_as_float(v.z); xv[e + 3] = __uint_as_float(v.w);
      }
      float mx = -INFINITY;
#pragma unroll
      for (int e = 0; e < PER; ++e) mx = fmaxf(mx, xv[e]);
      mx = wave_max_dpp(mx);
      float se = 0.f;
#pragma unroll
      for (int e = 0; e < PER; ++e) se += expf(xv[e] - mx);
      se = wave_sum_dpp(se);
      const int tl = tg / PER, te = tg - tl * PER;
      float cand = 0.f;
#pragma unroll
      for (int e = 0; e < PER; ++e) cand = e == te ? xv[e] : cand;
      const float xt = rdl(cand, tl);
      int rank = 0;
#pragma unroll
      for (int e = 0; e < PER; ++e) {
        const int j = sl * PER + e;
        const bool above = xv[e] > xt || (xv[e] == xt && j < tg);
        rank += __builtin_popcountll(__ballot(above));
      }
      if (lane == 0) {
        stok[t] = (xt - mx) - logf(se);
        srank[t] = rank;
      }
    }
    __syncthreads();
    if (tid < ML) {   // masked positions: 0 and -1
      a.tok_logp[(size_t)b * ML + tid] = tid < nt ? stok[tid] : 0.f;
      a.rank[(size_t)b * ML + tid] = tid < nt ? srank[tid] : -1;
    }
    if (tid == 0) {
      float sum = 0.f;
      for (int t = 0; t < nt; ++t) sum += stok[t];   // step order
      a.name_logp[b] = sum;
      a.n_tok[b] = nt;
    }
  }
  // ---- the last workgroup out zeroes the flags for the next launch (nobody polls them any more)
  __syncthreads();
  if (tid == 0) s_last = __hip_atomic_fetch_add(done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == kG - 1;
  __syncthreads();
  if (s_last) {
    for (int i = tid; i < 2 * kG * kFS; i += 512) flags[i] = 0u;
    if (tid == 0) *done = 0u;
  }
}

// (KJ = H / 32, L): gen_persist.hip's GP_VARIANTS, per vocabulary.  Every instance has ScratchSize 0 in the
// -Rpass-analysis=kernel-resource-usage table (docs/DESIGN.md §4a holds it)
#define GPS_VARIANTS(X) X(8, 1) X(8, 2) X(8, 3) X(8, 4) X(16, 1) X(16, 2) X(16, 3) X(16, 4) X(32, 1) X(32, 2)

// resident workgroups of the variant on the whole device (0: no such variant, or a query failed)
static int gps_resident(int KJ, int L, int PER) {
  int dev = 0, cus = 0, nb = 0;
  bool found = false;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
#define XP(K, LL, P)                                                                                                \
  if (KJ == K && L == LL) {                                                                                         \
    found = true;                                                                                                   \
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, gen_persist_score_kernel<K, LL, P>, 512, 0) != hipSuccess) \
      return 0;                                                                                                     \
  }
#define X(K, LL) XP(K, LL, 4)
  if (PER == 4) { GPS_VARIANTS(X) }
#undef X
#define X(K, LL) XP(K, LL, 8)
  if (PER == 8) { GPS_VARIANTS(X) }
#undef X
#undef XP
  return found && cus >= kG ? cus * nb : 0;   // one workgroup per CU is the layout; fewer CUs: unsupported
}

bool gen_persist_score_supported(int H, int L, int V, int N, int ML) {
  if (N < 1 || N > kNmax || L < 1 || L > 4 || H < 256 || H % 256 || (V != 256 && V != 512) || ML < 1 || ML > kSML)
    return false;
  const int KJ = H / 32;
  if (KJ != 8 && KJ != 16 && KJ != 32) return false;
  if (2 * L * KJ > 128) return false;   // resident weight registers per lane
  return gps_resident(KJ, L, V / 64) >= kG;
}

long gen_persist_score_ws_floats(int H, int L, int V, int ML) { return ((long)L * kNmax * H + (long)kNmax * V) * ML; }
long gen_persist_score_sync_words() { return (long)2 * kG * kFS + 16; }

void gen_persist_score_f32(const GenPersistScoreArgs& a, hipStream_t s) {
  if (!gen_persist_score_supported(a.H, a.L, a.V, a.N, a.ML))
    throw std::runtime_error("gen_persist_score_f32: unsupported shape or device (see gen_persist_score_supported)");
  if (!a.ws || !a.sync || !a.err || !a.P || !a.Wfc || !a.bfc || !a.rows || !a.tok_logp || !a.rank || !a.name_logp || !a.n_tok)
    throw std::runtime_error("gen_persist_score_f32: missing buffer");
  for (int l = 0; l < a.L; ++l)
    if (!a.Whh[l] || !a.bhh[l] || (l > 0 && (!a.Wih[l] || !a.bih[l])))
      throw std::runtime_error("gen_persist_score_f32: missing layer weights");
  if (a.sos < 0 || a.sos >= a.V || a.eos < 0)
    throw std::runtime_error("gen_persist_score_f32: needs 0 <= sos < V and eos >= 0");
  const int KJ = a.H / 32;
#define XP(K, LL, P)                                                                          \
  if (KJ == K && a.L == LL) {                                                                 \
    hipLaunchKernelGGL((gen_persist_score_kernel<K, LL, P>), dim3(kG), dim3(512), 0, s, a);   \
    return;                                                                                   \
  }
#define X(K, LL) XP(K, LL, 4)
  if (a.V == 256) { GPS_VARIANTS(X) }
#undef X
#define X(K, LL) XP(K, LL, 8)
  if (a.V == 512) { GPS_VARIANTS(X) }
#undef X
#undef XP
  throw std::runtime_error("gen_persist_score_f32: no variant");
}

}  // namespace gk

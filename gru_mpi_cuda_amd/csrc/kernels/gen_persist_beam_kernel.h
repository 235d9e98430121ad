// Beam search for small batches as ONE persistent launch (docs/DESIGN.md §4d, "Inside the persistent
// launch"; the rule: cpu_ref.beam_search; the per-char graph it replaces: Generator::record_beam).
//
// The grid, the residency and the weight layout are gen_persist_kernel's (gen_persist_kernel.h): 256
// workgroups x 512 threads, workgroup b owns U = H / 256 units of every recurrent matrix and VR = V / 256
// FC rows, the fp32 MFMA A-fragments stay in VGPRs for the launch, the 8 wave partials meet in LDS and
// are summed in wave order.  A beam row (row = prefix n x W + beam) is a "name" of that kernel, and its
// model step is that kernel's step of the same (KJ, L) and the same row count, operation for operation
// (the one-row VALU products, the single-tile gates of wave 0, the several-tile products with gh beside
// gi): a width-1 search returns the bytes of the greedy controlled launch.
//
// What is new is between two chars:
//   * Selection.  After the logits hand-off of char t workgroup n < N selects for prefix n: wave w owns
//     beams w, w + 8, w + 16, w + 24 and keeps their candidates' keys in registers (V / 64 per lane and
//     beam); lp is beam_select_f32's (max-subtracted, logf of the sum of expf, the fixed-order DPP
//     helpers), then W rounds of a block-wide arg-max on (order key of the score, -j) through LDS, one
//     barrier per round, only the winner's owner rescanning.  A forced char offers only prefix[t], a
//     finished beam its carry, a dead beam nothing.
//   * Records.  The selecting workgroup publishes per new beam two words -- (parent + 1) | (char + 1) << 6 |
//     state << 16, and the score -- with write-through stores, then its flag of kind L + 1; every
//     workgroup waits for the N flags and reads the N W records back (always this distributed form).
//   * The state follows the parent.  Every char has its own exchange slots and every state that is read
//     from them at char t was produced at char t, in the new order; what crosses a char inside a
//     workgroup is its own units' carry h(t-1) and the early-computed gh = h(t-1) W_hh^T + b_hh.  Both are
//     gathered by parent through LDS, never in place (set A: as computed, set B: as gathered; a dead
//     slot: h = 0, gh = b_hh, input SOS, as beam_reorder leaves it).
//   * Rows, lengths, scores and states of prefix n live in workgroup n's LDS in two sets by step parity;
//     only workgroup n writes prefix n's outputs, after the loop.
//   * The launch ends early once no beam of any prefix is live: every later step would carry every beam
//     to its own slot.
// Every hand-off uses flags (no data-tagged slots: the workspace needs no fill).  Spins are bounded (error
// bit 32, then every wait returns at once and the grid drains; what is read from a record is clamped, so
// a drained launch forms no address from garbage); the last workgroup out zeroes the flags.
// Constraints (CON = kConMask / kConAuto, instantiated by gen_persist_beam_con.hip; docs/DESIGN.md §4d,
// "Constraints inside the launch"): beam_select_f32's MASK / AUTO rule on the caller's tables.  The lines of
// prefix n at char t are staged in workgroup n's LDS before the wait for the logits (search_con_dev.h), a
// live beam's disallowed candidate keeps key 0 -- what a dead beam offers -- and lp stays the log-softmax over
// all V.  A beam's automaton state lives beside its score, state and length, two sets by step parity; the
// publishing thread looks the child's state up after the record is out.  Only workgroup n reads it, so it is
// not in the record: workspace, records and flags are the unconstrained launch's.  CON = kConNone is the
// kernel as it was (every constraint line is under if constexpr).
// Out of scope: sample_distinct / sample_conditional (the same loop with other selections), bf16.
#pragma once
#include "gen_persist_kernel.h"
#include "search_con_dev.h"

namespace gk {

namespace {
constexpr int kBDead = 0, kBLive = 1, kBFin = 2;   // BeamSelectArgs::state values
constexpr int kBW = 32;     // beams per prefix
constexpr int kBML = 64;    // chars per row
constexpr int kBRL = 68;    // bytes of a row in LDS (max_len + 1 <= 65)

// beam.hip's keys: floats -> unsigned with the same order (-0 and +0 share a key); 0 = "no candidate"
DEV unsigned pb_key(float f) {
  unsigned b = __float_as_uint(f);
  if (b == 0x80000000u) b = 0u;
  b = (b >> 31) ? ~b : (b | 0x80000000u);
  return b ? b : 1u;
}
DEV unsigned pb_umax(unsigned u) {   // identical in every lane
  return ~(unsigned)wave_min_dpp((int)~(u ^ 0x80000000u)) ^ 0x80000000u;
}
}  // namespace

// PER = V / 64 logits per lane and beam row
template <int KJ, int L, int PER, int CON = kConNone>
__global__ void __launch_bounds__(512, 1) gen_persist_beam_kernel(GenPersistBeamArgs a) {
  constexpr int U = KJ / 8, H = 32 * KJ, KW = H / 8, NT = 2 * L - 1, R3 = 3 * U;
  constexpr int V = 64 * PER, VR = V / kG;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, q4 = lane >> 4;
  const int N = a.N, W = a.W, NR = N * W, Np = (NR + 15) & ~15, nnt = Np / 16, ML = a.ML;

  __shared__ float sP[V * R3];                   // P[v][g H + b U + u] -> sP[v][g U + u]
  __shared__ float red[kNmax / 16][2][8][256];   // wave partials of two products, per row tile
  __shared__ float sghA[L][16][kNmax];           // gh rows (incl. b_hh) x beam rows, as computed at this char
  __shared__ float sghB[L][16][kNmax];           // ... gathered by parent: what the gates read
  __shared__ float sgi[16][kNmax];               // gi rows (incl. b_ih) / logits
  __shared__ float shA[L][kNmax][U];             // own units' hidden states, as computed
  __shared__ float shB[L][kNmax][U];             // ... gathered by parent: the carry of z * h_prev
  __shared__ float sbh[L][16], sbi[L][16], sbf[16];
  __shared__ __attribute__((aligned(16))) float sWf[VR][H];   // this workgroup's FC rows
  __shared__ int sid[kNmax], spar[kNmax];        // a row's input id and its parent row (-1: dead)
  __shared__ int s_last, s_live, s_plen;
  // the selecting workgroup's prefix: the rounds, and the beams' scores, states, lengths and rows by step parity
  __shared__ unsigned s_key[2][8];
  __shared__ int s_j[2][8];
  __shared__ unsigned s_wk[kBW];
  __shared__ int s_wj[kBW], s_wpar[kBW], s_wchr[kBW];
  __shared__ float sScore[2][kBW];
  __shared__ int sState[2][kBW], sLen[2][kBW];
  __shared__ unsigned char sRows[2][kBW][kBRL];
  // CON: the staged lines of this char (search_con_dev.h) and the beams' automaton states by step parity
  __shared__ unsigned sOk[scon_lines<CON>()][V / 32];
  __shared__ int sAuto[2][kBW];

  // one slot per char: X_l[t][row][H], LG[t][row][V], then REC[t][row][2]
  const size_t ws_floats = (size_t)L * ML * kNmax * H + (size_t)ML * kNmax * (V + 2);
  const prsrc_t xr = prsrc(a.ws, (unsigned)(ws_floats * 4));
  const unsigned lg0 = (unsigned)((size_t)L * ML * kNmax * H * 4);
  const unsigned rc0 = lg0 + (unsigned)((size_t)ML * kNmax * V * 4);
  const bool fastg = NR <= 16;   // one row tile, Np U <= 64: gates and publishes by wave 0 alone
  auto xoff = [&](int l, int t, int n, int col) -> unsigned {
    return (unsigned)((((size_t)(l * ML + t) * kNmax + n) * H + col) * 4);
  };
  unsigned* flags = a.sync;   // kinds 0..L-1 layer states, L logits, L + 1 records
  unsigned* done = a.sync + (size_t)(L + 2) * kG * kFS;
  auto publish_flag = [&](int kind, int t) {   // wave 0, after its payload stores
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0)
      __hip_atomic_store(flags + ((size_t)kind * kG + b) * kFS, (unsigned)(t + 1), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
  };

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
  for (int i = tid; i < L * kNmax * U; i += 512) (&shB[0][0][0])[i] = 0.f;
  if (tid < kNmax) { sid[tid] = a.sos; spar[tid] = -1; }
  if (b < N) {   // the state before step 0: beam 0 live with score 0, the others dead
    if (tid < kBW) {
      sScore[0][tid] = tid == 0 ? 0.f : -INFINITY;
      sState[0][tid] = tid == 0 ? kBLive : kBDead;
      sLen[0][tid] = 0;
      if constexpr (CON == kConAuto) sAuto[0][tid] = tid == 0 ? a.allow_start[b] : 0;
    }
    for (int i = tid; i < kBW * kBRL; i += 512) (&sRows[0][0][0])[i] = 0;
    if (tid == 0) s_plen = a.plen[b];
  }
  __syncthreads();

  auto reduce_el = [&](float (*dst)[kNmax], int slot, int nt, const float* bias, int nrows, int i) {
    const int row = i >> 4, n = i & 15;
    float s = red[nt][slot][0][i];
#pragma unroll
    for (int k = 1; k < 8; ++k) s += red[nt][slot][k][i];
    if (row < nrows) dst[row][nt * 16 + n] = s + bias[row];
  };
  auto reduce_fc_el = [&](float (*dst)[kNmax], int nt, int i) {   // i < 16 VR
    const int row = i >> 4, n = i & 15;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
      for (int q = 0; q < 4; ++q) s += red[nt][0][k][(4 * q + row) * 16 + n];
    dst[row][nt * 16 + n] = s + sbf[row];
  };
  auto stash = [&](int nt, int slot, const f32x4& acc) {
#pragma unroll
    for (int r = 0; r < 4; ++r) red[nt][slot][w][(4 * q4 + r) * 16 + fr] = acc[r];
  };
  // gates of layer l for all rows: gh and the carry from the gathered set B, h -> set A; then wave 0
  // publishes h_l(t) and its flag
  auto gates_publish = [&](int l, int t) {
    if (fastg) {
      if (w == 0) {
        const int ln = lane_now();
        const int n = ln / U, u = ln % U;
        if (ln < Np * U) {
          float gi[3], gh[3];
#pragma unroll
          for (int g = 0; g < 3; ++g) {
            gh[g] = sghB[l][g * U + u][n];
            if (l == 0) {
              gi[g] = sP[sid[n] * R3 + g * U + u];
            } else {
              const int e = (g * U + u) * 16 + n;
              float sum = red[0][0][0][e];
#pragma unroll
              for (int k = 1; k < 8; ++k) sum += red[0][0][k][e];
              gi[g] = sum + sbi[l][g * U + u];
            }
          }
          const float r = sig_ieee(gi[0] + gh[0]);
          const float z = sig_ieee(gi[1] + gh[1]);
          const float nn = tanhf(gi[2] + r * gh[2]);
          const float hv = (1.f - z) * nn + z * shB[l][n][u];
          shA[l][n][u] = hv;
          if (n < NR) st_sc1(xr, xoff(l, t, n, b * U + u), hv);
        }
        publish_flag(l, t);
      }
      __syncthreads();
      return;
    }
    for (int i = tid; i < Np * U; i += 512) {
      const int n = i / U, u = i % U;
      float gi[3], gh[3];
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        gh[g] = sghB[l][g * U + u][n];
        gi[g] = l == 0 ? sP[sid[n] * R3 + g * U + u] : sgi[g * U + u][n];
      }
      const float r = sig_ieee(gi[0] + gh[0]);
      const float z = sig_ieee(gi[1] + gh[1]);
      const float nn = tanhf(gi[2] + r * gh[2]);
      shA[l][n][u] = (1.f - z) * nn + z * shB[l][n][u];
    }
    __syncthreads();
    if (w == 0) {
      if (lane < Np) {
        if constexpr (U == 4) {
          const pu32x4 v = {__float_as_uint(shA[l][lane][0]), __float_as_uint(shA[l][lane][1]),
                            __float_as_uint(shA[l][lane][2]), __float_as_uint(shA[l][lane][3])};
          __builtin_amdgcn_raw_buffer_store_b128(v, xr, xoff(l, t, lane, b * U), 0, 16);
        } else {
          for (int u = 0; u < U; ++u) st_sc1(xr, xoff(l, t, lane, b * U + u), shA[l][lane][u]);
        }
      }
      publish_flag(l, t);
    }
  };

  // gh_l of the next char is computed beside the product that consumes h_l(t) (set A); at t = 0 the
  // gathered set is the bias
  for (int i = tid; i < L * 16 * kNmax; i += 512) {
    const int l = i / (16 * kNmax), row = (i / kNmax) % 16;
    (&sghB[0][0][0])[i] = sbh[l][row];
  }
  __syncthreads();
  float xk[KJ];   // this wave's x of the last row tile, kept for the gh pass after the publish
  const bool one = NR == 1;
  auto vdot_q = [&](auto ti_tag) -> float {
    constexpr int TI = decltype(ti_tag)::value;
    float p = 0.f;
#pragma unroll
    for (int j = 0; j < KJ; ++j) p = fmaf(Wr[TI][j], xk[j], p);
    p += __shfl_xor(p, 16, 64);
    p += __shfl_xor(p, 32, 64);
    return p;
  };
  auto stash_one = [&](int slot, float p) {
    if (q4 == 0) red[0][slot][w][fr * 16] = p;
  };
  auto product = [&](auto ta_tag, auto src_tag, int t, float (*dst)[kNmax], const float* bias, int nrows) {
    constexpr int TA = decltype(ta_tag)::value, SRC = decltype(src_tag)::value;   // TA = NT: the FC rows
    const int kw0 = w * KW + q4 * KJ;
    const int xn = one ? 0 : fr;
    const bool xv = one || fr < NR;
    pwait(flags, SRC, w * 32, 32, (unsigned)(t + 1), a.err);
    load_x<KJ>(xr, xoff(SRC, t, xn, kw0), xv, xk);
    const bool gh = nnt > 1 && t + 1 < ML;
    auto whh = [&](int j) { return Wr[SRC][j]; };
    for (int nt = 0; nt < nnt; ++nt) {
      constexpr bool kRollPF = NT * KJ <= 80;
      const bool pf = kRollPF && nt + 1 < nnt;
      const unsigned noff = xoff(SRC, t, (nt + 1) * 16 + fr, kw0);
      const bool nvalid = (nt + 1) * 16 + fr < NR;
      f32x4 o0, o1;
      if constexpr (TA == NT) {
        float p0 = 0.f, p1 = 0.f;
        auto dot = [&](const float* wr, float& p) {
#pragma unroll
          for (int j = 0; j < KJ; j += 8) {
            const float4 u = *reinterpret_cast<const float4*>(wr + j);
            const float4 v = *reinterpret_cast<const float4*>(wr + j + 4);
            p = fmaf(u.x, xk[j], p); p = fmaf(u.y, xk[j + 1], p);
            p = fmaf(u.z, xk[j + 2], p); p = fmaf(u.w, xk[j + 3], p);
            p = fmaf(v.x, xk[j + 4], p); p = fmaf(v.y, xk[j + 5], p);
            p = fmaf(v.z, xk[j + 6], p); p = fmaf(v.w, xk[j + 7], p);
          }
        };
        dot(&sWf[0][kw0], p0);
        if constexpr (VR > 1) dot(&sWf[VR - 1][kw0], p1);
        red[nt][0][w][(4 * q4) * 16 + fr] = p0;
        red[nt][0][w][(4 * q4 + 1) * 16 + fr] = p1;
        if (gh) {
          tile_mm2<KJ, false>(whh, whh, xk, o1, o0, pf, xr, noff, nvalid);
          stash(nt, 1, o1);
        } else if (pf) {
          load_x<KJ>(xr, noff, nvalid, xk);
        }
      } else if (one) {
        stash_one(0, vdot_q(ic<TA>{}));
      } else {
        auto wta = [&](int j) { return Wr[TA][j]; };
        if (gh) tile_mm2<KJ, true>(wta, whh, xk, o0, o1, pf, xr, noff, nvalid);
        else tile_mm2<KJ, false>(wta, wta, xk, o0, o1, pf, xr, noff, nvalid);
        stash(nt, 0, o0);
        if (gh) stash(nt, 1, o1);
      }
      if (!pf && nt + 1 < nnt) {
        __builtin_amdgcn_sched_barrier(0);
        load_x<KJ>(xr, noff, nvalid, xk);
      }
    }
    lds_barrier();
    if (fastg && TA != NT) return;   // the gates read the partials themselves (gates_publish)
    for (int i = tid; i < nnt * 256; i += 512) {
      const int nt = i >> 8, e = i & 255;
      if constexpr (TA == NT) {
        if (e < 16 * nrows) {
          reduce_fc_el(dst, nt, e);
          if (fastg) {   // wave 0 lanes store their logit at once
            const int ln = lane_now(), row = ln >> 4, n = ln & 15;
            if (n < NR) st_sc1(xr, lg0 + (unsigned)(((size_t)t * kNmax + n) * V + b * VR + row) * 4, dst[row][n]);
          }
        }
      } else {
        reduce_el(dst, 0, nt, bias, nrows, e);
      }
      if (gh) reduce_el(sghA[SRC], 1, nt, sbh[SRC], R3, e);
    }
    lds_barrier();
  };
  auto product_gh = [&](auto src_tag, int t) {
    constexpr int SRC = decltype(src_tag)::value;
    if (t + 1 >= ML || nnt > 1) return;   // (several row tiles: done inside product)
    if (one) stash_one(1, vdot_q(ic<SRC>{}));
    else stash(0, 1, tile_mm<KJ>([&](int j) { return Wr[SRC][j]; }, xk));
    lds_barrier();
    if (tid < 256) reduce_el(sghA[SRC], 1, 0, sbh[SRC], R3, tid);
    lds_barrier();
  };

  // ---- the selection of step st for prefix b (b < N, all 8 waves): sets cur -> cur ^ 1, the records out
  auto select = [&](int st, int cur) {
#pragma clang fp contract(off)
    const int nxt = cur ^ 1;
    // CON: this char's lines into LDS while the other workgroups' model step is in flight (the states of set
    // `cur` are behind the previous selection's last barrier)
    if constexpr (CON != kConNone) scon_stage<CON, V>(a, b, st, W, sAuto[cur], sOk);
    if (w == 0) pwait(flags, L, 0, kG, (unsigned)(st + 1), a.err);
    __syncthreads();
    const bool forced = st < s_plen;
    int fc = 0;
    if (forced) {
      fc = a.prefix[(size_t)b * ML + st];
      if (fc >= V) {   // never expected (the host checks first): flag it instead of offering it
        if (tid == 0) {
          __hip_atomic_fetch_or(a.err, 16u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          a.err[1] = (unsigned)fc;
          a.err[2] = (unsigned)(b * W);
        }
        fc = 0;
      }
    }
    // candidates of this wave's beams: key 0 = not offered.  (The lane id is recomputed inside the selection:
    // hoisted out of the char loop, its address math would live across the weight-resident products)
    const int sl = lane_now();
    unsigned key[4][PER];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int bm = w + 8 * r;   // wave-uniform
#pragma unroll
      for (int e = 0; e < PER; ++e) key[r][e] = 0u;
      if (bm >= W) continue;
      const unsigned base = lg0 + (unsigned)(((size_t)st * kNmax + (b * W + bm)) * V + sl * PER) * 4;
      float xv[PER];
#pragma unroll
      for (int e = 0; e < PER; e += 4) {
        const pu32x4 v = __builtin_amdgcn_raw_buffer_load_b128(xr, base + 4 * e, 0, 0);
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
      const float lse = logf(se);
      const float sb = sScore[cur][bm];
      const int stt = sState[cur][bm];
      unsigned ok = ~0u;   // CON: bit e = this lane's char e is allowed (one LDS word, dead after this beam)
      if constexpr (CON != kConNone) ok = scon_bits<CON, V>(sOk, bm, sl * PER);
#pragma unroll
      for (int e = 0; e < PER; ++e) {
        const int c = sl * PER + e;
        const float lp = (xv[e] - mx) - lse;
        if (stt == kBLive) {
          if ((!forced || c == fc) && (CON == kConNone || ((ok >> e) & 1u))) key[r][e] = pb_key(sb + lp);
        } else if (stt == kBFin && c == 0) {
          key[r][e] = pb_key(sb);   // the carry, j = bm V
        }
      }
    }
    // this wave's best: the largest key, then the lowest j
    auto wave_best = [&](unsigned& bk, int& bj) {
      unsigned lk = 0u;
      int lj = 0x7fffffff;
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int e = 0; e < PER; ++e)
          if (key[r][e] > lk) { lk = key[r][e]; lj = (w + 8 * r) * V + sl * PER + e; }   // ascending j: first wins
      bk = pb_umax(lk);
      bj = wave_min_dpp((lk == bk && bk != 0u) ? lj : 0x7fffffff);
    };
    unsigned bk;
    int bj;
    wave_best(bk, bj);
    if (lane == 0) { s_key[0][w] = bk; s_j[0][w] = bj; }
    __syncthreads();
    for (int k = 0; k < W; ++k) {
      const int kc = k & 1;
      // every wave reduces the 8 slots itself, a lane per slot
      const unsigned ki = sl < 8 ? s_key[kc][sl] : 0u;
      const int ji = sl < 8 ? s_j[kc][sl] : 0x7fffffff;
      const unsigned wk = pb_umax(ki);
      const int wj = wave_min_dpp((ki == wk && wk != 0u) ? ji : 0x7fffffff);
      const bool any = wk != 0u;
      const int pb = any ? wj / V : 0, pc = any ? wj - pb * V : 0;
      if (any && (pb & 7) == w) {   // the owner takes it out and rescans (wave-uniform branch)
        const int r = pb >> 3, e = pc - sl * PER;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
#pragma unroll
          for (int ee = 0; ee < PER; ++ee)
            if (rr == r && ee == e) key[rr][ee] = 0u;
        wave_best(bk, bj);
      }
      if (lane == 0) { s_key[kc ^ 1][w] = bk; s_j[kc ^ 1][w] = bj; }
      if (tid == 0) { s_wk[k] = wk; s_wj[k] = wj; }
      __syncthreads();
    }
    // the W new beams, one thread each (all in wave 0): the next set's score, state and length, the record
    if (tid < W) {
      const int k = tid;
      const unsigned wk = s_wk[k];
      const int wj = s_wj[k];
      const bool any = wk != 0u;
      const int pb = any ? wj / V : 0, pc = any ? wj - pb * V : 0;
      float sc = -INFINITY;
      int parent = -1, ch = -1, stn = kBDead, len = 0;
      if (any) {
        parent = pb;
        len = sLen[cur][pb];
        if (sState[cur][pb] == kBFin) {
          sc = sScore[cur][pb]; stn = kBFin;
        } else {
          // the candidate's score back from its key (the key keeps every bit but the sign of zero)
          sc = __uint_as_float((wk & 0x80000000u) ? (wk & 0x7fffffffu) : ~wk);
          ch = pc;
          stn = pc == a.eos ? kBFin : kBLive;
          if (len < ML) ++len;
        }
      }
      sScore[nxt][k] = sc; sState[nxt][k] = stn; sLen[nxt][k] = len;
      s_wpar[k] = parent; s_wchr[k] = ch;
      if (st + 1 < ML) {   // (the last step's beams feed nothing)
        const unsigned off = rc0 + (unsigned)(((size_t)st * kNmax + (b * W + k)) * 2) * 4;
        __builtin_amdgcn_raw_buffer_store_b32((unsigned)(parent + 1) | (unsigned)(ch + 1) << 6 | (unsigned)stn << 16, xr, off, 0, 16);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(sc), xr, off + 4, 0, 16);
      }
    }
    if (w == 0 && st + 1 < ML) publish_flag(L + 1, st);
    if constexpr (CON == kConAuto) {   // the children's states, behind the record (a carry or a dead slot: 0)
      if (tid < W) {
        const int p = s_wpar[tid], ch = s_wchr[tid];   // this thread's own stores
        sAuto[nxt][tid] = (p >= 0 && ch >= 0) ? scon_next(a, sAuto[cur][p], ch) : 0;
      }
    }
    __syncthreads();
    // the rows gathered by parent, the char appended (beam_reorder's rule), off the other workgroups' path
    const int RL = ML + 1;
    for (int i = tid; i < W * RL; i += 512) {
      const int k = i / RL, c = i - k * RL;
      const int p = s_wpar[k];
      unsigned char v = 0;
      if (p >= 0) {
        const int len = sLen[cur][p], ch = s_wchr[k];
        v = sRows[cur][p][c];
        if (ch >= 0 && c == len && len < ML) v = (unsigned char)ch;
      }
      sRows[nxt][k][c] = v;
    }
    __syncthreads();
  };

  int pc = 0;   // (b < N) the set that holds the prefix's beams
  for (int t = 0; t <= ML; ++t) {
    if (t == ML && b >= N) break;   // the last char is only selected
    if (t > 0) {
      if (b < N) { select(t - 1, pc); pc ^= 1; }
      if (t == ML) break;
      // ---- every workgroup reads the N W records of step t - 1: parents, input ids, "any beam live"
      if (w == 0) {
        pwait(flags, L + 1, 0, N, (unsigned)t, a.err);
        const int ln = lane_now();
        int par = -1, id = a.sos, live = 0;
        if (ln < NR) {
          const unsigned v = __builtin_amdgcn_raw_buffer_load_b32(xr, rc0 + (unsigned)(((size_t)(t - 1) * kNmax + ln) * 2) * 4, 0, 0);
          const int p = (int)(v & 63u) - 1, c = (int)((v >> 6) & 1023u) - 1, s = (int)((v >> 16) & 3u);
          if (p >= 0 && p < W) par = (ln / W) * W + p;
          if (par >= 0 && s == kBLive && c >= 0 && c < V) { id = c; live = 1; }
        }
        if (ln < kNmax) { spar[ln] = par; sid[ln] = id; }
        const unsigned long long lv = __ballot(live != 0);
        if (lane == 0) s_live = lv != 0ull;
      }
      __syncthreads();
      if (!s_live) break;   // every beam finished or dead: the later steps carry each beam to its own slot
      // ---- the carry follows the parent: set A (as computed at char t - 1) -> set B (what char t reads)
      for (int i = tid; i < L * 16 * Np; i += 512) {
        const int l = i / (16 * Np), row = (i / Np) % 16, n = i % Np;
        const int p = spar[n];
        sghB[l][row][n] = p >= 0 ? sghA[l][row][p] : sbh[l][row];
      }
      for (int i = tid; i < L * Np * U; i += 512) {
        const int l = i / (Np * U), n = (i / U) % Np, u = i % U;
        const int p = spar[n];
        shB[l][n][u] = p >= 0 ? shA[l][p][u] : 0.f;
      }
      __syncthreads();
    }
    // ---- layer 0: gi = P[id]
    gates_publish(0, t);
    // ---- layers >= 1: gi_l = h_{l-1}(t) W_ih_l^T + b_ih_l  (+ gh_{l-1} of the next char)
    static_for<1, L>([&](auto lt) {
      constexpr int l = decltype(lt)::value;
      product(ic<L + l - 1>{}, ic<l - 1>{}, t, sgi, sbi[l], R3);
      gates_publish(l, t);
      product_gh(ic<l - 1>{}, t);
    });
    // ---- FC: logits rows b VR .. b VR + VR  (+ gh_{L-1} of the next char)
    product(ic<NT>{}, ic<L - 1>{}, t, sgi, sbf, VR);
    if (w == 0) {
      if (lane < Np && !fastg)   // (fastg: stored inside the product's reduce)
        for (int r = 0; r < VR; ++r)
          st_sc1(xr, lg0 + (unsigned)(((size_t)t * kNmax + lane) * V + b * VR + r) * 4, sgi[r][lane]);
      publish_flag(L, t);
    }
    product_gh(ic<L - 1>{}, t);
  }

  // ---- prefix b's outputs, in the layout Generator::beam returns: one writer, its selecting workgroup
  if (b < N) {
    const int RL = ML + 1;
    for (int i = tid; i < W * RL; i += 512) {
      const int k = i / RL, c = i - k * RL;
      a.rows[((size_t)b * W + k) * RL + c] = sRows[pc][k][c];
    }
    if (w == 0) {
      const bool in = lane < W;
      const int stf = in ? sState[pc][lane] : kBDead;
      if (in) {
        a.logp[(size_t)b * W + lane] = sScore[pc][lane];
        a.n_tok[(size_t)b * W + lane] = sLen[pc][lane];
      }
      const int cnt = __popcll(__ballot(stf != kBDead));
      if (lane == 0) a.n_beams[b] = cnt;
    }
  }
  // ---- the last workgroup out zeroes the flags for the next launch (nobody polls them any more)
  __syncthreads();
  if (tid == 0) s_last = __hip_atomic_fetch_add(done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == kG - 1;
  __syncthreads();
  if (s_last) {
    for (long i = tid; i < (long)(L + 2) * kG * kFS; i += 512) flags[i] = 0u;
    if (tid == 0) *done = 0u;
  }
}

}  // namespace gk

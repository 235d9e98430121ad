// Sequential Monte Carlo under constraints for small calls as ONE persistent launch (docs/DESIGN.md §4j, "Inside
// the persistent launch"; the rule: cpu_ref.sample_conditional; the per-char graph it replaces:
// Generator::record_beam with smc_select_f32 as the selection).
//
// The grid, the residency and the weight layout are gen_persist_kernel's (gen_persist_kernel.h): 256
// workgroups x 512 threads, workgroup b owns U = H / 256 units of every recurrent matrix and VR = V / 256
// FC rows, the fp32 MFMA A-fragments stay in VGPRs for the launch, the 8 wave partials meet in LDS and
// are summed in wave order.  A slot row (row = system n x W + slot) is a "name" of that kernel, and its
// model step is that kernel's step of the same (KJ, L) and the same row count, operation for operation, as
// in gen_persist_smc_kernel (whose step code this file repeats: that kernel stays as it is).
//
// What is this kernel's own is between two chars:
//   * Selection.  After the logits hand-off of step l workgroup n < N selects for system n by
//     smc_select_f32's rule in its order, contraction off, in three phases with LDS between them:
//     (a) wave w owns slots w, w + 8, w + 16, w + 24: per live slot y = x * inv_t, lse_all over the vocabulary,
//         (max_A, sum_A, lse_A) over the allowed set, logm = lse_A - lse_all (0 on a forced step and for a
//         finished slot) and u = logw + logm, left in LDS;
//     (b) after one barrier every thread derives the same ESS, the same decision against thr W, the same
//         ancestors (systematic resampling; the fan-out at step 0) and the same new logw from the at most 32
//         published u, in slot order.  The step's uniform is word 1 of slot 0's Philox block (counter (i, l,
//         start + n), key the seed), computed on a resampling step only;
//     (c) wave i re-reads ancestor a_i's logits, forms the running sums with wave_scan_incl_dpp and draws the
//         char by the inverse CDF inside the allowed set (word 0 of slot i's block); a forced step gives
//         prefix[l], a finished ancestor is carried; logq_i = logq_a + (y_a[c] - lse_A).
//   * Constraints.  The allowed set is a line of the caller's allow_tab ([allow_rows][V / 32] words, L2-resident):
//     line allow_idx[n][l] (per position), or the line of the slot's automaton state, which becomes
//     allow_next[line of a_i][c] with every char, forced ones too, and starts at allow_start[n].  What is read
//     back is clamped before it indexes anything (error bit 16, as smc_select_f32).  No table: every char.
//   * Records.  The selecting workgroup publishes per new slot four words -- (ancestor + 1) | (char + 1) << 6 |
//     state << 16, the automaton state, logq, logw -- with one write-through store, then its flag of kind
//     L + 1; every workgroup waits for the N flags and reads the N W records back.
//   * The state follows the ancestor.  Every char has its own exchange slots; what crosses a char inside a
//     workgroup is its own units' carry h(t-1) and the early-computed gh = h(t-1) W_hh^T + b_hh.  Both are
//     gathered by ancestor through LDS, never in place (set A: as computed, set B: as gathered; a dead
//     slot: h = 0, gh = b_hh, input SOS, as beam_reorder leaves it).
//   * Rows, lengths, logw, logq, states and automaton states of system n live in workgroup n's LDS in two sets
//     by step parity; only workgroup n writes system n's outputs, after the loop.
//   * The launch's model steps end once no slot of any system is live.  The rule goes on: finished slots with
//     unequal weights can still be resampled, so workgroup n runs the remaining selections on its LDS alone
//     (no logits are read, nothing is published).
// Every hand-off uses flags (the workspace needs no fill).  Spins are bounded (error bit 32, then every wait
// returns at once and the grid drains; what is read from a record is clamped, so a drained launch forms no
// address from garbage); the last workgroup out zeroes the flags.  No float atomics.
// Out of scope: bf16, the optional logm / lq / ess outputs of smc_select_f32.
#include "gen_persist_kernel.h"
#include "smc_dev.h"

namespace gk {

namespace {
constexpr int kBW = 32;     // slots per system
constexpr int kBML = 64;    // chars per row
constexpr int kBRL = 68;    // bytes of a row in LDS (max_len + 1 <= 65)
constexpr int kRec = 4;     // words of a record
}  // namespace

// PER = V / 64 logits per lane and slot row
template <int KJ, int L, int PER>
__global__ void __launch_bounds__(512, 1) gen_persist_smc_kernel(GenPersistSmcArgs a) {
  constexpr int U = KJ / 8, H = 32 * KJ, KW = H / 8, NT = 2 * L - 1, R3 = 3 * U;
  constexpr int V = 64 * PER, VR = V / kG;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, q4 = lane >> 4;
  const int N = a.N, W = a.W, NR = N * W, Np = (NR + 15) & ~15, nnt = Np / 16, ML = a.ML;

  __shared__ float sP[V * R3];                   // P[v][g H + b U + u] -> sP[v][g U + u]
  __shared__ float red[kNmax / 16][2][8][256];   // wave partials of two products, per row tile
  __shared__ float sghA[L][16][kNmax];           // gh rows (incl. b_hh) x slot rows, as computed at this char
  __shared__ float sghB[L][16][kNmax];           // ... gathered by parent: what the gates read
  __shared__ float sgi[16][kNmax];               // gi rows (incl. b_ih) / logits
  __shared__ float shA[L][kNmax][U];             // own units' hidden states, as computed
  __shared__ float shB[L][kNmax][U];             // ... gathered by parent: the carry of z * h_prev
  __shared__ float sbh[L][16], sbi[L][16], sbf[16];
  __shared__ __attribute__((aligned(16))) float sWf[VR][H];   // this workgroup's FC rows
  __shared__ int sid[kNmax], spar[kNmax];        // a row's input id and its parent row (-1: dead)
  __shared__ int s_last, s_live, s_plen;
  // the selecting workgroup's system: phase (a)'s look-ahead weights and allowed-set statistics of this step, the
  // new slots' ancestors and chars, and the slots' logw, logq, states, lengths, automaton states and rows by
  // step parity
  __shared__ float s_u[kBW], s_mxa[kBW], s_sea[kBW], s_lsa[kBW];
  __shared__ int s_wpar[kBW], s_wchr[kBW];
  __shared__ float sLogw[2][kBW], sLogq[2][kBW];
  __shared__ int sState[2][kBW], sLen[2][kBW], sAut[2][kBW];
  __shared__ int s_nres;
  __shared__ unsigned char sRows[2][kBW][kBRL];

  // one slot per char: X_l[t][row][H], LG[t][row][V], then REC[t][row][kRec]
  const size_t ws_floats = (size_t)L * ML * kNmax * H + (size_t)ML * kNmax * (V + kRec);
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
  if (b < N) {   // the state before step 0: slot 0 live with logw = logq = 0, the others dead
    if (tid < kBW) {
      sLogq[0][tid] = sLogw[0][tid] = tid == 0 ? 0.f : -INFINITY;
      sState[0][tid] = tid == 0 ? kLive : kDead;
      sLen[0][tid] = 0;
      sAut[0][tid] = (tid == 0 && a.allow_start) ? a.allow_start[b] : 0;
    }
    for (int i = tid; i < kBW * kBRL; i += 512) (&sRows[0][0][0])[i] = 0;
    if (tid == 0) { s_plen = a.plen[b]; s_nres = 0; }
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

  // ---- the selection of step st for system b (b < N, all 8 waves): sets cur -> cur ^ 1, the records out.
  // shared: the model steps still run (wait for the logits, publish the records); otherwise every slot of every
  // system is finished and the selection works on this workgroup's LDS alone
  auto select = [&](int st, int cur, bool shared) {
#pragma clang fp contract(off)
    const int nxt = cur ^ 1;
    if (shared && w == 0) pwait(flags, L, 0, kG, (unsigned)(st + 1), a.err);
    __syncthreads();
    const bool forced = st < s_plen;
    int fc = 0;
    if (forced) {
      fc = a.prefix[(size_t)b * ML + st];
      if (fc >= V) {   // never expected (the host checks first): flag it instead of drawing it
        if (tid == 0) {
          __hip_atomic_fetch_or(a.err, 16u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          a.err[1] = (unsigned)fc;
          a.err[2] = (unsigned)(b * W);
        }
        fc = 0;
      }
    }
    const bool aut = a.allow_next != nullptr, mask = a.allow_tab != nullptr;
    int arn = 0;   // per position: the system's line of this step
    if (mask && !aut) {
      arn = a.allow_idx[(size_t)b * ML + st];
      if (arn < 0 || arn >= a.allow_rows) {   // never expected (the host builds both): flag it, no constraint
        if (tid == 0) {
          __hip_atomic_fetch_or(a.err, 16u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          a.err[1] = (unsigned)arn;
          a.err[2] = (unsigned)(b * W);
        }
        arn = 0;
      }
    }
    const float inv_t = a.inv_t[b];
    // (the lane id is recomputed inside the selection: hoisted out of the char loop, its address math would
    // live across the weight-resident products)
    const int sl = lane_now();
    // slot bm's automaton line, clamped (wave-uniform)
    auto line_of = [&](int bm, bool flag) -> int {
      int q = sAut[cur][bm];
      if (q < 0 || q >= a.allow_rows) {   // never expected (the host builds start and next): flag it, the free state
        if (flag && sl == 0) {
          __hip_atomic_fetch_or(a.err, 16u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          a.err[1] = (unsigned)q;
          a.err[2] = (unsigned)(b * W + bm);
        }
        q = 0;
      }
      return q;
    };
    // slot bm's scaled logits and this lane's allowed bits (bit e: char sl PER + e)
    auto load_row = [&](int bm, float (&y)[PER], unsigned& ok, bool flag) {
      ok = ~0u;
      if (mask) {
        const int ar = aut ? line_of(bm, flag) : arn;
        ok = a.allow_tab[(size_t)ar * (V >> 5) + ((sl * PER) >> 5)] >> ((sl * PER) & 31);
      }
      const unsigned base = lg0 + (unsigned)(((size_t)st * kNmax + (b * W + bm)) * V + sl * PER) * 4;
#pragma unroll
      for (int e = 0; e < PER; e += 4) {
        const pu32x4 v = __builtin_amdgcn_raw_buffer_load_b128(xr, base + 4 * e, 0, 0);
        y[e] = __uint_as_float(v.x) * inv_t; y[e + 1] = __uint_as_float(v.y) * inv_t;
        y[e + 2] = __uint_as_float(v.z) * inv_t; y[e + 3] = __uint_as_float(v.w) * inv_t;
      }
    };
    // ---- (a) the slots' masses and look-ahead weights (not unrolled: the weight fragments leave few registers)
#pragma unroll 1
    for (int r = 0; r < 4; ++r) {
      const int bm = w + 8 * r;   // wave-uniform
      if (bm >= W) continue;
      const int stt = sState[cur][bm];
      float logm = 0.f;
      if (stt == kLive) {   // (a finished or dead slot: no mass to weigh, and nothing of its row is read again)
        float y[PER];
        unsigned ok;
        load_row(bm, y, ok, true);
        float mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < PER; ++e) mx = fmaxf(mx, y[e]);
        mx = wave_max_dpp(mx);
        float se = 0.f;
#pragma unroll
        for (int e = 0; e < PER; ++e) se += expf(y[e] - mx);
        se = wave_sum_dpp(se);
        const float lse_all = mx + logf(se);
        float mxa = -INFINITY;
#pragma unroll
        for (int e = 0; e < PER; ++e) mxa = fmaxf(mxa, ((ok >> e) & 1u) ? y[e] : -INFINITY);
        mxa = wave_max_dpp(mxa);
        float sea = 0.f;
#pragma unroll
        for (int e = 0; e < PER; ++e) sea += ((ok >> e) & 1u) ? expf(y[e] - mxa) : 0.f;
        sea = wave_sum_dpp(sea);
        const float lsa = mxa + logf(sea);
        if (!forced) logm = lsa - lse_all;
        if (sl == 0) { s_mxa[bm] = mxa; s_sea[bm] = sea; s_lsa[bm] = lsa; }
      }
      const float u = sLogw[cur][bm] + logm;
      if (sl == 0) s_u[bm] = u;
    }
    __syncthreads();
    // ---- (b) ESS, the decision and the ancestors: every thread the same arithmetic, in slot order
    float mu = -INFINITY;
    int last = 0;   // the last slot that is not dead
    for (int bm = 0; bm < W; ++bm)
      if (sState[cur][bm] != kDead) { mu = fmaxf(mu, s_u[bm]); last = bm; }
    float S = 0.f, Q = 0.f;
    for (int bm = 0; bm < W; ++bm)
      if (sState[cur][bm] != kDead) {
        const float e = expf(s_u[bm] - mu);
        S += e;
        Q += e * e;
      }
    const float ess = (S * S) / Q;
    const bool fan = st == 0;
    const bool res = !fan && ess < a.thr * (float)W;
    const unsigned long long gidx = a.start + (unsigned long long)b;   // the system's global index
    const unsigned k0 = (unsigned)a.seed, k1 = (unsigned)(a.seed >> 32), g0 = (unsigned)gidx, g1 = (unsigned)(gidx >> 32);
    float Ur = 0.f;
    if (res) {
      unsigned wd[4];
      philox4x32_10(0u, (unsigned)st, g0, g1, k0, k1, wd);
      Ur = smc_unit(wd[1]);
    }
    if (tid == 0 && res) ++s_nres;   // (the fan-out is step 0: nothing counted before it)
    // ---- (c) new slot i: its ancestor, its weight, its char
#pragma unroll 1
    for (int r = 0; r < 4; ++r) {
      const int i = w + 8 * r;   // wave-uniform
      if (i >= W) continue;
      int anc = i;
      float lw;
      if (fan) {
        anc = 0;
        lw = s_u[0];
      } else if (res) {
        const float t = ((float)i + Ur) / (float)W * S;
        float cum = 0.f;
        anc = -1;
        for (int bm = 0; bm < W; ++bm)
          if (sState[cur][bm] != kDead) {
            cum += expf(s_u[bm] - mu);
            if (anc < 0 && cum > t) anc = bm;
          }
        if (anc < 0) anc = last;
        lw = mu + logf(S / (float)W);
      } else {
        lw = s_u[i];
      }
      const int ast = sState[cur][anc];
      float lq = -INFINITY;
      int parent = -1, ch = -1, stn = kDead, qn = 0, len = 0;
      if (ast == kFin) {          // carried: row, length and logq unchanged
        parent = anc; stn = kFin; lq = sLogq[cur][anc]; len = sLen[cur][anc];
      } else if (ast == kLive) {
        parent = anc;
        float dl = 0.f;
        if (forced) {
          ch = fc;
        } else {
          float y[PER];
          unsigned ok;
          load_row(anc, y, ok, false);
          const float mxa = s_mxa[anc], sea = s_sea[anc];
          unsigned wd[4];
          philox4x32_10((unsigned)i, (unsigned)st, g0, g1, k0, k1, wd);
          const float target = smc_unit(wd[0]) * sea;
          float ex[PER];
          float loc = 0.f;
#pragma unroll
          for (int e = 0; e < PER; ++e) {
            ex[e] = ((ok >> e) & 1u) ? expf(y[e] - mxa) : 0.f;
            loc += ex[e];
          }
          float run = wave_scan_incl_dpp(loc) - loc;
          int hit = V, top = -1;   // the first allowed char whose running sum exceeds the target; the last allowed char
#pragma unroll
          for (int e = 0; e < PER; ++e) {
            run += ex[e];
            const bool al = (ok >> e) & 1u;
            if (al) top = sl * PER + e;
            if (al && hit == V && run > target) hit = sl * PER + e;
          }
          hit = wave_min_dpp(hit);
          top = -wave_min_dpp(-top);
          ch = hit < V ? hit : (top >= 0 ? top : V - 1);
          const int e = ch - sl * PER;   // the owner lane's y[ch] to every lane
          float yc = -INFINITY;
#pragma unroll
          for (int ee = 0; ee < PER; ++ee)
            if (ee == e) yc = y[ee];
          yc = wave_max_dpp(yc);
          dl = yc - s_lsa[anc];
        }
        lq = sLogq[cur][anc] + dl;
        stn = ch == a.eos ? kFin : kLive;
        len = sLen[cur][anc];
        if (len < ML) ++len;
        if (aut) qn = a.allow_next[(size_t)line_of(anc, false) * V + ch];   // ch < V: drawn above, or the clamped prefix char
      } else {
        lw = -INFINITY;
      }
      if (sl == 0) {
        sLogw[nxt][i] = lw; sLogq[nxt][i] = lq; sState[nxt][i] = stn; sLen[nxt][i] = len; sAut[nxt][i] = qn;
        s_wpar[i] = parent; s_wchr[i] = ch;
      }
    }
    __syncthreads();
    // the W records, one thread each (all in wave 0), then the flag
    if (shared && st + 1 < ML) {   // (the last step's slots feed nothing)
      if (tid < W) {
        const unsigned off = rc0 + (unsigned)(((size_t)st * kNmax + (b * W + tid)) * kRec) * 4;
        const pu32x4 rec = {(unsigned)(s_wpar[tid] + 1) | (unsigned)(s_wchr[tid] + 1) << 6 | (unsigned)sState[nxt][tid] << 16,
                            (unsigned)sAut[nxt][tid], __float_as_uint(sLogq[nxt][tid]), __float_as_uint(sLogw[nxt][tid])};
        __builtin_amdgcn_raw_buffer_store_b128(rec, xr, off, 0, 16);
      }
      if (w == 0) publish_flag(L + 1, st);
    }
    // the rows gathered by ancestor, the char appended (beam_reorder's rule), off the other workgroups' path
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

  int pc = 0;       // (b < N) the set that holds the system's slots
  int nsel = 0;     // (b < N) selections done
  for (int t = 0; t <= ML; ++t) {
    if (t == ML && b >= N) break;   // the last char is only selected
    if (t > 0) {
      if (b < N) { select(t - 1, pc, true); pc ^= 1; nsel = t; }
      if (t == ML) break;
      // ---- every workgroup reads the N W records of step t - 1: parents, input ids, "any slot live"
      if (w == 0) {
        pwait(flags, L + 1, 0, N, (unsigned)t, a.err);
        const int ln = lane_now();
        int par = -1, id = a.sos, live = 0;
        if (ln < NR) {
          const unsigned v = __builtin_amdgcn_raw_buffer_load_b32(xr, rc0 + (unsigned)(((size_t)(t - 1) * kNmax + ln) * kRec) * 4, 0, 0);
          const int p = (int)(v & 63u) - 1, c = (int)((v >> 6) & 1023u) - 1, s = (int)((v >> 16) & 3u);
          if (p >= 0 && p < W) par = (ln / W) * W + p;
          if (par >= 0 && s == kLive && c >= 0 && c < V) { id = c; live = 1; }
        }
        if (ln < kNmax) { spar[ln] = par; sid[ln] = id; }
        const unsigned long long lv = __ballot(live != 0);
        if (lane == 0) s_live = lv != 0ull;
      }
      __syncthreads();
      if (!s_live) break;   // every slot finished or dead: no model step is needed any more
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

  // ---- system b's outputs, in the layout Generator::conditional returns: one writer, its selecting workgroup
  if (b < N) {
    // after an early end the rule goes on without the model: finished slots can still be resampled
    for (int st = nsel; st < ML; ++st) { select(st, pc, false); pc ^= 1; }
    const int RL = ML + 1;
    for (int i = tid; i < W * RL; i += 512) {
      const int k = i / RL, c = i - k * RL;
      a.rows[((size_t)b * W + k) * RL + c] = sRows[pc][k][c];
    }
    if (w == 0) {
      if (lane < W) {
        a.logq[(size_t)b * W + lane] = sLogq[pc][lane];
        a.logw[(size_t)b * W + lane] = sLogw[pc][lane];
        a.n_tok[(size_t)b * W + lane] = sLen[pc][lane];
      }
      if (lane == 0) a.n_res[b] = s_nres;
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

// (KJ = H / 32, L) per vocabulary: gen_persist.hip's GP_VARIANTS at V = 256 and at V = 512.  The selection keeps
// one row's y and expf values per lane (the distinct launch: four slots' keys), so the three V = 512 shapes
// that spill there fit here -- with the slot loops of phases (a) and (c) rolled; unrolled, six instances
// spilled 8-52 bytes per lane.  Every instance listed has ScratchSize 0 in the
// -Rpass-analysis=kernel-resource-usage table (docs/DESIGN.md §4j holds it)
#define GPQ_VARIANTS_256(X) X(8, 1) X(8, 2) X(8, 3) X(8, 4) X(16, 1) X(16, 2) X(16, 3) X(16, 4) X(32, 1) X(32, 2)
#define GPQ_VARIANTS_512(X) X(8, 1) X(8, 2) X(8, 3) X(8, 4) X(16, 1) X(16, 2) X(16, 3) X(16, 4) X(32, 1) X(32, 2)

// resident workgroups of the variant on the whole device (0: no such variant, or a query failed)
static int gpq_resident(int KJ, int L, int PER) {
  int dev = 0, cus = 0, nb = 0;
  bool found = false;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
#define XP(K, LL, P)                                                                                               \
  if (KJ == K && L == LL) {                                                                                        \
    found = true;                                                                                                  \
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, gen_persist_smc_kernel<K, LL, P>, 512, 0) != hipSuccess) \
      return 0;                                                                                                    \
  }
#define X(K, LL) XP(K, LL, 4)
  if (PER == 4) { GPQ_VARIANTS_256(X) }
#undef X
#define X(K, LL) XP(K, LL, 8)
  if (PER == 8) { GPQ_VARIANTS_512(X) }
#undef X
#undef XP
  return found && cus >= kG ? cus * nb : 0;   // one workgroup per CU is the layout; fewer CUs: unsupported
}

bool gen_persist_smc_supported(int H, int L, int V, int N, int W, int ML) {
  if (N < 1 || W < 1 || W > kBW || (long)N * W > kNmax || L < 1 || L > 4 || H < 256 || H % 256 || (V != 256 && V != 512) ||
      ML < 1 || ML > kBML)
    return false;
  const int KJ = H / 32;
  if (KJ != 8 && KJ != 16 && KJ != 32) return false;
  return gpq_resident(KJ, L, V / 64) >= kG;
}

long gen_persist_smc_ws_floats(int H, int L, int V, int ML) { return ((long)L * kNmax * H + (long)kNmax * (V + kRec)) * ML; }
long gen_persist_smc_sync_words(int L) { return (long)(L + 2) * kG * kFS + 16; }

void gen_persist_smc_f32(const GenPersistSmcArgs& a, hipStream_t s) {
  if (!gen_persist_smc_supported(a.H, a.L, a.V, a.N, a.W, a.ML))
    throw std::runtime_error("gen_persist_smc_f32: unsupported shape or device (see gen_persist_smc_supported)");
  if (!a.ws || !a.sync || !a.err || !a.P || !a.Wfc || !a.bfc || !a.plen || !a.prefix || !a.inv_t || !a.rows || !a.logq ||
      !a.logw || !a.n_tok || !a.n_res)
    throw std::runtime_error("gen_persist_smc_f32: missing buffer");
  if (!(a.thr >= 0.f && a.thr <= 1.f)) throw std::runtime_error("gen_persist_smc_f32: needs 0 <= ess threshold <= 1");
  const bool aut = a.allow_next || a.allow_start;
  if (aut && (!a.allow_next || !a.allow_start || !a.allow_tab || a.allow_idx || a.allow_rows < 1 || a.allow_rows > 65535))
    throw std::runtime_error("gen_persist_smc_f32: an automaton needs allow_tab, allow_next and allow_start, no allow_idx "
                             "and 1 <= allow_rows <= 65535");
  if (!aut && ((a.allow_tab != nullptr) != (a.allow_idx != nullptr) || (a.allow_tab && a.allow_rows < 1)))
    throw std::runtime_error("gen_persist_smc_f32: constraints need allow_tab, allow_idx and allow_rows >= 1");
  for (int l = 0; l < a.L; ++l)
    if (!a.Whh[l] || !a.bhh[l] || (l > 0 && (!a.Wih[l] || !a.bih[l])))
      throw std::runtime_error("gen_persist_smc_f32: missing layer weights");
  if (a.sos < 0 || a.sos >= a.V || a.eos < 0)
    throw std::runtime_error("gen_persist_smc_f32: needs 0 <= sos < V and eos >= 0");
  const int KJ = a.H / 32;
#define XP(K, LL, P)                                                                                    \
  if (KJ == K && a.L == LL) {                                                                           \
    hipLaunchKernelGGL((gen_persist_smc_kernel<K, LL, P>), dim3(kG), dim3(512), 0, s, a);              \
    return;                                                                                             \
  }
#define X(K, LL) XP(K, LL, 4)
  if (a.V == 256) { GPQ_VARIANTS_256(X) }
#undef X
#define X(K, LL) XP(K, LL, 8)
  if (a.V == 512) { GPQ_VARIANTS_512(X) }
#undef X
#undef XP
  throw std::runtime_error("gen_persist_smc_f32: no variant");
}

}  // namespace gk

// Sequential Monte Carlo over the constrained sampler on the fp32 per-char path (Generator::conditional,
// docs/DESIGN.md §4j; the rule and the CPU twin: cpu_ref.sample_conditional / cpu_ref.smc_step, the
// per-element reference models/smc_ref.py).
//
// smc_select_f32 has sbs_select_f32's geometry (sbs.hip: one workgroup per name, a wave per slot row or two,
// V / 64 consecutive chars per lane) and three phases with LDS between them:
//   (a) wave w computes, for its slots b, y = x * inv_t, lse_all over the vocabulary and (max_A, sum_A, lse_A)
//       over the allowed set, logm_b = lse_A - lse_all (0 on a forced step and for a finished slot) and the
//       look-ahead weight u_b = logw_b + logm_b, and publishes them;
//   (b) after the barrier every thread derives the same ESS, the same decision and the same ancestors from
//       the at most 32 published values, in slot order;
//   (c) wave i reloads its ancestor's row, draws one char by the inverse CDF over the allowed set and lane 0
//       writes the new slot.
// Noise: Philox-4x32-10, key the seed, counter (slot i, step, the name's global index); word 0 is slot i's
// uniform, word 1 of slot 0's block the step's resampling uniform.  seed, start, the ESS threshold and 1 / T
// are read from device memory: one recording serves every value.  No global memory between the phases but
// the logits, no atomics but the error word, no cross-workgroup communication.
#include <cmath>
#include <stdexcept>
#include "kernels.h"
#include "common.h"
#include "gen_sample.h"

#pragma clang fp contract(off)

namespace gk {

namespace {
constexpr int kDead = 0, kLive = 1, kFin = 2;   // SmcSelectArgs::state values (BeamSelectArgs')
constexpr int kMaxWaves = 16;

DEV float smc_unit(unsigned word) { return (float)(2u * (word >> 9) + 1u) * 0x1p-24f; }   // exact, in [2^-24, 1 - 2^-24]
}  // namespace

// R: slot rows per wave (wave w owns slots w and w + nw), MAXPER: logits per lane and row
template <int R, int MAXPER, bool MASK, bool AUTO = false>
__global__ void __launch_bounds__(1024) smc_select_f32_kernel(SmcSelectArgs a) {
#pragma clang fp contract(off)
  __shared__ float s_u[32];      // the slots' look-ahead weights
  __shared__ float s_mxa[32];    // max_A y, sum_A expf(y - max_A y), lse_A
  __shared__ float s_sea[32];
  __shared__ float s_lsa[32];
  __shared__ int s_st[32];
  const int n = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int V = a.V, W = a.W, per = V / 64;
  const int pl = a.plen[n];
  const bool forced = a.step < pl;
  int fc = 0;
  if (forced) {
    fc = a.prefix[(size_t)n * a.max_len + a.step];
    if (fc >= V) {   // never expected (the host checks first): flag it instead of drawing it
      if (a.err && threadIdx.x == 0) {
        atomicOr(a.err, 16u);
        a.err[1] = (unsigned)fc;
        a.err[2] = (unsigned)(n * W);
      }
      fc = 0;
    }
  }
  unsigned okn = 0u;   // MASK without AUTO: bit e = this lane's char e is allowed (the name's line)
  if constexpr (MASK && !AUTO) {
    int ar = a.allow_idx[(size_t)n * a.max_len + a.step];
    if (ar < 0 || ar >= a.allow_rows) {   // never expected (the host builds both): flag it, no constraint
      if (a.err && threadIdx.x == 0) {
        atomicOr(a.err, 16u);
        a.err[1] = (unsigned)ar;
        a.err[2] = (unsigned)(n * W);
      }
      ar = 0;
    }
    okn = a.allow_tab[(size_t)ar * (V >> 5) + ((lane * per) >> 5)] >> ((lane * per) & 31);
  }
  const float inv_t = a.inv_t[n];
  // a row's scaled logits and its allowed bits (AUTO: the row's own state line)
  auto load_row = [&](size_t row, float (&y)[MAXPER], unsigned& ok, bool flag) {
    ok = okn;
    if constexpr (AUTO) {
      int q = a.allow_state_in[row];
      if (q < 0 || q >= a.allow_rows) {   // never expected (the host builds start and next): flag it, the free state
        if (flag && a.err && lane == 0) {
          atomicOr(a.err, 16u);
          a.err[1] = (unsigned)q;
          a.err[2] = (unsigned)row;
        }
        q = 0;
      }
      ok = a.allow_tab[(size_t)q * (V >> 5) + ((lane * per) >> 5)] >> ((lane * per) & 31);
    }
    const float* x = a.logits + row * V + lane * per;
#pragma unroll
    for (int e = 0; e < MAXPER; ++e) {
      if (e < per) {
        float v = x[e];
        for (int s2 = 1; s2 < a.splits; ++s2) v += x[s2 * a.slab + e];   // split-K slabs, fixed order
        if (a.bias) v += a.bias[lane * per + e];
        y[e] = v * inv_t;
      } else {
        y[e] = -INFINITY;
      }
    }
  };
  // ---- (a) the slots' masses and look-ahead weights
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int b = w + r * nw;
    if (b >= W) continue;
    const size_t row = (size_t)n * W + b;
    const int st = a.state_in[row];
    float y[MAXPER];
    unsigned ok;
    load_row(row, y, ok, true);
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < MAXPER; ++e) mx = fmaxf(mx, y[e]);
    mx = wave_max_dpp(mx);
    float se = 0.f;
#pragma unroll
    for (int e = 0; e < MAXPER; ++e) se += e < per ? expf(y[e] - mx) : 0.f;
    se = wave_sum_dpp(se);
    const float lse_all = mx + logf(se);
    float mxa = mx, sea = se, lsa = lse_all;   // no constraint: the very same values
    if constexpr (MASK) {
      mxa = -INFINITY;
#pragma unroll
      for (int e = 0; e < MAXPER; ++e) mxa = fmaxf(mxa, (e < per && ((ok >> e) & 1u)) ? y[e] : -INFINITY);
      mxa = wave_max_dpp(mxa);
      sea = 0.f;
#pragma unroll
      for (int e = 0; e < MAXPER; ++e) sea += (e < per && ((ok >> e) & 1u)) ? expf(y[e] - mxa) : 0.f;
      sea = wave_sum_dpp(sea);
      lsa = mxa + logf(sea);
    }
    const float logm = (st == kLive && !forced) ? lsa - lse_all : 0.f;
    const float u = a.logw_in[row] + logm;
    if (a.logm && lane == 0) a.logm[row] = st == kDead ? NAN : logm;
    if (a.lq) {
#pragma unroll
      for (int e = 0; e < MAXPER; ++e)
        if (e < per) a.lq[row * V + lane * per + e] = (st == kLive && (!MASK || ((ok >> e) & 1u))) ? y[e] - lsa : NAN;
    }
    if (lane == 0) { s_u[b] = u; s_mxa[b] = mxa; s_sea[b] = sea; s_lsa[b] = lsa; s_st[b] = st; }
  }
  __syncthreads();
  // ---- (b) ESS, the decision and the ancestors: every thread the same arithmetic, in slot order
  float mu = -INFINITY;
  int last = 0;   // the last slot that is not dead
  for (int b = 0; b < W; ++b)
    if (s_st[b] != kDead) { mu = fmaxf(mu, s_u[b]); last = b; }
  float S = 0.f, Q = 0.f;
  for (int b = 0; b < W; ++b)
    if (s_st[b] != kDead) {
      const float e = expf(s_u[b] - mu);
      S += e;
      Q += e * e;
    }
  const float ess = (S * S) / Q;
  const float thr = *a.thr;
  const bool fan = a.step == 0;
  const bool res = !fan && ess < thr * (float)W;
  float U = 0.f;
  const unsigned long long seed = *a.seed, gidx = *a.start + (unsigned long long)n;
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32), g0 = (unsigned)gidx, g1 = (unsigned)(gidx >> 32);
  if (res) {
    unsigned wd[4];
    philox4x32_10(0u, (unsigned)a.step, g0, g1, k0, k1, wd);
    U = smc_unit(wd[1]);
  }
  if (threadIdx.x == 0) {
    if (a.ess) a.ess[n] = ess;
    if (a.n_res) a.n_res[n] = (fan ? 0 : a.n_res[n]) + (res ? 1 : 0);
  }
  // ---- (c) new slot i: its ancestor, its weight, its char
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = w + r * nw;
    if (i >= W) continue;
    int anc = i;
    float lw;
    if (fan) {
      anc = 0;
      lw = s_u[0];
    } else if (res) {
      const float t = ((float)i + U) / (float)W * S;
      float cum = 0.f;
      anc = -1;
      for (int b = 0; b < W; ++b)
        if (s_st[b] != kDead) {
          cum += expf(s_u[b] - mu);
          if (anc < 0 && cum > t) anc = b;
        }
      if (anc < 0) anc = last;
      lw = mu + logf(S / (float)W);
    } else {
      lw = s_u[i];
    }
    const size_t o = (size_t)n * W + i, prow = (size_t)n * W + anc;
    const int ast = s_st[anc];
    float lq = -INFINITY;
    int parent = -1, ch = -1, st = kDead, nxt = a.sos, qn = 0;
    if (ast == kFin) {          // carried: row, length and logq unchanged
      parent = anc; st = kFin; lq = a.logq_in[prow];
    } else if (ast == kLive) {
      parent = anc;
      float dl = 0.f;
      if (forced) {
        ch = fc;
      } else {
        float y[MAXPER];
        unsigned ok;
        load_row(prow, y, ok, false);
        const float mxa = s_mxa[anc], sea = s_sea[anc];
        unsigned wd[4];
        philox4x32_10((unsigned)i, (unsigned)a.step, g0, g1, k0, k1, wd);
        const float target = smc_unit(wd[0]) * sea;
        float ex[MAXPER];
        float loc = 0.f;
#pragma unroll
        for (int e = 0; e < MAXPER; ++e) {
          ex[e] = (e < per && (!MASK || ((ok >> e) & 1u))) ? expf(y[e] - mxa) : 0.f;
          loc += ex[e];
        }
        float run = wave_scan_incl_dpp(loc) - loc;
        int hit = V, top = -1;   // the first allowed char whose running sum exceeds the target; the last allowed char
#pragma unroll
        for (int e = 0; e < MAXPER; ++e) {
          run += ex[e];
          const bool al = e < per && (!MASK || ((ok >> e) & 1u));
          if (al) top = lane * per + e;
          if (al && hit == V && run > target) hit = lane * per + e;
        }
        hit = wave_min_dpp(hit);
        top = -wave_min_dpp(-top);
        ch = hit < V ? hit : (top >= 0 ? top : V - 1);
        const int e = ch - lane * per;   // the owner lane's y[ch] to every lane
        float yc = -INFINITY;
#pragma unroll
        for (int ee = 0; ee < MAXPER; ++ee)
          if (ee == e) yc = y[ee];
        yc = wave_max_dpp(yc);
        dl = yc - s_lsa[anc];
      }
      lq = a.logq_in[prow] + dl;
      st = ch == a.eos ? kFin : kLive;
      if (st == kLive) nxt = ch;
      if constexpr (AUTO) {
        int q = a.allow_state_in[prow];
        if (q < 0 || q >= a.allow_rows) q = 0;   // (flagged above)
        qn = a.allow_next[(size_t)q * V + ch];
      }
    } else {
      lw = -INFINITY;
    }
    if (lane == 0) {
      a.logw_out[o] = lw; a.logq_out[o] = lq; a.parent[o] = parent; a.chr[o] = ch; a.state_out[o] = st; a.next_id[o] = nxt;
      if constexpr (AUTO) a.allow_state_out[o] = qn;
    }
  }
}

// seed, start and the ESS threshold into their device words, from kernel arguments: stream-ordered
__global__ void smc_stage_kernel(unsigned long long* words, unsigned long long seed_v, unsigned long long start_v, float thr_v) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    words[0] = seed_v;
    words[1] = start_v;
    *reinterpret_cast<float*>(words + 2) = thr_v;
  }
}

void smc_stage(unsigned long long* words, unsigned long long seed_v, unsigned long long start_v, float thr_v, hipStream_t s) {
  if (!words) throw std::runtime_error("smc_stage: the three words are required");
  hipLaunchKernelGGL(smc_stage_kernel, dim3(1), dim3(64), 0, s, words, seed_v, start_v, thr_v);
}

void smc_select_f32(const SmcSelectArgs& a, hipStream_t s) {
  if (a.V % 64 || a.V > 512 || a.V <= 0) throw std::runtime_error("smc_select_f32: needs V % 64 == 0 and V <= 512");
  if (a.W < 1 || a.W > 32 || a.W > a.V) throw std::runtime_error("smc_select_f32: needs 1 <= W <= min(32, V)");
  if (!a.logits || !a.logw_in || !a.logq_in || !a.state_in || !a.plen || !a.prefix || !a.logw_out || !a.logq_out ||
      !a.parent || !a.chr || !a.state_out || !a.next_id || !a.seed || !a.start || !a.thr || !a.inv_t)
    throw std::runtime_error("smc_select_f32: logits, logw, logq, states, plen, prefix, seed, start, thr, inv_t and the six "
                             "outputs are required");
  if (a.logw_in == a.logw_out || a.logq_in == a.logq_out || a.logw_in == a.logq_out || a.logq_in == a.logw_out ||
      a.logw_out == a.logq_out || a.state_in == a.state_out)
    throw std::runtime_error("smc_select_f32: the new slots' logw, logq and states never overwrite the inputs");
  if (a.step < 0 || a.step >= a.max_len || a.eos < 0 || a.sos < 0 || a.sos >= a.V)
    throw std::runtime_error("smc_select_f32: needs 0 <= step < max_len, eos >= 0 and 0 <= sos < V");
  if (a.splits < 1 || (a.splits > 1 && a.slab < (long)a.N * a.W * a.V))
    throw std::runtime_error("smc_select_f32: split-K slabs overlap");
  const bool aut = a.allow_state_in || a.allow_state_out || a.allow_next;
  if (aut && (!a.allow_state_in || !a.allow_state_out || !a.allow_next || !a.allow_tab || a.allow_idx ||
              a.allow_state_in == a.allow_state_out || a.allow_rows > 65535 || (a.V != 256 && a.V != 512)))
    throw std::runtime_error("smc_select_f32: an automaton needs allow_state_in, allow_state_out (another buffer), "
                             "allow_next and allow_tab, no allow_idx, at most 65535 states and V = 256 or 512");
  if (!aut && (a.allow_tab != nullptr) != (a.allow_idx != nullptr))
    throw std::runtime_error("smc_select_f32: allow_tab and allow_idx are set together or not at all");
  const bool mask = a.allow_tab != nullptr;
  if (mask && (a.allow_rows < 1 || 32 % (a.V / 64)))
    throw std::runtime_error("smc_select_f32: constraints need allow_rows >= 1 and V / 64 in {1, 2, 4, 8}");
  if (a.N <= 0) return;
  const int nw = a.W <= kMaxWaves ? a.W : kMaxWaves;
  const dim3 grid(a.N), block(64 * nw);
  if (aut) {
    if (a.W <= kMaxWaves) {
      if (a.V <= 256) hipLaunchKernelGGL((smc_select_f32_kernel<1, 4, true, true>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((smc_select_f32_kernel<1, 8, true, true>), grid, block, 0, s, a);
    } else {
      if (a.V <= 256) hipLaunchKernelGGL((smc_select_f32_kernel<2, 4, true, true>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((smc_select_f32_kernel<2, 8, true, true>), grid, block, 0, s, a);
    }
  } else if (mask) {
    if (a.W <= kMaxWaves) {
      if (a.V <= 256) hipLaunchKernelGGL((smc_select_f32_kernel<1, 4, true>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((smc_select_f32_kernel<1, 8, true>), grid, block, 0, s, a);
    } else {
      if (a.V <= 256) hipLaunchKernelGGL((smc_select_f32_kernel<2, 4, true>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((smc_select_f32_kernel<2, 8, true>), grid, block, 0, s, a);
    }
  } else if (a.W <= kMaxWaves) {
    if (a.V <= 256) hipLaunchKernelGGL((smc_select_f32_kernel<1, 4, false>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((smc_select_f32_kernel<1, 8, false>), grid, block, 0, s, a);
  } else {
    if (a.V <= 256) hipLaunchKernelGGL((smc_select_f32_kernel<2, 4, false>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((smc_select_f32_kernel<2, 8, false>), grid, block, 0, s, a);
  }
}

}  // namespace gk

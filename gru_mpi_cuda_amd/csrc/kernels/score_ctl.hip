// Scoring under the sampler (Generator::score with controls, docs/DESIGN.md §4f; the CPU twin and oracle
// is cpu_ref.score with its keywords): how likely is a row under the tempered, top-k / top-p cut,
// prefix-forced and per-position masked distribution that sample_ctl_f32 draws from.
//
// score_logprob_f32's shape: one wave per name walks its n_tok logits rows in step order, a lane owns
// V/64 consecutive logits, split-K slabs are summed in slab order and the bias is added after the sum;
// the cross-lane steps are the fixed-order DPP / readlane helpers of gen_sample.h.  No LDS, no atomics
// on the results, no sort.  The name's four scalar controls are read once before the loop.
//
// The kept set is found as in sample_ctl_f32_kernel (gen_ctl.hip): the 32-probe bisection over the
// order-preserving key for top-k, the 30-probe bisection over the bits of q for top-p, both branched
// around when they are off, contraction off so that y = x * (1 / T) is rounded as defined.  This is the
// third copy of that rule (gen_ctl.hip, gen_sample_ctl.h: ctl_sample_wave): a change to one belongs in
// the others (tests/test_score_ctl_gpu.py holds this one).  With nothing filtered every statistic is
// formed by the operations of score_logprob_f32_kernel in its order, so neutral controls give its bytes.
//
// Soft controls (docs/DESIGN.md §4h, the SOFT instantiations; gen_ctl.hip's and this copy only, the
// persistent sampler has none): the name's bias line and two penalties are read once before the loop, and
// the counts n[c] of the scored row's bytes before position l are kept per lane as the loop advances (the
// targets are the row's bytes).  v = (x + bias) - pen takes x's place in the kept-set rule; rank stays
// the model's, on the raw logits.  SOFT = false is the kernel as it was.
#include <cmath>
#include <stdexcept>
#include "kernels.h"
#include "common.h"
#include "gen_sample.h"

namespace gk {

// floats -> unsigned keys with the same order (-0 and +0 share a key); gen_ctl.hip: order_key
DEV unsigned score_order_key(float f) {
  unsigned b = __float_as_uint(f);
  if (b == 0x80000000u) b = 0u;
  return (b >> 31) ? ~b : (b | 0x80000000u);
}

// One wave per name (block b of Bp): rows b >= N have n_tok = 0, read no control and only write their
// masked outputs.
template <int MAXPER, bool MASK, bool SOFT = false>
__global__ void __launch_bounds__(64) score_ctl_logprob_f32_kernel(ScoreCtlArgs c) {
#pragma clang fp contract(off)
  const ScoreLogprobArgs& a = c.s;
  const int b = blockIdx.x, lane = threadIdx.x, V = a.V, per = V / 64, ML = a.ML;
  const int nt = min(max(__builtin_amdgcn_readfirstlane(a.ntok[b]), 0), ML);
  const int cb = b + c.row0;   // this name's controls
  float it = 1.f, tp = 1.f;
  int k = 0, pl = 0;
  if (nt > 0) {
    it = c.inv_temp[cb];   // 0: greedy
    k = c.top_k[cb];
    tp = c.top_p[cb];
    pl = c.plen[cb];
  }
  const float scale = it == 0.f ? 1.f : it;
  float sbias[SOFT ? MAXPER : 1];   // SOFT: this lane's biases, the name's penalties and the counts so far
  int scnt[SOFT ? MAXPER : 1];
  float pres = 0.f, freq = 0.f;
  if constexpr (SOFT) {
#pragma unroll
    for (int e = 0; e < MAXPER; ++e) {
      sbias[e] = 0.f;
      scnt[e] = 0;
    }
    if (nt > 0) {
      int sr = c.soft_idx[cb];
      if (sr < 0 || sr >= c.soft_rows) {   // never expected (the host builds both): flag it, no bias
        if (c.err && lane == 0) {
          atomicOr(c.err, 16u);
          c.err[1] = (unsigned)sr;
          c.err[2] = (unsigned)b;
        }
        sr = 0;
      }
      const float* brow = c.soft_tab + (size_t)sr * V + lane * per;
#pragma unroll
      for (int e = 0; e < MAXPER; ++e)
        if (e < per) sbias[e] = brow[e];
      pres = c.soft_pres[cb];
      freq = c.soft_freq[cb];
    }
  }
  float sum = 0.f;
  for (int l = 0; l < nt; ++l) {
    const size_t row = (size_t)l * a.Bp + b;
    int t = __builtin_amdgcn_readfirstlane(a.tgt[row]);
    t = min(max(t, 0), V - 1);
    const float* x = a.logits + row * V + lane * per;
    float xv[MAXPER];
#pragma unroll
    for (int e = 0; e < MAXPER; ++e) {
      if (e < per) {
        float v = x[e];
        for (int s2 = 1; s2 < a.splits; ++s2) v += x[s2 * a.slab + e];   // split-K slabs, fixed order
        if (a.bias) v += a.bias[lane * per + e];
        xv[e] = v;
      } else {
        xv[e] = -INFINITY;
      }
    }
    // the target's logit from the lane that owns it, and the model's rank of it: raw logits, unmasked
    const int tl = t / per, te = t - tl * per;
    float cand = 0.f;
#pragma unroll
    for (int e = 0; e < MAXPER; ++e) cand = e == te ? xv[e] : cand;
    const float xt = rdl(cand, tl);
    int rank = 0;
#pragma unroll
    for (int e = 0; e < MAXPER; ++e) {
      const int j = lane * per + e;
      const bool above = e < per && (xv[e] > xt || (xv[e] == xt && j < t));
      rank += __builtin_popcountll(__ballot(above));
    }
    float lp;
    int nk = 1;
    if (l < pl) {   // forced: the sampler writes the prefix byte whatever the logits are
      lp = t == (int)c.prefix[(size_t)cb * ML + l] ? 0.f : -INFINITY;
    } else {
      unsigned ok = 0u;   // MASK: bit e = this lane's char e is allowed
      if constexpr (MASK) {
        int ar = c.allow_idx[(size_t)cb * ML + l];
        if (ar < 0 || ar >= c.allow_rows) {   // never expected (the host builds both): flag it, no constraint
          if (c.err && lane == 0) {
            atomicOr(c.err, 16u);
            c.err[1] = (unsigned)ar;
            c.err[2] = (unsigned)b;
          }
          ar = 0;
        }
        ok = c.allow_tab[(size_t)ar * (V >> 5) + ((lane * per) >> 5)] >> ((lane * per) & 31);
      }
      float y[MAXPER];
      float mx = -INFINITY;
#pragma unroll
      for (int e = 0; e < MAXPER; ++e) {
        float v = xv[e];
        if constexpr (SOFT) {
          float pn = freq * (float)scnt[e];
          if (scnt[e] > 0) pn = pn + pres;
          v = (v + sbias[e]) - pn;
        }
        y[e] = e < per ? v * scale : -INFINITY;
        if constexpr (MASK)
          if (!((ok >> e) & 1u)) y[e] = -INFINITY;
        mx = fmaxf(mx, y[e]);
      }
      mx = wave_max_dpp(mx);
      if (it == 0.f) {   // greedy: the lowest index of the maximum
        int first = V;
#pragma unroll
        for (int e = MAXPER - 1; e >= 0; --e)
          if (e < per && y[e] == mx && (!MASK || ((ok >> e) & 1u))) first = lane * per + e;
        int sel = wave_min_dpp(first);
        if (sel >= V) sel = V - 1;   // (only a row of NaNs gets here)
        lp = t == sel ? 0.f : -INFINITY;
      } else {
        bool keep[MAXPER];
#pragma unroll
        for (int e = 0; e < MAXPER; ++e) keep[e] = e < per && (!MASK || ((ok >> e) & 1u));
        if (k > 0 && k < V) {   // th = key of the k-th largest value: the largest th with #{key >= th} >= k
          unsigned key[MAXPER];
#pragma unroll
          for (int e = 0; e < MAXPER; ++e) key[e] = score_order_key(y[e]);
          unsigned th = 0u;
          for (int bit = 31; bit >= 0; --bit) {
            const unsigned cd = th | (1u << bit);
            int cnt = 0;
#pragma unroll
            for (int e = 0; e < MAXPER; ++e) cnt += __popcll(__ballot(keep[e] && key[e] >= cd));
            if (cnt >= k) th = cd;
          }
#pragma unroll
          for (int e = 0; e < MAXPER; ++e) keep[e] = keep[e] && key[e] >= th;
        }
        float ex[MAXPER];
        float se = 0.f;
#pragma unroll
        for (int e = 0; e < MAXPER; ++e) {
          ex[e] = keep[e] ? expf(y[e] - mx) : 0.f;
          se += ex[e];
        }
        se = wave_sum_dpp(se);
        if (tp < 1.f) {
          float q[MAXPER];
#pragma unroll
          for (int e = 0; e < MAXPER; ++e) q[e] = ex[e] / se;
          // above(u) = the mass of the q_j whose bits exceed u; P(u) = above(u) < p is monotone in u.
          // lo = the smallest u with P(u): i is kept iff bits(q_i) >= lo
          auto above = [&](unsigned u) {
            float sacc = 0.f;
#pragma unroll
            for (int e = 0; e < MAXPER; ++e) sacc += __float_as_uint(q[e]) > u ? q[e] : 0.f;
            return wave_sum_dpp(sacc);
          };
          unsigned lo = 0u;
          if (!(above(0u) < tp)) {
            unsigned u = 0u;   // the largest u with P(u) false; P(bits(1.0f)) holds, so u < 2^30
            for (int bit = 29; bit >= 0; --bit) {
              const unsigned cd = u | (1u << bit);
              if (!(above(cd) < tp)) u = cd;
            }
            lo = u + 1u;
          }
          se = 0.f;
#pragma unroll
          for (int e = 0; e < MAXPER; ++e) {
            keep[e] = keep[e] && __float_as_uint(q[e]) >= lo;
            ex[e] = keep[e] ? ex[e] : 0.f;
            se += ex[e];
          }
          se = wave_sum_dpp(se);
        }
        nk = 0;
#pragma unroll
        for (int e = 0; e < MAXPER; ++e) nk += __popcll(__ballot(keep[e]));
        // membership and y_t from the target's owner lane (mx = the maximum over K: the maximum of the
        // allowed set survives both cuts)
        float yc = 0.f;
        int kc = 0;
#pragma unroll
        for (int e = 0; e < MAXPER; ++e) {
          yc = e == te ? y[e] : yc;
          kc = e == te ? (int)keep[e] : kc;
        }
        const float yt = rdl(yc, tl);
        const int kt = __builtin_amdgcn_readlane(kc, tl);
        lp = kt ? (yt - mx) - logf(se) : -INFINITY;
      }
    }
    if constexpr (SOFT) {   // the row's byte at l joins the counts of the later positions (a forced one too)
#pragma unroll
      for (int e = 0; e < MAXPER; ++e) scnt[e] += (e < per && lane * per + e == t) ? 1 : 0;
    }
    sum += lp;   // step order, the same value in every lane; -inf stays -inf (no +inf ever joins it)
    if (lane == 0) {
      a.tok_logp[(size_t)b * ML + l] = lp;
      a.rank[(size_t)b * ML + l] = rank;
      c.n_kept[(size_t)b * ML + l] = nk;
    }
  }
  if (lane < ML - nt) {   // masked positions (ML <= 64, checked by the launcher)
    a.tok_logp[(size_t)b * ML + nt + lane] = 0.f;
    a.rank[(size_t)b * ML + nt + lane] = -1;
    c.n_kept[(size_t)b * ML + nt + lane] = -1;
  }
  if (lane == 0) {
    a.name_logp[b] = sum;
    a.ntok_out[b] = nt;
  }
}

void score_ctl_logprob_f32(const ScoreCtlArgs& c, hipStream_t s) {
  const ScoreLogprobArgs& a = c.s;
  if (a.V % 64 || a.V > 512 || a.V <= 0) throw std::runtime_error("score_ctl_logprob_f32: needs V % 64 == 0 and V <= 512");
  if (a.ML <= 0 || a.ML > 64) throw std::runtime_error("score_ctl_logprob_f32: needs 0 < max_len <= 64");
  if (a.splits < 1 || (a.splits > 1 && a.slab < (long)a.ML * a.Bp * a.V))
    throw std::runtime_error("score_ctl_logprob_f32: split-K slabs overlap");
  if (!c.inv_temp || !c.top_k || !c.top_p || !c.plen || !c.prefix || !c.n_kept || c.row0 < 0)
    throw std::runtime_error("score_ctl_logprob_f32: inv_temp, top_k, top_p, plen, prefix and n_kept are required");
  if ((c.allow_tab != nullptr) != (c.allow_idx != nullptr))
    throw std::runtime_error("score_ctl_logprob_f32: allow_tab and allow_idx are set together or not at all");
  const bool mask = c.allow_tab != nullptr;
  if (mask && (c.allow_rows < 1 || 32 % (a.V / 64)))
    throw std::runtime_error("score_ctl_logprob_f32: constraints need allow_rows >= 1 and V / 64 in {1, 2, 4, 8}");
  const bool soft = c.soft_tab != nullptr;
  if (soft != (c.soft_idx != nullptr) || soft != (c.soft_pres != nullptr) || soft != (c.soft_freq != nullptr) ||
      (soft && c.soft_rows < 1))
    throw std::runtime_error("score_ctl_logprob_f32: soft_tab, soft_idx, soft_pres and soft_freq are set together, with soft_rows >= 1");
  if (a.Bp <= 0) return;
  const dim3 grid(a.Bp), block(64);
  if (soft) {   // the SOFT instantiations; every other call launches what it launched before
    if (a.V <= 256) {
      if (mask) hipLaunchKernelGGL((score_ctl_logprob_f32_kernel<4, true, true>), grid, block, 0, s, c);
      else hipLaunchKernelGGL((score_ctl_logprob_f32_kernel<4, false, true>), grid, block, 0, s, c);
    } else {
      if (mask) hipLaunchKernelGGL((score_ctl_logprob_f32_kernel<8, true, true>), grid, block, 0, s, c);
      else hipLaunchKernelGGL((score_ctl_logprob_f32_kernel<8, false, true>), grid, block, 0, s, c);
    }
    return;
  }
  if (a.V <= 256) {
    if (mask) hipLaunchKernelGGL((score_ctl_logprob_f32_kernel<4, true>), grid, block, 0, s, c);
    else hipLaunchKernelGGL((score_ctl_logprob_f32_kernel<4, false>), grid, block, 0, s, c);
  } else {
    if (mask) hipLaunchKernelGGL((score_ctl_logprob_f32_kernel<8, true>), grid, block, 0, s, c);
    else hipLaunchKernelGGL((score_ctl_logprob_f32_kernel<8, false>), grid, block, 0, s, c);
  }
}

}  // namespace gk

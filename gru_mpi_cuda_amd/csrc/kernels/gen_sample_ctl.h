// The controlled sampling rule (docs/DESIGN.md §4b steps 1-7: forced prefix char, greedy,
// temperature, top-k, top-p, renormalise, `psum > r`) for one row held by one wave, PER = V / 64
// values per lane: the sampler of the persistent generator's controlled variants (gen_persist_ctl.hip).
//
// It is the rule of sample_ctl_f32_kernel (gen_ctl.hip), which stays the per-char graph's sampler: the
// two copies sit side by side, and a change to the kept-set rule of one belongs in the other (and in the
// scorer's copy of it, score_ctl_logprob_f32_kernel in score_ctl.hip).  The soft terms (logit bias,
// presence and frequency penalties, docs/DESIGN.md §4h) are not in this function: they replace the logits
// before the temperature scale, so the persistent generator's soft variants (SOFT in gen_persist_kernel.h,
// the third copy of that rule) adjust y[] just before the call, where a lane's bias and count values are
// dead again before this function's own registers go live.  This one is written for a
// kernel whose weights fill the register file: it keeps only y[PER] live (plus q[PER] during the top-p
// search) where gen_ctl.hip keeps key[] / ex[] / keep[] as well.  A filtered entry is marked by
// y = -inf, so its expf(y - mx) is exactly the 0 that gen_ctl.hip selects, and every expf / key is
// recomputed where it is used: the same values in the same order, hence the same bits.  (A logit that
// is -inf by itself counts as filtered; finite logits never get there.)
//
// With nothing filtered every statistic is formed by the operations of softmax_sample_wave in its
// order, so neutral controls give the plain sampler's bytes.
#pragma once
#include "gen_sample.h"

namespace gk {

// floats -> unsigned keys with the same order (-0 and +0 share a key); gen_ctl.hip: order_key
DEV unsigned ctl_order_key(float f) {
  unsigned b = __float_as_uint(f);
  if (b == 0x80000000u) b = 0u;
  return (b >> 31) ? ~b : (b | 0x80000000u);
}

// one-hot row of a forced or greedy char
template <int PER>
DEV void ctl_one_hot(float* prow, int sel) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int e = 0; e < PER; ++e) prow[lane * PER + e] = (lane * PER + e == sel) ? 1.f : 0.f;
}

// y[e]: logits V[lane * PER + e] on entry (overwritten).  The controls are wave-uniform: inv_temp
// (0: greedy), top_k (<= 0 or >= V: off), top_p (>= 1: off), forced (>= 0: this char, nothing else is
// looked at).  Returns the chosen index, identical in every lane; prow (nullable) gets the
// renormalised filtered row, one-hot for a forced or greedy char.
//
// MASKED (the constrained variants, gen_persist_con.hip; docs/DESIGN.md §4e / §4g): bit e of `ok` = char
// lane * PER + e is in the row's set.  An entry outside it is -inf after the temperature scale, so it is
// filtered like any other; and, as in gen_ctl.hip's MASK instantiations, only a kept char is a hit of
// the CDF search (a lane past the last kept char can hold a running sum one ulp above an earlier
// lane's).  A forced step does not look at `ok`.  MASKED = false is the sampler as it was.
template <int PER, bool MASKED = false>
DEV int ctl_sample_wave(float (&y)[PER], int V, float rnd, float* prow, float inv_temp, int top_k, float top_p,
                        int forced, unsigned ok = 0u) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  if (forced >= 0) {   // the uniform of this step is ignored
    if (prow) ctl_one_hot<PER>(prow, forced);
    return forced;
  }
  const float scale = inv_temp == 0.f ? 1.f : inv_temp;
  float mx = -INFINITY;
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    y[e] = y[e] * scale;
    if constexpr (MASKED)
      if (!((ok >> e) & 1u)) y[e] = -INFINITY;
    mx = fmaxf(mx, y[e]);
  }
  mx = wave_max_dpp(mx);
  if (inv_temp == 0.f) {   // greedy: the lowest index of the maximum
    int first = V;
#pragma unroll
    for (int e = PER - 1; e >= 0; --e)
      if (y[e] == mx) first = lane * PER + e;
    int sel = wave_min_dpp(first);
    if (sel >= V) sel = V - 1;   // (only a row of NaNs gets here)
    if (prow) ctl_one_hot<PER>(prow, sel);
    return sel;
  }
  if (top_k > 0 && top_k < V) {   // t = key of the k-th largest value: the largest t with #{key >= t} >= k
    unsigned t = 0u;
    for (int bit = 31; bit >= 0; --bit) {
      const unsigned cand = t | (1u << bit);
      int cnt = 0;
#pragma unroll
      for (int e = 0; e < PER; ++e) cnt += __popcll(__ballot(ctl_order_key(y[e]) >= cand));
      if (cnt >= top_k) t = cand;
    }
#pragma unroll
    for (int e = 0; e < PER; ++e) y[e] = ctl_order_key(y[e]) >= t ? y[e] : -INFINITY;
  }
  auto mass = [&]() {   // sum of expf(y - mx) over the kept set, in softmax_sample_wave's order
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < PER; ++e) s += expf(y[e] - mx);
    return wave_sum_dpp(s);
  };
  float se = mass();
  if (top_p < 1.f) {
    float q[PER];
#pragma unroll
    for (int e = 0; e < PER; ++e) q[e] = expf(y[e] - mx) / se;
    // above(u) = the mass of the q_j whose bits exceed u; P(u) = above(u) < p is monotone in u.
    // lo = the smallest u with P(u): i is kept iff bits(q_i) >= lo
    auto above = [&](unsigned u) {
      float sacc = 0.f;
#pragma unroll
      for (int e = 0; e < PER; ++e) sacc += __float_as_uint(q[e]) > u ? q[e] : 0.f;
      return wave_sum_dpp(sacc);
    };
    unsigned lo = 0u;
    if (!(above(0u) < top_p)) {
      unsigned u = 0u;   // the largest u with P(u) false; P(bits(1.0f)) holds, so u < 2^30
      for (int bit = 29; bit >= 0; --bit) {
        const unsigned cand = u | (1u << bit);
        if (!(above(cand) < top_p)) u = cand;
      }
      lo = u + 1u;
    }
#pragma unroll
    for (int e = 0; e < PER; ++e) y[e] = __float_as_uint(q[e]) >= lo ? y[e] : -INFINITY;
    se = mass();
  }
  // renormalised distribution over the kept set, then softmax_sample_wave's CDF search
  float p[PER];
  float loc = 0.f;
  int last = -1;
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    p[e] = expf(y[e] - mx) / se;
    loc += p[e];
    if (y[e] != -INFINITY) last = lane * PER + e;
    if (prow) prow[lane * PER + e] = p[e];
  }
  const float inc = wave_scan_incl_dpp(loc);
  float psum = inc - loc;
  int hit = V;
#pragma unroll
  for (int e = 0; e < PER; ++e) {
    psum += p[e];
    if (hit == V && psum > rnd && (!MASKED || y[e] != -INFINITY)) hit = lane * PER + e;
  }
  hit = wave_min_dpp(hit);
  last = -wave_min_dpp(-last);   // the highest kept index (V - 1 with nothing filtered)
  return hit >= V ? (last < 0 ? V - 1 : last) : hit;
}

}  // namespace gk

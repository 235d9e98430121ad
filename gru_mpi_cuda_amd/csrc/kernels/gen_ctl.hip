// Controlled sampling for the fp32 / bf16x3 per-char generation graph: forced prefix chars, greedy,
// temperature, top-k and top-p (docs/DESIGN.md §4b; the CPU twin and oracle is
// cpu_ref.sample_controlled).  One wave per row like sample_f32_kernel, the same logits / slab / bias
// inputs and the same ids / out / alive outputs; the per-row controls are read from device memory,
// so a captured graph bakes no control value in.
//
// Both cuts are pure set definitions and need neither a sort nor LDS:
//   * top-k keeps i iff #{j : y_j > y_i} < k, i.e. y_i >= the k-th largest value.  That value is
//     found by a 32-step bisection over an order-preserving integer key of the floats; a probe is
//     V/64 compares per lane plus a ballot popcount;
//   * top-p keeps i iff sum{q_j : q_j > q_i} < p.  A fixed-order fp32 sum of non-negative terms is
//     monotone when terms are replaced by 0, so "the mass above a threshold is < p" is monotone in
//     the threshold and the smallest passing threshold is found by the same bisection over the bits
//     of the non-negative q (30 steps: q <= 1), a fixed-order wave sum per probe.
// With nothing filtered every statistic is formed by the operations of softmax_sample_wave in its
// order, so neutral controls give the plain sampler's bytes.
//
// The persistent generator's controlled variants carry a second copy of this rule, ctl_sample_wave
// (gen_sample_ctl.h), written for a kernel with no registers to spare: a change to the kept-set rule in
// one belongs in the other (tests/test_sampling_ctl_gpu.py holds this one,
// tests/test_gen_persist_ctl_gpu.py that).  A third copy scores rows under this distribution:
// score_ctl_logprob_f32_kernel (score_ctl.hip, tests/test_score_ctl_gpu.py).
// The soft terms below (SOFT) have three copies: this one, the scoring one, and the persistent
// generator's soft variants (SOFT in gen_persist_kernel.h, opt-in: docs/DESIGN.md §4h), which adjust the
// logits just before ctl_sample_wave and count a name's history in LDS instead of its output row.
// ctl_sample_wave itself is unchanged.  A change to v's formula or to what n[c] counts belongs in all
// three (tests/test_soft_ctl_gpu.py holds this one, tests/test_gen_persist_soft_gpu.py that).
//
// Constraints (docs/DESIGN.md §4e, the MASK instantiations; the persistent copy's: MASKED, gen_sample_ctl.h): a row's
// allowed chars at this step are one line of a bit table.  A lane's V/64 consecutive chars lie in one
// 32-bit word of that line -- one load per lane and row -- and a masked char takes y = -inf after the
// temperature scale and is in no kept set.  MASK = false is the kernel as it was.
//
// Automaton (docs/DESIGN.md §4g, the AUTO instantiations, always with MASK): the line index is not a
// function of the step but a per-row state in device memory.  Every lane reads it (one uniform 4-byte
// load), and once the char is known lane 0 stores the successor, a 2-byte load from allow_next -- on a
// forced step too, which reads no mask but still advances.  AUTO = false is the kernel as it was.
//
// Soft controls (docs/DESIGN.md §4h, the SOFT instantiations, with any MASK / AUTO): a row has a line of
// a table of fp32 logit biases (one uniform index load, V/64 loads per lane), a presence and a frequency
// penalty.  n[c] counts char c among the row's own output bytes 0 .. step-1 -- at most max_len
// wave-uniform byte loads, each compared against the lane's chars, skipped when both penalties are 0 --
// and v = (x + bias) - (frequency * n (+ presence if n > 0)), three fp32 operations in this order with
// contraction off, takes x's place before the temperature scale.  A forced step reads none of it.
// SOFT = false is the kernel as it was.
#include "kernels.h"
#include "common.h"
#include "gen_sample.h"

namespace gk {

// floats -> unsigned keys with the same order (-0 and +0 share a key)
DEV unsigned order_key(float f) {
  unsigned b = __float_as_uint(f);
  if (b == 0x80000000u) b = 0u;
  return (b >> 31) ? ~b : (b | 0x80000000u);
}

template <int MAXPER, bool MASK, bool AUTO = false, bool SOFT = false>
__global__ void __launch_bounds__(64) sample_ctl_f32_kernel(SampleCtlArgs c) {
#pragma clang fp contract(off)
  const SampleF32Args& a = c.s;
  const int b = blockIdx.x, lane = threadIdx.x, V = a.V, per = V / 64;
  if (b >= a.N) return;
  const int cb = b + c.row0;   // this row's controls
  float* prow = a.probs ? a.probs + (size_t)b * V : nullptr;
  int sel;
  int q = 0;   // AUTO: this row's automaton state = its table line
  if constexpr (AUTO) {
    q = c.allow_state[cb];
    if (q < 0 || q >= c.allow_rows) {   // never expected (the host builds start and next): flag it, the free state
      if (c.err && lane == 0) {
        atomicOr(c.err, 16u);
        c.err[1] = (unsigned)q;
        c.err[2] = (unsigned)b;
      }
      q = 0;
    }
  }
  if (a.step < c.plen[cb]) {   // forced: the uniform of this step is ignored
    sel = c.prefix[(size_t)cb * a.max_len + a.step];
    if (sel >= V) {   // never expected (the host checks first): flag it instead of feeding it on
      if (c.err && lane == 0) {
        atomicOr(c.err, 16u);
        c.err[1] = (unsigned)sel;
        c.err[2] = (unsigned)b;
      }
      sel = 0;
    }
    if (prow)
#pragma unroll
      for (int e = 0; e < MAXPER; ++e)
        if (e < per) prow[lane * per + e] = (lane * per + e == sel) ? 1.f : 0.f;
  } else {
    const float* x = a.logits + (size_t)b * V + lane * per;
    const float it = c.inv_temp[cb];   // 0: greedy
    const int k = c.top_k[cb];
    const float tp = c.top_p[cb];
    const float scale = it == 0.f ? 1.f : it;
    unsigned ok = 0u;   // MASK: bit e = this lane's char e is allowed
    if constexpr (AUTO) {
      ok = c.allow_tab[(size_t)q * (V >> 5) + ((lane * per) >> 5)] >> ((lane * per) & 31);
    } else if constexpr (MASK) {
      int ar = c.allow_idx[(size_t)cb * a.max_len + a.step];
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
    float sbias[SOFT ? MAXPER : 1];   // SOFT: this lane's biases and penalties
    float spen[SOFT ? MAXPER : 1];
    if constexpr (SOFT) {
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
      const float pres = c.soft_pres[cb], freq = c.soft_freq[cb];
      int cnt[MAXPER];
#pragma unroll
      for (int e = 0; e < MAXPER; ++e) cnt[e] = 0;
      if (pres != 0.f || freq != 0.f) {   // (with both 0 every penalty is +0 whatever the counts are)
        const unsigned char* orow = a.out + (size_t)b * (a.max_len + 1);
        for (int j = 0; j < a.step; ++j) {
          const int ch = orow[j];
#pragma unroll
          for (int e = 0; e < MAXPER; ++e) cnt[e] += (e < per && lane * per + e == ch) ? 1 : 0;
        }
      }
#pragma unroll
      for (int e = 0; e < MAXPER; ++e) {
        sbias[e] = e < per ? brow[e] : 0.f;
        float pn = freq * (float)cnt[e];
        if (cnt[e] > 0) pn = pn + pres;
        spen[e] = pn;
      }
    }
    float y[MAXPER];
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < MAXPER; ++e) {
      if (e < per) {
        float v = x[e];
        for (int s2 = 1; s2 < a.splits; ++s2) v += x[s2 * a.slab + e];   // split-K slabs, fixed order
        if (a.bias) v += a.bias[lane * per + e];
        if constexpr (SOFT) v = (v + sbias[e]) - spen[e];
        y[e] = v * scale;
        if constexpr (MASK)
          if (!((ok >> e) & 1u)) y[e] = -INFINITY;
      } else {
        y[e] = -INFINITY;
      }
      mx = fmaxf(mx, y[e]);
    }
    mx = wave_max_dpp(mx);
    if (it == 0.f) {   // greedy: the lowest index of the maximum
      int first = V;
#pragma unroll
      for (int e = MAXPER - 1; e >= 0; --e)
        if (e < per && y[e] == mx && (!MASK || ((ok >> e) & 1u))) first = lane * per + e;
      sel = wave_min_dpp(first);
      if (sel >= V) sel = V - 1;   // (only a row of NaNs gets here)
      if (prow)
#pragma unroll
        for (int e = 0; e < MAXPER; ++e)
          if (e < per) prow[lane * per + e] = (lane * per + e == sel) ? 1.f : 0.f;
    } else {
      bool keep[MAXPER];
#pragma unroll
      for (int e = 0; e < MAXPER; ++e) keep[e] = e < per && (!MASK || ((ok >> e) & 1u));
      if (k > 0 && k < V) {   // t = key of the k-th largest value: the largest t with #{key >= t} >= k
        unsigned key[MAXPER];
#pragma unroll
        for (int e = 0; e < MAXPER; ++e) key[e] = order_key(y[e]);
        unsigned t = 0u;
        for (int bit = 31; bit >= 0; --bit) {
          const unsigned cand = t | (1u << bit);
          int cnt = 0;
#pragma unroll
          for (int e = 0; e < MAXPER; ++e) cnt += __popcll(__ballot((MASK ? keep[e] : e < per) && key[e] >= cand));
          if (cnt >= k) t = cand;
        }
#pragma unroll
        for (int e = 0; e < MAXPER; ++e) keep[e] = (MASK ? keep[e] : e < per) && key[e] >= t;
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
            const unsigned cand = u | (1u << bit);
            if (!(above(cand) < tp)) u = cand;
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
      // renormalised distribution over the kept set, then softmax_sample_wave's CDF search
      float p[MAXPER];
      float loc = 0.f;
      int last = -1;
#pragma unroll
      for (int e = 0; e < MAXPER; ++e) {
        p[e] = e < per ? ex[e] / se : 0.f;
        loc += p[e];
        if (keep[e]) last = lane * per + e;
        if (prow && e < per) prow[lane * per + e] = p[e];
      }
      const float rnd = a.rf[(size_t)b * a.max_len + a.step];
      const float inc = wave_scan_incl_dpp(loc);
      float psum = inc - loc;
      int hit = V;
#pragma unroll
      for (int e = 0; e < MAXPER; ++e) {
        psum += p[e];
        // MASK: only a kept char is a hit.  The scan's lanes associate their sums differently, so a lane
        // past the last kept char can hold a total one ulp above an earlier lane's and exceed an r that
        // no kept char's running sum exceeded; unmasked, any index it picks is at least a legal char
        if (e < per && hit == V && psum > rnd && (!MASK || keep[e])) hit = lane * per + e;
      }
      hit = wave_min_dpp(hit);
      last = -wave_min_dpp(-last);   // the highest kept index (V - 1 with nothing filtered)
      sel = hit >= V ? (last < 0 ? V - 1 : last) : hit;
    }
  }
  if (lane == 0) {
    if (a.alive[b]) {
      a.out[(size_t)b * (a.max_len + 1) + a.step] = (unsigned char)sel;
      if (sel == a.eos) a.alive[b] = 0;
    }
    a.ids[b] = sel;
    if constexpr (AUTO) c.allow_state[cb] = c.allow_next[(size_t)q * V + sel];   // 0 <= sel < V on every branch
  }
}

__global__ void __launch_bounds__(256) automaton_reset_kernel(int* state, const int* start, int n, int Bp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < Bp) state[i] = i < n ? start[i] : 0;
}

void automaton_reset(int* state, const int* start, int n, int Bp, hipStream_t s) {
  if (!state || !start || n < 0 || n > Bp) throw std::runtime_error("automaton_reset: state, start and 0 <= n <= Bp required");
  if (Bp <= 0) return;
  hipLaunchKernelGGL(automaton_reset_kernel, dim3((Bp + 255) / 256), dim3(256), 0, s, state, start, n, Bp);
}

void sample_ctl_f32(const SampleCtlArgs& c, hipStream_t s) {
  const SampleF32Args& a = c.s;
  if (a.V % 64 || a.V > 512 || a.V <= 0) throw std::runtime_error("sample_ctl_f32: needs V % 64 == 0 and V <= 512");
  if (!c.inv_temp || !c.top_k || !c.top_p || !c.plen || !c.prefix || c.row0 < 0)
    throw std::runtime_error("sample_ctl_f32: inv_temp, top_k, top_p, plen and prefix are required");
  if (!c.allow_state && !c.allow_next && (c.allow_tab != nullptr) != (c.allow_idx != nullptr))
    throw std::runtime_error("sample_ctl_f32: allow_tab and allow_idx are set together or not at all");
  const bool mask = c.allow_tab != nullptr;
  if (mask && (c.allow_rows < 1 || 32 % (a.V / 64)))
    throw std::runtime_error("sample_ctl_f32: constraints need allow_rows >= 1 and V / 64 in {1, 2, 4, 8}");
  if ((c.allow_state != nullptr) != (c.allow_next != nullptr) || (c.allow_state && (!c.allow_tab || c.allow_idx)))
    throw std::runtime_error("sample_ctl_f32: allow_state and allow_next are set together, with allow_tab and without allow_idx");
  if (c.allow_state && c.allow_rows > 65535)
    throw std::runtime_error("sample_ctl_f32: an automaton has at most 65535 states");
  const bool soft = c.soft_tab != nullptr;
  if (soft != (c.soft_idx != nullptr) || soft != (c.soft_pres != nullptr) || soft != (c.soft_freq != nullptr) ||
      (soft && c.soft_rows < 1))
    throw std::runtime_error("sample_ctl_f32: soft_tab, soft_idx, soft_pres and soft_freq are set together, with soft_rows >= 1");
  if (a.N <= 0) return;
  const dim3 grid(a.N), block(64);
  if (soft) {   // the SOFT instantiations; every other call launches what it launched before
    if (c.allow_state) {
      if (a.V == 256) hipLaunchKernelGGL((sample_ctl_f32_kernel<4, true, true, true>), grid, block, 0, s, c);
      else if (a.V == 512) hipLaunchKernelGGL((sample_ctl_f32_kernel<8, true, true, true>), grid, block, 0, s, c);
      else throw std::runtime_error("sample_ctl_f32: the automaton instantiations need V = 256 or 512");
    } else if (a.V == 256) {
      if (mask) hipLaunchKernelGGL((sample_ctl_f32_kernel<4, true, false, true>), grid, block, 0, s, c);
      else hipLaunchKernelGGL((sample_ctl_f32_kernel<4, false, false, true>), grid, block, 0, s, c);
    } else {
      if (mask) hipLaunchKernelGGL((sample_ctl_f32_kernel<8, true, false, true>), grid, block, 0, s, c);
      else hipLaunchKernelGGL((sample_ctl_f32_kernel<8, false, false, true>), grid, block, 0, s, c);
    }
    return;
  }
  if (c.allow_state) {
    if (a.V == 256) hipLaunchKernelGGL((sample_ctl_f32_kernel<4, true, true>), grid, block, 0, s, c);
    else if (a.V == 512) hipLaunchKernelGGL((sample_ctl_f32_kernel<8, true, true>), grid, block, 0, s, c);
    else throw std::runtime_error("sample_ctl_f32: the automaton instantiations need V = 256 or 512");
    return;
  }
  if (a.V == 256) {
    if (mask) hipLaunchKernelGGL((sample_ctl_f32_kernel<4, true>), grid, block, 0, s, c);
    else hipLaunchKernelGGL((sample_ctl_f32_kernel<4, false>), grid, block, 0, s, c);
  } else {
    if (mask) hipLaunchKernelGGL((sample_ctl_f32_kernel<8, true>), grid, block, 0, s, c);
    else hipLaunchKernelGGL((sample_ctl_f32_kernel<8, false>), grid, block, 0, s, c);
  }
}

}  // namespace gk

// Teacher-forced scoring kernels (Generator::score): how likely is a given output row under the model.
//
// A row is the generator's own output format, max_len + 1 bytes.  Its token count n_tok is the index
// of the first EOS byte among c[0 .. ML-1] plus one, or ML when there is none -- the generator's
// stopping rule (EOS written, then stop).  Step l < n_tok feeds x_l = SOS (l = 0) or c[l-1] and is
// scored against the target c[l]:
//   * score_prep: rows -> time-major input ids / targets [ML][Bp] and n_tok [Bp], one kernel node
//     (no memset nodes, for the reason recorded at Generator::reset_batch);
//   * score_logprob_f32: one wave per name walks its n_tok logits rows in step order: max-subtracted
//     log-sum-exp, the target's log-prob and rank, and the name's sum.  A lane owns V/64 consecutive
//     logits as in sample_f32_kernel; the cross-lane steps are the fixed-order DPP helpers of
//     gen_sample.h, so a row's statistics -- and the per-name sum, which one lane adds in step
//     order -- are bitwise the same on every call.  No atomics on the results.
#include <cmath>
#include <stdexcept>
#include "kernels.h"
#include "common.h"
#include "gen_sample.h"

namespace gk {

__global__ void __launch_bounds__(256) score_prep_kernel(ScorePrepArgs a) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.Bp) return;
  const int ML = a.ML;
  const int N = a.n_dev ? a.n_dev[0] : a.N;
  if (b >= N) {   // pad row: SOS in, nothing scored
    for (int l = 0; l < ML; ++l) {
      a.ids[(size_t)l * a.Bp + b] = a.sos;
      a.tgt[(size_t)l * a.Bp + b] = -1;
    }
    a.ntok[b] = 0;
    return;
  }
  const unsigned char* c = a.rows + (size_t)b * (ML + 1);
  int nt = ML;
  for (int l = 0; l < ML; ++l)
    if (c[l] == a.eos) { nt = l + 1; break; }
  bool bad = false;
  int prev = a.sos;
  for (int l = 0; l < ML; ++l) {
    int x = a.sos, t = -1;
    if (l < nt) {
      x = prev;
      t = c[l];
      if (t >= a.V) { bad = true; t = 0; }   // caller error: clamp, flag (gru_gates_f32's bit)
      prev = t;                              // the next input: in range like every target
    }
    a.ids[(size_t)l * a.Bp + b] = x;
    a.tgt[(size_t)l * a.Bp + b] = t;
  }
  a.ntok[b] = nt;
  if (bad && a.err) atomicOr(a.err, 16u);
}

__global__ void score_set_count_kernel(int* n_dev, int n) {
  if (blockIdx.x == 0 && threadIdx.x == 0) n_dev[0] = n;
}
void score_set_count(int* n_dev, int n, hipStream_t s) {
  hipLaunchKernelGGL(score_set_count_kernel, dim3(1), dim3(64), 0, s, n_dev, n);
}

void score_prep(const ScorePrepArgs& a, hipStream_t s) {
  if (a.Bp <= 0 || a.ML <= 0 || a.V <= 0 || a.sos < 0 || a.sos >= a.V)
    throw std::runtime_error("score_prep: needs Bp, ML > 0 and 0 <= sos < V");
  hipLaunchKernelGGL(score_prep_kernel, dim3((a.Bp + 255) / 256), dim3(256), 0, s, a);
}

// One wave per name (block b of Bp): rows b >= N have n_tok = 0 and only write their masked outputs.
template <int MAXPER>
__global__ void __launch_bounds__(64) score_logprob_f32_kernel(ScoreLogprobArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x, per = a.V / 64, ML = a.ML;
  const int nt = min(max(__builtin_amdgcn_readfirstlane(a.ntok[b]), 0), ML);
  float sum = 0.f;
  for (int l = 0; l < nt; ++l) {
    const size_t row = (size_t)l * a.Bp + b;
    int t = __builtin_amdgcn_readfirstlane(a.tgt[row]);
    t = min(max(t, 0), a.V - 1);
    const float* x = a.logits + row * a.V + lane * per;
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
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < MAXPER; ++e) mx = fmaxf(mx, xv[e]);
    mx = wave_max_dpp(mx);
    float se = 0.f;
#pragma unroll
    for (int e = 0; e < MAXPER; ++e) se += e < per ? expf(xv[e] - mx) : 0.f;
    se = wave_sum_dpp(se);
    // the target's logit from the lane that owns it
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
    const float lp = (xt - mx) - logf(se);
    sum += lp;   // step order, the same value in every lane
    if (lane == 0) {
      a.tok_logp[(size_t)b * ML + l] = lp;
      a.rank[(size_t)b * ML + l] = rank;
    }
  }
  if (lane < ML - nt) {   // masked positions (ML <= 64, checked by the launcher)
    a.tok_logp[(size_t)b * ML + nt + lane] = 0.f;
    a.rank[(size_t)b * ML + nt + lane] = -1;
  }
  if (lane == 0) {
    a.name_logp[b] = sum;
    a.ntok_out[b] = nt;
  }
}

void score_logprob_f32(const ScoreLogprobArgs& a, hipStream_t s) {
  if (a.V % 64 || a.V > 512 || a.V <= 0) throw std::runtime_error("score_logprob_f32: needs V % 64 == 0 and V <= 512");
  if (a.ML <= 0 || a.ML > 64) throw std::runtime_error("score_logprob_f32: needs 0 < max_len <= 64");
  if (a.splits < 1 || (a.splits > 1 && a.slab < (long)a.ML * a.Bp * a.V))
    throw std::runtime_error("score_logprob_f32: split-K slabs overlap");
  if (a.Bp <= 0) return;
  if (a.V <= 256) hipLaunchKernelGGL(score_logprob_f32_kernel<4>, dim3(a.Bp), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(score_logprob_f32_kernel<8>, dim3(a.Bp), dim3(64), 0, s, a);
}

}  // namespace gk

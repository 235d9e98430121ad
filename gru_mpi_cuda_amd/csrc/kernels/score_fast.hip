// Head of the bf16 fast scorer (Generator::score_fast, docs/DESIGN.md §4a "Fast bf16 scoring").
//
// score_head_bf16: logits = h W_fc^T + b_fc for 64 names of one step per workgroup, fused with the
// log-softmax, the target's log-prob and its rank -- the [ML Bp][V] logits of the fp32 schedule (its
// largest buffer, written once and read once) never exist.
//   * grid (Bp / 64, ML), 256 threads.  A workgroup first reads its names' n_tok: when all 64 are masked
//     at its step it writes the masked values (0, -1) and leaves; with real name lengths that is a large
//     share of the late steps.
//   * product: 64 tokens x V logits, K = H, on v_mfma_f32_16x16x32_bf16.  Wave w owns names 16 w .. 16 w + 15
//     and ALL V columns (V / 16 accumulator tiles), so a token's whole logits row lives in the 16 lanes of
//     one DPP row of one wave: lane (lq, lr), register i of tile t holds token 16 w + 4 lq + i, column 16 t + lr.
//   * staging: per 64-deep k-tile the A tile (64 x 64 of h) and the B tile (V x 64 of W_fc) by LDS-DMA
//     (global_load_lds_dwordx4: one instruction lands 8 rows of 128 B lane-linearly) into a two-slot ring, the
//     XOR swizzle of gru_step_lds.hip on the source address, so the ds_read_b128 fragment reads are
//     conflict-free.  One vmcnt(0) + barrier per k-tile: it publishes tile kt and proves every wave is done
//     with the slot tile kt + 1 is about to overwrite.  2 x (8 + 64) KiB at V = 512.
//   * epilogue in registers: + b_fc; row max and sum of expf(x - max) over the tiles in order, then the
//     fixed-order DPP reductions of common.h over the 16 lanes of the row; the target's logit from its owner
//     lane (every other lane offers -inf to the same max reduction: exact); the rank as the sum of per-lane
//     counts under score_logprob_f32's tie rule; tok_logp = (x_t - max) - logf(sum), that kernel's form.
// score_name_sum: name_logp = the fp32 sum of the name's stored tok_logp in step order, and n_tok.
// No atomics on the results: every replay writes the same bytes.
#include <cmath>
#include <stdexcept>
#include "kernels.h"
#include "common.h"

namespace gk {
namespace {

typedef __attribute__((address_space(3))) void lds_void_t;

DEV int sh_swz(int r, int c) { return c ^ ((r >> 1) & 7); }

template <int NV>   // V = 64 NV
__global__ void __launch_bounds__(256) score_head_bf16_kernel(ScoreHeadArgs a) {
  constexpr int V = 64 * NV, NT = 4 * NV;   // NT accumulator tiles of 16 columns
  constexpr int NB = 2 * NV;                // B-tile LDS-DMA instructions per wave and k-tile (A: 2)
  __shared__ __attribute__((aligned(16))) u16 lds[2][(64 + V) * 64];
  const int st = blockIdx.y, b0 = blockIdx.x * 64, ML = a.ML, H = a.H;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int lr = lane & 15, lq = lane >> 4;

  // every wave looks at all 64 names: the same answer in each, no LDS needed
  if (__ballot(st < a.ntok[b0 + lane]) == 0) {
    if (w == 0) {
      a.tok_logp[(size_t)(b0 + lane) * ML + st] = 0.f;
      a.rank[(size_t)(b0 + lane) * ML + st] = -1;
    }
    return;
  }

  const int srow = lane >> 3, sslot = lane & 7;
  const u16* Am = a.h + ((size_t)st * a.Bp + b0) * H;
  auto stage = [&](int buf, int kt) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int r = (2 * w + q) * 8 + srow;   // 0 .. 63
      __builtin_amdgcn_global_load_lds(Am + (size_t)r * H + kt * 64 + sh_swz(r, sslot) * 8,
                                       (lds_void_t*)(&lds[buf][(2 * w + q) * 8 * 64]), 16, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const int r = (NB * w + q) * 8 + srow;  // 0 .. V - 1
      __builtin_amdgcn_global_load_lds(a.Wfc + (size_t)r * H + kt * 64 + sh_swz(r, sslot) * 8,
                                       (lds_void_t*)(&lds[buf][(64 + (NB * w + q) * 8) * 64]), 16, 0, 0);
    }
  };

  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nk = H / 64;
  stage(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's part of tile kt has landed
    lds_barrier();
    if (kt + 1 < nk) stage((kt + 1) & 1, kt + 1);
    const u16* LA = lds[kt & 1];
    const u16* LB = LA + 64 * 64;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int c = ks * 4 + lq;
      const int ra = 16 * w + lr;
      const bf16x8 af = *reinterpret_cast<const bf16x8*>(&LA[ra * 64 + sh_swz(ra, c) * 8]);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int rb = t * 16 + lr;
        const bf16x8 bfr = *reinterpret_cast<const bf16x8*>(&LB[rb * 64 + sh_swz(rb, c) * 8]);
        acc[t] = mfma16(af, bfr, acc[t]);
      }
    }
  }

#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const float bb = a.bfc[t * 16 + lr];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[t][i] += bb;
  }
  bool bad = false;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int b = b0 + 16 * w + lq * 4 + i;
    const int nt = min(max(a.ntok[b], 0), ML);
    const bool scored = st < nt;
    const int traw = a.tgt[(size_t)st * a.Bp + b];
    bad |= scored && (traw < 0 || traw >= V);
    const int tc = min(max(traw, 0), V - 1);
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t) mx = fmaxf(mx, acc[t][i]);
    mx = max16(mx);
    float se = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) se += expf(acc[t][i] - mx);
    se = sum16(se);
    float cand = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t) cand = t == (tc >> 4) ? acc[t][i] : cand;
    const float xt = max16(lr == (tc & 15) ? cand : -INFINITY);
    int cnt = 0;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const float x = acc[t][i];
      cnt += (x > xt || (x == xt && t * 16 + lr < tc)) ? 1 : 0;
    }
    const int rk = (int)sum16((float)cnt);   // counts <= 512: exact in fp32
    const float lp = (xt - mx) - logf(se);
    if (lr == 0) {
      a.tok_logp[(size_t)b * ML + st] = scored ? lp : 0.f;
      a.rank[(size_t)b * ML + st] = scored ? rk : -1;
    }
  }
  if (bad && lr == 0 && a.err) atomicOr(a.err, 16u);
}

__global__ void __launch_bounds__(256) score_name_sum_kernel(ScoreHeadArgs a) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= a.Bp) return;
  const int nt = min(max(a.ntok[b], 0), a.ML);
  float sum = 0.f;
  for (int l = 0; l < nt; ++l) sum += a.tok_logp[(size_t)b * a.ML + l];   // step order
  a.name_logp[b] = sum;
  a.ntok_out[b] = nt;
}

}  // namespace

bool score_head_supported(int H, int V, int ML) {
  return H >= 64 && H % 64 == 0 && V >= 64 && V % 64 == 0 && V <= 512 && ML >= 1 && ML <= 64;
}

void score_head_bf16(const ScoreHeadArgs& a, hipStream_t s) {
  if (!score_head_supported(a.H, a.V, a.ML))
    throw std::runtime_error("score_head_bf16: needs H % 64 == 0, V % 64 == 0, V <= 512 and 0 < max_len <= 64");
  if (a.Bp <= 0 || a.Bp % 64) throw std::runtime_error("score_head_bf16: needs Bp > 0, Bp % 64 == 0");
  if (!a.h || !a.Wfc || !a.bfc || !a.tgt || !a.ntok || !a.tok_logp || !a.rank || !a.name_logp || !a.ntok_out)
    throw std::runtime_error("score_head_bf16: h, Wfc, bfc, tgt, ntok, tok_logp, rank, name_logp, ntok_out required");
  const dim3 grid(a.Bp / 64, a.ML), block(256);
  switch (a.V / 64) {
#define SH_CASE(NVV) case NVV: hipLaunchKernelGGL(score_head_bf16_kernel<NVV>, grid, block, 0, s, a); break;
    SH_CASE(1) SH_CASE(2) SH_CASE(3) SH_CASE(4) SH_CASE(5) SH_CASE(6) SH_CASE(7) SH_CASE(8)
#undef SH_CASE
  }
  hipLaunchKernelGGL(score_name_sum_kernel, dim3((a.Bp + 255) / 256), dim3(256), 0, s, a);
}

}  // namespace gk

// Kernels of the bf16 fast distinct names (Generator::distinct_fast, docs/DESIGN.md §4i "Fast bf16 distinct
// names"; the rule and CPU twin: cpu_ref.sample_distinct(round_operands=True)).
//
// sbs_head_bf16: logits = h W_fc^T + b_fc for 64 slot rows per workgroup, fused with sbs_select_f32's steps in
// its order -- the sampler's log-softmax, psi, the Gumbel noise, the truncation -- and each row's top W
// candidates: the [rows][V] logits of the fp32 loop (a GEMM's split-K slabs written and read back every char
// step) never exist.
//   * geometry and staging are beam_head_bf16's: grid Bp / 64, 256 threads; wave w owns rows 16 w .. 16 w + 15
//     and ALL V columns (V / 16 accumulator tiles of v_mfma_f32_16x16x32_bf16): lane (lq, lr), register i of
//     tile t holds row 16 w + 4 lq + i, column 16 t + lr, a row's whole line in the 16 lanes of one DPP row.
//     h and W_fc k-tiles (64 deep) arrive by LDS-DMA in a two-slot ring, XOR-swizzled on the source address;
//     one vmcnt(0) + barrier per k-tile.
//   * a workgroup without a live row writes the carries and the fill and leaves -- no product (a launch that
//     asks for the lq debug output needs the product and never skips).
//   * epilogue, in registers, register i at a time (four rows per wave side by side, one per DPP row):
//     y = (acc + b_fc) * inv_t[n] replaces the logit; max and sum of expf(y - max) over the tiles in order,
//     then the fixed-order DPP reductions; lq = (y - max) - logf(sum); psi = logq_b + (forced ? 0 : lq) goes
//     to V / 16 registers of its own and g = psi + gum replaces y; Z = the row's max of g over the offered
//     children; sbs_key(sbs_truncate(G_b, g, Z)) replaces g (sbs_dev.h: the exact path's text, so the best
//     child keeps Gt == G_b bitwise).  Key 0 = not offered.
//   * noise: child j = b V + c reads word j & 3 of Philox-4x32-10(key = seed, counter = (j >> 2, step, g lo,
//     g hi)) -- §4i's words.  A lane's columns are 16 t + lr, so the four children of a block are the four
//     lanes of a quad in one tile: lane q of a quad computes the block of tile 4 u + q (one Philox call per
//     four candidates) and the words travel by DPP quad broadcasts.  A wave whose live rows are all on a forced
//     step draws nothing: the one offered child is the row's maximum and keeps G_b whatever its noise.
//   * top W per row as in beam_head_bf16: a lane caches its best (key, tile, psi); a round is three DPP row
//     reductions -- the largest key, the lowest column among its holders, that lane's psi -- and ONLY the
//     winner's lane clears its entry and rescans.  Round k is parked in lane k & 15; the rounds stop when no
//     row of the wave has a candidate left.
// sbs_merge: one wave per name, four names per workgroup.  The W lists are staged in LDS, lane b holds list
// b's head, W rounds of a wave arg-max on (key, lowest j), the winner's lane advances its head.  A row's list
// is the total order restricted to that row and a name's top W lie in the union of its rows' top W: this is
// sbs_select_f32's selection on the same candidates, and its outputs.
// No atomics on results: every replay writes the same bytes.
#include <cmath>
#include <stdexcept>
#include "kernels.h"
#include "common.h"
#include "gen_sample.h"
#include "sbs_dev.h"

#pragma clang fp contract(off)

namespace gk {
namespace {

constexpr int kDead = 0, kLive = 1, kFin = 2;   // SbsSelectArgs::state values
typedef __attribute__((address_space(3))) void lds_void_t;

DEV int sh_swz(int r, int c) { return c ^ ((r >> 1) & 7); }

template <int CTRL>
DEV unsigned dppu(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false); }
DEV unsigned umax16(unsigned v) {   // identical in the 16 lanes of a row
  v = max(v, dppu<0xB1>(v));
  v = max(v, dppu<0x4E>(v));
  v = max(v, dppu<0x141>(v));
  v = max(v, dppu<0x140>(v));
  return v;
}
DEV int imin16(int v) {
  v = min(v, (int)dppu<0xB1>((unsigned)v));
  v = min(v, (int)dppu<0x4E>((unsigned)v));
  v = min(v, (int)dppu<0x141>((unsigned)v));
  v = min(v, (int)dppu<0x140>((unsigned)v));
  return v;
}
// word q of the block that lane SRC of this lane's quad holds (quad_perm broadcast of each word, then a select)
template <int SRC>
DEV unsigned quad_word(const unsigned (&wd)[4], int q) {
  constexpr int C = SRC * 0x55;
  const unsigned w0 = dppu<C>(wd[0]), w1 = dppu<C>(wd[1]), w2 = dppu<C>(wd[2]), w3 = dppu<C>(wd[3]);
  return q == 0 ? w0 : q == 1 ? w1 : q == 2 ? w2 : w3;
}

template <int NV>   // V = 64 NV
__global__ void __launch_bounds__(256) sbs_head_bf16_kernel(SbsHeadArgs a) {
#pragma clang fp contract(off)
  constexpr int V = 64 * NV, NT = 4 * NV;   // NT accumulator tiles of 16 columns
  constexpr int NB = 2 * NV;                // B-tile LDS-DMA instructions per wave and k-tile (A: 2)
  __shared__ __attribute__((aligned(16))) u16 lds[2][(64 + V) * 64];
  const int b0 = blockIdx.x * 64, H = a.H, W = a.W, NW = a.N * a.W;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int lr = lane & 15, lq = lane >> 4;

  {   // every wave looks at all 64 rows: the same answer in each, no LDS needed
    const int row = b0 + lane;
    const int st = row < NW ? a.state_in[row] : kDead;
    if (__ballot(st == kLive) == 0 && !a.lq) {
      if (w == 0 && row < NW) {
        const float qb = a.logq_in[row], Gb = a.G_in[row];
        for (int k = 0; k < W; ++k) {
          const bool carry = k == 0 && st == kFin;
          a.cand_gt[(size_t)row * W + k] = carry ? Gb : -INFINITY;
          a.cand_chr[(size_t)row * W + k] = carry ? 0 : -1;
          a.cand_psi[(size_t)row * W + k] = carry ? qb : -INFINITY;
        }
        if (a.zmax) a.zmax[row] = NAN;
      }
      if (a.gt) {
        for (int r = w; r < 64 && b0 + r < NW; r += 4) {
          const bool fin = a.state_in[b0 + r] == kFin;
          for (int c = lane; c < V; c += 64) a.gt[(size_t)(b0 + r) * V + c] = (fin && c == 0) ? a.G_in[b0 + r] : NAN;
        }
      }
      return;
    }
  }

  const int srow = lane >> 3, sslot = lane & 7;
  const u16* Am = a.h + (size_t)b0 * H;
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
  const unsigned long long seed = *a.seed, gstart = *a.start;
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
  const int qd = lr & 3;   // this lane's word of a block, and the tile of a group of four whose block it computes
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = b0 + 16 * w + lq * 4 + i;
    const bool real = row < NW;
    const int st = real ? a.state_in[row] : kDead;
    const float qb = real ? a.logq_in[row] : -INFINITY, Gb = real ? a.G_in[row] : -INFINITY;
    const bool live = st == kLive;
    const int n = real ? row / W : 0, b = real ? row - n * W : 0;
    const float inv_t = a.inv_t[n];
    int fc = -1;   // the forced char of a live row
    if (live && a.step < a.plen[n]) {
      fc = a.prefix[(size_t)n * a.max_len + a.step];
      if (fc >= V) {   // never expected (the host checks first): flag it instead of offering it
        if (a.err && lr == 0) {
          atomicOr(a.err, 16u);
          a.err[1] = (unsigned)fc;
          a.err[2] = (unsigned)(n * W);
        }
        fc = 0;
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      acc[t][i] = acc[t][i] * inv_t;
      mx = fmaxf(mx, acc[t][i]);
    }
    mx = max16(mx);
    float se = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) se += expf(acc[t][i] - mx);
    se = sum16(se);
    const float lse = logf(se);
    // psi and g = psi + gum; a wave draws noise only where a live row of it is on a free step (or Z is asked for)
    const bool noise = __ballot(live && (fc < 0 || a.zmax != nullptr)) != 0;   // wave-uniform
    const unsigned long long gidx = gstart + (unsigned long long)n;
    float psi[NT];
    float Z = -INFINITY;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      unsigned wd[4] = {0u, 0u, 0u, 0u};
      if (noise)
        philox4x32_10((unsigned)(b * (V / 4) + 4 * (4 * u + qd) + (lr >> 2)), (unsigned)a.step, (unsigned)gidx,
                      (unsigned)(gidx >> 32), k0, k1, wd);
      auto child = [&](int t, unsigned word) {
        const int c = t * 16 + lr;
        const float lqv = (acc[t][i] - mx) - lse;
        if (a.lq && real) a.lq[(size_t)row * V + c] = lqv;
        float gum = 0.f;
        if (noise) {
          const float uu = (float)(2u * (word >> 9) + 1u) * 0x1p-24f;   // exact, in [2^-24, 1 - 2^-24]
          gum = -logf(-logf(uu));
        }
        psi[t] = qb + (fc >= 0 ? 0.f : lqv);
        const float g = psi[t] + gum;
        acc[t][i] = g;
        if (live && (fc < 0 || c == fc)) Z = fmaxf(Z, g);
      };
      child(4 * u + 0, quad_word<0>(wd, qd));
      child(4 * u + 1, quad_word<1>(wd, qd));
      child(4 * u + 2, quad_word<2>(wd, qd));
      child(4 * u + 3, quad_word<3>(wd, qd));
    }
    Z = max16(Z);
    if (a.zmax && real && lr == 0) a.zmax[row] = (live && Z != -INFINITY) ? Z : NAN;
    // the candidates' keys replace g; the lane's best on the way (ascending c: the first wins)
    unsigned bk = 0u;
    int bt = 0;
    float bp = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int c = t * 16 + lr;
      float gt = NAN;
      unsigned k = 0u;
      if (live && (fc < 0 || c == fc)) {
        gt = sbs_truncate(Gb, acc[t][i], Z);
        k = sbs_key(gt);
      } else if (st == kFin && c == 0) {   // the carry, j = b V
        gt = Gb;
        k = sbs_key(Gb);
        psi[t] = qb;
      }
      if (a.gt && real) a.gt[(size_t)row * V + c] = gt;
      acc[t][i] = __uint_as_float(k);
      if (k > bk) { bk = k; bt = t; bp = psi[t]; }
    }
    float og0 = -INFINITY, og1 = -INFINITY, op0 = -INFINITY, op1 = -INFINITY;   // rounds lr and lr + 16 of this row
    int oc0 = -1, oc1 = -1;
    for (int k = 0; k < W; ++k) {
      const unsigned wk = umax16(bk);
      if (__ballot(wk != 0u) == 0) break;   // no row of this wave has a candidate left
      const int myc = (wk != 0u && bk == wk) ? bt * 16 + lr : 0x7fffffff;
      const int wc = imin16(myc);
      const bool mine = wk != 0u && myc == wc;
      const float wp = max16(mine ? bp : -INFINITY);   // one lane owns (wk, wc)
      if (wk != 0u && lr == (k & 15)) {
        if (k < 16) { og0 = sbs_unkey(wk); oc0 = wc; op0 = wp; }
        else { og1 = sbs_unkey(wk); oc1 = wc; op1 = wp; }
      }
      if (mine) {   // the winner's lane takes it out and rescans
        const int rt = bt;
        bk = 0u;
        bt = 0;
        bp = -INFINITY;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const unsigned kk = t == rt ? 0u : __float_as_uint(acc[t][i]);
          acc[t][i] = __uint_as_float(kk);
          if (kk > bk) { bk = kk; bt = t; bp = psi[t]; }
        }
      }
    }
    if (real) {
      const size_t o = (size_t)row * W + lr;
      if (lr < W) { a.cand_gt[o] = og0; a.cand_chr[o] = oc0; a.cand_psi[o] = op0; }
      if (lr + 16 < W) { a.cand_gt[o + 16] = og1; a.cand_chr[o + 16] = oc1; a.cand_psi[o + 16] = op1; }
    }
  }
}

// four names per workgroup, a wave each
__global__ void __launch_bounds__(256) sbs_merge_kernel(SbsMergeArgs a) {
  __shared__ float s_gt[4][32 * 32];
  __shared__ float s_psi[4][32 * 32];
  __shared__ int s_c[4][32 * 32];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int n = blockIdx.x * 4 + w, W = a.W, V = a.V;
  const bool active = n < a.N;
  if (active) {
    const size_t base = (size_t)n * W * W;   // the name's W lists are one block
    for (int i = lane; i < W * W; i += 64) {
      s_gt[w][i] = a.cand_gt[base + i]; s_psi[w][i] = a.cand_psi[base + i]; s_c[w][i] = a.cand_chr[base + i];
    }
  }
  __syncthreads();
  if (!active) return;
  const size_t r0 = (size_t)n * W;
  int p = 0;   // lane b < W: the head of list b
  unsigned hk = 0u;
  int hj = 0x7fffffff;
  float hp = -INFINITY;
  auto head = [&]() {
    hk = 0u;
    hj = 0x7fffffff;
    hp = -INFINITY;
    if (lane < W && p < W) {
      const int c = s_c[w][lane * W + p];
      if (c >= 0) { hk = sbs_key(s_gt[w][lane * W + p]); hj = lane * V + c; hp = s_psi[w][lane * W + p]; }
    }
  };
  head();
  unsigned mk = 0u;   // lane k: round k's winner
  int mj = -1;
  float mp = -INFINITY;
  for (int k = 0; k < W; ++k) {
    const unsigned wk = sbs_umax(hk);
    const int wj = wave_min_dpp((wk != 0u && hk == wk) ? hj : 0x7fffffff);
    const bool mine = wk != 0u && hk == wk && hj == wj;
    const float wp = wave_max_dpp(mine ? hp : -INFINITY);   // one lane owns (wk, wj)
    if (lane == k) { mk = wk; mj = wj; mp = wp; }
    if (wk == 0u) break;   // wave-uniform: nothing left
    if (mine) { ++p; head(); }
  }
  if (lane < W) {
    const bool any = mk != 0u;
    const int pb = any ? mj / V : 0, pc = any ? mj - pb * V : 0;
    float lq = -INFINITY, G = -INFINITY;
    int parent = -1, ch = -1, st = kDead, nxt = a.sos;
    if (any) {
      parent = pb;
      if (a.state_in[r0 + pb] == kFin) {
        lq = a.logq_in[r0 + pb]; G = a.G_in[r0 + pb]; st = kFin;
      } else {
        lq = mp;               // psi, bit for bit: the head's register
        G = sbs_unkey(mk);     // the key keeps every bit of Gt but the sign of zero
        ch = pc;
        st = pc == a.eos ? kFin : kLive;
        if (st == kLive) nxt = pc;
      }
    }
    const size_t o = r0 + lane;
    a.logq_out[o] = lq; a.G_out[o] = G; a.parent[o] = parent; a.chr[o] = ch; a.state_out[o] = st; a.next_id[o] = nxt;
    if (a.sel) a.sel[o] = any ? mj : -1;
  }
}

}  // namespace

// every instance V = 64 .. 512 reports scratch 0 (docs/DESIGN.md §4i's table); one that did not would be
// refused here, before any launch
bool sbs_head_supported(int H, int V, int ML) {
  return H >= 64 && H % 64 == 0 && V >= 64 && V % 64 == 0 && V <= 512 && ML >= 1 && ML <= 64;
}

void sbs_head_bf16(const SbsHeadArgs& a, hipStream_t s) {
  if (!sbs_head_supported(a.H, a.V, a.max_len))
    throw std::runtime_error("sbs_head_bf16: needs H % 64 == 0, V % 64 == 0, V <= 512 and 0 < max_len <= 64");
  if (a.W < 1 || a.W > 32 || a.W > a.V) throw std::runtime_error("sbs_head_bf16: needs 1 <= W <= min(32, V)");
  if (a.Bp <= 0 || a.Bp % 64 || a.N < 0 || (long)a.N * a.W > a.Bp)
    throw std::runtime_error("sbs_head_bf16: needs Bp > 0, Bp % 64 == 0 and N W <= Bp");
  if (a.step < 0 || a.step >= a.max_len) throw std::runtime_error("sbs_head_bf16: needs 0 <= step < max_len");
  if (!a.h || !a.Wfc || !a.bfc || !a.logq_in || !a.G_in || !a.state_in || !a.plen || !a.prefix || !a.seed || !a.start ||
      !a.inv_t || !a.cand_gt || !a.cand_chr || !a.cand_psi)
    throw std::runtime_error("sbs_head_bf16: h, Wfc, bfc, logq, G, states, plen, prefix, seed, start, inv_t, cand_gt, "
                             "cand_chr and cand_psi are required");
  if (a.N == 0) return;
  const dim3 grid(a.Bp / 64), block(256);
  switch (a.V / 64) {
#define SH_CASE(NVV) case NVV: hipLaunchKernelGGL(sbs_head_bf16_kernel<NVV>, grid, block, 0, s, a); break;
    SH_CASE(1) SH_CASE(2) SH_CASE(3) SH_CASE(4) SH_CASE(5) SH_CASE(6) SH_CASE(7) SH_CASE(8)
#undef SH_CASE
  }
}

void sbs_merge(const SbsMergeArgs& a, hipStream_t s) {
  if (a.W < 1 || a.W > 32 || a.W > a.V || a.V <= 0) throw std::runtime_error("sbs_merge: needs 1 <= W <= min(32, V)");
  if (!a.cand_gt || !a.cand_chr || !a.cand_psi || !a.logq_in || !a.G_in || !a.state_in || !a.logq_out || !a.G_out ||
      !a.parent || !a.chr || !a.state_out || !a.next_id)
    throw std::runtime_error("sbs_merge: the candidate lists, logq, G, states and the six outputs are required");
  if (a.logq_in == a.logq_out || a.G_in == a.G_out || a.G_in == a.logq_out || a.logq_in == a.G_out ||
      a.logq_out == a.G_out || a.state_in == a.state_out)
    throw std::runtime_error("sbs_merge: the new slots' logq, G and states never overwrite the inputs");
  if (a.eos < 0 || a.sos < 0 || a.sos >= a.V) throw std::runtime_error("sbs_merge: needs eos >= 0 and 0 <= sos < V");
  if (a.N <= 0) return;
  hipLaunchKernelGGL(sbs_merge_kernel, dim3((a.N + 3) / 4), dim3(256), 0, s, a);
}

}  // namespace gk

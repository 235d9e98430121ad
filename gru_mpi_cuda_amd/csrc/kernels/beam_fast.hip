// Kernels of the bf16 fast beam search (Generator::beam_fast, docs/DESIGN.md §4d "Fast bf16 beam search"; the
// rule and CPU twin: cpu_ref.beam_search(round_operands=True)).
//
// beam_head_bf16: logits = h W_fc^T + b_fc for 64 beam rows per workgroup, fused with the log-softmax, the
// candidate scores s_b + lp[c] and the row's top W of them -- the [rows][V] logits of the fp32 loop (a GEMM's
// split-K slabs written and read back every char step) never exist.
//   * geometry and staging are score_head_bf16's: grid Bp / 64, 256 threads; wave w owns rows 16 w .. 16 w + 15
//     and ALL V columns (V / 16 accumulator tiles of v_mfma_f32_16x16x32_bf16), so a row's whole logits line
//     lives in the 16 lanes of one DPP row: lane (lq, lr), register i of tile t holds row 16 w + 4 lq + i,
//     column 16 t + lr.  h and W_fc k-tiles (64 deep) arrive by LDS-DMA in a two-slot ring, XOR-swizzled on the
//     source address so the ds_read_b128 fragment reads are conflict-free; one vmcnt(0) + barrier per k-tile.
//   * a workgroup first looks at its 64 rows' states: without a live row (all dead, finished or padding) it
//     writes the carries and the fill and leaves -- no product.  Late steps of a search are mostly that.
//   * epilogue, in registers, register i at a time (four rows per wave side by side, one per DPP row):
//     + b_fc; max and sum of expf(x - max) over the tiles in order, then the fixed-order DPP reductions;
//     lp = (x - max) - logf(sum); the accumulator register is then OVERWRITTEN by the candidate's order-
//     preserving key (beam.hip's beam_key; 0 = not offered), so the top-W rounds need no further registers.
//     A lane caches its best (key, tile); a round is two DPP row reductions -- the largest key, then the
//     lowest column among its holders: "score descending, c ascending" on s_b + lp[c], the sum, since the
//     addition can create ties that lp alone does not have -- and ONLY the winner's lane clears its entry and
//     rescans its V / 16 registers.  Round k's result is parked in lane k & 15 (two registers for W <= 32) and
//     the row's W entries leave as one coalesced store per array.  The rounds stop as soon as no row of the
//     wave has a candidate left: a forced step costs one round.
// beam_merge: one wave per name.  The W lists (W x W entries, one contiguous block) are staged in LDS; lane b
// holds list b's head; W rounds of a wave arg-max on (key, -j), the winner's lane advances its head.  Since a
// row's list is in the total order restricted to that row, and the name's top W lie in the union of its
// rows' top W, the result is beam_select_f32's selection on the same candidate scores.
// beam_reorder_bf16: beam_reorder's gather plus the bf16 copy of every gathered h row, re-rounded from the
// fp32 row: every step kernel stores h_bf = f2bf(h_f) beside h_f, so f2bf of the gathered fp32 row IS the
// parent's bf16 row, and the kernel reads 4 bytes per element instead of 6.
// No atomics on results: every replay writes the same bytes.
#include <cmath>
#include <stdexcept>
#include "kernels.h"
#include "common.h"
#include "gen_sample.h"

namespace gk {
namespace {

constexpr int kDead = 0, kLive = 1, kFin = 2;   // BeamSelectArgs::state values
typedef __attribute__((address_space(3))) void lds_void_t;

DEV int bh_swz(int r, int c) { return c ^ ((r >> 1) & 7); }

// beam.hip's key: floats -> unsigned with the same order (-0 and +0 share a key); 0 is "no candidate"
DEV unsigned bf_key(float f) {
  unsigned b = __float_as_uint(f);
  if (b == 0x80000000u) b = 0u;
  b = (b >> 31) ? ~b : (b | 0x80000000u);
  return b ? b : 1u;
}
DEV float bf_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

template <int CTRL>
DEV int dppi(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false); }
DEV unsigned umax16(unsigned v) {   // identical in the 16 lanes of a row
  v = max(v, (unsigned)dppi<0xB1>((int)v));
  v = max(v, (unsigned)dppi<0x4E>((int)v));
  v = max(v, (unsigned)dppi<0x141>((int)v));
  v = max(v, (unsigned)dppi<0x140>((int)v));
  return v;
}
DEV int imin16(int v) {
  v = min(v, dppi<0xB1>(v));
  v = min(v, dppi<0x4E>(v));
  v = min(v, dppi<0x141>(v));
  v = min(v, dppi<0x140>(v));
  return v;
}
DEV unsigned wave_umax(unsigned u) {   // identical in every lane
  return ~(unsigned)wave_min_dpp((int)~(u ^ 0x80000000u)) ^ 0x80000000u;
}

template <int NV>   // V = 64 NV
__global__ void __launch_bounds__(256) beam_head_bf16_kernel(BeamHeadArgs a) {
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
    if (__ballot(st == kLive) == 0) {
      if (w == 0 && row < NW) {
        const float sb = a.score_in[row];
        for (int k = 0; k < W; ++k) {
          const bool carry = k == 0 && st == kFin;
          a.cand_score[(size_t)row * W + k] = carry ? sb : -INFINITY;
          a.cand_chr[(size_t)row * W + k] = carry ? 0 : -1;
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
      __builtin_amdgcn_global_load_lds(Am + (size_t)r * H + kt * 64 + bh_swz(r, sslot) * 8,
                                       (lds_void_t*)(&lds[buf][(2 * w + q) * 8 * 64]), 16, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const int r = (NB * w + q) * 8 + srow;  // 0 .. V - 1
      __builtin_amdgcn_global_load_lds(a.Wfc + (size_t)r * H + kt * 64 + bh_swz(r, sslot) * 8,
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
      const bf16x8 af = *reinterpret_cast<const bf16x8*>(&LA[ra * 64 + bh_swz(ra, c) * 8]);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int rb = t * 16 + lr;
        const bf16x8 bfr = *reinterpret_cast<const bf16x8*>(&LB[rb * 64 + bh_swz(rb, c) * 8]);
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
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = b0 + 16 * w + lq * 4 + i;
    const bool real = row < NW;
    const int st = real ? a.state_in[row] : kDead;
    const float sb = real ? a.score_in[row] : -INFINITY;
    const bool live = st == kLive;
    int fc = -1;   // the forced char of a live row
    if (live) {
      const int n = row / W;
      if (a.step < a.plen[n]) {
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
    }
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t) mx = fmaxf(mx, acc[t][i]);
    mx = max16(mx);
    float se = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) se += expf(acc[t][i] - mx);
    se = sum16(se);
    const float lse = logf(se);
    // the candidates' keys replace the logits; the lane's best on the way (ascending c: the first wins)
    unsigned bk = 0u;
    int bt = 0;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int c = t * 16 + lr;
      const float lp = (acc[t][i] - mx) - lse;
      if (a.lp && live) a.lp[(size_t)row * V + c] = lp;
      unsigned k = 0u;
      if (live) {
        if (fc < 0 || c == fc) k = bf_key(sb + lp);
      } else if (st == kFin && c == 0) {
        k = bf_key(sb);   // the carry, j = b V
      }
      acc[t][i] = __uint_as_float(k);
      if (k > bk) { bk = k; bt = t; }
    }
    float os0 = -INFINITY, os1 = -INFINITY;   // rounds lr and lr + 16 of this row
    int oc0 = -1, oc1 = -1;
    for (int k = 0; k < W; ++k) {
      const unsigned wk = umax16(bk);
      if (__ballot(wk != 0u) == 0) break;   // no row of this wave has a candidate left
      const int myc = (wk != 0u && bk == wk) ? bt * 16 + lr : 0x7fffffff;
      const int wc = imin16(myc);
      if (wk != 0u && lr == (k & 15)) {
        if (k < 16) { os0 = bf_unkey(wk); oc0 = wc; }
        else { os1 = bf_unkey(wk); oc1 = wc; }
      }
      if (wk != 0u && myc == wc) {   // the winner's lane takes it out and rescans
        const int rt = bt;
        bk = 0u;
        bt = 0;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const unsigned kk = t == rt ? 0u : __float_as_uint(acc[t][i]);
          acc[t][i] = __uint_as_float(kk);
          if (kk > bk) { bk = kk; bt = t; }
        }
      }
    }
    if (real) {
      if (lr < W) { a.cand_score[(size_t)row * W + lr] = os0; a.cand_chr[(size_t)row * W + lr] = oc0; }
      if (lr + 16 < W) { a.cand_score[(size_t)row * W + lr + 16] = os1; a.cand_chr[(size_t)row * W + lr + 16] = oc1; }
    }
  }
}

// four names per workgroup, a wave each
__global__ void __launch_bounds__(256) beam_merge_kernel(BeamMergeArgs a) {
  __shared__ float s_sc[4][32 * 32];
  __shared__ int s_c[4][32 * 32];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int n = blockIdx.x * 4 + w, W = a.W, V = a.V;
  const bool active = n < a.N;
  if (active) {
    const size_t base = (size_t)n * W * W;   // the name's W lists are one block
    for (int i = lane; i < W * W; i += 64) { s_sc[w][i] = a.cand_score[base + i]; s_c[w][i] = a.cand_chr[base + i]; }
  }
  __syncthreads();
  if (!active) return;
  const size_t r0 = (size_t)n * W;
  int p = 0;   // lane b < W: the head of list b
  unsigned hk = 0u;
  int hj = 0x7fffffff;
  auto head = [&]() {
    hk = 0u;
    hj = 0x7fffffff;
    if (lane < W && p < W) {
      const int c = s_c[w][lane * W + p];
      if (c >= 0) { hk = bf_key(s_sc[w][lane * W + p]); hj = lane * V + c; }
    }
  };
  head();
  unsigned mk = 0u;   // lane k: round k's winner
  int mj = -1;
  for (int k = 0; k < W; ++k) {
    const unsigned wk = wave_umax(hk);
    const int wj = wave_min_dpp((wk != 0u && hk == wk) ? hj : 0x7fffffff);
    if (lane == k) { mk = wk; mj = wj; }
    if (wk == 0u) break;   // wave-uniform: nothing left
    if (hk == wk && hj == wj) { ++p; head(); }
  }
  if (lane < W) {
    const bool any = mk != 0u;
    const int pb = any ? mj / V : 0, pc = any ? mj - pb * V : 0;
    float sc = -INFINITY;
    int parent = -1, ch = -1, st = kDead, nxt = a.sos;
    if (any) {
      parent = pb;
      if (a.state_in[r0 + pb] == kFin) {
        sc = a.score_in[r0 + pb]; st = kFin;
      } else {
        sc = bf_unkey(mk);
        ch = pc;
        st = pc == a.eos ? kFin : kLive;
        if (st == kLive) nxt = pc;
      }
    }
    const size_t o = r0 + lane;
    a.score_out[o] = sc; a.parent[o] = parent; a.chr[o] = ch; a.state_out[o] = st; a.next_id[o] = nxt;
    if (a.sel) a.sel[o] = any ? mj : -1;
  }
}

// grid (N, L + 1): y < L gathers layer y's hidden rows (fp32, and their bf16 rounding), y == L the output
// rows, lengths, ids and count
__global__ void __launch_bounds__(256) beam_reorder_bf16_kernel(BeamReorderBf16Args a) {
  const int n = blockIdx.x, y = blockIdx.y, W = a.W, t = threadIdx.x;
  const size_t r0 = (size_t)n * W;
  if (y < a.L) {
    typedef unsigned u32x2_ __attribute__((ext_vector_type(2)));
    const int H4 = a.H / 4;
    const float4* src = reinterpret_cast<const float4*>(a.h_src[y]);
    float4* dst = reinterpret_cast<float4*>(a.h_dst[y]);
    u32x2_* dstb = reinterpret_cast<u32x2_*>(a.hb_dst[y]);
    for (int i = t; i < W * H4; i += blockDim.x) {
      const int k = i / H4, c = i - k * H4;
      const int p = a.parent[r0 + k];
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);   // a dead beam's state
      if (p >= 0 && p < W) v = src[(r0 + p) * H4 + c];
      dst[(r0 + k) * H4 + c] = v;
      dstb[(r0 + k) * H4 + c] = u32x2_{(unsigned)f2bf(v.x) | ((unsigned)f2bf(v.y) << 16),
                                       (unsigned)f2bf(v.z) | ((unsigned)f2bf(v.w) << 16)};
    }
    return;
  }
  const int RL = a.max_len + 1;
  for (int i = t; i < W * RL; i += blockDim.x) {
    const int k = i / RL, c = i - k * RL;
    const int p = a.parent[r0 + k];
    unsigned char v = 0;
    if (p >= 0 && p < W) {
      const int len = a.len_src[r0 + p], ch = a.chr[r0 + k];
      v = a.rows_src[(r0 + p) * RL + c];
      if (ch >= 0 && c == len && len < a.max_len) v = (unsigned char)ch;
    }
    a.rows_dst[(r0 + k) * RL + c] = v;
  }
  int live = 0;
  for (int k = t; k < W; k += blockDim.x) {
    const int p = a.parent[r0 + k];
    int len = 0;
    if (p >= 0 && p < W) {
      len = a.len_src[r0 + p];
      if (a.chr[r0 + k] >= 0 && len < a.max_len) ++len;
      ++live;
    }
    a.len_dst[r0 + k] = len;
    a.ids[r0 + k] = a.next_id[r0 + k];
  }
  if (t < 64) {   // W <= 32: the counts live in wave 0
    const int cnt = __popcll(__ballot(live != 0));
    if (t == 0) a.n_beams[n] = cnt;
  }
}

}  // namespace

bool beam_head_supported(int H, int V, int ML) {
  return H >= 64 && H % 64 == 0 && V >= 64 && V % 64 == 0 && V <= 512 && ML >= 1 && ML <= 64;
}

void beam_head_bf16(const BeamHeadArgs& a, hipStream_t s) {
  if (!beam_head_supported(a.H, a.V, a.max_len))
    throw std::runtime_error("beam_head_bf16: needs H % 64 == 0, V % 64 == 0, V <= 512 and 0 < max_len <= 64");
  if (a.W < 1 || a.W > 32 || a.W > a.V) throw std::runtime_error("beam_head_bf16: needs 1 <= W <= min(32, V)");
  if (a.Bp <= 0 || a.Bp % 64 || a.N < 0 || (long)a.N * a.W > a.Bp)
    throw std::runtime_error("beam_head_bf16: needs Bp > 0, Bp % 64 == 0 and N W <= Bp");
  if (a.step < 0 || a.step >= a.max_len) throw std::runtime_error("beam_head_bf16: needs 0 <= step < max_len");
  if (!a.h || !a.Wfc || !a.bfc || !a.score_in || !a.state_in || !a.plen || !a.prefix || !a.cand_score || !a.cand_chr)
    throw std::runtime_error("beam_head_bf16: h, Wfc, bfc, scores, states, plen, prefix, cand_score and cand_chr are required");
  if (a.N == 0) return;
  const dim3 grid(a.Bp / 64), block(256);
  switch (a.V / 64) {
#define BH_CASE(NVV) case NVV: hipLaunchKernelGGL(beam_head_bf16_kernel<NVV>, grid, block, 0, s, a); break;
    BH_CASE(1) BH_CASE(2) BH_CASE(3) BH_CASE(4) BH_CASE(5) BH_CASE(6) BH_CASE(7) BH_CASE(8)
#undef BH_CASE
  }
}

void beam_merge(const BeamMergeArgs& a, hipStream_t s) {
  if (a.W < 1 || a.W > 32 || a.W > a.V || a.V <= 0)
    throw std::runtime_error("beam_merge: needs 1 <= W <= min(32, V)");
  if (!a.cand_score || !a.cand_chr || !a.score_in || !a.state_in || !a.score_out || !a.parent || !a.chr ||
      !a.state_out || !a.next_id)
    throw std::runtime_error("beam_merge: the candidate lists, scores, states and the five outputs are required");
  if (a.score_in == a.score_out || a.state_in == a.state_out)
    throw std::runtime_error("beam_merge: the new beams' scores and states never overwrite the inputs");
  if (a.eos < 0 || a.sos < 0 || a.sos >= a.V) throw std::runtime_error("beam_merge: needs eos >= 0 and 0 <= sos < V");
  if (a.N <= 0) return;
  hipLaunchKernelGGL(beam_merge_kernel, dim3((a.N + 3) / 4), dim3(256), 0, s, a);
}

void beam_reorder_bf16(const BeamReorderBf16Args& a, hipStream_t s) {
  if (a.W < 1 || a.W > 32 || a.L < 1 || a.L > 4 || a.H <= 0 || a.H % 4 || a.max_len <= 0)
    throw std::runtime_error("beam_reorder_bf16: needs 1 <= W <= 32, 1 <= L <= 4, H % 4 == 0 and max_len > 0");
  for (int l = 0; l < a.L; ++l)
    if (!a.h_src[l] || !a.h_dst[l] || !a.hb_dst[l] || a.h_src[l] == a.h_dst[l])
      throw std::runtime_error("beam_reorder_bf16: L source, L fp32 and L bf16 destination slots, never in place");
  if (!a.parent || !a.chr || !a.next_id || !a.rows_src || !a.rows_dst || a.rows_src == a.rows_dst || !a.len_src ||
      !a.len_dst || a.len_src == a.len_dst || !a.ids || !a.n_beams)
    throw std::runtime_error("beam_reorder_bf16: parent, chr, next_id, two row buffers, two length buffers, ids and n_beams are required");
  if (a.N <= 0) return;
  hipLaunchKernelGGL(beam_reorder_bf16_kernel, dim3(a.N, a.L + 1), dim3(256), 0, s, a);
}

}  // namespace gk

// Stochastic beam search over the fp32 per-char path (Generator::distinct, docs/DESIGN.md §4i; the rule
// and the CPU twin: cpu_ref.sample_distinct / cpu_ref.sbs_step, the per-element reference models/sbs_ref.py).
//
// sbs_select_f32 is beam_select_f32's selection (beam.hip: one workgroup per name, a wave per slot row or
// two, V / 64 chars per lane, W rounds of a block-wide arg-max through double-buffered LDS slots) on other
// keys.  Per live slot b the row's logits become the SAMPLER's log-probabilities lq -- scaled by the name's
// 1 / T, renormalised over the allowed set -- every child j = b V + c gets a Gumbel perturbation from one
// 32-bit word of Philox-4x32-10 (key: the seed; counter: (j >> 2, step, the name's global index)), and the
// perturbed values g = (logq_b + lq[c]) + gum are truncated onto the parent's own perturbed value G_b:
//     d = g - Z (Z: the row's max),  v = (G_b - g) + log1mexp(d),  Gt = (G_b - max(0, v)) - log1p(exp(-|v|))
// so that the best child keeps Gt == G_b bitwise and no child lies above its parent.  The candidates are
// kept as order-preserving keys of Gt (0: not offered) and their psi = logq_b + lq[c] beside them: a key
// gives the winner's Gt back, but not its logq, so a wave publishes its best candidate's psi with the slot.
// seed, start and 1 / T are read from device memory: one recording serves every seed and temperature.
// No global memory inside the rounds, no atomics but the error word, no cross-workgroup communication.
#include <cmath>
#include <stdexcept>
#include "kernels.h"
#include "common.h"
#include "gen_sample.h"

#pragma clang fp contract(off)

namespace gk {

namespace {
constexpr int kDead = 0, kLive = 1, kFin = 2;   // SbsSelectArgs::state values (BeamSelectArgs')
constexpr int kMaxWaves = 16;

// floats -> unsigned keys with the same order (-0 and +0 share a key); 0 is kept free for "no candidate"
DEV unsigned sbs_key(float f) {
  unsigned b = __float_as_uint(f);
  if (b == 0x80000000u) b = 0u;
  b = (b >> 31) ? ~b : (b | 0x80000000u);
  return b ? b : 1u;
}
DEV float sbs_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
DEV unsigned sbs_umax(unsigned u) {   // identical in every lane
  return ~(unsigned)wave_min_dpp((int)~(u ^ 0x80000000u)) ^ 0x80000000u;
}

// the truncated perturbed value of a child: g its own, Z its row's maximum, Gb the parent's
DEV float sbs_truncate(float Gb, float g, float Z) {
  const float d = g - Z;   // <= 0
  const float l1 = d == 0.f ? -INFINITY : (d > -0.6931f ? logf(-expm1f(d)) : log1pf(-expf(d)));
  const float v = (Gb - g) + l1;
  return (Gb - fmaxf(0.f, v)) - log1pf(expf(-fabsf(v)));
}
}  // namespace

// R: slot rows per wave (wave w owns slots w and w + nw), MAXPER: logits per lane and row
template <int R, int MAXPER, bool MASK, bool AUTO = false>
__global__ void __launch_bounds__(1024) sbs_select_f32_kernel(SbsSelectArgs a) {
#pragma clang fp contract(off)
  __shared__ unsigned s_key[2][kMaxWaves];
  __shared__ int s_j[2][kMaxWaves];
  __shared__ float s_psi[2][kMaxWaves];
  __shared__ unsigned s_wk[32];   // the rounds' winners
  __shared__ int s_wj[32];
  __shared__ float s_wpsi[32];
  const int n = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int V = a.V, W = a.W, per = V / 64;
  const int pl = a.plen[n];
  const bool forced = a.step < pl;
  int fc = 0;
  if (forced) {
    fc = a.prefix[(size_t)n * a.max_len + a.step];
    if (fc >= V) {   // never expected (the host checks first): flag it instead of offering it
      if (a.err && threadIdx.x == 0) {
        atomicOr(a.err, 16u);
        a.err[1] = (unsigned)fc;
        a.err[2] = (unsigned)(n * W);
      }
      fc = 0;
    }
  }
  unsigned ok = 0u;   // MASK: bit e = this lane's char e is allowed
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
    ok = a.allow_tab[(size_t)ar * (V >> 5) + ((lane * per) >> 5)] >> ((lane * per) & 31);
  }
  const float inv_t = a.inv_t[n];
  const unsigned long long seed = *a.seed, gidx = *a.start + (unsigned long long)n;
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32), g0 = (unsigned)gidx, g1 = (unsigned)(gidx >> 32);
  // candidates of this wave's rows: key 0 = not offered; psi = the child's logq
  unsigned key[R][MAXPER];
  float psi[R][MAXPER];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int b = w + r * nw;
#pragma unroll
    for (int e = 0; e < MAXPER; ++e) { key[r][e] = 0u; psi[r][e] = -INFINITY; }
    if (b >= W) continue;
    const size_t row = (size_t)n * W + b;
    const float* x = a.logits + row * V + lane * per;
    const float qb = a.logq_in[row], Gb = a.G_in[row];
    const int st = a.state_in[row];
    if constexpr (AUTO) {   // this row's line
      int q = a.allow_state_in[row];
      if (q < 0 || q >= a.allow_rows) {   // never expected (the host builds start and next): flag it, the free state
        if (a.err && lane == 0) {
          atomicOr(a.err, 16u);
          a.err[1] = (unsigned)q;
          a.err[2] = (unsigned)row;
        }
        q = 0;
      }
      ok = a.allow_tab[(size_t)q * (V >> 5) + ((lane * per) >> 5)] >> ((lane * per) & 31);
    }
    float y[MAXPER];
    bool al[MAXPER];   // in the allowed set
#pragma unroll
    for (int e = 0; e < MAXPER; ++e) {
      al[e] = e < per && (!MASK || ((ok >> e) & 1u));
      if (e < per) {
        float v = x[e];
        for (int s2 = 1; s2 < a.splits; ++s2) v += x[s2 * a.slab + e];   // split-K slabs, fixed order
        if (a.bias) v += a.bias[lane * per + e];
        y[e] = v * inv_t;
      } else {
        y[e] = -INFINITY;
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < MAXPER; ++e) mx = fmaxf(mx, al[e] ? y[e] : -INFINITY);
    mx = wave_max_dpp(mx);
    float se = 0.f;
#pragma unroll
    for (int e = 0; e < MAXPER; ++e) se += al[e] ? expf(y[e] - mx) : 0.f;
    se = wave_sum_dpp(se);
    const float lse = logf(se);
    // the children's perturbed values; one Philox call covers four consecutive j
    float g[MAXPER];
    bool off[MAXPER];
    unsigned wd[4] = {0u, 0u, 0u, 0u};
    int blk = -1;
    float Z = -INFINITY;
#pragma unroll
    for (int e = 0; e < MAXPER; ++e) {
      off[e] = false;
      g[e] = -INFINITY;
      if (e >= per) continue;
      const int c = lane * per + e;
      const float lq = (y[e] - mx) - lse;
      if (a.lq) a.lq[row * V + c] = al[e] ? lq : NAN;
      if (st == kLive) {
        off[e] = al[e] && (!forced || c == fc);
        const int j = b * V + c;
        if ((j >> 2) != blk) {
          blk = j >> 2;
          philox4x32_10((unsigned)blk, (unsigned)a.step, g0, g1, k0, k1, wd);
        }
        const int q4 = j & 3;
        const unsigned word = q4 == 0 ? wd[0] : q4 == 1 ? wd[1] : q4 == 2 ? wd[2] : wd[3];
        const float u = (float)(2u * (word >> 9) + 1u) * 0x1p-24f;   // exact, in [2^-24, 1 - 2^-24]
        const float gum = -logf(-logf(u));
        psi[r][e] = qb + (forced ? 0.f : lq);
        g[e] = psi[r][e] + gum;
        if (off[e]) Z = fmaxf(Z, g[e]);
      }
    }
    Z = wave_max_dpp(Z);
    if (a.zmax && lane == 0) a.zmax[row] = (st == kLive && Z != -INFINITY) ? Z : NAN;
#pragma unroll
    for (int e = 0; e < MAXPER; ++e) {
      if (e >= per) continue;
      const int c = lane * per + e;
      float gt = NAN;
      if (off[e]) {
        gt = sbs_truncate(Gb, g[e], Z);
        key[r][e] = sbs_key(gt);
      } else if (st == kFin && c == 0) {   // the carry, j = b V
        gt = Gb;
        key[r][e] = sbs_key(Gb);
        psi[r][e] = qb;
      }
      if (a.gt) a.gt[row * V + c] = gt;
    }
  }
  // this wave's best: the largest key, then the lowest j; its psi goes with it
  auto wave_best = [&](unsigned& bk, int& bj, float& bp) {
    unsigned lk = 0u;
    int lj = 0x7fffffff;
    float lp = -INFINITY;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int e = 0; e < MAXPER; ++e)
        if (key[r][e] > lk) { lk = key[r][e]; lj = (w + r * nw) * V + lane * per + e; lp = psi[r][e]; }   // ascending j: first wins
    bk = sbs_umax(lk);
    bj = wave_min_dpp((lk == bk && bk != 0u) ? lj : 0x7fffffff);
    bp = wave_max_dpp((lk == bk && lj == bj && bk != 0u) ? lp : -INFINITY);   // one lane owns (bk, bj)
  };
  unsigned bk;
  int bj;
  float bp;
  wave_best(bk, bj, bp);
  if (lane == 0) { s_key[0][w] = bk; s_j[0][w] = bj; s_psi[0][w] = bp; }
  if (threadIdx.x >= nw && threadIdx.x < kMaxWaves) {   // unused slots: never a candidate (a round reads all 16)
    s_key[0][threadIdx.x] = s_key[1][threadIdx.x] = 0u;
    s_j[0][threadIdx.x] = s_j[1][threadIdx.x] = 0x7fffffff;
    s_psi[0][threadIdx.x] = s_psi[1][threadIdx.x] = -INFINITY;
  }
  __syncthreads();
  for (int k = 0; k < W; ++k) {
    const int cur = k & 1;
    // every wave reduces the 16 slots itself, a lane per slot
    const unsigned ki = lane < kMaxWaves ? s_key[cur][lane] : 0u;
    const int ji = lane < kMaxWaves ? s_j[cur][lane] : 0x7fffffff;
    const unsigned wk = sbs_umax(ki);
    const int wj = wave_min_dpp((ki == wk && wk != 0u) ? ji : 0x7fffffff);
    const bool any = wk != 0u;
    const int pb = any ? wj / V : 0, pc = any ? wj - pb * V : 0;
    if (threadIdx.x == 0) { s_wk[k] = wk; s_wj[k] = wj; s_wpsi[k] = any ? s_psi[cur][pb % nw] : -INFINITY; }
    if (any && (pb % nw) == w) {   // the owner takes it out and rescans (wave-uniform branch)
      const int r = pb / nw, e = pc - lane * per;
#pragma unroll
      for (int rr = 0; rr < R; ++rr)
#pragma unroll
        for (int ee = 0; ee < MAXPER; ++ee)
          if (rr == r && ee == e) key[rr][ee] = 0u;
      wave_best(bk, bj, bp);
    }
    if (lane == 0) { s_key[cur ^ 1][w] = bk; s_j[cur ^ 1][w] = bj; s_psi[cur ^ 1][w] = bp; }
    __syncthreads();
  }
  // the W winners' outputs, one thread each (the rounds above touch no global memory)
  if (threadIdx.x < W) {
    const int k = threadIdx.x;
    const unsigned wk = s_wk[k];
    const int wj = s_wj[k];
    const bool any = wk != 0u;
    const int pb = any ? wj / V : 0, pc = any ? wj - pb * V : 0;
    const size_t o = (size_t)n * W + k;
    float lq = -INFINITY, G = -INFINITY;
    int parent = -1, ch = -1, st = kDead, nxt = a.sos;
    int qn = 0;   // AUTO: the child's automaton state
    if (any) {
      const size_t prow = (size_t)n * W + pb;
      parent = pb;
      if (a.state_in[prow] == kFin) {
        lq = a.logq_in[prow]; G = a.G_in[prow]; st = kFin;
      } else {
        if constexpr (AUTO) {
          int q = a.allow_state_in[prow];
          if (q < 0 || q >= a.allow_rows) q = 0;   // (flagged above)
          qn = a.allow_next[(size_t)q * V + pc];
        }
        lq = s_wpsi[k];          // psi of step 4, bit for bit: the owner's register
        G = sbs_unkey(wk);       // the key keeps every bit of Gt but the sign of zero
        ch = pc;
        st = pc == a.eos ? kFin : kLive;
        if (st == kLive) nxt = pc;
      }
    }
    a.logq_out[o] = lq; a.G_out[o] = G; a.parent[o] = parent; a.chr[o] = ch; a.state_out[o] = st; a.next_id[o] = nxt;
    if (a.sel) a.sel[o] = any ? wj : -1;
    if constexpr (AUTO) a.allow_state_out[o] = qn;
  }
}

// seed and start into their device words, from kernel arguments: stream-ordered, no host buffer to keep alive
__global__ void sbs_stage_kernel(unsigned long long* seed, unsigned long long seed_v, unsigned long long* start,
                                 unsigned long long start_v) {
  if (threadIdx.x == 0 && blockIdx.x == 0) { *seed = seed_v; *start = start_v; }
}

void sbs_stage(unsigned long long* seed, unsigned long long seed_v, unsigned long long* start, unsigned long long start_v,
               hipStream_t s) {
  if (!seed || !start) throw std::runtime_error("sbs_stage: seed and start are required");
  hipLaunchKernelGGL(sbs_stage_kernel, dim3(1), dim3(64), 0, s, seed, seed_v, start, start_v);
}

void sbs_select_f32(const SbsSelectArgs& a, hipStream_t s) {
  if (a.V % 64 || a.V > 512 || a.V <= 0) throw std::runtime_error("sbs_select_f32: needs V % 64 == 0 and V <= 512");
  if (a.W < 1 || a.W > 32 || a.W > a.V) throw std::runtime_error("sbs_select_f32: needs 1 <= W <= min(32, V)");
  if (!a.logits || !a.logq_in || !a.G_in || !a.state_in || !a.plen || !a.prefix || !a.logq_out || !a.G_out || !a.parent ||
      !a.chr || !a.state_out || !a.next_id || !a.seed || !a.start || !a.inv_t)
    throw std::runtime_error("sbs_select_f32: logits, logq, G, states, plen, prefix, seed, start, inv_t and the six outputs "
                             "are required");
  if (a.logq_in == a.logq_out || a.G_in == a.G_out || a.G_in == a.logq_out || a.logq_in == a.G_out ||
      a.logq_out == a.G_out || a.state_in == a.state_out)
    throw std::runtime_error("sbs_select_f32: the new slots' logq, G and states never overwrite the inputs");
  if (a.step < 0 || a.step >= a.max_len || a.eos < 0 || a.sos < 0 || a.sos >= a.V)
    throw std::runtime_error("sbs_select_f32: needs 0 <= step < max_len, eos >= 0 and 0 <= sos < V");
  if (a.splits < 1 || (a.splits > 1 && a.slab < (long)a.N * a.W * a.V))
    throw std::runtime_error("sbs_select_f32: split-K slabs overlap");
  const bool aut = a.allow_state_in || a.allow_state_out || a.allow_next;
  if (aut && (!a.allow_state_in || !a.allow_state_out || !a.allow_next || !a.allow_tab || a.allow_idx ||
              a.allow_state_in == a.allow_state_out || a.allow_rows > 65535 || (a.V != 256 && a.V != 512)))
    throw std::runtime_error("sbs_select_f32: an automaton needs allow_state_in, allow_state_out (another buffer), "
                             "allow_next and allow_tab, no allow_idx, at most 65535 states and V = 256 or 512");
  if (!aut && (a.allow_tab != nullptr) != (a.allow_idx != nullptr))
    throw std::runtime_error("sbs_select_f32: allow_tab and allow_idx are set together or not at all");
  const bool mask = a.allow_tab != nullptr;
  if (mask && (a.allow_rows < 1 || 32 % (a.V / 64)))
    throw std::runtime_error("sbs_select_f32: constraints need allow_rows >= 1 and V / 64 in {1, 2, 4, 8}");
  if (a.N <= 0) return;
  const int nw = a.W <= kMaxWaves ? a.W : kMaxWaves;
  const dim3 grid(a.N), block(64 * nw);
  if (aut) {
    if (a.W <= kMaxWaves) {
      if (a.V <= 256) hipLaunchKernelGGL((sbs_select_f32_kernel<1, 4, true, true>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((sbs_select_f32_kernel<1, 8, true, true>), grid, block, 0, s, a);
    } else {
      if (a.V <= 256) hipLaunchKernelGGL((sbs_select_f32_kernel<2, 4, true, true>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((sbs_select_f32_kernel<2, 8, true, true>), grid, block, 0, s, a);
    }
  } else if (mask) {
    if (a.W <= kMaxWaves) {
      if (a.V <= 256) hipLaunchKernelGGL((sbs_select_f32_kernel<1, 4, true>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((sbs_select_f32_kernel<1, 8, true>), grid, block, 0, s, a);
    } else {
      if (a.V <= 256) hipLaunchKernelGGL((sbs_select_f32_kernel<2, 4, true>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((sbs_select_f32_kernel<2, 8, true>), grid, block, 0, s, a);
    }
  } else if (a.W <= kMaxWaves) {
    if (a.V <= 256) hipLaunchKernelGGL((sbs_select_f32_kernel<1, 4, false>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((sbs_select_f32_kernel<1, 8, false>), grid, block, 0, s, a);
  } else {
    if (a.V <= 256) hipLaunchKernelGGL((sbs_select_f32_kernel<2, 4, false>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((sbs_select_f32_kernel<2, 8, false>), grid, block, 0, s, a);
  }
}

}  // namespace gk

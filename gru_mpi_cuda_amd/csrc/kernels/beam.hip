// Beam search over the fp32 per-char path (Generator::beam, docs/DESIGN.md §4d; the CPU twin and
// oracle is cpu_ref.beam_search, the per-element reference models/beam_ref.py).
//
// A name owns W ordered beams = W consecutive rows of the batch.  Per char, after the model's step:
//   * beam_select_f32 (one workgroup per name): the log-softmax of the name's W logits rows, the
//     candidates j = b V + c with score s_b + lp[c], and the first W of them in the total order
//     "score descending, then j ascending";
//   * beam_reorder: the winners' parents' hidden rows and output rows gathered into the next step's
//     slots (never in place: a parent may be a row that was already overwritten), the char appended.
//   * beam_reset: the state before step 0, as one kernel node.
//
// The selection is W rounds of a block-wide arg-max on the key (order_key(score), -j) -- the simpler
// of the two shapes the design names.  A wave owns one or two beam rows and keeps their candidates in
// registers (V / 64 per lane and row); a round reads the waves' current bests from LDS (a lane per
// slot, reduced inside every wave, so all derive the same winner), and only the wave that owned the
// winner rescans its registers.  One barrier per round and no global memory inside the rounds, no
// atomics on results, no cross-workgroup communication; every cross-lane statistic is one of the
// fixed-order DPP helpers of gen_sample.h, in score_logprob_f32's order of operations.
//
// Constraints (docs/DESIGN.md §4e, the MASK instantiations): the name's allowed chars at this step are
// one line of a bit table; a lane loads the one word that covers its V/64 chars once, before the rows,
// and a live beam's masked candidate keeps key 0.  Carries are not masked.  MASK = false is the kernel
// as it was.
//
// Automaton (docs/DESIGN.md §4g, the AUTO instantiations, always with MASK): every beam row has a state
// of its own, so the word is loaded per row, from the line its state names; the winners' threads write
// the children's states -- allow_next[parent's line][chr], 0 for a carry or a dead slot -- into the
// other state buffer, as the reorder gathers h.  AUTO = false is the kernel as it was.
#include <cmath>
#include <stdexcept>
#include "kernels.h"
#include "common.h"
#include "gen_sample.h"

namespace gk {

namespace {
constexpr int kDead = 0, kLive = 1, kFin = 2;   // BeamSelectArgs::state values
constexpr int kMaxWaves = 16;

// floats -> unsigned keys with the same order (-0 and +0 share a key); 0 is kept free for "no candidate"
DEV unsigned beam_key(float f) {
  unsigned b = __float_as_uint(f);
  if (b == 0x80000000u) b = 0u;
  b = (b >> 31) ? ~b : (b | 0x80000000u);
  return b ? b : 1u;
}
DEV unsigned wave_umax(unsigned u) {   // identical in every lane
  return ~(unsigned)wave_min_dpp((int)~(u ^ 0x80000000u)) ^ 0x80000000u;
}
}  // namespace

// R: beam rows per wave (wave w owns beams w and w + nw), MAXPER: logits per lane and row
template <int R, int MAXPER, bool MASK, bool AUTO = false>
__global__ void __launch_bounds__(1024) beam_select_f32_kernel(BeamSelectArgs a) {
#pragma clang fp contract(off)
  __shared__ unsigned s_key[2][kMaxWaves];
  __shared__ int s_j[2][kMaxWaves];
  __shared__ unsigned s_wk[32];   // the rounds' winners
  __shared__ int s_wj[32];
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
  // candidates of this wave's rows: key 0 = not offered
  unsigned key[R][MAXPER];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int b = w + r * nw;
#pragma unroll
    for (int e = 0; e < MAXPER; ++e) key[r][e] = 0u;
    if (b >= W) continue;
    const size_t row = (size_t)n * W + b;
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
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < MAXPER; ++e) mx = fmaxf(mx, xv[e]);
    mx = wave_max_dpp(mx);
    float se = 0.f;
#pragma unroll
    for (int e = 0; e < MAXPER; ++e) se += e < per ? expf(xv[e] - mx) : 0.f;
    se = wave_sum_dpp(se);
    const float lse = logf(se);
    const float sb = a.score_in[row];
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
#pragma unroll
    for (int e = 0; e < MAXPER; ++e) {
      if (e >= per) continue;
      const int c = lane * per + e;
      const float lp = (xv[e] - mx) - lse;
      if (a.lp) a.lp[row * V + c] = lp;
      if (st == kLive) {
        if ((!forced || c == fc) && (!MASK || ((ok >> e) & 1u))) key[r][e] = beam_key(sb + lp);
      } else if (st == kFin && c == 0) {
        key[r][e] = beam_key(sb);   // the carry, j = b V
      }
    }
  }
  // this wave's best: the largest key, then the lowest j
  auto wave_best = [&](unsigned& bk, int& bj) {
    unsigned lk = 0u;
    int lj = 0x7fffffff;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int e = 0; e < MAXPER; ++e)
        if (key[r][e] > lk) { lk = key[r][e]; lj = (w + r * nw) * V + lane * per + e; }   // ascending j: first wins
    bk = wave_umax(lk);
    bj = wave_min_dpp((lk == bk && bk != 0u) ? lj : 0x7fffffff);
  };
  unsigned bk;
  int bj;
  wave_best(bk, bj);
  if (lane == 0) { s_key[0][w] = bk; s_j[0][w] = bj; }
  if (threadIdx.x >= nw && threadIdx.x < kMaxWaves) {   // unused slots: never a candidate (a round reads all 16)
    s_key[0][threadIdx.x] = s_key[1][threadIdx.x] = 0u;
    s_j[0][threadIdx.x] = s_j[1][threadIdx.x] = 0x7fffffff;
  }
  __syncthreads();
  for (int k = 0; k < W; ++k) {
    const int cur = k & 1;
    // every wave reduces the 16 slots itself, a lane per slot: two LDS reads per wave and round
    const unsigned ki = lane < kMaxWaves ? s_key[cur][lane] : 0u;
    const int ji = lane < kMaxWaves ? s_j[cur][lane] : 0x7fffffff;
    const unsigned wk = wave_umax(ki);
    const int wj = wave_min_dpp((ki == wk && wk != 0u) ? ji : 0x7fffffff);
    const bool any = wk != 0u;
    const int pb = any ? wj / V : 0, pc = any ? wj - pb * V : 0;
    if (any && (pb % nw) == w) {   // the owner takes it out and rescans (wave-uniform branch)
      const int r = pb / nw, e = pc - lane * per;
#pragma unroll
      for (int rr = 0; rr < R; ++rr)
#pragma unroll
        for (int ee = 0; ee < MAXPER; ++ee)
          if (rr == r && ee == e) key[rr][ee] = 0u;
      wave_best(bk, bj);
    }
    if (lane == 0) { s_key[cur ^ 1][w] = bk; s_j[cur ^ 1][w] = bj; }
    if (threadIdx.x == 0) { s_wk[k] = wk; s_wj[k] = wj; }
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
    float sc = -INFINITY;
    int parent = -1, ch = -1, st = kDead, nxt = a.sos;
    int qn = 0;   // AUTO: the child's automaton state
    if (any) {
      const size_t prow = (size_t)n * W + pb;
      parent = pb;
      if (a.state_in[prow] == kFin) {
        sc = a.score_in[prow]; st = kFin;
      } else {
        if constexpr (AUTO) {
          int q = a.allow_state_in[prow];
          if (q < 0 || q >= a.allow_rows) q = 0;   // (flagged above)
          qn = a.allow_next[(size_t)q * V + pc];
        }
        // the candidate's score back from its key (the key keeps every bit but the sign of zero)
        sc = __uint_as_float((wk & 0x80000000u) ? (wk & 0x7fffffffu) : ~wk);
        ch = pc;
        st = pc == a.eos ? kFin : kLive;
        if (st == kLive) nxt = pc;
      }
    }
    a.score_out[o] = sc; a.parent[o] = parent; a.chr[o] = ch; a.state_out[o] = st; a.next_id[o] = nxt;
    if (a.sel) a.sel[o] = any ? wj : -1;
    if constexpr (AUTO) a.allow_state_out[o] = qn;
  }
}

void beam_select_f32(const BeamSelectArgs& a, hipStream_t s) {
  if (a.V % 64 || a.V > 512 || a.V <= 0) throw std::runtime_error("beam_select_f32: needs V % 64 == 0 and V <= 512");
  if (a.W < 1 || a.W > 32 || a.W > a.V) throw std::runtime_error("beam_select_f32: needs 1 <= W <= min(32, V)");
  if (!a.logits || !a.score_in || !a.state_in || !a.plen || !a.prefix || !a.score_out || !a.parent || !a.chr ||
      !a.state_out || !a.next_id)
    throw std::runtime_error("beam_select_f32: logits, scores, states, plen, prefix and the five outputs are required");
  if (a.score_in == a.score_out || a.state_in == a.state_out)
    throw std::runtime_error("beam_select_f32: the new beams' scores and states never overwrite the inputs");
  if (a.step < 0 || a.step >= a.max_len || a.eos < 0 || a.sos < 0 || a.sos >= a.V)
    throw std::runtime_error("beam_select_f32: needs 0 <= step < max_len, eos >= 0 and 0 <= sos < V");
  if (a.splits < 1 || (a.splits > 1 && a.slab < (long)a.N * a.W * a.V))
    throw std::runtime_error("beam_select_f32: split-K slabs overlap");
  const bool aut = a.allow_state_in || a.allow_state_out || a.allow_next;
  if (aut && (!a.allow_state_in || !a.allow_state_out || !a.allow_next || !a.allow_tab || a.allow_idx ||
              a.allow_state_in == a.allow_state_out || a.allow_rows > 65535 || (a.V != 256 && a.V != 512)))
    throw std::runtime_error("beam_select_f32: an automaton needs allow_state_in, allow_state_out (another buffer), "
                             "allow_next and allow_tab, no allow_idx, at most 65535 states and V = 256 or 512");
  if (!aut && (a.allow_tab != nullptr) != (a.allow_idx != nullptr))
    throw std::runtime_error("beam_select_f32: allow_tab and allow_idx are set together or not at all");
  const bool mask = a.allow_tab != nullptr;
  if (mask && (a.allow_rows < 1 || 32 % (a.V / 64)))
    throw std::runtime_error("beam_select_f32: constraints need allow_rows >= 1 and V / 64 in {1, 2, 4, 8}");
  if (a.N <= 0) return;
  const int nw = a.W <= kMaxWaves ? a.W : kMaxWaves;
  const dim3 grid(a.N), block(64 * nw);
  if (aut) {
    if (a.W <= kMaxWaves) {
      if (a.V <= 256) hipLaunchKernelGGL((beam_select_f32_kernel<1, 4, true, true>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((beam_select_f32_kernel<1, 8, true, true>), grid, block, 0, s, a);
    } else {
      if (a.V <= 256) hipLaunchKernelGGL((beam_select_f32_kernel<2, 4, true, true>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((beam_select_f32_kernel<2, 8, true, true>), grid, block, 0, s, a);
    }
  } else if (mask) {
    if (a.W <= kMaxWaves) {
      if (a.V <= 256) hipLaunchKernelGGL((beam_select_f32_kernel<1, 4, true>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((beam_select_f32_kernel<1, 8, true>), grid, block, 0, s, a);
    } else {
      if (a.V <= 256) hipLaunchKernelGGL((beam_select_f32_kernel<2, 4, true>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((beam_select_f32_kernel<2, 8, true>), grid, block, 0, s, a);
    }
  } else if (a.W <= kMaxWaves) {
    if (a.V <= 256) hipLaunchKernelGGL((beam_select_f32_kernel<1, 4, false>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((beam_select_f32_kernel<1, 8, false>), grid, block, 0, s, a);
  } else {
    if (a.V <= 256) hipLaunchKernelGGL((beam_select_f32_kernel<2, 4, false>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((beam_select_f32_kernel<2, 8, false>), grid, block, 0, s, a);
  }
}

// grid (N, L + 1): y < L gathers layer y's hidden rows, y == L the output rows, lengths, ids and count
__global__ void __launch_bounds__(256) beam_reorder_kernel(BeamReorderArgs a) {
  const int n = blockIdx.x, y = blockIdx.y, W = a.W, t = threadIdx.x;
  const size_t r0 = (size_t)n * W;
  if (y < a.L) {
    const int H4 = a.H / 4;
    const float4* src = reinterpret_cast<const float4*>(a.h_src[y]);
    float4* dst = reinterpret_cast<float4*>(a.h_dst[y]);
    for (int i = t; i < W * H4; i += blockDim.x) {
      const int k = i / H4, c = i - k * H4;
      const int p = a.parent[r0 + k];
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);   // a dead beam's state
      if (p >= 0 && p < W) v = src[(r0 + p) * H4 + c];
      dst[(r0 + k) * H4 + c] = v;
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
  // W <= 32: the counts live in wave 0
  if (t < 64) {
    const int cnt = __popcll(__ballot(live != 0));
    if (t == 0) a.n_beams[n] = cnt;
  }
}

void beam_reorder(const BeamReorderArgs& a, hipStream_t s) {
  if (a.W < 1 || a.W > 32 || a.L < 1 || a.L > 4 || a.H <= 0 || a.H % 4 || a.max_len <= 0)
    throw std::runtime_error("beam_reorder: needs 1 <= W <= 32, 1 <= L <= 4, H % 4 == 0 and max_len > 0");
  for (int l = 0; l < a.L; ++l)
    if (!a.h_src[l] || !a.h_dst[l] || a.h_src[l] == a.h_dst[l])
      throw std::runtime_error("beam_reorder: L source and L destination hidden slots, never the same (no in-place gather)");
  if (!a.parent || !a.chr || !a.next_id || !a.rows_src || !a.rows_dst || a.rows_src == a.rows_dst || !a.len_src ||
      !a.len_dst || a.len_src == a.len_dst || !a.ids || !a.n_beams)
    throw std::runtime_error("beam_reorder: parent, chr, next_id, two row buffers, two length buffers, ids and n_beams are required");
  if (a.N <= 0) return;
  hipLaunchKernelGGL(beam_reorder_kernel, dim3(a.N, a.L + 1), dim3(256), 0, s, a);
}

template <bool AUTO>
__global__ void __launch_bounds__(256) beam_reset_kernel(BeamResetArgs a) {
  const long n = (long)a.Bp * a.H, stride = (long)gridDim.x * blockDim.x;
  const long nrow = (long)a.Bp * (a.max_len + 1);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += stride) {
#pragma unroll
    for (int l = 0; l < 4; ++l)
      if (l < a.L) a.h[l][i] = 0.f;
    if (i < a.Bp) {
      const bool first = i < (long)a.N * a.W && i % a.W == 0;   // beam 0 of a name: live, score 0
      a.ids[i] = a.sos;
      a.score[i] = first ? 0.f : -INFINITY;
      a.state[i] = first ? kLive : kDead;
      a.len[i] = 0;
      if constexpr (AUTO) a.allow_state[i] = first ? a.allow_start[i / a.W] : 0;
    }
  }
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nrow; i += stride) a.rows[i] = 0;
}

void beam_reset(const BeamResetArgs& a, hipStream_t s) {
  if (a.L < 1 || a.L > 4 || a.Bp <= 0 || a.H <= 0 || a.max_len <= 0 || a.W < 1 || a.N < 0 || (long)a.N * a.W > a.Bp)
    throw std::runtime_error("beam_reset: needs 1 <= L <= 4, Bp, H, max_len > 0 and N * W <= Bp");
  for (int l = 0; l < a.L; ++l)
    if (!a.h[l]) throw std::runtime_error("beam_reset: null h");
  if (!a.ids || !a.score || !a.state || !a.len || !a.rows)
    throw std::runtime_error("beam_reset: ids, score, state, len and rows are required");
  if ((a.allow_state != nullptr) != (a.allow_start != nullptr))
    throw std::runtime_error("beam_reset: allow_state and allow_start are set together or not at all");
  if (a.allow_state) hipLaunchKernelGGL(beam_reset_kernel<true>, dim3(256), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(beam_reset_kernel<false>, dim3(256), dim3(256), 0, s, a);
}

}  // namespace gk

// One 32-token block of the V = 256 training FC head (logits, softmax-xent, dl^T, fused dH, loss
// partial) as a device function, so that the stand-alone launch (fc.hip fc_xent_v256_kernel) and the
// tail of the persistent forward (gru_seq.hip, gru_fwd_seq_tail) run ONE body: the MFMA k order, the
// DPP reductions, the LDS barriers and the dl^T swizzle are the same instructions in both, and their
// results are bit-for-bit equal by construction.  The callers differ only in how the block gets its
// X tile, which the policy argument says (FcXPlain below; FcXTail in gru_seq.hip).
#pragma once
#include "kernels.h"
#include "mma_tile.h"
#include "seq_sync.h"

namespace gk {

static constexpr int FROWS = 32;
static constexpr int kX2Pad = 8;   // bf16 of padding per staged X row

// dynamic LDS of one block: X tile | row statistics, label logits, row losses | dl^T staging | dl | labels
constexpr size_t fc_xent_v256_lds(int H) {
  return (size_t)FROWS * (H + kX2Pad) * 2 + (2 * 8 * 32 + 64) * 4 + 256 * 40 * 2 + (size_t)FROWS * (256 + 8) * 2 + FROWS * 4;
}

// fragments from the FT layout (kernels.h ft_offset): one whole 1-KB block per load instruction
template <int NKC>
DEV void fc2_load_w(bf16x8 (&b)[NKC][2], const u16* Wf, int H, int v0, int ks, int lane) {
#pragma unroll
  for (int kk = 0; kk < NKC; ++kk)
#pragma unroll
    for (int c = 0; c < 2; ++c) b[kk][c] = ld8(Wf + ((size_t)((v0 / 16 + c) * (H / 32) + ks + kk) * 64 + lane) * 8);
}
template <int NKC>
DEV void fc2_mma(f32x4 (&acc)[2][2], const bf16x8 (&b)[NKC][2], const u16* xs, int ldx, int ks, int lane) {
  const int lr = lane & 15, lk = 8 * (lane >> 4);
#pragma unroll
  for (int kk = 0; kk < NKC; ++kk) {
    bf16x8 af[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) af[r] = *reinterpret_cast<const bf16x8*>(xs + (r * 16 + lr) * ldx + (ks + kk) * 32 + lk);
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 2; ++c) acc[r][c] = mfma16(af[r], b[kk][c], acc[r][c]);
  }
}
// W_fc^T fragments of one 64-column dH pass: [8 k-steps of V=256][4 column tiles]
DEV void fc2_load_wt(bf16x8 (&bt)[8][4], const u16* WTf, int n0, int lane) {
#pragma unroll
  for (int kk = 0; kk < 8; ++kk)
#pragma unroll
    for (int c = 0; c < 4; ++c) bt[kk][c] = ld8(WTf + ((size_t)((n0 / 16 + c) * 8 + kk) * 64 + lane) * 8);
}

// X tile policy of a stand-alone launch: X was complete before the kernel started, so it is read with
// plain loads, issued ahead of the weight stream (waiting for it leaves the weights in flight).
struct FcXPlain {
  static constexpr bool kWeightsFirst = false;
  DEV bool sc1() const { return false; }
  DEV void ready() const {}
  DEV int tid() const { return (int)threadIdx.x; }
  DEV void store_loss(float* p, float v) const { *p = v; }
};

// Policy XP:
//   kWeightsFirst  false: X loads, then the first two W_fc chunks (the stand-alone order);
//                  true: the W_fc chunks go out first, then ready() -- a bounded wait for X that
//                  leaves them in flight -- then the X loads;
//   sc1()          X with L1-bypassing sc1 loads (X handed off by other workgroups inside the same
//                  launch: the tail) or plain ones (X complete before the launch);
//   tid()          the thread index (the tail hands it over opaque, so that nothing of the block is
//                  computed ahead of the step loop it follows);
//   store_loss()   the block's loss partial: a plain store where its reader is a later launch, write-through
//                  where workgroup 0 of the same launch sums the partials (gru_fb_one_kernel).
// DH = true (every default plan): dH = dl · W_fc fused, the dlogits never leave LDS.  DH = false
// writes the row-major bf16 dl instead and leaves dH to a GEMM (a round-2 plan computed dy inside
// the backward sequence kernel from it: fc_xent 16.3 -> 11.4 us but the backward +7-10 us,
// profiles/r2_bwd_dh_ab.jsonl; that consumer was removed in round 4).
template <int HH, bool DH, class XP>
DEV void fc_xent_v256_block(const FcXentArgs& a, float* smem, int block, const XP& xp) {
  int nst = 0;
  const int tid = xp.tid(), lane = tid & 63, w = tid >> 6;
  auto STAMP = [&]() {
    if (a.dbg && block == 0 && tid == 0) a.dbg[nst] = __builtin_amdgcn_s_memrealtime();
    ++nst;
  };
  STAMP();
  constexpr int V = 256, NW = 8, NKC = 8, LDR = V + 8;
  const int lr = lane & 15, lq = lane >> 4;
  constexpr int H = HH;
  const int ldx = H + kX2Pad, m0 = block * FROWS;
  u16* xs = reinterpret_cast<u16*>(smem);                         // [32][H + 8]
  float* red = reinterpret_cast<float*>(xs + FROWS * ldx);         // [2][8][32]
  float* lab = red + 2 * NW * 32;                                  // [32]
  float* lrow = lab + 32;                                          // [32]
  u16* st = reinterpret_cast<u16*>(lrow + 32);                     // [V][40]   dl^T staging
  u16* dlr = st + V * 40;                                          // [32][V+8] dl row-major

  // ---- scalars first (a global load issued behind the weight stream would wait for all of it:
  // vmcnt retires in order), then stage X, and put the first two chunks of this wave's W_fc
  // slab in flight
  const int v0 = w * 32, nks = H / 32;
  const float inv = a.inv_count[0];
  float bias[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) bias[c] = a.b[v0 + c * 16 + lr];
  bf16x8 b0[NKC][2], b1[NKC][2];
  // X: H/128 16-B pieces per thread, loaded ahead of the weight stream
  constexpr int nxp = FROWS * H / 8 / 512;
  uint4 xv[nxp];
  auto load_x = [&]() {
    if (xp.sc1()) {
      const rsrc_t rX = make_rsrc(a.X, (unsigned)((size_t)a.M * H * 2));   // < 4 GB: checked on the host
#pragma unroll
      for (int e = 0; e < nxp; ++e) {
        const int q = tid + e * 512, row = q / (H / 8), c8 = q % (H / 8);
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rX, (unsigned)(((size_t)(m0 + row) * H + c8 * 8) * 2), 0, 16);
        xv[e] = make_uint4(v.x, v.y, v.z, v.w);
      }
    } else {
#pragma unroll
      for (int e = 0; e < nxp; ++e) {
        const int q = tid + e * 512, row = q / (H / 8), c8 = q % (H / 8);
        xv[e] = *reinterpret_cast<const uint4*>(a.X + (size_t)(m0 + row) * H + c8 * 8);
      }
    }
  };
  int ylab;
  if constexpr (XP::kWeightsFirst) {
    ylab = tid < FROWS ? a.labels[m0 + tid] : 0;
    fc2_load_w<NKC>(b0, a.Wf, H, v0, 0, lane);
    if (nks > NKC) fc2_load_w<NKC>(b1, a.Wf, H, v0, NKC, lane);
    xp.ready();
    load_x();
  } else {
    load_x();
    ylab = tid < FROWS ? a.labels[m0 + tid] : 0;
    fc2_load_w<NKC>(b0, a.Wf, H, v0, 0, lane);
    if (nks > NKC) fc2_load_w<NKC>(b1, a.Wf, H, v0, NKC, lane);
  }
#pragma unroll
  for (int e = 0; e < nxp; ++e) {
    const int q = tid + e * 512, row = q / (H / 8), c8 = q % (H / 8);
    *reinterpret_cast<uint4*>(xs + row * ldx + c8 * 8) = xv[e];
  }
  int* ys = reinterpret_cast<int*>(dlr + FROWS * LDR);           // [32] labels of the block
  if (tid < FROWS) ys[tid] = ylab;
  lds_barrier();   // LDS hand-off only: the weight loads stay in flight
  STAMP();

  // ---- logits: 32 rows x this wave's 32 columns, K = H in chunks of 8 k-steps (2 in flight)
  f32x4 acc[2][2];
  zero_acc(acc);
  for (int ks = 0; ks < nks; ks += 2 * NKC) {
    fc2_mma<NKC>(acc, b0, xs, ldx, ks, lane);
    if (ks + 2 * NKC < nks) fc2_load_w<NKC>(b0, a.Wf, H, v0, ks + 2 * NKC, lane);
    if (ks + NKC < nks) {
      fc2_mma<NKC>(acc, b1, xs, ldx, ks + NKC, lane);
      if (ks + 3 * NKC < nks) fc2_load_w<NKC>(b1, a.Wf, H, v0, ks + 3 * NKC, lane);
    }
  }
  // the first dH pass's W_fc^T fragments go out now, under the softmax reductions (not earlier:
  // the scheduler barrier keeps them from overlapping the W_fc slab's registers)
  __builtin_amdgcn_sched_barrier(0);
  STAMP();
  const int per = H / NW;                 // dH columns of this wave (a multiple of 64)
  bf16x8 bt[8][4];
  if constexpr (DH) fc2_load_wt(bt, a.WTf, w * per, lane);
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[r][c][i] += bias[c];

  // ---- softmax statistics over the 8 waves' columns
  float mx[2][4], se[2][4];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float m = max16(fmaxf(acc[r][0][i], acc[r][1][i]));
      if (lr == 0) red[w * 32 + r * 16 + lq * 4 + i] = m;
    }
  lds_barrier();   // LDS hand-off only: the weight loads stay in flight
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = r * 16 + lq * 4 + i;
      float m = red[row];
#pragma unroll
      for (int ww = 1; ww < NW; ++ww) m = fmaxf(m, red[ww * 32 + row]);
      mx[r][i] = m;
      const float e = sum16(__expf(acc[r][0][i] - m) + __expf(acc[r][1][i] - m));
      if (lr == 0) red[NW * 32 + w * 32 + row] = e;
    }
  lds_barrier();   // LDS hand-off only: the weight loads stay in flight
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = r * 16 + lq * 4 + i;
      float sum = 0.f;
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) sum += red[NW * 32 + ww * 32 + row];
      se[r][i] = sum;
      const int y = ys[row];
      const float scale = (y >= 0) ? inv : 0.f;
      const float rs = __builtin_amdgcn_rcpf(sum);
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int col = v0 + c * 16 + lr;
        const float x = acc[r][c][i];
        if (col == y) lab[row] = x;
        const float d = (__expf(x - mx[r][i]) * rs - (col == y ? 1.f : 0.f)) * scale;
        const u16 db = f2bf(d);
        // dl^T staging: row r of column col at r ^ 2 ((col >> 3) & 1) -- with the plain index, columns
        // col and col + 8 of a 32-lane write half met in one bank (40-u16 pitch: 20 dwords, period 8)
        st[col * 40 + (row ^ (((col >> 3) & 1) << 1))] = db;
        dlr[row * LDR + col] = db;
      }
    }
  lds_barrier();   // LDS hand-off only: the weight loads stay in flight
  STAMP();
  // per-row nll (one thread per row; the statistics are still in LDS)
  if (tid < FROWS) {
    const int row = tid, y = ys[row];
    float m = red[row], sum = 0.f;
    for (int ww = 1; ww < NW; ++ww) m = fmaxf(m, red[ww * 32 + row]);
    for (int ww = 0; ww < NW; ++ww) sum += red[NW * 32 + ww * 32 + row];
    lrow[row] = (y >= 0) ? (logf(sum) + m - lab[row]) * inv : 0.f;
  }
  // dl^T: each column's 32 rows are 64 contiguous bytes -> four 16-B stores (rows XOR 2 undone by
  // swapping the dword pairs)
  for (int q = tid; q < V * 4; q += 512) {
    const int col = q >> 2, seg = q & 3;
    uint4 v = *reinterpret_cast<const uint4*>(st + col * 40 + seg * 8);
    if ((col >> 3) & 1) v = make_uint4(v.y, v.x, v.w, v.z);
    *reinterpret_cast<uint4*>(a.dlT + (size_t)col * a.ldT + a.colT + m0 + seg * 8) = v;
  }
  STAMP();
  if constexpr (!DH) {   // row-major dl: 32 rows x 512 B, whole 16-B pieces
    for (int q = tid; q < FROWS * V / 8; q += 512) {
      const int r2 = q / (V / 8), c8 = q % (V / 8);
      *reinterpret_cast<uint4*>(a.dl + (size_t)(m0 + r2) * V + c8 * 8) =
          *reinterpret_cast<const uint4*>(dlr + r2 * LDR + c8 * 8);
    }
  }
  // ---- dH = dl · W_fc: 32 rows x this wave's columns, 64 per pass, K = V = 256
  if constexpr (DH) for (int n0 = w * per; n0 < (w + 1) * per; n0 += 64) {
    if (n0 != w * per) fc2_load_wt(bt, a.WTf, n0, lane);
    f32x4 dacc[2][4];
    zero_acc(dacc);
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      bf16x8 af[2];
#pragma unroll
      for (int r = 0; r < 2; ++r) af[r] = *reinterpret_cast<const bf16x8*>(dlr + (r * 16 + lr) * LDR + kk * 32 + 8 * lq);
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) dacc[r][c] = mfma16(af[r], bt[kk][c], dacc[r][c]);
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          a.dy[(size_t)(m0 + r * 16 + lq * 4 + i) * H + n0 + c * 16 + lr] = dacc[r][c][i];
  }
  STAMP();
  __syncthreads();
  if (tid == 0) {
    float t = 0.f;
    for (int i = 0; i < FROWS; ++i) t += lrow[i];
    xp.store_loss(a.loss_part + block, t);
  }
  STAMP();
}

}  // namespace gk

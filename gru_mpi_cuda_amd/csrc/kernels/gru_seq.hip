// Persistent (whole-sequence) GRU recurrence kernels for gfx950: ONE launch runs all T
// timesteps of one layer, forward or backward.
//
// Why: at the headline shape (B = 256 per GPU, H = 512) one timestep's recurrent GEMM is
// 0.4 GFLOP -- a few hundred ns of MFMA work spread over 256 CUs -- so a per-step launch is
// dominated by the launch/drain floor (profiles/: ~1.6 us graph node + ~1 us store drain +
// ~1 us of load latency).  Here:
//   * grid = (H/16 unit tiles) x (Bp/32 row blocks), one 512-thread workgroup per CU, all
//     co-resident (checked on the host against the occupancy query);
//   * each wave keeps its K-slice of the recurrent weights in VGPRs for the whole sequence
//     (W_hh never re-read from memory);
//   * step t+1 of row block rb needs h_t of those 32 rows from all H/16 unit-tile workgroups:
//     the 1 KB tile each workgroup produces is stored write-through (sc1) by one wave, that
//     wave drains (s_waitcnt vmcnt(0)) and bumps the row block's counter (agent-scope atomic);
//     consumers poll the counter with sc1 loads and read the tiles with sc1 buffer loads
//     (cdna_hip_programming.md §6 Guideline 16, MI355X_MICROARCH.md 'Valid forms' row 1).
//     Every spin is bounded: on timeout an error word is set and the kernel runs to completion.
//   * backward additionally accumulates the weight gradients dW_hh = Σ_t dGh_t^T h_{t-1} and
//     the embedding-side dP = Σ_t onehot(x_t)^T dGi_t (layer 0) plus both bias gradients in
//     registers, using the MFMA pipe that the latency-bound recurrence leaves idle; partial
//     sums per row block are reduced by one small kernel afterwards, or -- the dP ones, in the one-layer
//     H = 512 step -- by the backward itself as its tail (gru_bwd_seq_tail); no float atomics.
// Reference mapping: this is the whole per-char hot loop of /root/reference/namegensf.cu:661-872
// (for all names at once), plus the BPTT half the reference does not have.
#include "kernels.h"
#include "mma_tile.h"
#include "seq_sync.h"
#include "fc_block.h"
#include "optim_dev.h"
#include <type_traits>

namespace gk {

// ==================================================================== forward
// RS = 1: every wave covers both 16-row tiles of the row block over a K/8 slice (NKW = H/256
//         k-steps); the 8 partial sums of each output meet in LDS.
// RS = 2: waves 0-3 own row tile 0, waves 4-7 row tile 1, each over a K/4 slice (NKW = H/128):
//         the same MFMAs and exchange loads per wave, half the LDS partial traffic (4 partials of
//         3 gates per output instead of 8, read by the epilogue thread of the same row tile).
// (Rejected and removed in round 4, history in docs/DESIGN.md §6.3: a table-free layer 0 computing
// its P-table columns in every workgroup, layer 0's input projection in the post-publish slack, the
// FC / softmax-xent pipeline inside the forward, and the saves issued inside the publish drain.)
// FC = true (gru_fwd_seq_fc): the same recurrence in blocks [0, H/16 * Bp/32), plus kFcCons FC
// consumer workgroups per row block behind them in the same grid (fwd_fc_consumer below); the
// recurrence then also drains its h copies before each step's first barrier and signals T + 1
// after the last step, so a consumer that saw epoch t + 2 may read HSb / HF of step t.
static constexpr size_t kFwdRecLds = sizeof(float) * 8 * 6 * 256 + sizeof(u16) * 32 * 24 + sizeof(u16) * 16 * 40;
static constexpr size_t kFwdFcLds = sizeof(u16) * 32 * (512 + 8) + sizeof(u16) * 32 * (256 + 8) +
                                    sizeof(float) * (2 * 8 * 32 + 3 * 32);

// ---------------------------------------------------------------------------- FC consumers
// Workgroup ci of the consumer part of gru_fwd_seq_fc's grid serves row block rbk = ci % nrb as its
// consumer c = ci / nrb (placed on rbk's XCD by the dispatcher's round-robin; the placement census
// covers producers and consumers, so a row block whose members are not all on one XCD takes the
// write-through protocol for every hand-off).  Two phases, both behind the recurrence:
//  1. items: step t = c, c + kFcCons, ... of the row block -- the 32 x V logits of h_t (X tile read
//     from HSb once the row block's producers signalled t + 2, W_fc fragments already in flight),
//     softmax-xent, the loss partial, dl as bf16 fragment blocks (dlF), dy_t = dl · W_fc (fp32); then
//     the consumer's own flag line carries "items done".
//  2. dW_fc: consumer c owns the 64 x 64 tile c of the row block's V x H partial and accumulates
//     dl_t^T h_t over t = 0 .. T-1 in order (one flag check per step: the item of step t done), from
//     dlF and the backward's fragment-tiled HF copy -- K = 32 rows per step, one MFMA per 16 x 16
//     tile; the tiles of unit column 0 also take db_fc (row sums of dl^T, an MFMA against ones).
//     The row block's partial lands in slab rbk (the trainer's dW_fc / db_fc slabs, summed in Adam).
// The recurrence never waits on a consumer.  This is the FC / softmax-xent / dH work of fc_xent and
// the dW_fc K-slices of the post-backward group, off the step's serial tail (VERDICT r5 item 1;
// reference: the per-char FC + softmax of /root/reference/namegensf.cu:856-873).
template <int H>
DEV void fwd_fc_consumer(const SeqFwdArgs& a, const SeqFcArgs& f, unsigned char* smem, int ci) {
  constexpr int V = 256, NW = 8, LDX = H + 8, LDR = V + 8, NKS = H / 32, NKC = 4;
  static_assert((V / 64) * (H / 64) == kFcCons, "one 64 x 64 dW_fc tile per consumer");
  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lq = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: fragment offsets go to soffset
  const int T = a.T, Bp = a.Bp, nrb = Bp / 32;
  constexpr int nunit = H / 16;
  const int rbk = ci % nrb, c = ci / nrb, b0 = rbk * 32;
  unsigned* const fl = a.cnt + (size_t)rbk * (nunit + kFcCons) * kFlagStride;   // producers' lines
  unsigned* const cfl = fl + (size_t)nunit * kFlagStride;                       // consumers' lines
  const int probe = f.probe & 7;
  if (probe == 3) return;
  const bool loc = a.allow_local && row_block_local(fl, nunit + c, nunit + kFcCons, a.err);
  if (probe == 1) return;
  u16* xs = reinterpret_cast<u16*>(smem);              // [32][H + 8] X tile
  u16* dlr = xs + 32 * LDX;                            // [32][V + 8] dl row-major (dH A operand)
  float* red = reinterpret_cast<float*>(dlr + 32 * LDR);   // [2][8][32] row max / sum-exp partials
  float* lab = red + 2 * NW * 32;                      // [32] label logit
  float* lrow = lab + 32;                              // [32] row loss
  int* ys = reinterpret_cast<int*>(lrow + 32);         // [32] labels
  const rsrc_t rH = make_rsrc(a.HSb, (unsigned)((size_t)(T + 1) * Bp * H * 2));
  const rsrc_t rD = make_rsrc(f.dlF, (unsigned)((size_t)T * Bp * V * 2));
  const int v0 = w * 32;
  float bias[2];
#pragma unroll
  for (int cc = 0; cc < 2; ++cc) bias[cc] = f.b[v0 + cc * 16 + lr];
  // W_fc fragments (FT layout, 1 KB per load instruction): wave w's 2 vocab tiles, k-steps ks..ks+NKC;
  // buffer loads with the lane's 16 B in the VGPR offset and the block in the scalar offset (64-bit
  // VGPR addresses per fragment pushed the consumer past its 128-register budget)
  const rsrc_t rWf = make_rsrc(f.Wf, (unsigned)(V * H * 2)), rWt = make_rsrc(f.WTf, (unsigned)(V * H * 2));
  const unsigned l16 = (unsigned)lane * 16u;
  auto load_w = [&](bf16x8 (&b)[NKC][2], int ks) {
    if (probe == 4) {   // diagnostic: the items without their weight stream
#pragma unroll
      for (int kk = 0; kk < NKC; ++kk) b[kk][0] = b[kk][1] = zero8();
      return;
    }
#pragma unroll
    for (int kk = 0; kk < NKC; ++kk)
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) b[kk][cc] = ld8_plain_s(rWf, l16, ((v0 / 16 + cc) * NKS + ks + kk) * 1024);
  };
  auto mma_w = [&](f32x4 (&acc)[2][2], const bf16x8 (&b)[NKC][2], int ks) {
#pragma unroll
    for (int kk = 0; kk < NKC; ++kk) {
      bf16x8 af[2];
#pragma unroll
      for (int r = 0; r < 2; ++r) af[r] = *reinterpret_cast<const bf16x8*>(xs + (r * 16 + lr) * LDX + (ks + kk) * 32 + 8 * lq);
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) acc[r][cc] = mfma16(af[r], b[kk][cc], acc[r][cc]);
    }
  };
  // W_fc^T fragments of wave w's 64 dH columns, two k-steps of V
  auto load_wt = [&](bf16x8 (&b)[2][4], int kk0) {
    if (probe == 4) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) b[kk][cc] = zero8();
      return;
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) b[kk][cc] = ld8_plain_s(rWt, l16, ((w * 4 + cc) * (V / 32) + kk0 + kk) * 1024);
  };
  auto mma_t = [&](f32x4 (&acc)[2][4], const bf16x8 (&b)[2][4], int kk0) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[2];
#pragma unroll
      for (int r = 0; r < 2; ++r) af[r] = *reinterpret_cast<const bf16x8*>(dlr + (r * 16 + lr) * LDR + (kk0 + kk) * 32 + 8 * lq);
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) acc[r][cc] = mfma16(af[r], b[kk][cc], acc[r][cc]);
    }
  };

  // ---- phase 1: the FC items of this consumer
  for (int t = c; t < T; t += kFcCons) {
    const int m0 = t * Bp + b0;
    bf16x8 wa[NKC][2], wb[NKC][2];
    load_w(wa, 0);
    load_w(wb, NKC);
    const int ylab = tid < 32 ? f.labels[m0 + tid] : 0;
    const float inv = f.inv_count[0];
    // h_t of the whole row block is in HSb once every producer signalled t + 2 (T + 1: the final signal).
    // The producers' flag lines are the recurrence's own hot lines: until this item is near, one lane
    // polls one of them with a long back-off (a full 32-lane sweep every ~100 clocks by each waiting
    // consumer measured +0.7 us per recurrence step), then the sweep of all producers.
    if (tid < 64) {
      SpinBudget spin(a.err);
      for (;;) {
        unsigned v = 0;
        if (lane == 0) v = __hip_atomic_load(fl + (size_t)(c % nunit) * kFlagStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v = __builtin_amdgcn_readfirstlane(v);
        if (v + 1u >= (unsigned)(t + 2)) break;
        __builtin_amdgcn_s_sleep(16);
        if (spin.expired()) break;   // the full wait below reports it
      }
    }
    wait_flags(fl, nunit, (unsigned)(t + 2), a.err);
    stamp(a.dbg, t, 0);
    constexpr int NXP = 32 * H / 8 / 512;
    u32x4 xv[NXP];
#pragma unroll
    for (int e = 0; e < NXP; ++e) {
      const int q = tid + e * 512, row = q / (H / 8), c8 = q % (H / 8);
      xv[e] = __builtin_amdgcn_raw_buffer_load_b128(rH, (unsigned)((((size_t)(t + 1) * Bp + b0 + row) * H + c8 * 8) * 2), 0, 16);
    }
#pragma unroll
    for (int e = 0; e < NXP; ++e) {
      const int q = tid + e * 512, row = q / (H / 8), c8 = q % (H / 8);
      *reinterpret_cast<u32x4*>(xs + row * LDX + c8 * 8) = xv[e];
    }
    if (tid < 32) ys[tid] = ylab;
    lds_barrier();
    stamp(a.dbg, t, 1);
    f32x4 acc[2][2];
    zero_acc(acc);
#pragma unroll
    for (int ks = 0; ks < NKS; ks += 2 * NKC) {
      mma_w(acc, wa, ks);
      if (ks + 2 * NKC < NKS) load_w(wa, ks + 2 * NKC);
      mma_w(acc, wb, ks + NKC);
      if (ks + 3 * NKC < NKS) load_w(wb, ks + 3 * NKC);
    }
    bf16x8 ta[2][4], tb[2][4];   // the dH pass's first W_fc^T fragments, under the softmax
    load_wt(ta, 0);
    load_wt(tb, 2);
#pragma unroll
    for (int cc = 0; cc < 2; ++cc)
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[r][cc][i] += bias[cc];
    // softmax statistics across the 8 waves' columns
    float mx[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float m = max16(fmaxf(acc[r][0][i], acc[r][1][i]));
        if (lr == 0) red[w * 32 + r * 16 + lq * 4 + i] = m;
      }
    lds_barrier();
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
    lds_barrier();
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      u16 dv[2][4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = r * 16 + lq * 4 + i;
        float sum = 0.f;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) sum += red[NW * 32 + ww * 32 + row];
        const int y = ys[row];
        const float scale = (y >= 0) ? inv : 0.f;
        const float rs = __builtin_amdgcn_rcpf(sum);
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
          const int col = v0 + cc * 16 + lr;
          const float x = acc[r][cc][i];
          if (col == y) lab[row] = x;
          const float d = (__expf(x - mx[r][i]) * rs - (col == y ? 1.f : 0.f)) * scale;
          dv[cc][i] = f2bf(d);
          dlr[row * LDR + col] = dv[cc][i];
        }
      }
      // dlF block (t, rbk, vocab tile): lane L holds rows 8(L >> 4) .. +8 of vocab column L & 15; this
      // lane's 4 rows r*16 + 4lq .. +4 are half of lane (2r + lq/2)*16 + lr's slot
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) {
        const unsigned lo = (unsigned)dv[cc][0] | ((unsigned)dv[cc][1] << 16);
        const unsigned hi = (unsigned)dv[cc][2] | ((unsigned)dv[cc][3] << 16);
        const unsigned off = (unsigned)(((((size_t)(t * nrb + rbk) * (V / 16) + v0 / 16 + cc) * 64 +
                                          (2 * r + (lq >> 1)) * 16 + lr) * 8 + (lq & 1) * 4) * 2);
        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
        const u32x2 pv = {lo, hi};
        if (loc) __builtin_amdgcn_raw_buffer_store_b64(pv, rD, off, 0, 0);
        else __builtin_amdgcn_raw_buffer_store_b64(pv, rD, off, 0, 16);
      }
    }
    lds_barrier();   // dl row-major and the label logits in LDS
    stamp(a.dbg, t, 2);
    if (tid < 32) {
      const int row = tid, y = ys[row];
      float m = red[row], sum = 0.f;
      for (int ww = 1; ww < NW; ++ww) m = fmaxf(m, red[ww * 32 + row]);
      for (int ww = 0; ww < NW; ++ww) sum += red[NW * 32 + ww * 32 + row];
      lrow[row] = (y >= 0) ? (logf(sum) + m - lab[row]) * inv : 0.f;
    }
    // dy_t = dl · W_fc: wave w's 64 columns, K = V
    f32x4 dacc[2][4];
    zero_acc(dacc);
#pragma unroll
    for (int kk0 = 0; kk0 < V / 32; kk0 += 4) {
      mma_t(dacc, ta, kk0);
      if (kk0 + 4 < V / 32) load_wt(ta, kk0 + 4);
      mma_t(dacc, tb, kk0 + 2);
      if (kk0 + 6 < V / 32) load_wt(tb, kk0 + 6);
    }
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int cc = 0; cc < 4; ++cc)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          f.dy[(size_t)(m0 + r * 16 + lq * 4 + i) * H + w * 64 + cc * 16 + lr] = dacc[r][cc][i];
    lds_barrier();   // lrow complete
    if (tid == 0) {
      float s = 0.f;
      for (int i = 0; i < 32; ++i) s += lrow[i];
      f.loss_part[m0 / 32] = s;
    }
    // item done: every wave's dlF stores complete, then one flag
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    stamp(a.dbg, t, 3);
    if (tid == 0) {
      if (loc) signal_flag_local(cfl + (size_t)c * kFlagStride, (unsigned)(t / kFcCons + 1));
      else signal_flag(cfl + (size_t)c * kFlagStride, (unsigned)(t / kFcCons + 1));
    }
  }

  if (probe == 2 || probe == 4) return;
  // ---- phase 2: this consumer's 64 x 64 tile of the row block's dW_fc partial, t = 0 .. T-1 in order
  constexpr int TPH = H / 64;
  const int tv = (c / TPH) * 4 + (w >> 1);          // 16-row vocab tile
  const int th = (c % TPH) * 4 + 2 * (w & 1);       // first of two 16-column unit tiles
  const bool rs_on = (c % TPH) == 0 && (w & 1) == 0;
  const rsrc_t rF = make_rsrc(a.HF, (unsigned)((size_t)(T + 1) * Bp * H * 2));
  bf16x8 ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;
  f32x4 aw[2], ab;
  aw[0] = f32x4{0.f, 0.f, 0.f, 0.f};
  aw[1] = aw[0];
  ab = aw[0];
  // steps in groups of DG: one poll covers the group's items (lane i: step t0 + i), then all of its
  // fragments are loaded at once and accumulated in step order (deterministic)
  constexpr int DG = 4;
  for (int t0 = 0; t0 < T; t0 += DG) {
    const int n = T - t0 < DG ? T - t0 : DG;
    {
      SpinBudget spin(a.err);
      for (;;) {
        bool ok = true;
        if (lane < n)
          ok = __hip_atomic_load(cfl + (size_t)((t0 + lane) % kFcCons) * kFlagStride, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT) >= (unsigned)((t0 + lane) / kFcCons + 1);
        if (__all(ok)) break;
        __builtin_amdgcn_s_sleep(8);
        if (spin.expired()) {
          if (lane == 0) __hip_atomic_fetch_or(a.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          break;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    bf16x8 A[DG], Bf[DG][2];
#pragma unroll
    for (int i = 0; i < DG; ++i) {
      if (i < n) {
        const int t = t0 + i;
        A[i] = ld8_sc1(rD, (unsigned)((((size_t)(t * nrb + rbk) * (V / 16) + tv) * 512 + lane * 8) * 2));
#pragma unroll
        for (int j = 0; j < 2; ++j)
          Bf[i][j] = ld8_sc1(rF, (unsigned)(((((size_t)(t + 1) * nunit + th + j) * nrb + rbk) * 512 + lane * 8) * 2));
      }
    }
#pragma unroll
    for (int i = 0; i < DG; ++i) {
      if (i < n) {
#pragma unroll
        for (int j = 0; j < 2; ++j) aw[j] = mfma16(A[i], Bf[i][j], aw[j]);
        if (rs_on) ab = mfma16(A[i], ones, ab);
      }
    }
  }
  float* W = f.dW + (size_t)rbk * V * H;
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) W[(size_t)(tv * 16 + lq * 4 + i) * H + (th + j) * 16 + lr] = aw[j][i];
  if (rs_on && lr == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) f.db[(size_t)rbk * V + tv * 16 + lq * 4 + i] = ab[i];
  }
}


// X tile policy of the tail (fc_block.h): the block's W_fc chunks go out first, then the wait for the
// row block's producers (epoch T + 1: every h of the row block is in HSb), then the X loads.  X is a
// hand-off inside the launch, so every load of it is an L1-bypassing sc1 load behind a poll that saw the
// flags -- the consumer side of both exchange protocols (seq_sync.h row_block_local): served by the
// XCD's own L2 where the row block is local and HSb was written with plain stores, by memory where it
// went out write-through.  (No agent acquire: its vmcnt(0) would wait for the W_fc chunks in flight.)
struct FcXTail {
  static constexpr bool kWeightsFirst = true;
  const unsigned* fl;
  int nunit;
  unsigned epoch;
  unsigned* err;
  DEV bool sc1() const { return true; }
  DEV void store_loss(float* p, float v) const { *p = v; }
  DEV void ready() const { wait_flags_keep(fl, nunit, epoch, err); }
  // opaque: every per-thread address of the block is a function of the thread index alone, and the
  // compiler computed them ahead of the step loop, where their registers pushed scalars into VGPR lanes
  DEV int tid() const {
    int t = (int)threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
  }
};

// The tail itself.  It takes nothing from the step loop but `loc`: the launch's arguments are read again
// from the kernel-argument segment, through a pointer the compiler cannot see through (explicit
// arguments lie in order at their natural alignment: a at 0, the head's FcXentArgs behind it), and the
// thread index is opaque too.  Taken from the kernel's parameters, the head's ~40 SGPRs and the values the
// tail shares with the loop were live across the step loop, which then parked scalars in VGPR lanes
// (96 v_readlane / v_writelane per step against the plain kernel's 17); per-thread addresses of the
// block were computed ahead of the loop; and, as invariants of the item loop, the 64-bit address of
// every weight fragment load (42 VGPR pairs) was hoisted out of it and spilled to scratch.
// What this buys depends on the kernel-argument layout (asserted below and at the kernel) and on the
// compiler's register allocation: the figures here and at the saves (no lane spill, 381 against 414
// instructions per step, 200-201 VGPRs, no scratch) are those of AMD clang 22.0.0git (ROCm 7.2.0) and
// want checking again (-Rpass-analysis=kernel-resource-usage, the loop's ISA) at a compiler upgrade.
static_assert(std::is_trivially_copyable<SeqFwdArgs>::value && std::is_trivially_copyable<FcXentArgs>::value,
              "the tail reads both argument structs back from the kernel-argument segment byte for byte");
// The same policy inside gru_fb_one_kernel: the loss partials reach workgroup 0 -- any XCD -- at the end
// of the same launch, so they leave write-through (an agent-scope store: sc1) and are read back sc1.
struct FcXTailOne : FcXTail {
  DEV void store_loss(float* p, float v) const { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

// ONE (gru_fb_one_kernel): the flag lines are those of the launch's flag set, foff words behind a.cnt.
template <bool ONE>
DEV void fwd_fc_tail(bool loc, unsigned char* smem, unsigned foff) {
  typedef const __attribute__((address_space(4))) char* kptr_t;
  kptr_t kp = (kptr_t)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(kp));
  const SeqFwdArgs& a = *(const SeqFwdArgs*)kp;
  constexpr size_t fc_off = (sizeof(SeqFwdArgs) + alignof(FcXentArgs) - 1) / alignof(FcXentArgs) * alignof(FcXentArgs);
  const int T = a.T, nrb = a.Bp / 32, nunit = a.H / 16;
  const int ut = seq_unit_tile(nrb), rbk = seq_row_block(nrb);
  unsigned* const fl = a.cnt + (ONE ? (size_t)foff : (size_t)0) + (size_t)rbk * nunit * kFlagStride;   // the row block's producer lines
  const FcXTail xb{fl, nunit, (unsigned)(T + 1), a.err};
  const typename std::conditional<ONE, FcXTailOne, FcXTail>::type xp{xb};
  const int tid = xp.tid();
  // h of the last step in HSb -> epoch T + 1.  Only wave 0 wrote HSb, and each of its publish drains
  // covered the step before, so its own drain is the only one needed; the other waves go on to their
  // weight loads at once (none of them sits in front of a poll of the step loop or in this drain).
  stamp(a.dbg, T + 1, 5);
  if (tid < 64) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (tid == 0) {
      if (loc) signal_flag_local(fl + (size_t)ut * kFlagStride, (unsigned)(T + 1));
      else signal_flag(fl + (size_t)ut * kFlagStride, (unsigned)(T + 1));
    }
  }
  // (the first block's wait_flags_keep barrier also separates the last step's staging reads from the
  // block's LDS writes: one union)
  for (int t = ut; t < T; t += nunit) {
    kptr_t kf = kp + fc_off;
    asm volatile("" : "+s"(kf));
    const FcXentArgs f = *(const FcXentArgs*)kf;
    fc_xent_v256_block<512, true>(f, reinterpret_cast<float*>(smem), t * nrb + rbk, xp);
  }
  stamp(a.dbg, T + 1, 6);
}

// TAIL = true (gru_fwd_seq_tail): the recurrence's own grid and step loop; after its last timestep each
// workgroup signals epoch T + 1 and runs the FC head's 32-token blocks (t, rbk), t = ut, ut + nunit, ..
// of its own row block -- fc_xent_v256_block, the body of the stand-alone fc_xent launch -- before
// it exits.  The second kernel argument is then the FcXentArgs of that launch.
template <bool TAIL> struct FwdFcArg { typedef SeqFcArgs type; };
template <> struct FwdFcArg<true> { typedef FcXentArgs type; };
static constexpr size_t kFwdTailLds = fc_xent_v256_lds(512) > kFwdRecLds ? fc_xent_v256_lds(512) : kFwdRecLds;

template <int NKW, int RS, bool FC, int WPE = FC ? 4 : 1, bool TAIL = false>
__global__ void __launch_bounds__(512, WPE) gru_fwd_seq_kernel(SeqFwdArgs a, typename FwdFcArg<TAIL>::type fc) {
  static_assert(!(FC && TAIL), "the FC consumers and the FC tail exclude each other");
  static_assert(!TAIL || (NKW == 4 && RS == 2), "the tail is built for H = 512");
  // (fwd_fc_tail's hand-computed offset: the parameter list is exactly these two, in this order)
  static_assert(std::is_same<decltype(&gru_fwd_seq_kernel<NKW, RS, FC, WPE, TAIL>),
                             void (*)(SeqFwdArgs, typename FwdFcArg<TAIL>::type)>::value,
                "gru_fwd_seq_kernel takes (SeqFwdArgs, FC arguments) and nothing else");
  __shared__ __attribute__((aligned(16))) unsigned char smem[TAIL ? kFwdTailLds : FC ? (kFwdFcLds > kFwdRecLds ? kFwdFcLds : kFwdRecLds) : kFwdRecLds];
#include "gru_seq_fwd_body.h"
  if constexpr (TAIL) fwd_fc_tail<false>(loc, smem, 0u);
}

// ==================================================================== two-layer wavefront forward
// Layer hi at step t depends on layer lo only through h_lo(t) (/root/reference/namegensf.cu:773-854:
// layer 1's input is layer 0's output for the same char), so one launch runs lo's step s and hi's
// step s-1 in iteration s = 0..T.  Both operands -- h_lo(s-1) and h_hi(s-2) -- were published by
// the previous iteration, so one poll loop waits for both (lanes 0-31 poll lo's producers, 32-63
// hi's).  The h_lo(s-1) K-slice feeds BOTH lo's recurrent product (W_hh,lo) and hi's input product
// (W_ih,hi): hi needs no Gi GEMM and no Gi buffer.  hi's r/z gates accumulate W_ih x + W_hh h in
// one MFMA chain; its n gate keeps the two apart (n = tanh(gi_n + r gh_n)).
//
// Register/LDS budget (H = 1024, 8 waves, 256 registers each): the three resident weight K-slices
// (W_hh,lo, W_ih,hi, W_hh,hi over K/8) take 36 * NKW = 144.  The exchange operands are loaded
// straight into LDS (buffer_load ... lds, 16 B per lane in MFMA fragment order, 16 KB per wave for
// both streams) and read back per k-step, so they hold no registers across the poll loop.  After
// its MFMAs a wave writes its 14 K-partial tiles over its own staging area (nothing else reads it
// by then); the epilogue sums the eight waves' partials.  (A transposed product -- weights as the
// A operand -- scattered each save store over 16 rows: 1.5 us more per iteration.)  The wave index is read as a scalar so everything derived from it stays in SGPRs.  (Builds that
// kept the operands in registers spilled 51-110 VGPRs; a 4-wave build fit but ran one wave per
// SIMD and exposed every LDS and memory latency: 8.9 us per iteration.)
// Exchange layout, flags, saves and the L2-local hand-off are gru_fwd_seq_kernel's, per layer;
// lo's tile publishes from wave 0 and hi's from wave 1, so the two drains overlap.
template <int NKW>   // k-steps per wave: H / 256
__global__ void __launch_bounds__(512, 1) gru_fwd_seq2_kernel(SeqFwd2Args a) {
  constexpr int NKS = NKW < 4 ? 4 : NKW;   // staging k-steps (>= 4: the area also holds 14 x 256 floats)
  // [wave][stream lo/hi][k-step][row tile][lane] MFMA B fragments; reused as float partials
  // [wave][14][256] (lo r,z,n x 2 row tiles | hi r, z (input + recurrent), gi_n, gh_n x 2)
  __shared__ __attribute__((aligned(16))) bf16x8 stage[8][2][NKS][2][64];
  __shared__ __attribute__((aligned(16))) u16 stg[2][32][24];
  __shared__ __attribute__((aligned(16))) u16 stgT[2][16][40];
  typedef __attribute__((address_space(3))) void lds_void;
  const SeqFwdArgs& L0 = a.lo;
  const SeqFwdArgs& L1 = a.hi;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H = L0.H, Bp = L0.Bp, T = L0.T;
  const int nrb = Bp / 32, ut = seq_unit_tile(nrb);
  const int j0 = ut * 16, rbk = seq_row_block(nrb), b0 = rbk * 32;
  const int lr = lane & 15, lk = 8 * (lane >> 4);
  const int k0 = w * NKW * 32;
  const unsigned nunit = (unsigned)(H / 16);

  bf16x8 wh0[NKW][3], wi1[NKW][3], wh1[NKW][3];
#pragma unroll
  for (int kk = 0; kk < NKW; ++kk)
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      const size_t o = (size_t)(g * H + j0 + lr) * H + k0 + kk * 32 + lk;
      wh0[kk][g] = ld8(L0.Whh + o);
      wi1[kk][g] = ld8(a.Wih + o);
      wh1[kk][g] = ld8(L1.Whh + o);
    }

  // this thread's epilogue item: row tile q = w / 4, element e = w % 4 of lane `lane`'s accumulator
  // -> (batch row 16 q + 4 (lane >> 4) + e, unit lane & 15), partial index e * 64 + lane; a wave's
  // 64 items are 4 rows x 16 consecutive units, so every save store is 4 whole 64-B segments
  const int q = w >> 2, e = w & 3;
  const int row = q * 16 + 4 * (lane >> 4) + e, col = lane & 15;
  const int b = b0 + row, j = j0 + col, pidx = e * 64 + lane;
  float bh0[3], bh1[3], bi1[3];
#pragma unroll
  for (int g = 0; g < 3; ++g) {
    bh0[g] = L0.bhh[g * H + j];
    bh1[g] = L1.bhh[g * H + j];
    bi1[g] = a.bih[g * H + j];
  }
  float hp0 = L0.h0 ? L0.h0[(size_t)b * H + j] : 0.f;
  float hp1 = L1.h0 ? L1.h0[(size_t)b * H + j] : 0.f;
  const unsigned hs_bytes = (unsigned)((size_t)(T + 1) * Bp * H * 2), x_bytes = (unsigned)((size_t)T * Bp * H * 2);
  const rsrc_t rH0 = make_rsrc(L0.HSb, hs_bytes), rX0 = make_rsrc(L0.xch, x_bytes);
  const rsrc_t rH1 = make_rsrc(L1.HSb, hs_bytes), rX1 = make_rsrc(L1.xch, x_bytes);
  // exchange rings as gru_fwd_seq_kernel's (L0.xring for both layers): lo's tile of step t is read in
  // iteration t + 1, hi's in t + 2; a slot is rewritten xr steps later, after every producer of the
  // row block published the iteration in which it was last read
  const int xr = L0.xring >= 2 ? L0.xring : T;
  zero_next_flags(L0.zero_next, L0.zero_words);
  zero_next_flags(L1.zero_next, L1.zero_words);
  unsigned* const fl0 = L0.cnt + (size_t)rbk * nunit * kFlagStride;
  unsigned* const fl1 = L1.cnt + (size_t)rbk * nunit * kFlagStride;
  const bool loc = L0.allow_local && row_block_local(fl0, ut, (int)nunit, L0.err);

  // k-step kk of stream st (both row tiles) into this wave's staging area, from exchange slot ts
  // (sc1, after a poll saw the producers) or from the row-major HS[0] (the carried state).  Byte
  // offsets: one per-lane VGPR for the launch, the rest (slot, k-step, row tile) in the scalar offset.
  const unsigned xl = (unsigned)((((lk >> 4) * 32 + lr) * 16 + (lk & 15)) * 2);
  const unsigned hl = (unsigned)((lr * H + lk) * 2);
  auto stage_x = [&](int st, int kk, int ts) {
    const rsrc_t rX = st == 0 ? rX0 : rX1;
    const int so = (int)((((size_t)(ts % xr) * nrb + rbk) * nunit + (k0 + kk * 32) / 16) * 1024);
#pragma unroll
    for (int r = 0; r < 2; ++r)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rX, (lds_void*)(&stage[w][st][kk][r][0]), 16, xl, so + r * 512, 0, 16);
  };
  auto stage_h0 = [&](int st) {
    const rsrc_t rH = st == 0 ? rH0 : rH1;
#pragma unroll
    for (int kk = 0; kk < NKW; ++kk)
#pragma unroll
      for (int r = 0; r < 2; ++r)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rH, (lds_void*)(&stage[w][st][kk][r][0]), 16, hl,
                                                 (int)((((size_t)b0 + r * 16) * H + k0 + kk * 32) * 2), 0, 16);
  };
  float* const mypart = reinterpret_cast<float*>(&stage[w][0][0][0][0]);
  auto partial = [&](int ww, int set) -> float {
    return reinterpret_cast<const float*>(&stage[ww][0][0][0][0])[set * 256 + pidx];
  };

  // lo's input projection for step t, gathered one iteration ahead (off the critical path), from
  // a char id loaded one iteration before that (the gather never waits on an id load)
  int idn = L0.ids ? L0.ids[b] : 0;
  auto load_gi0 = [&](int t, float (&gi)[3]) {
    if (t >= T) return;
    const float* src = L0.ids ? L0.P + (size_t)idn * 3 * H : L0.Gi + ((size_t)t * Bp + b) * 3 * H;
#pragma unroll
    for (int g = 0; g < 3; ++g) gi[g] = src[g * H + j];
    if (L0.ids && t + 1 < T) idn = L0.ids[(size_t)(t + 1) * Bp + b];
  };
  float gin[3] = {0.f, 0.f, 0.f};
  load_gi0(0, gin);
  for (int s = 0; s <= T; ++s) {
    const bool do0 = s < T, do1 = s > 0;   // lo's step s, hi's step s - 1
    stamp(L0.dbg, s, 0);
    float gi0[3] = {gin[0], gin[1], gin[2]};
    const bool hasA = s > 0 || L0.h0, hasB = do1 && (s > 1 || L1.h0);   // h_lo(s-1), h_hi(s-2)
    if (s >= 2) {
      wave_wait_load2<NKW>(fl0, fl1, k0 / 16, (unsigned)s, (unsigned)(s - 1), L0.err,
                           [&](int kk) { stage_x(0, kk, s - 1); }, [&](int kk) { stage_x(1, kk, s - 2); });
    } else {
      if (s == 1) wave_wait_load<NKW>(fl0, lane < 2 * NKW, k0 / 16 + lane, 1u, L0.err, [&](int kk) { stage_x(0, kk, 0); });
      else if (hasA) stage_h0(0);
      if (hasB) stage_h0(1);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's staged operands are in LDS
    stamp(L0.dbg, s, 5);
    f32x4 acc0[2][3], acc1[2][4];   // acc1: hi's r, z (input + recurrent), gi_n, gh_n
    zero_acc(acc0);
    zero_acc(acc1);
    if (hasA && hasB) {   // the steady state: every product, no branches between the MFMAs
#pragma unroll
      for (int kk = 0; kk < NKW; ++kk)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const bf16x8 x = stage[w][0][kk][r][lane], y = stage[w][1][kk][r][lane];
#pragma unroll
          for (int g = 0; g < 3; ++g) acc0[r][g] = mfma16(x, wh0[kk][g], acc0[r][g]);
#pragma unroll
          for (int g = 0; g < 3; ++g) acc1[r][g] = mfma16(x, wi1[kk][g], acc1[r][g]);
          acc1[r][0] = mfma16(y, wh1[kk][0], acc1[r][0]);
          acc1[r][1] = mfma16(y, wh1[kk][1], acc1[r][1]);
          acc1[r][3] = mfma16(y, wh1[kk][2], acc1[r][3]);
        }
    } else {
#pragma unroll
      for (int kk = 0; kk < NKW; ++kk)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          if (hasA) {
            const bf16x8 x = stage[w][0][kk][r][lane];
#pragma unroll
            for (int g = 0; g < 3; ++g) acc0[r][g] = mfma16(x, wh0[kk][g], acc0[r][g]);
#pragma unroll
            for (int g = 0; g < 3; ++g) acc1[r][g] = mfma16(x, wi1[kk][g], acc1[r][g]);
          }
          if (hasB) {
            const bf16x8 y = stage[w][1][kk][r][lane];
            acc1[r][0] = mfma16(y, wh1[kk][0], acc1[r][0]);
            acc1[r][1] = mfma16(y, wh1[kk][1], acc1[r][1]);
            acc1[r][3] = mfma16(y, wh1[kk][2], acc1[r][3]);
          }
        }
    }
    stamp(L0.dbg, s, 1);
    // partials over this wave's own staging area (its reads above precede these writes in the
    // wave's in-order LDS queue; no other wave reads it before the barrier)
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int g = 0; g < 3; ++g) mypart[(r * 3 + g) * 256 + i * 64 + lane] = acc0[r][g][i];
#pragma unroll
        for (int g = 0; g < 4; ++g) mypart[(6 + r * 4 + g) * 256 + i * 64 + lane] = acc1[r][g][i];
      }
    __syncthreads();
    stamp(L0.dbg, s, 2);
    float h0v = 0.f, r0 = 0.f, z0 = 0.f, n0 = 0.f, ghn0 = 0.f;
    float h1v = 0.f, r1 = 0.f, z1 = 0.f, n1 = 0.f, ghn1 = 0.f;
    if (do0) {
      float gh[3];
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        float sum = 0.f;
#pragma unroll
        for (int ww = 0; ww < 8; ++ww) sum += partial(ww, q * 3 + g);
        gh[g] = sum + bh0[g];
      }
      r0 = sigmoidf_(gi0[0] + gh[0]);
      z0 = sigmoidf_(gi0[1] + gh[1]);
      n0 = tanhf_(gi0[2] + r0 * gh[2]);
      ghn0 = gh[2];
      h0v = n0 + z0 * (hp0 - n0);
      hp0 = h0v;
      const u16 hb = f2bf(h0v);
      stg[0][row][col] = hb;
      stgT[0][col][row] = hb;
    }
    if (do1) {
      float v[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float sum = 0.f;
#pragma unroll
        for (int ww = 0; ww < 8; ++ww) sum += partial(ww, 6 + q * 4 + g);
        v[g] = sum;
      }
      r1 = sigmoidf_(v[0] + bi1[0] + bh1[0]);
      z1 = sigmoidf_(v[1] + bi1[1] + bh1[1]);
      ghn1 = v[3] + bh1[2];
      n1 = tanhf_(v[2] + bi1[2] + r1 * ghn1);
      h1v = n1 + z1 * (hp1 - n1);
      hp1 = h1v;
      const u16 hb = f2bf(h1v);
      stg[1][row][col] = hb;
      stgT[1][col][row] = hb;
    }
    __syncthreads();   // also: every partial read before the next iteration's staging overwrites it
    stamp(L0.dbg, s, 3);
    if (w < 2) {
      // publish (lo from wave 0, hi from wave 1): the 32x16 bf16 tile, write-through unless the row
      // block is XCD-local; drain; one signal.  Then the row-major copy for the later GEMMs.
      const int ly = w, t = s - ly;
      if (ly == 0 ? do0 : do1) {
        const SeqFwdArgs& Y = ly == 0 ? L0 : L1;
        const u32x4 v = *reinterpret_cast<const u32x4*>(&stg[ly][lane >> 1][(lane & 1) * 8]);
        const unsigned xo = (unsigned)((((size_t)(t % xr) * nrb + rbk) * nunit + ut) * 512 + lane * 8) * 2;
        unsigned* fl = (ly == 0 ? fl0 : fl1) + (size_t)ut * kFlagStride;
        const rsrc_t rX = ly == 0 ? rX0 : rX1;
        if (loc) {
          st16_plain(rX, xo, v);
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          if (lane == 0) signal_flag_local(fl, (unsigned)(t + 1));
        } else {
          st16_sc1(rX, xo, v);
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          if (lane == 0) signal_flag(fl, (unsigned)(t + 1));
        }
        if (ly == 0) stamp(L0.dbg, s, 4);
        *reinterpret_cast<u32x4*>(Y.HSb + ((size_t)(t + 1) * Bp + b0 + (lane >> 1)) * H + j0 + (lane & 1) * 8) = v;
      }
    } else if (w < 6) {
      // waves 2, 3: lo's transposed and fragment-tiled copies; waves 4, 5: hi's
      const int ly = (w - 2) >> 1, t = s - ly;
      const SeqFwdArgs& Y = ly == 0 ? L0 : L1;
      if (ly == 0 ? do0 : do1) {
        if (((w - 2) & 1) == 0) {
          if (Y.HT) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(&stgT[ly][lane >> 2][(lane & 3) * 8]);
            *reinterpret_cast<u32x4*>(Y.HT + (size_t)(j0 + (lane >> 2)) * Y.ldT + (size_t)(t + 1) * Bp + b0 + (lane & 3) * 8) = v;
          }
        } else if (Y.HF) {
          const u32x4 v = *reinterpret_cast<const u32x4*>(&stgT[ly][lane & 15][8 * (lane >> 4)]);
          *reinterpret_cast<u32x4*>(Y.HF + (((size_t)(t + 1) * nunit + ut) * nrb + rbk) * 512 + lane * 8) = v;
        }
      }
    }
    // next step's input gather and the saves for the backward pass after the publishes (a load
    // issued before wave 0's drain would be part of it: vmcnt retires in order)
    load_gi0(s + 1, gin);
    if (do0) {
      L0.HSf[((size_t)(s + 1) * Bp + b) * H + j] = h0v;
      const size_t so = ((size_t)s * Bp + b) * H + j;
      if (L0.s16) st_save16(L0.s16 + so * 4, r0, z0, n0, ghn0);
      else if (L0.sr) { L0.sr[so] = r0; L0.sz[so] = z0; L0.sn[so] = n0; L0.sghn[so] = ghn0; }
    }
    if (do1) {
      L1.HSf[((size_t)s * Bp + b) * H + j] = h1v;
      const size_t so = ((size_t)(s - 1) * Bp + b) * H + j;
      if (L1.s16) st_save16(L1.s16 + so * 4, r1, z1, n1, ghn1);
      else if (L1.sr) { L1.sr[so] = r1; L1.sz[so] = z1; L1.sn[so] = n1; L1.sghn[so] = ghn1; }
    }
  }
}

// ==================================================================== backward
// NKW3: k-steps per wave of the dh GEMM (K = 3H split over 8 waves)
// NTW : 16-col tiles per wave of the fused dW_hh accumulator (H / 128); 0 = not fused
// NTP : 16-col tiles per wave of the fused dP accumulator (V / 128); 0 = not fused
// (Rejected and removed in round 4: dy = dl · W_fc inside this kernel, and the fused weight-gradient
// MFMAs inside the publish drain; docs/DESIGN.md §3.4, §6.3.)
//
// TAIL = true (gru_bwd_seq_tail): the same grid and step loop; the end of the kernel also does the work of
// the single-GPU step's reduce_multi launch (bwd_dp_tail below).  The kernel argument is then
// SeqBwdTailK: the SeqBwdArgs with the tail's own behind them.
struct SeqBwdTailK : SeqBwdArgs { BwdTailArgs t; };
template <bool TAIL> struct BwdKArg { typedef SeqBwdArgs type; };
template <> struct BwdKArg<true> { typedef SeqBwdTailK type; };
// gru_fb_one_kernel's single argument: the three launches' arguments in order, then its own.  Every phase
// reads its part back from the kernel-argument segment at these offsets.
struct FbOneArgs { SeqFwdArgs f; FcXentArgs fc; SeqBwdTailK b; FbOneX x; };
static_assert(std::is_trivially_copyable<FbOneArgs>::value, "the phases read their arguments back byte for byte");
constexpr size_t karg_align(size_t off, size_t al) { return (off + al - 1) / al * al; }
static constexpr size_t kFbOneFcOff = karg_align(sizeof(SeqFwdArgs), alignof(FcXentArgs));
static constexpr size_t kFbOneBOff = karg_align(kFbOneFcOff + sizeof(FcXentArgs), alignof(SeqBwdTailK));
static constexpr size_t kFbOneXOff = karg_align(kFbOneBOff + sizeof(SeqBwdTailK), alignof(FbOneX));
static_assert(sizeof(FbOneArgs) == karg_align(kFbOneXOff + sizeof(FbOneX), alignof(FbOneArgs)),
              "members in declaration order at their natural alignment");

// The end of the TAIL kernel, in this order (with 2. behind 4. the step measured the same, docs/DESIGN.md §6.9):
//  1. every wave's dP partials to slab rbk as 16-B write-through stores (accP[g][nt] is 4 consecutive
//     columns of one row), the bias sums to LDS; drain (s_waitcnt vmcnt(0)), workgroup barrier, one lane
//     signals epoch T + 1 on the workgroup's own flag line (the step loop's last signal was T);
//  2. the bias partials and the dW_hh partials as plain stores (Adam reads them after the launch): they
//     drain while the flags of the partners travel;
//  3. wave 0 polls epoch T + 1 of the nrb workgroups (0 .. nrb-1, ut) -- the writers of this unit tile's 48
//     columns in every slab, one lane each, bounded like every wait here -- then a barrier;
//  4. rows [rbk * V / nrb, (rbk + 1) * V / nrb) x the 48 columns, 32 rows at a time: thread (row, gate,
//     half) loads its 8 columns of every slab with L1-bypassing sc1 loads (its own slab included), all in
//     flight at once, sums them in reduce_multi's order (slab 0, += 1, 2, ..: sum_slabs4), rounds, writes
//     16 B of dP_bf and stages them in LDS (the dead `part`); then dPT_bf in 16-B pieces of 8 rows;
//  5. workgroup 0: the loss partials (reduce_multi's tiny-job sum) and the step counter.
// The hand-off is MI355X_MICROARCH.md 'Valid forms' row 1 in every cell and does not depend on where the
// workgroups run.  Like fwd_fc_tail it takes nothing from the step loop but the accumulators: arguments
// re-read from the kernel-argument segment through an opaque pointer, the thread index opaque.
static_assert(std::is_trivially_copyable<SeqBwdTailK>::value, "the tail reads its arguments back from the kernel-argument segment");
// ONE (gru_fb_one_kernel): the arguments lie at kFbOneBOff, the flag lines foff words behind a.cnt (the
// launch's flag set); the loss partials were written inside this launch and are read sc1; workgroup 0 also
// bumps the launch counter whose parity picks the next launch's flag set.
template <int NTW, int NTP, bool ONE = false>
DEV void bwd_dp_tail(const f32x4 (&accW)[3][NTW], const f32x4 (&accP)[3][NTP], const float (&dbh)[3], float dbi,
                     float (*red)[16][33], unsigned char* stage /* >= 32 * 56 u16 */, unsigned foff = 0u) {
  typedef const __attribute__((address_space(4))) char* kptr_t;
  kptr_t kp = (kptr_t)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(kp));
  const SeqBwdTailK& k = *(const SeqBwdTailK*)(kp + (ONE ? kFbOneBOff : 0));
  const SeqBwdArgs& a = k;
  unsigned* const cnt = a.cnt + (ONE ? (size_t)foff : (size_t)0);
  int tid = (int)threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int lane = tid & 63, w = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int H = a.H, H3 = 3 * H, V = a.V, T = a.T, nrb = a.Bp / 32;
  const int nunit = H / 16, ut = seq_unit_tile(nrb), rbk = seq_row_block(nrb), j0 = ut * 16;
  const unsigned slab_bytes = (unsigned)((size_t)V * H3 * 4);
  const rsrc_t rP = make_rsrc(a.dP_part, (unsigned)nrb * slab_bytes);   // <= 8 slabs of 1.5 MB
  stamp(a.dbg, T + 1, 0);
  // ---- 1. dP partials out write-through, then the signal
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int nt = 0; nt < NTP; ++nt) {
      const unsigned o = (unsigned)rbk * slab_bytes +
                         (unsigned)((((w * NTP + nt) * 16 + lr) * H3 + g * H + j0 + lq * 4) * 4);
      st16_sc1(rP, o, __builtin_bit_cast(u32x4, accP[g][nt]));
    }
  {
    const int rb = tid >> 8, reg = (tid >> 6) & 3, ln = tid & 63;
    const int row = rb * 16 + (ln >> 4) * 4 + reg, col = ln & 15;
    red[0][col][row] = dbh[0]; red[1][col][row] = dbh[1]; red[2][col][row] = dbh[2];
    red[3][col][row] = dbh[0]; red[4][col][row] = dbh[1]; red[5][col][row] = dbi;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  lds_barrier();
  if (tid == 0) signal_flag(cnt + ((size_t)rbk * nunit + ut) * kFlagStride, (unsigned)(T + 1));
  stamp(a.dbg, T + 1, 1);
  // ---- 2. bias and dW_hh partials of this row block (plain)
  if (tid < 96) {
    const int kk = tid >> 4, c = tid & 15;
    float sum = 0.f;
    for (int rr = 0; rr < 32; ++rr) sum += red[kk][c][rr];
    float* dst = (kk < 3 ? a.dbhh_part : a.dbih_part);
    if (dst) dst[(size_t)rbk * H3 + (kk % 3) * H + j0 + c] = sum;
  }
  {
    float* W = a.dWhh_part + (size_t)rbk * H3 * H;
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          W[(size_t)(g * H + j0 + lq * 4 + i) * H + (w * NTW + nt) * 16 + lr] = accW[g][nt][i];
  }
  // ---- 3. the partners: every writer of these 48 columns
  if (tid < 64) {
    SpinBudget spin(a.err);
    for (;;) {
      bool ok = true;
      if (lane < nrb)
        ok = __hip_atomic_load(cnt + ((size_t)lane * nunit + ut) * kFlagStride, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT) >= (unsigned)(T + 1);
      if (__all(ok)) break;
      __builtin_amdgcn_s_sleep(GK_POLL_SLEEP);
      if (spin.expired()) {
        if (lane == 0) __hip_atomic_fetch_or(a.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
    }
  }
  lds_barrier();   // (no vmcnt wait: the plain stores above stay in flight)
  stamp(a.dbg, T + 1, 2);
  // ---- 4. sum the slabs of this workgroup's share, write the bf16 operands
  constexpr int LDS_P = 56;   // u16 per staged row: 48 columns, 16-B aligned rows
  u16* const tile = reinterpret_cast<u16*>(stage);
  const int rows = V / nrb, v0 = rbk * rows;
  const int irow = tid / 6, ipc = tid % 6;           // item: row of the chunk, 8-column piece (gate, half)
  const int icol = (ipc >> 1) * H + j0 + (ipc & 1) * 8;
  const int tcol = tid >> 2, tseg = tid & 3;         // transposed piece: column, 8-row segment
  for (int r0 = 0; r0 < rows; r0 += 32) {
    if (tid < 192 && r0 + irow < rows) {
      const size_t e = (size_t)(v0 + r0 + irow) * H3 + icol;
      f32x4 x[8][2];
#pragma unroll
      for (int s = 0; s < 8; ++s)
        if (s < nrb) {
          const unsigned o = (unsigned)s * slab_bytes + (unsigned)(e * 4);
          x[s][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rP, o, 0, 16));
          x[s][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rP, o + 16u, 0, 16));
        }
      f32x4 s0 = x[0][0], s1 = x[0][1];
#pragma unroll
      for (int s = 1; s < 8; ++s)
        if (s < nrb) {
#pragma unroll
          for (int i = 0; i < 4; ++i) { s0[i] += x[s][0][i]; s1[i] += x[s][1][i]; }
        }
      u32x4 pv;
      pv[0] = (unsigned)f2bf(s0[0]) | ((unsigned)f2bf(s0[1]) << 16);
      pv[1] = (unsigned)f2bf(s0[2]) | ((unsigned)f2bf(s0[3]) << 16);
      pv[2] = (unsigned)f2bf(s1[0]) | ((unsigned)f2bf(s1[1]) << 16);
      pv[3] = (unsigned)f2bf(s1[2]) | ((unsigned)f2bf(s1[3]) << 16);
      *reinterpret_cast<u32x4*>(k.t.dP_bf + e) = pv;
      *reinterpret_cast<u32x4*>(tile + irow * LDS_P + ipc * 8) = pv;
    }
    lds_barrier();
    if (tid < 192 && r0 + tseg * 8 < rows) {
      u16 v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = tile[(tseg * 8 + q) * LDS_P + tcol];
      const int gcol = (tcol >> 4) * H + j0 + (tcol & 15);
      *reinterpret_cast<u32x4*>(k.t.dPT_bf + (size_t)gcol * V + v0 + r0 + tseg * 8) = *reinterpret_cast<const u32x4*>(v);
    }
    if (r0 + 32 < rows) lds_barrier();   // the tile is written again
  }
  // ---- 5. the loss and the step counter
  if (blockIdx.x == 0 && tid < 64) {
    float l;
    if constexpr (ONE) {   // wave_strided_sum's order over sc1 loads
      float acc = 0.f;
      for (int s = lane; s < k.t.nloss; s += 64)
        acc += __hip_atomic_load(k.t.loss_part + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      l = wave_sum(acc);
    } else l = wave_strided_sum(k.t.loss_part, k.t.nloss, 1, 0, lane);
    if (tid == 0) {
      k.t.loss[0] = l;
      *k.t.step += 1;
      if constexpr (ONE) {
        kptr_t kx = kp + kFbOneXOff;
        asm volatile("" : "+s"(kx));
        *((const FbOneX*)kx)->launches += 1u;
      }
    }
  }
  stamp(a.dbg, T + 1, 3);
}

template <int NKW3, int NTW, int NTP, bool TAIL = false>
__global__ void __launch_bounds__(512, 1) gru_bwd_seq_kernel(typename BwdKArg<TAIL>::type a) {
  static_assert(!TAIL || (NKW3 == 6 && NTW == 4 && NTP == 2), "the tail is built for H = 512, V = 256");
  // (bwd_dp_tail reads the argument back from offset 0 of the kernel-argument segment)
  static_assert(std::is_same<decltype(&gru_bwd_seq_kernel<NKW3, NTW, NTP, TAIL>), void (*)(typename BwdKArg<TAIL>::type)>::value,
                "gru_bwd_seq_kernel takes one argument struct and nothing else");
  // (TAIL: built for the plan that takes it alone -- packed saves, the HF copy, no transposed or row-major
  // dG copies -- so the step loop carries none of the other forms' pointers: with them its scalars were
  // parked in VGPR lanes, ~50 v_readlane per step against the plain kernel's 4)
  __shared__ __attribute__((aligned(16))) float part[8][2][256];      // 16 KB
  __shared__ __attribute__((aligned(16))) u16 srow[3][32][24];        // dGh tile, gate-major (exchange; 48-B rows)
  __shared__ __attribute__((aligned(16))) u16 sgT[4][16][40];         // dGh^T gates r,z,n + dGi_n^T (padded rows)
  __shared__ __attribute__((aligned(16))) float red[6][16][33];
  // the resident W_hh^T K-slice of the variants that keep it in LDS, lane-linear; the step's 32 row ids
  constexpr bool kBwL = NTW > 0 || NTP > 0 || NKW3 >= 12;
  __shared__ __attribute__((aligned(16))) bf16x8 bwL[kBwL ? NKW3 : 1][kBwL ? 512 : 1];
  __shared__ __attribute__((aligned(16))) int idsL[NTP > 0 ? 32 : 1];
#include "gru_seq_bwd_body.h"

  if constexpr (TAIL) {   // the partials, their dP sum, the loss and the step counter
    bwd_dp_tail<NTW, NTP>(accW, accP, dbh, dbi, red, reinterpret_cast<unsigned char*>(&part[0][0][0]));
    return;
  }
  // ---- partial weight gradients of this row block
  if constexpr (NTW > 0) {
    float* W = a.dWhh_part + (size_t)rbk * H3 * H;
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          W[(size_t)(g * H + j0 + (lane >> 4) * 4 + i) * H + (w * NTW + nt) * 16 + lr] = accW[g][nt][i];
  }
  if constexpr (NTP > 0) {
    float* Pp = a.dP_part + (size_t)rbk * a.V * H3;
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int nt = 0; nt < NTP; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          Pp[(size_t)((w * NTP + nt) * 16 + lr) * H3 + g * H + j0 + (lane >> 4) * 4 + i] = accP[g][nt][i];
  }
  // ---- bias gradients: reduce the per-thread sums over the 32 rows of the block
  red[0][col][row] = dbh[0]; red[1][col][row] = dbh[1]; red[2][col][row] = dbh[2];
  red[3][col][row] = dbh[0]; red[4][col][row] = dbh[1]; red[5][col][row] = dbi;
  __syncthreads();
  if (tid < 96) {
    const int k = tid >> 4, c = tid & 15;
    float sum = 0.f;
    for (int rr = 0; rr < 32; ++rr) sum += red[k][c][rr];
    float* dst = (k < 3 ? a.dbhh_part : a.dbih_part);
    if (dst) dst[(size_t)rbk * H3 + (k % 3) * H + j0 + c] = sum;
  }
}

// ==================================================================== forward + backward in one launch
// gru_fb_one_kernel: the one-layer H = 512, V = 256 single-GPU step's two persistent launches as one, on
// their common grid (H/16 x Bp/32 workgroups, the same block -> (unit tile, row block) map and the same
// per-thread item): forward loop, FC head tail, a hand-over per ROW BLOCK, backward loop, dP tail.  The
// backward of a row block needs nothing of another row block's forward, so a workgroup waits only for
// the nunit workgroups of its own row block -- not for the slowest FC tail of the chip -- keeps `loc`
// (no second placement census) and has its W_hh^T slice in flight across the wait.
//
// Hand-over (docs/DESIGN.md section 6.11).  Bytes that cross workgroups: dy (every FC tail of the row block ->
// every backward workgroup of it), HF (forward wave 2 -> the backward's fused dW_hh operand loads).  Both
// are plain stores and plain loads, so the hand-over is the release / acquire form of MI355X_MICROARCH.md
// 'Valid forms': producer = every wave's s_waitcnt vmcnt(0), workgroup barrier, lane 0's agent release,
// vmcnt(0), relaxed agent flag store of epoch T + 2 on the workgroup's own forward line; consumer = wave 0's
// poll of the row block's nunit lines, ONE agent acquire, vmcnt(0), workgroup barrier, plain loads.  An
// XCD-local row block leaves out the release (the bytes stay in the L2 all its workgroups share, as in the
// recurrence's local form) and signals with the plain flag store; its consumers still invalidate their L1.
// HSf and the packed saves are written and read by the same thread.  The loss partials: FcXTailOne.
//
// Flags: two sets of (forward block, backward block); the parity of a device launch counter, read at
// kernel start, picks this launch's set, the prologue zeroes the other set for the next launch (the
// kernel boundary orders that), workgroup 0 bumps the counter as its last act (every workgroup read it
// at its start, long before any row block can have finished).  The two exchange rings have regions of
// their own: row block A may be in its backward while row block B is still in its forward.
// LDS: the forward's union and the backward's arrays overlaid (together they would not fit 160 KB).
struct FbOneBwdLds {
  float part[8][2][256];
  u16 srow[3][32][24];
  u16 sgT[4][16][40];
  float red[6][16][33];
  bf16x8 bwL[6][512];
  int idsL[32];
};
static constexpr size_t kFbOneLds = sizeof(FbOneBwdLds) > kFwdTailLds ? sizeof(FbOneBwdLds) : kFwdTailLds;

// (a template only so that the bodies' discarded `if constexpr` branches stay unchecked, as in their own kernels)
template <int NKW, int RS, int NKW3, int NTW, int NTP, bool FC = false>
__global__ void __launch_bounds__(512, 1) gru_fb_one_kernel(FbOneArgs k) {
  static_assert(NKW == 4 && RS == 2 && NKW3 == 6 && NTW == 4 && NTP == 2 && !FC, "built for H = 512, V = 256");
  static_assert(std::is_same<decltype(&gru_fb_one_kernel<NKW, RS, NKW3, NTW, NTP, FC>), void (*)(FbOneArgs)>::value,
                "one argument struct and nothing else");
  static_assert(kFbOneFcOff == (sizeof(SeqFwdArgs) + alignof(FcXentArgs) - 1) / alignof(FcXentArgs) * alignof(FcXentArgs),
                "fwd_fc_tail finds the head's arguments where the two-argument forward has them");
  __shared__ __attribute__((aligned(16))) unsigned char smem[kFbOneLds];
  typedef const __attribute__((address_space(4))) char* kptr_t;
  constexpr bool TAIL = true;
  // ---- the launch's flag set; the other one zeroed for the next launch
  unsigned foff;
  {
    const unsigned par = __builtin_amdgcn_readfirstlane(__hip_atomic_load(k.x.launches, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) & 1u;
    foff = par * (unsigned)k.x.set_words;
    zero_next_flags(k.f.cnt + (size_t)(par ^ 1u) * k.x.set_words, k.x.set_words);
  }
#define GK_FB_ONE 1
  // ---- forward loop, FC head tail
  bool loc_f;
  {
    const SeqFwdArgs& a = k.f;
    const typename FwdFcArg<!FC>::type& fc = k.fc;   // (the FC consumers' arguments: unused, FC is false)
    (void)fc;
#include "gru_seq_fwd_body.h"
    loc_f = loc;
  }
  fwd_fc_tail<true>(loc_f, smem, foff);
  // ---- hand-over: this workgroup's FC blocks are done
  bf16x8 wpre[NKW3];
  {
    kptr_t kp = (kptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kp));
    const SeqFwdArgs& a = *(const SeqFwdArgs*)kp;
    const SeqBwdArgs& b = *(const SeqBwdTailK*)(kp + kFbOneBOff);
    int tid = (int)threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, w = tid >> 6, lr = lane & 15, lk = 8 * (lane >> 4);
    const int T = a.T, nrb = a.Bp / 32, nunit = a.H / 16;
    const int ut = seq_unit_tile(nrb), rbk = seq_row_block(nrb);
    // the backward's W_hh^T slice depends only on the launch before: in flight across the wait
#pragma unroll
    for (int kk = 0; kk < NKW3; ++kk)
      wpre[kk] = ld8(b.WhhT + (size_t)(ut * 16 + lr) * (3 * 512) + w * NKW3 * 32 + kk * 32 + lk);
    unsigned* const fl = a.cnt + (size_t)foff + (size_t)rbk * nunit * kFlagStride;
    stamp(a.dbg, T + 1, 7);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every wave: its dy / HF / HSf / save stores (and wpre)
    __syncthreads();
    if (tid == 0) {
      if (loc_f) signal_flag_local(fl + (size_t)ut * kFlagStride, (unsigned)(T + 2));
      else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        signal_flag(fl + (size_t)ut * kFlagStride, (unsigned)(T + 2));
      }
    }
    sweep_flags(fl, nunit, (unsigned)(T + 2), a.err);
    if (tid < 64) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();   // also: the forward's use of the LDS union is over
    stamp(a.dbg, T + 2, 0);
  }
  // ---- backward loop, dP tail
  {
    kptr_t kp = (kptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kp));
    const SeqBwdTailK& a = *(const SeqBwdTailK*)(kp + kFbOneBOff);
    FbOneBwdLds& L = *reinterpret_cast<FbOneBwdLds*>(smem);
    auto& part = L.part;
    auto& srow = L.srow;
    auto& sgT = L.sgT;
    auto& red = L.red;
    auto& bwL = L.bwL;
    auto& idsL = L.idsL;
#include "gru_seq_bwd_body.h"
    bwd_dp_tail<NTW, NTP, true>(accW, accP, dbh, dbi, red, reinterpret_cast<unsigned char*>(&part[0][0][0]), foff);
  }
#undef GK_FB_ONE
}

// ==================================================================== host side
template <class K>
static int resident_blocks(K kernel, int block = 512) {
  int dev = 0, ncu = 0, per = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, block, 0) != hipSuccess) return 0;
  return ncu * per;
}

// row-tile split: RS = 2 up to H = 512 (H=512 forward kernel 77.5 -> 72.5 us, per step 2.16 ->
// 2.00 us); RS = 1 at H = 1024, where the K/4 slice's 16 producers per wave measured no better
// (profiles/r1_fwd_row_split_ab.json).
static int fwd_rs(int H) { return H <= 512 ? 2 : 1; }

#define FWD_VARIANTS(X) X(256, 1, 1) X(256, 2, 2) X(512, 2, 1) X(512, 4, 2) X(1024, 4, 1) X(1024, 8, 2)

bool gru_fwd_seq_supported(int H, int Bp) {
  if (Bp % 32) return false;
  const int rs = fwd_rs(H);
  int cap = -1;
#define X(HH, NK, RS) if (H == HH && rs == RS) cap = resident_blocks(gru_fwd_seq_kernel<NK, RS, false>);
  FWD_VARIANTS(X)
#undef X
  return cap >= (H / 16) * (Bp / 32);
}

void gru_fwd_seq(const SeqFwdArgs& a, hipStream_t s) {
  if ((size_t)(a.T + 1) * a.Bp * a.H * (a.s16 ? 8 : 4) >= (1ull << 31))
    throw std::runtime_error("gru_fwd_seq: saves exceed the 2 GB buffer-offset range");
  dim3 grid((a.H / 16) * (a.Bp / 32)), block(512);
  const int rs = fwd_rs(a.H);
#define X(HH, NK, RS)                                                          \
  if (a.H == HH && rs == RS) {                                                \
    hipLaunchKernelGGL((gru_fwd_seq_kernel<NK, RS, false>), grid, block, 0, s, a, SeqFcArgs{});   \
    return;                                                                    \
  }
  FWD_VARIANTS(X)
#undef X
  throw std::runtime_error("gru_fwd_seq: no kernel variant for this shape");
}

// The one-layer forward with the FC consumers in the same grid (H = 512, V = 256): co-residency of
// the H/16 x Bp/32 recurrence blocks AND nrb x kFcCons consumers (two 512-thread workgroups per CU at
// <= 128 VGPRs and ~52 KB of LDS each), and room for both in one 64-lane placement census.
bool gru_fwd_seq_fc_supported(int H, int Bp, int V) {
  if (H != 512 || V != 256 || Bp % 32 || fwd_rs(H) != 2) return false;
  if (H / 16 + kFcCons > 64) return false;
  const int cap = resident_blocks(gru_fwd_seq_kernel<4, 2, true>);
  return cap >= (H / 16 + kFcCons) * (Bp / 32);
}

void gru_fwd_seq_fc(const SeqFwdArgs& a, const SeqFcArgs& f, hipStream_t s) {
  if (a.H != 512 || f.V != 256 || !a.HF || !f.Wf || !f.WTf || !f.dlF || !f.dy || !f.dW || !f.db || !f.loss_part ||
      !f.labels || !f.inv_count || !f.b)
    throw std::runtime_error("gru_fwd_seq_fc: needs H = 512, V = 256, the HF copy and every FC buffer");
  if ((size_t)(a.T + 1) * a.Bp * a.H * (a.s16 ? 8 : 4) >= (1ull << 31))
    throw std::runtime_error("gru_fwd_seq_fc: saves exceed the 2 GB buffer-offset range");
  const int nrb = a.Bp / 32;
  dim3 grid((a.H / 16) * nrb + kFcCons * nrb), block(512);
  if (f.probe & 16)   // diagnostic: the FC build without the 128-VGPR cap (cannot host consumers)
    hipLaunchKernelGGL((gru_fwd_seq_kernel<4, 2, true, 1>), grid, block, 0, s, a, f);
  else
    hipLaunchKernelGGL((gru_fwd_seq_kernel<4, 2, true>), grid, block, 0, s, a, f);
}

// The one-layer forward with the FC head as its tail (H = 512, V = 256): the recurrence's own grid.
// (H = 1024 is not built: no plan of the trainer would take it untested.)
bool gru_fwd_seq_tail_supported(int H, int Bp, int V) {
  if (H != 512 || V != 256 || Bp % 32 || fwd_rs(H) != 2) return false;
  const int cap = resident_blocks(gru_fwd_seq_kernel<4, 2, false, 1, true>);
  return cap >= (H / 16) * (Bp / 32);
}

static void check_fwd_tail_args(const SeqFwdArgs& a, const FcXentArgs& f) {
  if (a.H != 512 || f.H != 512 || f.V != 256 || f.M != a.T * a.Bp || f.X != a.HSb + (size_t)a.Bp * a.H || !f.Wf || !f.WTf ||
      !f.dy || f.dl || !f.dlT || !f.loss_part || !f.labels || !f.inv_count || !f.b || !a.s16)
    throw std::runtime_error("gru_fwd_seq_tail: needs H = 512, V = 256, the packed saves (s16), X = HSb + Bp * H and the "
                             "fused-dH FC arguments");
  if ((size_t)(a.T + 1) * a.Bp * a.H * (a.s16 ? 8 : 4) >= (1ull << 31))
    throw std::runtime_error("gru_fwd_seq_tail: saves exceed the 2 GB buffer-offset range");
}

void gru_fwd_seq_tail(const SeqFwdArgs& a, const FcXentArgs& f, hipStream_t s) {
  check_fwd_tail_args(a, f);
  dim3 grid((a.H / 16) * (a.Bp / 32)), block(512);
  hipLaunchKernelGGL((gru_fwd_seq_kernel<4, 2, false, 1, true>), grid, block, 0, s, a, f);
}

#define FWD2_VARIANTS(X) X(256, 1) X(512, 2) X(1024, 4)

bool gru_fwd_seq2_supported(int H, int Bp) {
  if (Bp % 32) return false;
  int cap = -1;
#define X(HH, NK) if (H == HH) cap = resident_blocks(gru_fwd_seq2_kernel<NK>);
  FWD2_VARIANTS(X)
#undef X
  return cap >= (H / 16) * (Bp / 32);
}

void gru_fwd_seq2(const SeqFwd2Args& a, hipStream_t s) {
  const SeqFwdArgs& l0 = a.lo;
  const SeqFwdArgs& l1 = a.hi;
  if (l1.H != l0.H || l1.Bp != l0.Bp || l1.T != l0.T || !a.Wih || !a.bih || !l1.HSf || !l1.HSb || !l1.xch ||
      !l1.cnt || l1.xch == l0.xch || l1.cnt == l0.cnt)
    throw std::runtime_error("gru_fwd_seq2: inconsistent layer arguments");
  dim3 grid((l0.H / 16) * (l0.Bp / 32)), block(512);
#define X(HH, NK)                                                           \
  if (l0.H == HH) {                                                         \
    hipLaunchKernelGGL((gru_fwd_seq2_kernel<NK>), grid, block, 0, s, a);    \
    return;                                                                 \
  }
  FWD2_VARIANTS(X)
#undef X
  throw std::runtime_error("gru_fwd_seq2: no kernel variant for H=" + std::to_string(l0.H));
}

// fused-variant table: (H, fuse dW_hh, fuse dP) -> kernel
#define BWD_VARIANTS(X)               \
  X(256, 3, 2, 2) X(256, 3, 2, 0) X(256, 3, 0, 0) \
  X(512, 6, 4, 2) X(512, 6, 4, 0) X(512, 6, 0, 0) \
  X(1024, 12, 0, 2) X(1024, 12, 0, 0)

bool gru_bwd_seq_supported(int H, int Bp, bool fuse_w, bool fuse_p) {
  if (Bp % 32) return false;
  int cap = -1;
#define X(HH, NK, NW, NP) \
  if (H == HH && (NW > 0) == fuse_w && (NP > 0) == fuse_p) cap = resident_blocks(gru_bwd_seq_kernel<NK, NW, NP>);
  BWD_VARIANTS(X)
#undef X
  return cap >= (H / 16) * (Bp / 32);
}

void gru_bwd_seq(const SeqBwdArgs& a, hipStream_t s) {
  dim3 grid((a.H / 16) * (a.Bp / 32)), block(512);
  const bool fw = a.dWhh_part != nullptr, fp = a.dP_part != nullptr;
#define X(HH, NK, NW, NP)                                                              \
  if (a.H == HH && (NW > 0) == fw && (NP > 0) == fp) {                                \
    hipLaunchKernelGGL((gru_bwd_seq_kernel<NK, NW, NP>), grid, block, 0, s, a);       \
    return;                                                                            \
  }
  BWD_VARIANTS(X)
#undef X
  // an unmatched (H, fuse dW_hh, fuse dP) must not silently leave the gradients untouched
  throw std::runtime_error("gru_bwd_seq: no kernel variant for H=" + std::to_string(a.H) +
                           " fuse_w=" + std::to_string(fw) + " fuse_p=" + std::to_string(fp));
}

// The fused backward with the dP / loss / step-counter sums as its tail (H = 512, V = 256; at most 8 row
// blocks: the tail keeps one 8-column piece of every slab in registers).
bool gru_bwd_seq_tail_supported(int H, int Bp, int V) {
  if (H != 512 || V != 256 || Bp < 32 || Bp % 32 || Bp / 32 > 8) return false;
  const int nrb = Bp / 32;
  if (V % nrb || (V / nrb) % 8) return false;
  const int cap = resident_blocks(gru_bwd_seq_kernel<6, 4, 2, true>);
  return cap >= (H / 16) * nrb;
}

static void check_bwd_tail_args(const SeqBwdArgs& a, const BwdTailArgs& t) {
  const int nrb = a.Bp / 32;
  if (a.H != 512 || a.V != 256 || a.Bp < 32 || a.Bp % 32 || nrb > 8 || a.V % nrb || (a.V / nrb) % 8 || !a.dWhh_part || !a.dP_part ||
      !a.s16 || !a.HF || a.dghT || a.dgiT || a.dgi || !a.ids || !a.cnt || !a.err || !t.dP_bf || !t.dPT_bf || !t.loss_part || !t.loss || !t.step || t.nloss <= 0)
    throw std::runtime_error("gru_bwd_seq_tail: needs H = 512, V = 256, at most 8 row blocks dividing V into multiples "
                             "of 8 rows, the packed saves (s16), the HF copy, no dG copies, the fused dW_hh / dP "
                             "partials and every tail buffer");
}

void gru_bwd_seq_tail(const SeqBwdArgs& a, const BwdTailArgs& t, hipStream_t s) {
  check_bwd_tail_args(a, t);
  dim3 grid((a.H / 16) * (a.Bp / 32)), block(512);
  SeqBwdTailK k{a, t};
  hipLaunchKernelGGL((gru_bwd_seq_kernel<6, 4, 2, true>), grid, block, 0, s, k);
}

// Both of the above as one launch (gru_fb_one_kernel): the shapes of both, T >= 2, and all H/16 x Bp/32
// workgroups of the merged kernel co-resident.
bool gru_fb_one_supported(int H, int Bp, int V) {
  if (!gru_fwd_seq_tail_supported(H, Bp, V) || !gru_bwd_seq_tail_supported(H, Bp, V)) return false;
  return resident_blocks(gru_fb_one_kernel<4, 2, 6, 4, 2>) >= (H / 16) * (Bp / 32);
}

void gru_fb_one(const SeqFwdArgs& a, const FcXentArgs& f, const SeqBwdArgs& b, const BwdTailArgs& t, const FbOneX& x, hipStream_t s) {
  check_fwd_tail_args(a, f);
  check_bwd_tail_args(b, t);
  const long fw = (long)(a.Bp / 32) * (a.H / 16) * kFlagStride;
  if (a.T < 2 || b.T != a.T || b.Bp != a.Bp || a.h0 || !x.launches || x.set_words < 2 * fw || b.cnt < a.cnt + fw ||
      b.cnt + fw > a.cnt + x.set_words || (const void*)b.xbuf == (const void*)a.xch || b.dy != f.dy || b.HF != a.HF ||
      b.HSf != a.HSf || b.s16 != a.s16 || t.loss_part != f.loss_part)
    throw std::runtime_error("gru_fb_one: needs T >= 2, no carried state, one set of buffers for both phases, the "
                             "backward's flag block behind the forward's inside each of the two flag sets, an "
                             "exchange region per phase and the launch counter");
  dim3 grid((a.H / 16) * (a.Bp / 32)), block(512);
  FbOneArgs k{a, f, SeqBwdTailK{b, t}, x};
  hipLaunchKernelGGL((gru_fb_one_kernel<4, 2, 6, 4, 2>), grid, block, 0, s, k);
}

}  // namespace gk

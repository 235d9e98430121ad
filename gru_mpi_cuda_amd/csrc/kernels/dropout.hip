// Training dropout on the non-recurrent connections (docs/DESIGN.md §3.5; the rule: cpu_ref.dropout_mask).
//
// Two elementwise kernels around a layer's output sequence, both plain grid launches that wait on no other
// workgroup and read the step counter from device memory (one recording serves every replay):
//   dropout_fwd_seq  the bf16 saved states HSb -> the masked, scaled copy Xd [tok][H] the layer's consumer
//                    reads as a GEMM A operand, and its transpose XdT [H][ldT] the weight-gradient products
//                    read as their B operand (Layer::HT's layout and pitch);
//   dropout_bwd_seq  the gradient arriving from above, fp32 dy [tok][H], masked and scaled in place.
// A lane owns four adjacent units of one token: one Philox-4x32-10 call, one 8-byte (forward) or 16-byte
// (backward) access.  The forward's transposed copy goes through an LDS tile of 64 units x 64 tokens held as
// token PAIRS packed in dwords (every LDS access is a whole dword), rows 33 dwords apart: the tile writes
// of a 32-lane group land 2-way on 16 of the 32 write banks (twice a conflict-free ds_write_b32's LDS-array
// cycles, which its own address / data transfer is expected to cover; not measured), its reads on distinct banks.
#include <stdexcept>
#include <string>
#include "kernels.h"
#include "common.h"

#pragma clang fp contract(off)

namespace gk {

namespace {
constexpr int kTile = 64;            // units and tokens per forward tile
constexpr int kPitch = kTile / 2 + 1;   // dwords per tile row (32 token pairs + 1 of padding)

// the four mask words of units j .. j + 3 (j % 4 == 0) of token `tok`
DEV void drop_words(const DropoutArgs& a, unsigned step, long tok, int j, unsigned (&w)[4]) {
  const int t = (int)(tok / a.Bp), b = (int)(tok - (long)t * a.Bp);
  philox4x32_10((unsigned)(j >> 2), (unsigned)(a.b0 + b), ((unsigned)a.layer << 24) | (unsigned)t, step,
              (unsigned)(a.seed & 0xffffffffull), (unsigned)(a.seed >> 32), w);
}

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
}  // namespace

__global__ void __launch_bounds__(256) dropout_fwd_seq_kernel(DropoutArgs a) {
#pragma clang fp contract(off)
  __shared__ unsigned tile[kTile * kPitch];
  const long ntok = (long)a.T * a.Bp;
  const long tok0 = (long)blockIdx.x * kTile;
  const int j0 = (int)blockIdx.y * kTile;
  const int tid = (int)threadIdx.x;
  const unsigned step = (unsigned)*a.step;
  {
    // 16 lanes cover the tile's 64 units of one token (128 B); a thread takes the two tokens of a pair
    const int jq = tid & 15, j = j0 + 4 * jq;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int pr = (tid >> 4) + 16 * p;   // token pair 0 .. 31
      unsigned short v[2][4];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const long tok = tok0 + 2 * pr + e;
        v[e][0] = v[e][1] = v[e][2] = v[e][3] = 0;
        if (tok < ntok && j < a.H) {
          const u32x2 h = *reinterpret_cast<const u32x2*>(a.hsb + (size_t)(tok + a.Bp) * a.H + j);
          unsigned w[4];
          drop_words(a, step, tok, j, w);
          const unsigned short x[4] = {(unsigned short)(h.x & 0xffffu), (unsigned short)(h.x >> 16),
                                       (unsigned short)(h.y & 0xffffu), (unsigned short)(h.y >> 16)};
#pragma unroll
          for (int k = 0; k < 4; ++k) v[e][k] = w[k] >= a.thr ? f2bf(bf2f(x[k]) * a.scale) : (unsigned short)0;
          const u32x2 d = {(unsigned)v[e][0] | ((unsigned)v[e][1] << 16), (unsigned)v[e][2] | ((unsigned)v[e][3] << 16)};
          *reinterpret_cast<u32x2*>(a.xd + (size_t)tok * a.H + j) = d;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) tile[(4 * jq + k) * kPitch + pr] = (unsigned)v[0][k] | ((unsigned)v[1][k] << 16);
    }
  }
  __syncthreads();
  {
    // 16 lanes cover the tile's 64 tokens of one unit (128 B of a row of xdT); ntok % 4 == 0, so a
    // thread's four tokens are inside the sequence together or not at all
    const int c = tid & 15;
    const long tok = tok0 + 4 * c;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int jr = (tid >> 4) + 16 * p, j = j0 + jr;
      if (tok < ntok && j < a.H) {
        const u32x2 d = {tile[jr * kPitch + 2 * c], tile[jr * kPitch + 2 * c + 1]};
        *reinterpret_cast<u32x2*>(a.xdT + (size_t)j * a.ldT + a.Bp + tok) = d;
      }
    }
  }
}

__global__ void __launch_bounds__(256) dropout_bwd_seq_kernel(DropoutArgs a) {
#pragma clang fp contract(off)
  const int hq = a.H >> 2;
  const long n = (long)a.T * a.Bp * hq;
  const unsigned step = (unsigned)*a.step;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long tok = i / hq;
    const int j = (int)(i - tok * hq) * 4;
    f32x4* p = reinterpret_cast<f32x4*>(a.dy + (size_t)tok * a.H + j);
    f32x4 v = *p;
    unsigned w[4];
    drop_words(a, step, tok, j, w);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = w[k] >= a.thr ? v[k] * a.scale : 0.f;
    *p = v;
  }
}

static void dropout_check(const DropoutArgs& a, const char* what) {
  if (!a.step || a.T < 1 || a.Bp < 4 || a.H < 4 || a.Bp % 4 || a.H % 4 || a.T >= (1 << 24) || a.layer < 0 ||
      a.layer > 255 || a.b0 < 0)
    throw std::runtime_error(std::string(what) + ": needs a step word, T in [1, 2^24), Bp % 4 == 0, H % 4 == 0, layer in "
                             "[0, 256) and b0 >= 0");
}

void dropout_fwd_seq(const DropoutArgs& a, hipStream_t s) {
  dropout_check(a, "dropout_fwd_seq");
  const long ntok = (long)a.T * a.Bp;
  if (!a.hsb || !a.xd || !a.xdT || a.ldT < ntok + a.Bp || a.ldT % 4)
    throw std::runtime_error("dropout_fwd_seq: needs hsb, xd, xdT and ldT >= (T + 1) Bp, ldT % 4 == 0");
  if (((uintptr_t)a.hsb | (uintptr_t)a.xd | (uintptr_t)a.xdT) & 7)
    throw std::runtime_error("dropout_fwd_seq: hsb, xd and xdT must be 8-byte aligned");
  const long tb = (ntok + kTile - 1) / kTile;
  if (tb > 0x7fffffffL) throw std::runtime_error("dropout_fwd_seq: too many tokens");
  hipLaunchKernelGGL(dropout_fwd_seq_kernel, dim3((unsigned)tb, (unsigned)((a.H + kTile - 1) / kTile)), dim3(256), 0, s, a);
}

void dropout_bwd_seq(const DropoutArgs& a, hipStream_t s) {
  dropout_check(a, "dropout_bwd_seq");
  if (!a.dy || ((uintptr_t)a.dy & 15)) throw std::runtime_error("dropout_bwd_seq: needs a 16-byte aligned dy");
  const long n = (long)a.T * a.Bp * (a.H / 4);
  long nb = (n + 255) / 256;
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(dropout_bwd_seq_kernel, dim3((unsigned)nb), dim3(256), 0, s, a);
}

}  // namespace gk

// The constrained variants of the persistent small-batch generator: gen_persist_kernel<KJ, L, true, PER,
// CON> (gen_persist_kernel.h) with the MASKED ctl_sample_wave (gen_sample_ctl.h), CON = per-position
// mask or automaton (docs/DESIGN.md §4e / §4g).  A translation unit of its own, so that it compiles
// beside the plain (gen_persist.hip) and the controlled (gen_persist_ctl.hip) variants.
//
// The constraint reaches the kernel as ONE pointer in GenPersistArgs to a GenPersistCon in device
// memory, read where it is used: six flat fields in the kernel argument cost the variants at the
// 256-VGPR cap their last scalar registers (SGPR spills into VGPR lanes, then scratch).
//
// GPN_VARIANTS lists what is supported, in both modes: every variant here has ScratchSize 0 and
// occupancy 2 in the -Rpass-analysis=kernel-resource-usage table (docs/DESIGN.md §4e holds the table).
// It is gen_persist_ctl.hip's list: a shape that is not listed stays on the per-char constrained graph.
#include "gen_persist_kernel.h"

namespace gk {

// (KJ = H / 32, L, PER = V / 64)
#define GPN_VARIANTS(X)                                                                                               \
  X(8, 1, 4) X(8, 2, 4) X(8, 3, 4) X(8, 4, 4) X(16, 1, 4) X(16, 2, 4) X(16, 3, 4) X(16, 4, 4) X(32, 1, 4) X(32, 2, 4) \
  X(8, 1, 8) X(8, 2, 8) X(8, 3, 8) X(8, 4, 8) X(16, 1, 8) X(16, 2, 8) X(16, 3, 8) X(32, 1, 8)

// resident workgroups of the variant on the whole device (0: no such variant, or a query failed)
static int gpn_resident(int KJ, int L, int PER, int mode) {
  int dev = 0, cus = 0, nb = 0;
  bool found = false;
  if (mode != kGenConMask && mode != kGenConAuto) return 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
#define X(K, LL, P)                                                                                                  \
  if (KJ == K && L == LL && PER == P) {                                                                              \
    found = true;                                                                                                    \
    const hipError_t e =                                                                                             \
        mode == kGenConMask                                                                                          \
            ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, gen_persist_kernel<K, LL, true, P, kConMask>, 512, 0) \
            : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, gen_persist_kernel<K, LL, true, P, kConAuto>, 512, 0); \
    if (e != hipSuccess) return 0;                                                                                   \
  }
  GPN_VARIANTS(X)
#undef X
  return found && cus >= kG ? cus * nb : 0;
}

bool gen_persist_con_supported(int H, int L, int V, int N, int ML, int mode) {
  if (!gen_persist_ctl_supported(H, L, V, N, ML)) return false;
  return gpn_resident(H / 32, L, V / 64, mode) >= kG;
}

int gen_persist_con_mode(const GenPersistCon& h) {
  const bool aut = h.allow_next != nullptr || h.allow_start != nullptr;
  if (!h.allow_tab && !h.allow_idx && !aut && !h.allow_state) return kGenConNone;
  if (aut) {
    if (!h.allow_next || !h.allow_start || !h.allow_tab || h.allow_idx)
      throw std::runtime_error("gen_persist_f32: allow_next and allow_start are set together, with allow_tab and without allow_idx");
    if (h.allow_rows > 65535) throw std::runtime_error("gen_persist_f32: an automaton has at most 65535 states");
  } else {
    if (!h.allow_tab || !h.allow_idx)
      throw std::runtime_error("gen_persist_f32: allow_tab and allow_idx are set together or not at all");
    if (h.allow_state) throw std::runtime_error("gen_persist_f32: allow_state belongs to an automaton (allow_next, allow_start)");
  }
  if (h.allow_rows < 1) throw std::runtime_error("gen_persist_f32: constraints need allow_rows >= 1");
  return aut ? kGenConAuto : kGenConMask;
}

__global__ void __launch_bounds__(64) gen_persist_con_store_kernel(GenPersistCon* dev, GenPersistCon h) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *dev = h;
}

void gen_persist_con_store(GenPersistCon* dev, const GenPersistCon& h, hipStream_t s) {
  if (!dev) throw std::runtime_error("gen_persist_con_store: a device struct is required");
  hipLaunchKernelGGL(gen_persist_con_store_kernel, dim3(1), dim3(64), 0, s, dev, h);
}

// gen_persist_f32 has checked the buffers, the shape, the parity and that con / con_mode go together
void gen_persist_con_launch(const GenPersistArgs& a, hipStream_t s) {
  const int KJ = a.H / 32, PER = a.V / 64;
  if (gpn_resident(KJ, a.L, PER, a.con_mode) < kG)
    throw std::runtime_error("gen_persist_f32: no constrained variant for this shape (see gen_persist_con_supported)");
#define X(K, LL, P)                                                                                           \
  if (KJ == K && a.L == LL && PER == P) {                                                                     \
    if (a.con_mode == kGenConMask)                                                                            \
      hipLaunchKernelGGL((gen_persist_kernel<K, LL, true, P, kConMask>), dim3(kG), dim3(512), 0, s, a);       \
    else                                                                                                      \
      hipLaunchKernelGGL((gen_persist_kernel<K, LL, true, P, kConAuto>), dim3(kG), dim3(512), 0, s, a);       \
    return;                                                                                                   \
  }
  GPN_VARIANTS(X)
#undef X
  throw std::runtime_error("gen_persist_f32: no constrained variant");
}

}  // namespace gk

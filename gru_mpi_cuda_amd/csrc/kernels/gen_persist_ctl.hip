// The controlled variants of the persistent small-batch generator: gen_persist_kernel<KJ, L, true, PER>
// (gen_persist_kernel.h) with ctl_sample_wave (gen_sample_ctl.h) as its sampler, PER = V / 64.  A
// translation unit of its own, so that it compiles beside the plain variants (gen_persist.hip).
//
// GPC_VARIANTS lists what is supported: every variant here has ScratchSize 0 and occupancy 2 in the
// -Rpass-analysis=kernel-resource-usage table (docs/DESIGN.md §4b holds the table).  A shape that is
// not listed stays on the per-char controlled graph (gen_persist_ctl_supported is false for it):
// V = 512 (PER = 8) at H = 512, L = 4 and at H = 1024, L = 2, the two shapes whose plain variants sit
// at the 256-VGPR cap, spill 28 and 60 bytes per lane with the 8-per-lane sampler.
#include "gen_persist_kernel.h"

namespace gk {

// (KJ = H / 32, L, PER = V / 64)
#define GPC_VARIANTS(X)                                                                                               \
  X(8, 1, 4) X(8, 2, 4) X(8, 3, 4) X(8, 4, 4) X(16, 1, 4) X(16, 2, 4) X(16, 3, 4) X(16, 4, 4) X(32, 1, 4) X(32, 2, 4) \
  X(8, 1, 8) X(8, 2, 8) X(8, 3, 8) X(8, 4, 8) X(16, 1, 8) X(16, 2, 8) X(16, 3, 8) X(32, 1, 8)

// resident workgroups of the variant on the whole device (0: no such variant, or a query failed)
static int gpc_resident(int KJ, int L, int PER) {
  int dev = 0, cus = 0, nb = 0;
  bool found = false;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
#define X(K, LL, P)                                                                                                 \
  if (KJ == K && L == LL && PER == P) {                                                                             \
    found = true;                                                                                                   \
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, gen_persist_kernel<K, LL, true, P>, 512, 0) != hipSuccess) \
      return 0;                                                                                                     \
  }
  GPC_VARIANTS(X)
#undef X
  return found && cus >= kG ? cus * nb : 0;
}

bool gen_persist_ctl_supported(int H, int L, int V, int N, int ML) {
  if (!gen_persist_supported(H, L, V, N, ML)) return false;
  return gpc_resident(H / 32, L, V / 64) >= kG;
}

// gen_persist_f32 has checked the buffers, the shape and the parity
void gen_persist_ctl_launch(const GenPersistArgs& a, hipStream_t s) {
  const int KJ = a.H / 32, PER = a.V / 64;
  if (gpc_resident(KJ, a.L, PER) < kG)
    throw std::runtime_error("gen_persist_f32: no controlled variant for this shape (see gen_persist_ctl_supported)");
#define X(K, LL, P)                                                                                        \
  if (KJ == K && a.L == LL && PER == P) {                                                                  \
    hipLaunchKernelGGL((gen_persist_kernel<K, LL, true, P>), dim3(kG), dim3(512), 0, s, a);                \
    return;                                                                                                \
  }
  GPC_VARIANTS(X)
#undef X
  throw std::runtime_error("gen_persist_f32: no controlled variant");
}

}  // namespace gk

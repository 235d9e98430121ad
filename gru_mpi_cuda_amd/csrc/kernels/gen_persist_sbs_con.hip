// The constrained instances of the persistent small-call stochastic beam search: gen_persist_sbs_kernel<KJ, L,
// PER, CON> (gen_persist_sbs_kernel.h) with CON = kConMask (a line per prefix and char) or kConAuto (a line per
// slot, by its automaton state): docs/DESIGN.md §4i, "Constraints inside the launch".  A translation unit of its
// own, so that the unconstrained instances (gen_persist_sbs.hip) keep their build and their resource numbers.
//
// GPSC_VARIANTS lists what is shipped, in both modes: every instance here has ScratchSize 0 in the
// -Rpass-analysis=kernel-resource-usage table (docs/DESIGN.md §4i holds it, with the instances left out).  It is
// gen_persist_sbs.hip's list: the mask costs one LDS word per lane and slot inside the selection and nothing
// across the weight-resident products, so no instance is lost to it.  A shape that is not listed keeps the graph.
#include "gen_persist_sbs_kernel.h"

namespace gk {

// (KJ = H / 32, L, PER = V / 64)
#define GPSC_VARIANTS(X)                                                                                              \
  X(8, 1, 4) X(8, 2, 4) X(8, 3, 4) X(8, 4, 4) X(16, 1, 4) X(16, 2, 4) X(16, 3, 4) X(16, 4, 4) X(32, 1, 4) X(32, 2, 4) \
  X(8, 1, 8) X(8, 2, 8) X(8, 3, 8) X(8, 4, 8) X(16, 1, 8) X(16, 2, 8) X(32, 1, 8)

// resident workgroups of the instance on the whole device (0: no such instance, or a query failed)
static int gpsc_resident(int KJ, int L, int PER, int mode) {
  int dev = 0, cus = 0, nb = 0;
  bool found = false;
  if (mode != kGenConMask && mode != kGenConAuto) return 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
#define X(K, LL, P)                                                                                                     \
  if (KJ == K && L == LL && PER == P) {                                                                                 \
    found = true;                                                                                                       \
    const hipError_t e =                                                                                                \
        mode == kGenConMask                                                                                             \
            ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, gen_persist_sbs_kernel<K, LL, P, kConMask>, 512, 0)    \
            : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, gen_persist_sbs_kernel<K, LL, P, kConAuto>, 512, 0);   \
    if (e != hipSuccess) return 0;                                                                                      \
  }
  GPSC_VARIANTS(X)
#undef X
  return found && cus >= kG ? cus * nb : 0;   // one workgroup per CU is the layout; fewer CUs: unsupported
}

bool gen_persist_sbs_con_supported(int H, int L, int V, int N, int W, int ML, int mode) {
  if (!gen_persist_sbs_supported(H, L, V, N, W, ML)) return false;
  return gpsc_resident(H / 32, L, V / 64, mode) >= kG;
}

int gen_persist_sbs_con_mode(const GenPersistSbsArgs& a) {
  const bool aut = a.allow_next != nullptr || a.allow_start != nullptr;
  if (!a.allow_tab && !a.allow_idx && !aut) return kGenConNone;
  if (aut && (!a.allow_next || !a.allow_start || !a.allow_tab || a.allow_idx || a.allow_rows > 65535))
    throw std::runtime_error("gen_persist_sbs_f32: an automaton needs allow_tab, allow_next and allow_start, no allow_idx "
                             "and at most 65535 states");
  if (!aut && (!a.allow_tab || !a.allow_idx))
    throw std::runtime_error("gen_persist_sbs_f32: allow_tab and allow_idx are set together or not at all");
  if (a.allow_rows < 1) throw std::runtime_error("gen_persist_sbs_f32: constraints need allow_rows >= 1");
  return aut ? kGenConAuto : kGenConMask;
}

// gen_persist_sbs_f32 has checked the shape, the buffers and the weights; mode is gen_persist_sbs_con_mode(a)
void gen_persist_sbs_con_launch(const GenPersistSbsArgs& a, int mode, hipStream_t s) {
  const int KJ = a.H / 32, PER = a.V / 64;
  if (gpsc_resident(KJ, a.L, PER, mode) < kG)
    throw std::runtime_error("gen_persist_sbs_f32: unsupported shape or device for a constrained launch "
                             "(see gen_persist_sbs_con_supported)");
#define X(K, LL, P)                                                                                                  \
  if (KJ == K && a.L == LL && PER == P) {                                                                            \
    if (mode == kGenConMask)                                                                                         \
      hipLaunchKernelGGL((gen_persist_sbs_kernel<K, LL, P, kConMask>), dim3(kG), dim3(512), 0, s, a);               \
    else                                                                                                             \
      hipLaunchKernelGGL((gen_persist_sbs_kernel<K, LL, P, kConAuto>), dim3(kG), dim3(512), 0, s, a);               \
    return;                                                                                                          \
  }
  GPSC_VARIANTS(X)
#undef X
  throw std::runtime_error("gen_persist_sbs_f32: no constrained variant");
}

}  // namespace gk

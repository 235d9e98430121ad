// The soft variants of the persistent small-batch generator: gen_persist_kernel<KJ, L, true, 4, CON, true>
// (gen_persist_kernel.h) -- logit bias, presence and frequency penalties (docs/DESIGN.md §4h) applied to
// the logits in registers just before ctl_sample_wave, in each constraint mode (none, per-position mask,
// automaton).  A translation unit of its own, so that it compiles beside the plain (gen_persist.hip), the
// controlled (gen_persist_ctl.hip) and the constrained (gen_persist_con.hip) variants.
//
// V = 256 only (PER = 4): the penalties count bytes, so they need a vocabulary of at most 256 anyway, and a
// V = 512 soft batch stays on the per-char soft graph.  A name's history is kGenSoftML bytes of LDS, so a
// larger max_len is unsupported (not truncated).
//
// The soft fields reach the kernel through the device-side GenPersistCon, like the constraint's (flat
// kernel arguments cost the variants at the 256-VGPR cap their last scalar registers, §4e).
//
// GPS_VARIANTS lists what is supported, per constraint mode: every variant here has ScratchSize 0 and
// occupancy 2 in the -Rpass-analysis=kernel-resource-usage table (docs/DESIGN.md §4h holds the table, and
// names what is left out).  A shape and mode that is not listed stays on the per-char soft graph.
#include "gen_persist_kernel.h"

namespace gk {

// (KJ = H / 32, L), per constraint mode
#define GPS_VARIANTS_NONE(X) X(8, 1) X(8, 2) X(8, 3) X(8, 4) X(16, 1) X(16, 2) X(16, 3) X(16, 4) X(32, 1) X(32, 2)
// (H = 1024, L = 2 with an automaton is left out: at the 256-VGPR cap that variant spills 16 bytes per lane)
#define GPS_VARIANTS_MASK(X) X(8, 1) X(8, 2) X(8, 3) X(8, 4) X(16, 1) X(16, 2) X(16, 3) X(16, 4) X(32, 1) X(32, 2)
#define GPS_VARIANTS_AUTO(X) X(8, 1) X(8, 2) X(8, 3) X(8, 4) X(16, 1) X(16, 2) X(16, 3) X(16, 4) X(32, 1)

// resident workgroups of the variant on the whole device (0: no such variant, or a query failed)
static int gps_resident(int KJ, int L, int PER, int mode) {
  int dev = 0, cus = 0, nb = 0;
  bool found = false;
  if (PER != 4) return 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
#define XM(K, LL, M)                                                                                              \
  if (KJ == K && L == LL) {                                                                                       \
    found = true;                                                                                                 \
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, gen_persist_kernel<K, LL, true, 4, M, true>, 512, 0) != \
        hipSuccess)                                                                                               \
      return 0;                                                                                                   \
  }
#define X(K, LL) XM(K, LL, kConNone)
  if (mode == kGenConNone) { GPS_VARIANTS_NONE(X) }
#undef X
#define X(K, LL) XM(K, LL, kConMask)
  if (mode == kGenConMask) { GPS_VARIANTS_MASK(X) }
#undef X
#define X(K, LL) XM(K, LL, kConAuto)
  if (mode == kGenConAuto) { GPS_VARIANTS_AUTO(X) }
#undef X
#undef XM
  return found && cus >= kG ? cus * nb : 0;
}

bool gen_persist_soft_check(const GenPersistCon& h) {
  const bool soft = h.soft_tab != nullptr;
  if (soft != (h.soft_idx != nullptr) || soft != (h.soft_pres != nullptr) || soft != (h.soft_freq != nullptr) ||
      (soft && h.soft_rows < 1))
    throw std::runtime_error("gen_persist_f32: soft_tab, soft_idx, soft_pres and soft_freq are set together, with soft_rows >= 1");
  return soft;
}

bool gen_persist_soft_supported(int H, int L, int V, int N, int ML, int con_mode) {
  if (V != 256 || ML > kGenSoftML) return false;
  if (con_mode == kGenConNone ? !gen_persist_ctl_supported(H, L, V, N, ML)
                              : !gen_persist_con_supported(H, L, V, N, ML, con_mode))
    return false;
  return gps_resident(H / 32, L, V / 64, con_mode) >= kG;
}

// gen_persist_f32 has checked the buffers, the shape, the parity and that con / con_mode / soft go together
void gen_persist_soft_launch(const GenPersistArgs& a, hipStream_t s) {
  const int KJ = a.H / 32, PER = a.V / 64;
  if (a.ML > kGenSoftML || gps_resident(KJ, a.L, PER, a.con_mode) < kG)
    throw std::runtime_error("gen_persist_f32: no soft variant for this shape (see gen_persist_soft_supported)");
#define XM(K, LL, M)                                                                                        \
  if (KJ == K && a.L == LL) {                                                                               \
    hipLaunchKernelGGL((gen_persist_kernel<K, LL, true, 4, M, true>), dim3(kG), dim3(512), 0, s, a);        \
    return;                                                                                                 \
  }
#define X(K, LL) XM(K, LL, kConNone)
  if (a.con_mode == kGenConNone) { GPS_VARIANTS_NONE(X) }
#undef X
#define X(K, LL) XM(K, LL, kConMask)
  if (a.con_mode == kGenConMask) { GPS_VARIANTS_MASK(X) }
#undef X
#define X(K, LL) XM(K, LL, kConAuto)
  if (a.con_mode == kGenConAuto) { GPS_VARIANTS_AUTO(X) }
#undef X
#undef XM
  throw std::runtime_error("gen_persist_f32: no soft variant");
}

}  // namespace gk

// Persistent fp32 generation for small batches: the plain variants of gen_persist_kernel
// (gen_persist_kernel.h, where the design is described) and the host side of the launch.  The
// controlled variants are instantiated in gen_persist_ctl.hip.
#include "gen_persist_kernel.h"

namespace gk {

#define GP_VARIANTS(X) X(8, 1) X(8, 2) X(8, 3) X(8, 4) X(16, 1) X(16, 2) X(16, 3) X(16, 4) X(32, 1) X(32, 2)

// resident workgroups of the variant on the whole device (0 on any query failure: unsupported)
static int gp_resident(int KJ, int L) {
  int dev = 0, cus = 0, nb = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
#define X(K, LL) \
  if (KJ == K && L == LL && hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, gen_persist_kernel<K, LL>, 512, 0) != hipSuccess) return 0;
  GP_VARIANTS(X)
#undef X
  return cus >= kG ? cus * nb : 0;   // one workgroup per CU is the layout; fewer CUs: unsupported
}

bool gen_persist_supported(int H, int L, int V, int N, int ML) {
  if (N < 1 || N > kNmax || L < 1 || L > 4 || H % 256 || (V != 256 && V != 512) || ML < 1) return false;
  const int KJ = H / 32;
  if (KJ != 8 && KJ != 16 && KJ != 32) return false;
  if (2 * L * KJ > 128) return false;   // resident weight registers per lane
  return gp_resident(KJ, L) >= kG;
}

long gen_persist_ws_floats(int H, int L, int V, int ML) { return 2 * ((long)L * kNmax * H + (long)kNmax * (V + 1)) * ML; }
long gen_persist_sync_words(int L) { return (long)(L + 2) * kG * kFS + 16; }

void gen_persist_fill_ws(float* ws, int H, int L, int V, int ML, hipStream_t s) {
  if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ws), (int)kEmpty, (size_t)gen_persist_ws_floats(H, L, V, ML), s) != hipSuccess)
    throw std::runtime_error("gen_persist_fill_ws: fill failed");
}

void gen_persist_f32(const GenPersistArgs& a, hipStream_t s) {
  if (!gen_persist_supported(a.H, a.L, a.V, a.N, a.ML))
    throw std::runtime_error("gen_persist_f32: unsupported shape or device (see gen_persist_supported)");
  if (!a.ws || !a.sync || !a.err || !a.P || !a.Wfc || !a.bfc || !a.rf || !a.out)
    throw std::runtime_error("gen_persist_f32: missing buffer");
  for (int l = 0; l < a.L; ++l)
    if (!a.Whh[l] || !a.bhh[l] || (l > 0 && (!a.Wih[l] || !a.bih[l])))
      throw std::runtime_error("gen_persist_f32: missing layer weights");
  const int KJ = a.H / 32;
  // tagged slots (poll_x / poll_xs) start as kEmpty: set a.par was refilled by the previous launch;
  // before the first launch the caller fills the whole workspace (gen_persist_fill_ws)
  static_assert((size_t)kG * kXLine <= (size_t)kNmax * 1024, "tagged layout inside the state slots");
  if (a.par != 0 && a.par != 1) throw std::runtime_error("gen_persist_f32: launch parity must be 0 or 1");
  // sampling controls: all five arrays (the controlled variants, gen_persist_ctl.hip) or none
  const int nctl = !!a.inv_temp + !!a.top_k + !!a.top_p + !!a.plen + !!a.prefix;
  if (nctl != 0 && nctl != 5)
    throw std::runtime_error("gen_persist_f32: inv_temp, top_k, top_p, plen and prefix go together (all or none)");
  // constraints: a device struct and its mode, only with the controls (the constrained variants, gen_persist_con.hip)
  // (soft: the struct holds soft controls too, or alone -- the soft variants, gen_persist_soft.hip)
  if ((a.con != nullptr) != (a.con_mode != kGenConNone || a.soft != 0) || (a.con && nctl != 5) ||
      (a.con_mode != kGenConNone && a.con_mode != kGenConMask && a.con_mode != kGenConAuto))
    throw std::runtime_error("gen_persist_f32: con, con_mode and soft go together, with the five controls");
  if (a.soft) { gen_persist_soft_launch(a, s); return; }
  if (a.con) { gen_persist_con_launch(a, s); return; }
  if (nctl == 5) { gen_persist_ctl_launch(a, s); return; }
#define X(K, LL) \
  if (KJ == K && a.L == LL) { hipLaunchKernelGGL((gen_persist_kernel<K, LL>), dim3(kG), dim3(512), 0, s, a); return; }
  GP_VARIANTS(X)
#undef X
  throw std::runtime_error("gen_persist_f32: no variant");
}

}  // namespace gk

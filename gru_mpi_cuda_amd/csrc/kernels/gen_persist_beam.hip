// Beam search for small batches as ONE persistent launch (docs/DESIGN.md §4d, "Inside the persistent
// launch"; the rule: cpu_ref.beam_search; the per-char graph it replaces: Generator::record_beam).
//
// The grid, the residency and the weight layout are gen_persist_kernel's (gen_persist_kernel.h): 256
// workgroups x 512 threads, workgroup b owns U = H / 256 units of every recurrent matrix and VR = V / 256
// FC rows, the fp32 MFMA A-fragments stay in VGPRs for the launch, the 8 wave partials meet in LDS and
// are summed in wave order.  A beam row (row = prefix n x W + beam) is a "name" of that kernel, and its
// model step is that kernel's step of the same (KJ, L) and the same row count, operation for operation
// (the one-row VALU products, the single-tile gates of wave 0, the several-tile products with gh beside
// gi): a width-1 search returns the bytes of the greedy controlled launch.
//
// What is new is between two chars:
//   * Selection.  After the logits hand-off of char t workgroup n < N selects for prefix n: wave w owns
//     beams w, w + 8, w + 16, w + 24 and keeps their candidates' keys in registers (V / 64 per lane and
//     beam); lp is beam_select_f32's (max-subtracted, logf of the sum of expf, the fixed-order DPP
//     helpers), then W rounds of a block-wide arg-max on (order key of the score, -j) through LDS, one
//     barrier per round, only the winner's owner rescanning.  A forced char offers only prefix[t], a
//     finished beam its carry, a dead beam nothing.
//   * Records.  The selecting workgroup publishes per new beam two words -- (parent + 1) | (char + 1) << 6 |
//     state << 16, and the score -- with write-through stores, then its flag of kind L + 1; every
//     workgroup waits for the N flags and reads the N W records back (always this distributed form).
//   * The state follows the parent.  Every char has its own exchange slots and every state that is read
//     from them at char t was produced at char t, in the new order; what crosses a char inside a
//     workgroup is its own units' carry h(t-1) and the early-computed gh = h(t-1) W_hh^T + b_hh.  Both are
//     gathered by parent through LDS, never in place (set A: as computed, set B: as gathered; a dead
//     slot: h = 0, gh = b_hh, input SOS, as beam_reorder leaves it).
//   * Rows, lengths, scores and states of prefix n live in workgroup n's LDS in two sets by step parity;
//     only workgroup n writes prefix n's outputs, after the loop.
//   * The launch ends early once no beam of any prefix is live: every later step would carry every beam
//     to its own slot.
// Every hand-off uses flags (no data-tagged slots: the workspace needs no fill).  Spins are bounded (error
// bit 32, then every wait returns at once and the grid drains; what is read from a record is clamped, so
// a drained launch forms no address from garbage); the last workgroup out zeroes the flags.
// The kernel is gen_persist_beam_kernel.h; this file holds the unconstrained instances and the host side.  The
// constrained instances are gen_persist_beam_con.hip's, a translation unit of their own.
// Out of scope: sample_distinct / sample_conditional (the same loop with other selections), bf16.
#include "gen_persist_beam_kernel.h"

namespace gk {

// (KJ = H / 32, L) per vocabulary: gen_persist.hip's GP_VARIANTS at V = 256; at V = 512 (eight keys per lane
// and beam) three of them spill at the 256-VGPR cap -- (16, 3) 8, (16, 4) 100 and (32, 2) 24 bytes per lane --
// and are left out: those shapes stay on the recorded graph.  Every instance listed has ScratchSize 0 in the
// -Rpass-analysis=kernel-resource-usage table (docs/DESIGN.md §4d holds it)
#define GPB_VARIANTS_256(X) X(8, 1) X(8, 2) X(8, 3) X(8, 4) X(16, 1) X(16, 2) X(16, 3) X(16, 4) X(32, 1) X(32, 2)
#define GPB_VARIANTS_512(X) X(8, 1) X(8, 2) X(8, 3) X(8, 4) X(16, 1) X(16, 2) X(32, 1)

// resident workgroups of the variant on the whole device (0: no such variant, or a query failed)
static int gpb_resident(int KJ, int L, int PER) {
  int dev = 0, cus = 0, nb = 0;
  bool found = false;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
#define XP(K, LL, P)                                                                                               \
  if (KJ == K && L == LL) {                                                                                        \
    found = true;                                                                                                  \
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, gen_persist_beam_kernel<K, LL, P>, 512, 0) != hipSuccess) \
      return 0;                                                                                                    \
  }
#define X(K, LL) XP(K, LL, 4)
  if (PER == 4) { GPB_VARIANTS_256(X) }
#undef X
#define X(K, LL) XP(K, LL, 8)
  if (PER == 8) { GPB_VARIANTS_512(X) }
#undef X
#undef XP
  return found && cus >= kG ? cus * nb : 0;   // one workgroup per CU is the layout; fewer CUs: unsupported
}

bool gen_persist_beam_supported(int H, int L, int V, int N, int W, int ML) {
  if (N < 1 || W < 1 || W > kBW || (long)N * W > kNmax || L < 1 || L > 4 || H < 256 || H % 256 || (V != 256 && V != 512) ||
      ML < 1 || ML > kBML)
    return false;
  const int KJ = H / 32;
  if (KJ != 8 && KJ != 16 && KJ != 32) return false;
  return gpb_resident(KJ, L, V / 64) >= kG;
}

long gen_persist_beam_ws_floats(int H, int L, int V, int ML) { return ((long)L * kNmax * H + (long)kNmax * (V + 2)) * ML; }
long gen_persist_beam_sync_words(int L) { return (long)(L + 2) * kG * kFS + 16; }

void gen_persist_beam_f32(const GenPersistBeamArgs& a, hipStream_t s) {
  if (!gen_persist_beam_supported(a.H, a.L, a.V, a.N, a.W, a.ML))
    throw std::runtime_error("gen_persist_beam_f32: unsupported shape or device (see gen_persist_beam_supported)");
  if (!a.ws || !a.sync || !a.err || !a.P || !a.Wfc || !a.bfc || !a.plen || !a.prefix || !a.rows || !a.logp || !a.n_tok ||
      !a.n_beams)
    throw std::runtime_error("gen_persist_beam_f32: missing buffer");
  for (int l = 0; l < a.L; ++l)
    if (!a.Whh[l] || !a.bhh[l] || (l > 0 && (!a.Wih[l] || !a.bih[l])))
      throw std::runtime_error("gen_persist_beam_f32: missing layer weights");
  if (a.sos < 0 || a.sos >= a.V || a.eos < 0)
    throw std::runtime_error("gen_persist_beam_f32: needs 0 <= sos < V and eos >= 0");
  if (const int mode = gen_persist_beam_con_mode(a); mode != kGenConNone) {
    gen_persist_beam_con_launch(a, mode, s);
    return;
  }
  const int KJ = a.H / 32;
#define XP(K, LL, P)                                                                                    \
  if (KJ == K && a.L == LL) {                                                                           \
    hipLaunchKernelGGL((gen_persist_beam_kernel<K, LL, P>), dim3(kG), dim3(512), 0, s, a);              \
    return;                                                                                             \
  }
#define X(K, LL) XP(K, LL, 4)
  if (a.V == 256) { GPB_VARIANTS_256(X) }
#undef X
#define X(K, LL) XP(K, LL, 8)
  if (a.V == 512) { GPB_VARIANTS_512(X) }
#undef X
#undef XP
  throw std::runtime_error("gen_persist_beam_f32: no variant");
}

}  // namespace gk

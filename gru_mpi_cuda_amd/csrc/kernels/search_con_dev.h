// Device helpers of the constraints inside the two persistent search launches, gen_persist_beam_kernel
// (gen_persist_beam_kernel.h) and gen_persist_sbs_kernel (gen_persist_sbs_kernel.h): docs/DESIGN.md §4d / §4i,
// "Constraints inside the launch".  The rule is beam_select_f32's / sbs_select_f32's MASK and AUTO rule (beam.hip,
// sbs.hip); the tables are the caller's, read in place (Args: GenPersistBeamArgs or GenPersistSbsArgs, which carry
// the same five fields).
//
// How the mask reaches a candidate without a register that lives across the weight-resident products:
//   * scon_stage: the selecting workgroup copies the lines its prefix needs at char st into LDS -- kConMask: the
//     one line allow_idx[n][st]; kConAuto: one line per beam, named by the beam's automaton state -- V / 32 words
//     each, a thread per word.  It runs BEFORE the wait for the logits hand-off of char st, so the two dependent
//     global reads (index or state -> line) overlap the other workgroups' model step.
//   * scon_bits: at key construction a lane reads the one LDS word that covers its V / 64 chars and tests a bit per
//     candidate; the word dies with the candidate loop of its beam.
//   * scon_next: a new beam's state, allow_next[line of its parent][char], looked up by the thread that publishes
//     the beam, after the record is out (no other workgroup reads the state: it is not in the record).
// A line or a state outside [0, allow_rows) ORs 16 into err[0] (err[1] = the value, err[2] = the row) and is taken
// as line 0, as in the per-char kernels and in gen_persist_smc_kernel.
#pragma once
#include "gen_persist_kernel.h"

namespace gk {

namespace {
constexpr int kSconW = 32;   // beams per prefix (the search kernels' kBW)

// lines of the staged table: one per beam under an automaton, one per prefix per position
template <int CON>
constexpr int scon_lines() { return CON == kConAuto ? kSconW : 1; }

// all threads of workgroup n (the barrier that follows is the caller's); q_of: the beams' states (kConAuto)
template <int CON, int V, class Args>
DEV void scon_stage(const Args& a, int n, int st, int W, const int* q_of, unsigned (*ok)[V / 32]) {
  constexpr int WD = V / 32;
  const int i = (int)threadIdx.x, bm = i / WD, wd = i % WD;
  if (bm >= (CON == kConAuto ? W : 1)) return;
  int q = CON == kConAuto ? q_of[bm] : a.allow_idx[(size_t)n * a.ML + st];
  if (q < 0 || q >= a.allow_rows) {   // never expected (the host builds the tables): flag it, line 0
    if (wd == 0) {
      __hip_atomic_fetch_or(a.err, 16u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      a.err[1] = (unsigned)q;
      a.err[2] = (unsigned)(n * W + bm);
    }
    q = 0;
  }
  ok[bm][wd] = a.allow_tab[(size_t)q * WD + wd];
}

// bit e of the result: char c0 + e is allowed (c0 a multiple of V / 64, which divides 32: one word)
template <int CON, int V>
DEV unsigned scon_bits(const unsigned (*ok)[V / 32], int bm, int c0) {
  return ok[CON == kConAuto ? bm : 0][c0 >> 5] >> (c0 & 31);
}

// the child's state: parent state q (clamped as scon_stage clamps it, flagged there), char ch < V
template <class Args>
DEV int scon_next(const Args& a, int q, int ch) {
  if (q < 0 || q >= a.allow_rows) q = 0;
  return a.allow_next[(size_t)q * a.V + ch];
}
}  // namespace

}  // namespace gk

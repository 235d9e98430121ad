// Device-resident batched name generator (reference parity half).
//
// The reference generates ONE name at a time with 51 launches + 2 blocking memcpys +
// host sampling per character (/root/reference/namegensf.cu:649-884).  Here all local
// names advance together: per character, one fused step launch per layer (layer >= 1 fuses
// its input projection W_ih·h_below as a second MFMA product) and one FC+softmax+sample
// launch that writes the chosen char straight into the next step's input ids and into the
// output rows.  The MAX_LEN loop is captured once into a hipGraph; the host touches the
// device only to upload the uniforms and to read the finished names.
#pragma once
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <utility>
#include <vector>
#include "../runtime/runtime.h"
#include "../kernels/kernels.h"

namespace gk {

struct GenDims {
  int V = 256, E = 512, H = 1024, L = 2, max_len = 10, sos = 0, eos = 0, max_batch = 4096;
  // 1: fp32-faithful (the reference's arithmetic: fp32 MFMA GEMMs on the fp32 master weights, IEEE
  // gates and softmax, gen_f32.hip); 0: bf16 MFMA fast mode; 2: bf16x3 -- the fp32 path with its
  // products as bf16 MFMA GEMMs over split operands (hi*hi + hi*lo + lo*hi, ~2^-16 relative error)
  int fp32 = 0;
};

class Generator {
 public:
  Generator(const GenDims& d, const float* params, const std::map<std::string, long>& offsets);
  ~Generator();
  void refresh_weights(hipStream_t s);   // bf16 weights + layer-0 table (call after params change)
  // rf: device [N][max_len] uniforms of THIS rank's names; out: device [N][max_len+1]
  void generate(const float* rf, int N, unsigned char* out, hipStream_t s);
  // generate() with per-name sampling controls (docs/DESIGN.md §4b; device arrays of N entries:
  // inv_temp = 1 / T or 0 for greedy, top_k, top_p, plen, prefix [N][max_len]).  The bf16 mode raises.
  // Per batch of n names: uses_persist_ctl(n) -> ONE controlled persistent launch that reads the
  // caller's uniforms, rows and controls in place (no staging, no arena); else the per-char fp32 /
  // bf16x3 graph with sample_ctl_f32 as its sampler node.  That graph reads the controls from buffers
  // of an arena of their own (allocated by the first batch that takes it) into which each batch's
  // slice is copied, so one recording per n serves every value.
  // Constraints (docs/DESIGN.md §4e; allow_tab [allow_rows][V / 32] and allow_idx [N][max_len], device
  // pointers, both or neither, allow_rows <= kAllowRows): a batch of a constrained call takes the
  // per-char graph in a recording of its own per n, whose sampler reads the table and the batch's idx
  // slice from two more buffers of that arena -- unless uses_persist_con(n, automaton) holds (opt-in,
  // off by default): then ONE constrained persistent launch on the caller's arrays, the table and
  // `next` by pointer, idx and start at the batch's rows: no staging, no arena, no recording.
  struct Ctl {
    const float* inv_temp = nullptr; const int* top_k = nullptr; const float* top_p = nullptr;
    const int* plen = nullptr; const unsigned char* prefix = nullptr;
    const unsigned* allow_tab = nullptr; const int* allow_idx = nullptr; int allow_rows = 0;
    // Automaton (docs/DESIGN.md §4g; both set with allow_tab, never with allow_idx; allow_rows = the
    // states, <= kAutoStates): allow_next [allow_rows][V], allow_start [N] the names' start states
    const unsigned short* allow_next = nullptr; const int* allow_start = nullptr;
    // Soft controls (docs/DESIGN.md §4h; all four set, or all null; 1 <= soft_rows <= kSoftRows):
    // soft_tab [soft_rows][V] the bias lines, soft_idx / soft_pres / soft_freq [N] the names' line and
    // penalties.  They combine with the constraints and with an automaton.
    const float* soft_tab = nullptr; const int* soft_idx = nullptr; int soft_rows = 0;
    const float* soft_pres = nullptr; const float* soft_freq = nullptr;
  };
  static constexpr int kAllowRows = 1024;   // lines of a constraint table
  static constexpr int kAutoStates = 65535; // states of an automaton
  static constexpr int kSoftRows = 256;     // lines of a soft-control bias table
  static constexpr size_t kAutoGraphs = 16; // automaton recordings kept per map (a full map is dropped before the next one)
  // An automaton-constrained generate_ctl() / beam() (score() never sees one: the host walks its known
  // rows into an allow_idx) uploads tab and next once per call into buffers that
  // grow on demand -- a table can be 32 MiB, too much to reserve for every generator -- and every
  // batch takes the controlled per-char graph (beam: its graph) in a recording of its own per (n,
  // states), whose head resets the per-row state buffer from the batch's start states and whose
  // sampler (select) advances it.  Growing the buffers drops those recordings.
  // A soft generate_ctl() / score() (c.soft_tab set) copies the bias table once per call and each batch's
  // soft_idx / soft_pres / soft_freq slice into buffers of their own -- plain allocations made by the first
  // soft call, so the arenas and the workspace sizes of calls without soft controls stay what they are.
  // A soft batch takes the controlled per-char graph, in recordings of their own, kept in maps apart
  // from the others': a call without soft controls never replays a soft recording, nor the reverse --
  // unless uses_persist_soft(n, mode) holds (opt-in, off by default): then ONE soft persistent launch on the
  // caller's arrays, the bias table by pointer, soft_idx / soft_pres / soft_freq at the batch's rows, and a
  // call made of such batches alone stages nothing, allocates nothing and records nothing.
  void generate_ctl(const float* rf, int N, const Ctl& c, unsigned char* out, hipStream_t s);
  int soft_graphs() const {   // soft recordings so far (generation and scoring)
    return (int)(csgraphs_.size() + asgraphs_.size() + scsgraphs_.size());
  }
  size_t ctl_workspace_bytes() const { return carena_.bytes(); }   // 0 until a batch takes the per-char controlled graph
  // generate_ctl() batches of n names run as one controlled persistent launch (exact fp32, as the plain
  // one): up to GK_GEN_PERSIST_CTL_MAX names (default and at most 64), where a controlled variant
  // exists (gen_persist_ctl_supported); off with GK_GEN_PERSIST=0 or set_persist(false)
  bool uses_persist_ctl(int n) const;
  void set_persist_ctl_max(int n) { persist_ctl_max_ = n; }
  // Constrained generate_ctl() batches of n names run as one constrained persistent launch: up to
  // GK_GEN_PERSIST_CON_MAX / set_persist_con_max(n) names -- 0 by default, the path is opt-in
  // (docs/DESIGN.md §4e) -- where uses_persist_ctl(n) holds and a constrained variant of the mode exists
  bool uses_persist_con(int n, bool automaton) const;
  void set_persist_con_max(int n) { persist_con_max_ = n; }
  long persist_con_launches() const { return persist_con_launches_; }   // constrained persistent launches so far
  // Soft generate_ctl() batches of n names run as one soft persistent launch: up to GK_GEN_PERSIST_SOFT_MAX /
  // set_persist_soft_max(n) names -- 0 by default, the path is opt-in (docs/DESIGN.md §4h) -- where
  // uses_persist_ctl(n) holds, for a constrained batch (con_mode = kGenConMask / kGenConAuto) uses_persist_con
  // as well, and a soft variant of the mode exists (gen_persist_soft_supported: V = 256, max_len <= 64)
  bool uses_persist_soft(int n, int con_mode) const;
  void set_persist_soft_max(int n) { persist_soft_max_ = n; }
  long persist_soft_launches() const { return persist_soft_launches_; }   // soft persistent launches so far
  // Teacher-forced scoring of N output rows (device [N][max_len+1], the generate() format): per token
  // log softmax(logits)[target] and the target's rank, per name their sum and the token count (all
  // device pointers: tok_logp / rank [N][max_len], name_logp / n_tok [N]).  Always the exact-fp32
  // arithmetic, whatever GenDims::fp32 says.  Layer-major schedule (the targets are known): per layer
  // ONE input-projection GEMM over all max_len * Bp rows, then its steps; ONE logits GEMM; one
  // log-prob launch.  Buffers are allocated on the first call.
  // With controls (c: generate_ctl's arrays and constraints for the N names, device pointers; n_kept
  // [N][max_len] then required; docs/DESIGN.md §4f): tok_logp is the log-probability under the sampler's
  // distribution, score_ctl_logprob_f32 in place of the last launch -- score_prep, the products and
  // the gates are the plain schedule's.  The controls live in an arena of their own, committed by the
  // first controlled call; each batch's slice is copied there and the table once per call, so a
  // recording bakes no value in: one per (Bp, table lines or 0).  c == nullptr is the call as it was,
  // on the graphs it had.  Every precision mode scores with controls (scoring is exact fp32 always).
  void score(const unsigned char* rows, int N, float* tok_logp, int* rank, float* name_logp, int* n_tok, hipStream_t s,
             const Ctl* c = nullptr, int* n_kept = nullptr);
  // 0 until the first score(); grows when the first controlled score() commits the control buffers
  size_t score_workspace_bytes() const { return sarena_.bytes() + scarena_.bytes(); }
  int score_graphs() const { return (int)(sgraphs_.size() + scgraphs_.size()); }   // recordings so far
  // Beam search (docs/DESIGN.md §4d; the rule: cpu_ref.beam_search): for each of N prefixes (device
  // plen [N], prefix [N][max_len], as generate_ctl's) the W most probable output rows in order:
  // rows [N][W][max_len+1], logp [N][W] (-inf for a dead slot), n_tok [N][W], n_beams [N], all device
  // pointers.  Always the exact-fp32 arithmetic, whatever GenDims::fp32 says.  A name is W rows of the
  // per-char fp32 step; a batch is floor(max_batch / W) names (throws when max_batch < W).  One
  // single-chain graph per (names, W): reset, then per char the step's products and gates on fixed
  // slots (read A, write B), beam_select_f32 and beam_reorder (gather B -> A).  Its buffers live in an
  // arena of their own, committed by the first call; plen / prefix are copied there per batch, so a
  // recording bakes no prefix in.  allow_tab / allow_idx ([N][max_len]) / allow_rows: the names'
  // constraints as in Ctl (null: none); a constrained call has its own graph per (names, W).
  void beam(const int* plen, const unsigned char* prefix, int N, int W, unsigned char* rows, float* logp, int* n_tok,
            int* n_beams, hipStream_t s, const unsigned* allow_tab = nullptr, const int* allow_idx = nullptr,
            int allow_rows = 0, const unsigned short* allow_next = nullptr, const int* allow_start = nullptr);
  // Distinct names (docs/DESIGN.md §4i; the rule: cpu_ref.sample_distinct): for each of N prefixes W rows
  // sampled without replacement, in draw order, from the distribution of inv_t (device [N], 1 / T), the
  // prefix and the constraints -- stochastic beam search.  rows [N][W][max_len+1], logq [N][W] (the rows'
  // log-probability under that distribution, -inf for a dead slot), gumbel [N][W] (the final perturbed
  // values), n_tok [N][W], n_found [N], all device pointers.  Name n draws its noise at the global index
  // start + n under seed.  It is beam()'s loop on beam()'s arena with sbs_select_f32 as the selection: the
  // same batches of floor(max_batch / W) names, the batch's first global index written to a device word
  // (the bytes do not depend on max_batch), recordings of its own per (names, W, constraint lines or
  // states) that bake in no seed, index or temperature.  Two G buffers and the seed / start / inv_t
  // staging are plain allocations made by the first call: no arena and no workspace size changes.
  void distinct(const int* plen, const unsigned char* prefix, int N, int W, unsigned long long seed,
                unsigned long long start, const float* inv_t, unsigned char* rows, float* logq, float* gumbel, int* n_tok,
                int* n_found, hipStream_t s, const unsigned* allow_tab = nullptr, const int* allow_idx = nullptr,
                int allow_rows = 0, const unsigned short* allow_next = nullptr, const int* allow_start = nullptr);
  int distinct_graphs() const { return (int)(dgraphs_.size() + adgraphs_.size()); }   // recordings so far
  // Conditional names (docs/DESIGN.md §4j; the rule: cpu_ref.sample_conditional): for each of N names W
  // weighted particles of a sequential Monte Carlo run over the constrained sampler.  rows [N][W][max_len+1],
  // logw [N][W] (the unnormalised log importance weights: their mean of exp is an unbiased estimate of the
  // rule's probability under the model), logq [N][W] (the rows' log-probability under the sampler), n_tok
  // [N][W], n_res [N] (the resampling steps), all device pointers.  thr: resample when ESS < thr W.  It is
  // distinct()'s loop with smc_select_f32 as the selection: the same batches, the batch's first global index,
  // the seed and thr in device words, recordings of its own per (names, W, constraint lines or states) that
  // bake in none of them.  Its buffers are plain allocations made by the first call.
  void conditional(const int* plen, const unsigned char* prefix, int N, int W, unsigned long long seed,
                   unsigned long long start, float thr, const float* inv_t, unsigned char* rows, float* logw, float* logq,
                   int* n_tok, int* n_res, hipStream_t s, const unsigned* allow_tab = nullptr,
                   const int* allow_idx = nullptr, int allow_rows = 0, const unsigned short* allow_next = nullptr,
                   const int* allow_start = nullptr);
  int conditional_graphs() const { return (int)(qgraphs_.size() + aqgraphs_.size()); }   // recordings so far
  size_t beam_workspace_bytes() const { return barena_.bytes(); }   // 0 until the first beam()
  int beam_graphs() const { return (int)bgraphs_.size(); }          // recordings so far, one per (names, W, constrained)
  int ctl_graphs() const { return (int)cgraphs_.size(); }           // ... of the controlled per-char graph, per (n, constrained)
  int automaton_graphs() const { return (int)(agraphs_.size() + abgraphs_.size()); }   // ... with an automaton
  void set_use_graph(bool g) { use_graph_ = g; }
  // optional: device [Bp][V] softmax of the last generated step (tests)
  void set_probe(float* probs) {
    probe_ = probs; graphs_.clear(); cgraphs_.clear(); agraphs_.clear(); csgraphs_.clear(); asgraphs_.clear();
  }
  // Small batches (fp32 modes: <= GK_GEN_PERSIST_MAX names, default and at most 64; bf16 mode: <= 24):
  // one persistent launch per batch (gen_persist.hip, exact fp32) instead of the per-char graph.
  // On by default; GK_GEN_PERSIST=0 or set_persist(false) turns it off.
  void set_persist(bool on) { persist_ = on; }
  void set_persist_max(int n) { persist_max_ = n; }
  void set_persist_dbg(unsigned long long* p) { persist_dbg_ = p; }   // diagnostic stamps (nullable)
  bool uses_persist(int n) const;
  // names in the whole (data-parallel) job; 0 = unknown (then the per-call count decides)
  void set_global_names(int n) { global_n_ = n > 0 ? n : 0; }
  unsigned read_error();   // blocking: device error word (fp32 path: bit 4 = char id out of range)
  // fault injection (tests): the next persistent launch starts with its spin-timeout bit set, as if
  // an earlier wait had given up -- generate() must notice and regenerate the batch
  void inject_persist_error() { inject_ = true; }
  // diagnostic: DOT dump of the per-char graph captured for batches of n names (false: none yet)
  bool dump_graph(int n, const std::string& path) const {
    auto it = graphs_.find(n);
    if (it == graphs_.end() || !it->second) return false;
    it->second->dot(path.c_str());
    return true;
  }

 private:
  void record_steps(int n_active, hipStream_t s);
  // ctl: sample_ctl_f32 as the sampler node; allow_rows > 0: with the constraint buffers
  // automaton: allow_rows states, the sampler reads atab_ / anxt_ / astate_ and the head resets astate_
  // soft: the sampler reads the soft-control buffers too (soft_rows lines)
  void record_steps_f32(int n_active, hipStream_t s, bool ctl = false, int allow_rows = 0, bool automaton = false,
                        int soft_rows = 0);
  // one product of the fp32 / bf16x3 path: C = h W^T (+ bias) -> splits (slabs of M x N at C).  fp32
  // reads A32 / W32; bf16x3 the split copies A3 ([hi|hi|lo] rows) / W3 ([hi|lo|hi] rows)
  int product_f32(const float* A32, const u16* A3, const float* W32, const u16* W3, const float* bias, int M, int N,
                  float* C, hipStream_t s);
  bool split3() const { return d_.fp32 == 2; }
  void reset_batch(int Bp, bool bf16, hipStream_t s);
  void score_alloc();
  void ctl_alloc();
  // one persistent launch for n names (c: the controlled one, its arrays already at this batch's rows;
  // with c->allow_tab the constrained one) and its error-word read-back.  false: the launch hit its spin limit -- the persistent path is now
  // off, the bit is cleared and the caller regenerates the batch on its per-char graph
  bool persist_launch(const float* rf, int n, const Ctl* c, unsigned char* out, bool last_batch, hipStream_t s);
  // ctl: score_ctl_logprob_f32 as the last launch; allow_rows > 0: with the constraint buffers
  void record_score(int Bp, hipStream_t s, bool ctl = false, int allow_rows = 0, int soft_rows = 0);
  void soft_alloc();
  void score_ctl_alloc();
  void beam_alloc();
  // the beam loop's selection: beam_select_f32; sbs_select_f32 (G by step parity, step 0 reads the reset scores
  // as G); smc_select_f32 (logw by step parity, step 0 reads the reset scores as logw)
  enum class BeamSelect { kBeam, kDistinct, kConditional };
  void record_beam(int n, int W, hipStream_t s, int allow_rows = 0, bool automaton = false,
                   BeamSelect sel = BeamSelect::kBeam);
  void distinct_alloc();
  void conditional_alloc();
  // the automaton buffers for `states` states (grown, never shrunk) and the call's tables into them
  void automaton_stage(const unsigned* tab, const unsigned short* next, int states, hipStream_t s);
  const float* P(const std::string& n) const { return params_ + off_.at(n); }

  GenDims d_;
  int Bmax_;
  const float* params_;
  std::map<std::string, long> off_;
  Arena arena_;
  hipStream_t cap_ = nullptr;
  bool use_graph_ = true;
  float* probe_ = nullptr;
  std::map<int, std::unique_ptr<Graph>> graphs_;   // keyed by active-name count
  // buffers
  std::vector<float*> hf_;             // [L*2][Bmax][H]
  std::vector<u16*> hb_;
  std::vector<u16*> Whh_, Wih_;
  u16 *Emb_, *Wfc_, *WfcF_;
  int step_algo_ = 0;
  float *Ptab_, *rf_;
  float* Ptab32_ = nullptr;     // fp32 layer-0 table of the persistent launch (= Ptab_ in the fp32 modes)
  int *ids_, *alive_;
  unsigned char* out_;
  float *gh_ = nullptr, *gi_ = nullptr, *logits_ = nullptr;   // fp32 mode: [Bmax][3H] x2, [Bmax][V]
  unsigned* err_ = nullptr;
  unsigned* err_pin_ = nullptr;   // pinned host word: the persistent launch's error-word read-back
  // the device error word is known to be zero (the last call ended on a persistent launch that read
  // it back as 0, nothing queued since): the next call skips its clearing memset
  bool err_clean_ = false;
  bool persist_ = true;
  bool inject_ = false;
  int global_n_ = 0;            // set_global_names
  int persist_max_ = 64;        // names per batch up to which the persistent launch is used
  int persist_ctl_max_ = 64;    // ... with sampling controls (GK_GEN_PERSIST_CTL_MAX)
  int persist_con_max_ = 0;     // ... with constraints (GK_GEN_PERSIST_CON_MAX): opt-in
  long persist_con_launches_ = 0;
  int persist_soft_max_ = 0;    // ... with soft controls (GK_GEN_PERSIST_SOFT_MAX): opt-in
  long persist_soft_launches_ = 0;
  // the constrained launch's device struct (plain allocation, made by the first such launch).  Written
  // in stream order before its launch; every persistent launch ends with its error-word read-back, so
  // no earlier launch can still read it when the next one's store is queued
  GenPersistCon* pcon_ = nullptr;
  int persist_max_bf16_ = 40;   // ... in the bf16 mode (it runs exact fp32, faster up to ~40 names:
                                // profiles/r5_gen_persist_vs_bf16_graph_final.jsonl)
  unsigned long long* persist_dbg_ = nullptr;
  float* pws_ = nullptr;        // persistent path: exchange buffers (two sets, by launch parity)
  int ppar_ = -1;               // the next persistent launch's set; -1: workspace not filled yet
  unsigned* psync_ = nullptr;   // persistent path: flags + done counter (self-cleaning, arena-zeroed)
  // scoring (second arena, committed by the first score() call)
  Arena sarena_;
  bool sready_ = false;
  std::map<int, std::unique_ptr<Graph>> sgraphs_;   // keyed by the padded batch Bp
  unsigned char* srows_ = nullptr;              // [Bmax][ML + 1] staged input rows
  int *sn_ = nullptr, *sids_ = nullptr, *stgt_ = nullptr, *sntok_ = nullptr;   // N word, [ML][Bmax] x2, [Bmax]
  float* sh0_ = nullptr;                        // [Bmax][H] zeros (arena-zeroed, never written): h before step 0
  std::vector<float*> shs_;                     // per layer [ML][Bp][H]: every step's h
  float *sgh_ = nullptr, *sgi_ = nullptr, *slogits_ = nullptr;   // step product slabs, [ML*Bp][3H], [ML*Bp][V] slabs
  float *stok_ = nullptr, *sname_ = nullptr;    // staged outputs [Bmax][ML], [Bmax]
  int *srank_ = nullptr, *sntok_out_ = nullptr;
  // scoring with controls (committed by the first controlled score() call)
  Arena scarena_;
  bool scready_ = false;
  std::map<std::pair<int, int>, std::unique_ptr<Graph>> scgraphs_;   // keyed by (Bp, constraint table lines or 0)
  float *scinv_ = nullptr, *sctopp_ = nullptr;  // [Bmax] each: the current batch's controls
  int *sctopk_ = nullptr, *scplen_ = nullptr;
  unsigned char* scprefix_ = nullptr;           // [Bmax][ML]
  unsigned* sctab_ = nullptr;                   // [kAllowRows][V / 32] the call's constraint table
  int* scidx_ = nullptr;                        // [Bmax][ML] the current batch's lines
  int* snkept_ = nullptr;                       // staged output [Bmax][ML]
  // sampling controls (third arena, committed by the first generate_ctl() call)
  Arena carena_;
  bool cready_ = false;
  // controlled per-char graphs, keyed by (active-name count, constraint table lines or 0)
  std::map<std::pair<int, int>, std::unique_ptr<Graph>> cgraphs_;
  float *cinv_ = nullptr, *ctopp_ = nullptr;    // [Bmax] each: the current batch's controls
  int *ctopk_ = nullptr, *cplen_ = nullptr;
  unsigned char* cprefix_ = nullptr;            // [Bmax][ML]
  unsigned* ctab_ = nullptr;                    // [kAllowRows][V / 32] the call's constraint table
  int* cidx_ = nullptr;                         // [Bmax][ML] the current batch's lines
  // beam search (fourth arena, committed by the first beam() call)
  Arena barena_;
  bool bready_ = false;
  std::map<std::tuple<int, int, int>, std::unique_ptr<Graph>> bgraphs_;   // keyed by (names, W, table lines or 0)
  std::vector<float*> bhA_, bhB_;               // per layer [Bmax][H]: a step's input / output states
  float *bgh_ = nullptr, *bgi_ = nullptr, *blogits_ = nullptr;   // product slabs, as gh_ / gi_ / logits_
  int* bids_ = nullptr;                         // [Bmax]
  float* bscore_[2] = {nullptr, nullptr};       // [Bmax] x2, by step parity, like the three below
  int* bstate_[2] = {nullptr, nullptr};
  int* blen_[2] = {nullptr, nullptr};
  unsigned char* brows_[2] = {nullptr, nullptr};   // [Bmax][ML + 1] x2
  int *bparent_ = nullptr, *bchr_ = nullptr, *bnext_ = nullptr, *bnb_ = nullptr;   // [Bmax] each
  int* bplen_ = nullptr;                        // [Bmax] the current batch's prefixes
  unsigned char* bprefix_ = nullptr;            // [Bmax][ML]
  unsigned* btab_ = nullptr;                    // [kAllowRows][V / 32] the call's constraint table
  int* bidx_ = nullptr;                         // [Bmax][ML] the current batch's lines
  // distinct names (plain allocations, made by the first distinct() call)
  float* dG_[2] = {nullptr, nullptr};           // [Bmax] x2 the slots' perturbed values, by step parity
  float* dinv_ = nullptr;                       // [Bmax] the current batch's 1 / T
  unsigned long long* dwords_ = nullptr;        // [2] the call's seed, the current batch's first global index
  std::map<std::tuple<int, int, int>, std::unique_ptr<Graph>> dgraphs_;    // keyed by (names, W, table lines or 0)
  std::map<std::tuple<int, int, int>, std::unique_ptr<Graph>> adgraphs_;   // keyed by (names, W, states)
  // conditional names (plain allocations, made by the first conditional() call)
  float* qw_[2] = {nullptr, nullptr};           // [Bmax] x2 the slots' log importance weights, by step parity
  float* qinv_ = nullptr;                       // [Bmax] the current batch's 1 / T
  int* qres_ = nullptr;                         // [Bmax] the current batch's resampling steps per name
  unsigned long long* qwords_ = nullptr;        // [4] the call's seed, the batch's first global index, the ESS threshold
  std::map<std::tuple<int, int, int>, std::unique_ptr<Graph>> qgraphs_;    // keyed by (names, W, table lines or 0)
  std::map<std::tuple<int, int, int>, std::unique_ptr<Graph>> aqgraphs_;   // keyed by (names, W, states)
  // automaton constraints (plain allocations, made by the first automaton call and grown on demand)
  unsigned* atab_ = nullptr;                    // [acap_][V / 32] the call's state sets
  unsigned short* anxt_ = nullptr;              // [acap_][V] the call's successor table
  int acap_ = 0;                                // states the two hold
  int *astart_ = nullptr, *astate_ = nullptr;   // [Bmax] the sampler's batch: start states, current states
  int* abstart_ = nullptr;                      // [Bmax] the beam batch's start states
  int* abstate_[2] = {nullptr, nullptr};        // [Bmax] x2 the beam rows' states, by step parity
  std::map<std::pair<int, int>, std::unique_ptr<Graph>> agraphs_;          // keyed by (n, states)
  std::map<std::tuple<int, int, int>, std::unique_ptr<Graph>> abgraphs_;   // keyed by (names, W, states)
  // soft controls (plain allocations, made by the first soft call): one set for generate_ctl(), one for score()
  struct SoftBufs {
    float* tab = nullptr;                       // [kSoftRows][V] the call's bias lines
    int* idx = nullptr;                         // [Bmax] the current batch's lines
    float *pres = nullptr, *freq = nullptr;     // [Bmax] each: its penalties
  };
  SoftBufs gsoft_, ssoft_;
  // soft recordings, keyed as cgraphs_ / agraphs_ / scgraphs_ with the bias table's line count added
  std::map<std::tuple<int, int, int>, std::unique_ptr<Graph>> csgraphs_;    // (n, constraint lines or 0, soft lines)
  std::map<std::tuple<int, int, int>, std::unique_ptr<Graph>> asgraphs_;    // (n, states, soft lines)
  std::map<std::tuple<int, int, int>, std::unique_ptr<Graph>> scsgraphs_;   // (Bp, constraint lines or 0, soft lines)
  static constexpr int kF32SlabRows = 2048;   // fp32 split-K slab capacity (rows x 3H)
};

}  // namespace gk

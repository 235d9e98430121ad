#include "generator.h"
#include "../runtime/trace.h"
#include "../runtime/blaslt.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace gk {

static int rup(int x, int m) { return (x + m - 1) / m * m; }

Generator::Generator(const GenDims& d, const float* params, const std::map<std::string, long>& offsets)
    : d_(d), params_(params), off_(offsets) {
  if (d_.V % 64 || d_.E % 64 || d_.H % 64)
    throw std::runtime_error("HIP generator needs vocab, embed and hidden to be multiples of 64");
  blaslt_init();   // before any graph capture (large prep GEMMs may go to the library)
  Bmax_ = rup(std::max(32, d_.max_batch), 64);
  const int V = d_.V, E = d_.E, H = d_.H, L = d_.L, B = Bmax_;
  std::vector<size_t> ohf, ohb, oWhh, oWih;
  // bf16x3: the bf16 weight / state copies hold split rows ([hi | lo | hi] / [hi | hi | lo], 3x wide)
  const size_t xw = d_.fp32 == 2 ? 3 : 1;
  for (int i = 0; i < 2 * L; ++i) { ohf.push_back(arena_.reserve((size_t)B * H * 4)); ohb.push_back(arena_.reserve((size_t)B * H * 2 * xw)); }
  for (int l = 0; l < L; ++l) {
    oWhh.push_back(arena_.reserve((size_t)3 * H * H * 2 * xw));
    oWih.push_back(arena_.reserve((size_t)3 * H * (l == 0 ? E : H) * 2 * xw));
  }
  size_t oEmb = arena_.reserve((size_t)V * E * 2), oWfc = arena_.reserve((size_t)V * H * 2 * xw);
  size_t oWfcF = arena_.reserve((size_t)V * H * 2);   // fragment-tiled copy for the 8-wave sampler
  size_t oP = arena_.reserve((size_t)V * 3 * H * 4), orf = arena_.reserve((size_t)B * d_.max_len * 4);
  size_t oids = arena_.reserve((size_t)B * 4), oal = arena_.reserve((size_t)B * 4);
  size_t oout = arena_.reserve((size_t)B * (d_.max_len + 1));
  size_t ogh = 0, ogi = 0, olg = 0, oerr = arena_.reserve(256), opws = 0, opsync = 0;
  // persistent small-batch path (every mode): exchange buffers, flags, and in bf16 mode an fp32
  // layer-0 table of its own (Ptab_ holds the bf16-product one there)
  opws = arena_.reserve((size_t)gen_persist_ws_floats(H, L, V, d_.max_len) * 4);
  opsync = arena_.reserve((size_t)gen_persist_sync_words(L) * 4);
  const size_t oP32 = d_.fp32 ? 0 : arena_.reserve((size_t)V * 3 * H * 4);
  if (d_.fp32) {
    // room for split-K slabs of small batches (f32_splits / split3_splits): kF32SlabRows rows
    const size_t rows = std::max<size_t>(B, kF32SlabRows);
    ogh = arena_.reserve(rows * 3 * H * 4);
    ogi = arena_.reserve(rows * 3 * H * 4);
    olg = arena_.reserve(rows * V * 4);
  }
  arena_.commit();
  err_ = arena_.get<unsigned>(oerr);
  pws_ = arena_.get<float>(opws); psync_ = arena_.get<unsigned>(opsync);
  if (d_.fp32) { gh_ = arena_.get<float>(ogh); gi_ = arena_.get<float>(ogi); logits_ = arena_.get<float>(olg); }
  for (int i = 0; i < 2 * L; ++i) { hf_.push_back(arena_.get<float>(ohf[i])); hb_.push_back(arena_.get<u16>(ohb[i])); }
  for (int l = 0; l < L; ++l) { Whh_.push_back(arena_.get<u16>(oWhh[l])); Wih_.push_back(arena_.get<u16>(oWih[l])); }
  Emb_ = arena_.get<u16>(oEmb); Wfc_ = arena_.get<u16>(oWfc); WfcF_ = arena_.get<u16>(oWfcF);
  Ptab_ = arena_.get<float>(oP);
  Ptab32_ = d_.fp32 ? Ptab_ : arena_.get<float>(oP32);
  rf_ = arena_.get<float>(orf); ids_ = arena_.get<int>(oids); alive_ = arena_.get<int>(oal);
  out_ = arena_.get<unsigned char>(oout);
  HIP_CHECK(hipStreamCreateWithFlags(&cap_, hipStreamNonBlocking));
  HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&err_pin_), 64, hipHostMallocDefault));
  const char* ng = std::getenv("GK_NO_GRAPH");
  if (ng && ng[0] == '1') use_graph_ = false;
  if (const char* sa = std::getenv("GK_STEP_ALGO")) step_algo_ = std::atoi(sa);   // 0 auto, 1 reg, 2 LDS
  const char* gp = std::getenv("GK_GEN_PERSIST");
  if (gp && gp[0] == '0') persist_ = false;
  if (const char* cm = std::getenv("GK_GEN_PERSIST_CTL_MAX")) persist_ctl_max_ = std::atoi(cm);
  if (const char* cm = std::getenv("GK_GEN_PERSIST_CON_MAX")) persist_con_max_ = std::atoi(cm);
  if (const char* cm = std::getenv("GK_GEN_PERSIST_SOFT_MAX")) persist_soft_max_ = std::atoi(cm);
}

bool Generator::uses_persist(int n) const {
  // bf16 mode: only where the persistent fp32 launch is faster than the bf16 per-char graph (up to
  // 40 names: 29.0 vs 33.2 us per char at 32, 33.7 vs 34.0 at 40, 34.8 vs 34.6 at 48 on the
  // reference model, launches included, profiles/r5_gen_persist_vs_bf16_graph.jsonl)
  // The bf16 mode's choice is PRECISION-visible (the persistent launch runs exact fp32), so it follows
  // the job's global name count when the caller gave one (set_global_names): a data-parallel call
  // then picks the same arithmetic on every world size.  fp32 mode: both paths are fp32.
  if (!d_.fp32 && std::max(n, global_n_) > persist_max_bf16_) return false;
  return persist_ && n <= persist_max_ && gen_persist_supported(d_.H, d_.L, d_.V, n, d_.max_len);
}

bool Generator::uses_persist_ctl(int n) const {
  // both paths are fp32-class here (generate_ctl raises in the bf16 mode), so the count alone decides
  return persist_ && d_.fp32 && n <= persist_ctl_max_ && gen_persist_ctl_supported(d_.H, d_.L, d_.V, n, d_.max_len);
}

bool Generator::uses_persist_con(int n, bool automaton) const {
  // opt-in (persist_con_max_ = 0 by default): docs/DESIGN.md §4e has the reason
  return uses_persist_ctl(n) && n <= persist_con_max_ &&
         gen_persist_con_supported(d_.H, d_.L, d_.V, n, d_.max_len, automaton ? kGenConAuto : kGenConMask);
}

bool Generator::uses_persist_soft(int n, int con_mode) const {
  // opt-in (persist_soft_max_ = 0 by default): docs/DESIGN.md §4h has the measurement
  if (con_mode != kGenConNone && con_mode != kGenConMask && con_mode != kGenConAuto) return false;
  if (!uses_persist_ctl(n) || n > persist_soft_max_) return false;
  if (con_mode != kGenConNone && !uses_persist_con(n, con_mode == kGenConAuto)) return false;
  return gen_persist_soft_supported(d_.H, d_.L, d_.V, n, d_.max_len, con_mode);
}

Generator::~Generator() {
  if (pcon_) (void)hipFree(pcon_);
  graphs_.clear();
  sgraphs_.clear();
  scgraphs_.clear();
  cgraphs_.clear();
  bgraphs_.clear();
  dgraphs_.clear();
  adgraphs_.clear();
  qgraphs_.clear();
  aqgraphs_.clear();
  agraphs_.clear();
  csgraphs_.clear();
  asgraphs_.clear();
  scsgraphs_.clear();
  for (SoftBufs* b : {&gsoft_, &ssoft_})
    for (void* p : {(void*)b->tab, (void*)b->idx, (void*)b->pres, (void*)b->freq})
      if (p) (void)hipFree(p);
  for (void* p : {(void*)atab_, (void*)anxt_, (void*)astart_, (void*)astate_, (void*)abstart_, (void*)abstate_[0],
                  (void*)abstate_[1]})
    if (p) (void)hipFree(p);
  for (void* p : {(void*)dG_[0], (void*)dG_[1], (void*)dinv_, (void*)dwords_})
    if (p) (void)hipFree(p);
  for (void* p : {(void*)qw_[0], (void*)qw_[1], (void*)qinv_, (void*)qres_, (void*)qwords_})
    if (p) (void)hipFree(p);
  if (cap_) (void)hipStreamDestroy(cap_);
  if (err_pin_) (void)hipHostFree(err_pin_);
}

void Generator::refresh_weights(hipStream_t s) {
  const int V = d_.V, E = d_.E, H = d_.H;
  if (d_.fp32) {   // fp32 layer-0 table P = Emb · W_ih0^T + b_ih0 from the master weights
    GemmF32Args g;
    g.A = P("embedding"); g.lda = E; g.B = P("weight_ih_l0"); g.ldb = E; g.C = Ptab_; g.ldc = 3 * H;
    g.bias = P("bias_ih_l0"); g.M = V; g.N = 3 * H; g.K = E;
    gemm_f32_nt(g, s);
    if (split3()) {   // the products' weight operands: [hi | lo | hi] rows
      for (int l = 0; l < d_.L; ++l) {
        const std::string k = std::to_string(l);
        split_bf16x3(P("weight_hh_l" + k), 3 * H, H, Whh_[l], s);
        if (l > 0) split_bf16x3(P("weight_ih_l" + k), 3 * H, H, Wih_[l], s);
      }
      split_bf16x3(P("fc.weight"), V, H, Wfc_, s);
    }
    HIP_LAUNCH_CHECK();
    return;
  }
  CastJobs j;
  j.add(P("embedding"), V, E, Emb_, nullptr);
  for (int l = 0; l < d_.L; ++l) {
    const std::string k = std::to_string(l);
    j.add(P("weight_hh_l" + k), 3 * H, H, Whh_[l], nullptr);
    j.add(P("weight_ih_l" + k), 3 * H, l == 0 ? E : H, Wih_[l], nullptr);
  }
  j.add(P("fc.weight"), V, H, Wfc_, nullptr, (V % 64 || H % 64) ? nullptr : WfcF_);
  cast_multi(j, s);
  {   // fp32 table for the persistent small-batch launch (exact fp32 there)
    GemmF32Args g;
    g.A = P("embedding"); g.lda = E; g.B = P("weight_ih_l0"); g.ldb = E; g.C = Ptab32_; g.ldc = 3 * H;
    g.bias = P("bias_ih_l0"); g.M = V; g.N = 3 * H; g.K = E;
    gemm_f32_nt(g, s);
  }
  GemmArgs g;   // layer-0 input projection table P = Emb · W_ih0^T + b_ih0  ([V][3H])
  g.A = Emb_; g.lda = E; g.B = Wih_[0]; g.ldb = E; g.C = Ptab_; g.ldc = 3 * H;
  g.bias = P("bias_ih_l0"); g.M = V; g.N = 3 * H; g.K = E;
  gemm_nt(g, s);
  HIP_LAUNCH_CHECK();
}

// Per-batch state reset as one kernel node.  Replays of a graph whose reset was five memset
// nodes (h, ids, alive, out) left stale and garbage ids in the padded rows of the fp32 path and
// made replays disagree (scripts/repro_gen_fp32.py with SYNC_FIRST=1: error word 16, replays not
// identical); a kernel node is ordered like every other node of the chain.
void Generator::reset_batch(int Bp, bool bf16, hipStream_t s) {
  // (round 3's memset-node diagnostics, scripts/gpu_graph_fault3.sh, profiles/r3_graph_replay.md)
  GenResetArgs r;
  r.L = d_.L; r.Bp = Bp; r.H = d_.H; r.ML = d_.max_len; r.sos = d_.sos;
  r.hb_cols = split3() ? 3 * d_.H : d_.H;
  for (int l = 0; l < d_.L; ++l) {
    r.hf[l] = hf_[2 * l];
    r.hb[l] = (bf16 || split3()) ? hb_[2 * l] : nullptr;
  }
  r.ids = ids_; r.alive = alive_; r.out = out_;
  gen_reset(r, s);
}

void Generator::record_steps(int n, hipStream_t s) {
  const int H = d_.H, L = d_.L, V = d_.V, ML = d_.max_len;
  const int Bp = rup(n, 32);
  // per-batch init (part of the graph): h = 0, input = SOS, alive = 1, output rows = NUL
  reset_batch(Bp, true, s);
  for (int st = 0; st < ML; ++st) {
    const int cur = st & 1, nxt = cur ^ 1;
    for (int l = 0; l < L; ++l) {
      const std::string k = std::to_string(l);
      FwdStepArgs a;
      a.hprev_bf = hb_[2 * l + cur]; a.hprev_f = hf_[2 * l + cur];
      a.Whh = Whh_[l]; a.bhh = P("bias_hh_l" + k);
      if (l == 0) { a.P = Ptab_; a.ids = ids_; }
      else { a.x_bf = hb_[2 * (l - 1) + nxt]; a.Wih = Wih_[l]; a.bih = P("bias_ih_l" + k); a.Kin = H; }
      a.h_f = hf_[2 * l + nxt]; a.h_bf = hb_[2 * l + nxt];
      a.Bp = Bp; a.H = H; a.algo = step_algo_;
      gru_fwd_step(a, s);
    }
    FcSampleArgs f;
    f.X = hb_[2 * (L - 1) + nxt]; f.W = Wfc_; f.Wf = WfcF_; f.b = P("fc.bias"); f.rf = rf_;
    f.ids = ids_; f.out = out_; f.alive = alive_; f.probs = (st == ML - 1) ? probe_ : nullptr;
    f.N = n; f.Bp = Bp; f.H = H; f.V = V; f.step = st; f.max_len = ML; f.eos = d_.eos;
    fc_sample(f, s);
  }
  HIP_LAUNCH_CHECK();
}

// fp32-faithful step: per layer gh = h W_hh^T + b_hh (and gi = x W_ih^T + b_ih above layer 0) as
// fp32 MFMA GEMMs on the master weights, the gates in IEEE fp32, then logits = h W_fc^T + b_fc and
// the fp32 softmax sampler -- the reference's per-char arithmetic (namegensf.cu:669-876) batched
// Split-K depth of a small-batch fp32 GEMM: enough 64 x 64 tiles x slabs to fill the chip
// (<= 512 workgroups), K-slices >= 64 deep, slabs within the buffer; 1 for big batches.
static int f32_splits(int M, int N, int K, int rows_cap) {
  const int tiles = (M / 64) * (N / 64);
  int sp = 1;
  while (sp < 32 && tiles * sp * 2 <= 512 && K % (sp * 2) == 0 && (K / (sp * 2)) % 16 == 0 &&
         K / (sp * 2) >= 64 && M * sp * 2 <= rows_cap)
    sp *= 2;
  return sp;
}

// bf16x3 split-K depth: unsplit when the LDS-staged kernels get a grid (>= 128 tiles of 128 x 128),
// else the one-shot small GEMM over the smallest K-slice count that gives ~256 workgroups (slices
// it supports: 2-4 or 8 k-blocks of 64, or whole multiples of 8 up to 32); slabs within rows_cap
static int split3_splits(int M, int N, int K3, int rows_cap) {
  if (M % 128 == 0 && N % 128 == 0 && (M / 128) * (N / 128) >= 128) return 1;
  const int tiles = (M / 64) * (N / 64);
  int last = 1;
  for (int sp = 2; sp <= 32; ++sp) {
    if (K3 % sp || (K3 / sp) % 64 || M * sp > rows_cap) continue;
    const int nkb = K3 / sp / 64;
    if (!(nkb == 2 || nkb == 3 || nkb == 4 || nkb == 8 || (nkb % 8 == 0 && nkb <= 32))) continue;
    last = sp;
    if (tiles * sp >= 256) return sp;
  }
  return last;
}

int Generator::product_f32(const float* A32, const u16* A3, const float* W32, const u16* W3, const float* bias, int M,
                           int N, float* C, hipStream_t s) {
  const int H = d_.H;
  const int cap = std::max(Bmax_, kF32SlabRows);
  if (!split3()) {
    GemmF32Args g;
    g.A = A32; g.lda = H; g.B = W32; g.ldb = H; g.C = C; g.ldc = N;
    g.bias = bias; g.M = M; g.N = N; g.K = H;
    g.splits = f32_splits(M, N, H, cap); g.slab = (long)M * N;
    gemm_f32_nt(g, s);
    return g.splits;
  }
  GemmArgs g;
  g.A = A3; g.lda = 3 * H; g.B = W3; g.ldb = 3 * H; g.C = C; g.ldc = N;
  g.M = M; g.N = N; g.K = 3 * H;
  g.splits = split3_splits(M, N, 3 * H, cap);
  if (g.splits == 1) {
    g.bias = bias;   // split: the consumer adds the bias after the slab sum
    // the 256 x 256 kernel from 3/4 of a wave of its tiles (4096 names x 3H: 192 tiles), where the
    // 128 x 128 kernel's 1.5 rounds of 512 slots leave as much idle
    if (M % 256 == 0 && N % 256 == 0 && (M / 256) * (N / 256) >= 192) g.algo = 5;
  } else {
    g.algo = 3;
  }
  gemm_nt(g, s);
  return g.splits;
}

void Generator::record_steps_f32(int n, hipStream_t s, bool ctl, int allow_rows, bool automaton, int soft_rows) {
  const int H = d_.H, L = d_.L, V = d_.V, ML = d_.max_len;
  const int Bp = rup(n, 64);
  const bool x3 = split3();
  reset_batch(Bp, false, s);
  if (automaton) automaton_reset(astate_, astart_, n, n, s);   // every name back to its start state
  for (int st = 0; st < ML; ++st) {
    const int cur = st & 1, nxt = cur ^ 1;
    for (int l = 0; l < L; ++l) {
      const std::string k = std::to_string(l);
      const float* bh = P("bias_hh_l" + k);
      const int sh = product_f32(hf_[2 * l + cur], hb_[2 * l + cur], P("weight_hh_l" + k), Whh_[l], bh, Bp, 3 * H, gh_, s);
      GruGatesF32Args a;
      if (l == 0) {
        a.P = Ptab_; a.ids = ids_;
      } else {
        const float* bi = P("bias_ih_l" + k);
        const int si = product_f32(hf_[2 * (l - 1) + nxt], hb_[2 * (l - 1) + nxt], P("weight_ih_l" + k), Wih_[l], bi,
                                   Bp, 3 * H, gi_, s);
        a.Gi = gi_; a.gi_splits = si; a.gi_slab = (long)Bp * 3 * H;
        if (x3 && si > 1) a.bgi = bi;
      }
      a.Gh = gh_; a.gh_splits = sh; a.gh_slab = (long)Bp * 3 * H; a.hprev = hf_[2 * l + cur]; a.hout = hf_[2 * l + nxt];
      if (x3 && sh > 1) a.bgh = bh;
      if (x3) a.hsplit = hb_[2 * l + nxt];
      a.Bp = Bp; a.H = H; a.V = V; a.err = err_;
      gru_gates_f32(a, s);
    }
    const float* bf = P("fc.bias");
    const int sf = product_f32(hf_[2 * (L - 1) + nxt], hb_[2 * (L - 1) + nxt], P("fc.weight"), Wfc_, bf, Bp, V, logits_, s);
    SampleF32Args q;
    q.logits = logits_; q.splits = sf; q.slab = (long)Bp * V; q.rf = rf_; q.ids = ids_; q.out = out_; q.alive = alive_;
    if (x3 && sf > 1) q.bias = bf;
    q.probs = (st == ML - 1) ? probe_ : nullptr;
    q.N = n; q.V = V; q.step = st; q.max_len = ML; q.eos = d_.eos;
    if (ctl) {
      SampleCtlArgs c;
      c.s = q; c.inv_temp = cinv_; c.top_k = ctopk_; c.top_p = ctopp_; c.plen = cplen_; c.prefix = cprefix_;
      c.row0 = 0; c.err = err_;
      if (automaton) { c.allow_tab = atab_; c.allow_next = anxt_; c.allow_state = astate_; c.allow_rows = allow_rows; }
      else if (allow_rows > 0) { c.allow_tab = ctab_; c.allow_idx = cidx_; c.allow_rows = allow_rows; }
      if (soft_rows > 0) {
        c.soft_tab = gsoft_.tab; c.soft_idx = gsoft_.idx; c.soft_rows = soft_rows;
        c.soft_pres = gsoft_.pres; c.soft_freq = gsoft_.freq;
      }
      sample_ctl_f32(c, s);
    } else {
      sample_f32(q, s);
    }
  }
  HIP_LAUNCH_CHECK();
}

bool Generator::persist_launch(const float* rf, int n, const Ctl* c, unsigned char* out, bool last_batch, hipStream_t s) {
  const int ML = d_.max_len;
  GenPersistArgs a;
  for (int l = 0; l < d_.L; ++l) {
    const std::string k = std::to_string(l);
    a.Whh[l] = P("weight_hh_l" + k); a.bhh[l] = P("bias_hh_l" + k);
    if (l > 0) { a.Wih[l] = P("weight_ih_l" + k); a.bih[l] = P("bias_ih_l" + k); }
  }
  a.Wfc = P("fc.weight"); a.bfc = P("fc.bias"); a.P = Ptab32_; a.probs = probe_;
  a.rf = rf; a.out = out;
  if (c) { a.inv_temp = c->inv_temp; a.top_k = c->top_k; a.top_p = c->top_p; a.plen = c->plen; a.prefix = c->prefix; }
  if (c && (c->allow_tab || c->soft_tab)) {   // constrained or soft: the device struct, stored in stream order ahead of the launch
    GenPersistCon h;
    h.allow_tab = c->allow_tab; h.allow_idx = c->allow_idx; h.allow_next = c->allow_next; h.allow_start = c->allow_start;
    h.allow_rows = c->allow_rows;
    h.soft_tab = c->soft_tab; h.soft_idx = c->soft_idx; h.soft_rows = c->soft_rows;
    h.soft_pres = c->soft_pres; h.soft_freq = c->soft_freq;
    a.con_mode = gen_persist_con_mode(h);
    a.soft = gen_persist_soft_check(h) ? 1 : 0;
    // (the first such launch allocates; the previous persistent launch has been waited for -- its error
    // read-back below -- so nothing on any stream still reads the struct)
    if (!pcon_) HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&pcon_), sizeof(GenPersistCon)));
    gen_persist_con_store(pcon_, h, s);
    a.con = pcon_;
  }
  a.ws = pws_; a.sync = psync_; a.err = err_; a.dbg = persist_dbg_;
  if (ppar_ < 0) {   // first launch: both sets' tagged slots -> kEmpty; later launches refill in-kernel
    gen_persist_fill_ws(pws_, d_.H, d_.L, d_.V, ML, s);
    ppar_ = 0;
  }
  a.par = ppar_;
  ppar_ ^= 1;
  a.N = n; a.H = d_.H; a.L = d_.L; a.V = d_.V; a.ML = ML; a.sos = d_.sos; a.eos = d_.eos;
  if (inject_) {   // test hook: OR the spin-limit bit into the word (earlier batches' bits stay)
    unsigned cur = 0;
    HIP_CHECK(hipMemcpyAsync(&cur, err_, 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    cur |= 32u;
    HIP_CHECK(hipMemcpyAsync(err_, &cur, 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    inject_ = false;
  }
  gen_persist_f32(a, s);
  if (a.soft) ++persist_soft_launches_;
  else if (a.con) ++persist_con_launches_;
  // small batch, latency-bound launch: check its error word now.  A spin timeout means the
  // workgroups were not co-resident (something else held CUs): the batch's output is garbage,
  // so say so, stop using the persistent path and regenerate the batch on the per-char graph.
  // (pinned host word: 138 vs 146-150 us per 1-name call against a pageable one; skipping the
  // next call's memset after a clean call another ~2 us: profiles/r5_gen_err_readback_ab.txt)
  HIP_CHECK(hipMemcpyAsync(err_pin_, err_, 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  const unsigned e = *reinterpret_cast<volatile unsigned*>(err_pin_);
  if (e == 0 && last_batch) err_clean_ = true;   // the call ends here, word still 0
  if (!(e & 32u)) return true;
  std::fprintf(stderr, "[generator] persistent launch hit its spin limit (error word %u): "
                       "disabling it, regenerating %d names on the per-char graph\n", e, n);
  persist_ = false;
  const unsigned keep = e & ~32u;   // the other bits stay (earlier batches' errors)
  HIP_CHECK(hipMemcpy(err_, &keep, 4, hipMemcpyHostToDevice));
  return false;
}

void Generator::generate(const float* rf, int N, unsigned char* out, hipStream_t s) {
  GK_TRACE("gk.generate");
  const int ML = d_.max_len;
  // the error word covers the whole call: every batch ORs its bits in, read_error() reports them all
  // (a persistent launch's spin-limit bit 32 is taken out again below once its batch is regenerated)
  if (!err_clean_) HIP_CHECK(hipMemsetAsync(err_, 0, 16, s));
  err_clean_ = false;
  for (int start = 0; start < N; start += Bmax_) {
    const int n = std::min(Bmax_, N - start);
    // one launch for the whole batch, no graph needed: the caller's uniforms and output rows directly
    // (no staging copies: two fewer stream operations per call on the latency-bound small-batch path)
    if (uses_persist(n) &&
        persist_launch(rf + (size_t)start * ML, n, nullptr, out + (size_t)start * (ML + 1), start + n >= N, s))
      continue;   // rows already in `out`
    HIP_CHECK(hipMemcpyAsync(rf_, rf + (size_t)start * ML, (size_t)n * ML * 4, hipMemcpyDeviceToDevice, s));
    if (use_graph_) {
      auto& g = graphs_[n];
      if (!g) {
        g.reset(new Graph());
        g->begin(cap_);
        if (d_.fp32) record_steps_f32(n, cap_); else record_steps(n, cap_);
        g->end(cap_);
      }
      g->launch(s);
    } else {
      if (d_.fp32) record_steps_f32(n, s); else record_steps(n, s);
    }
    HIP_CHECK(hipMemcpyAsync(out + (size_t)start * (ML + 1), out_, (size_t)n * (ML + 1), hipMemcpyDeviceToDevice, s));
  }
}

// ---------------------------------------------------------------------- controlled sampling
// The current batch's controls, sized for Bmax_ names: a generator that never samples with controls
// never allocates them.
void Generator::ctl_alloc() {
  if (cready_) return;
  const size_t B = Bmax_, ML = d_.max_len;
  const size_t oi = carena_.reserve(B * 4), ok = carena_.reserve(B * 4), op = carena_.reserve(B * 4);
  const size_t ol = carena_.reserve(B * 4), opre = carena_.reserve(B * ML);
  const size_t otab = carena_.reserve((size_t)kAllowRows * (d_.V / 32) * 4), oidx = carena_.reserve(B * ML * 4);
  carena_.commit();
  cinv_ = carena_.get<float>(oi); ctopk_ = carena_.get<int>(ok); ctopp_ = carena_.get<float>(op);
  cplen_ = carena_.get<int>(ol); cprefix_ = carena_.get<unsigned char>(opre);
  ctab_ = carena_.get<unsigned>(otab); cidx_ = carena_.get<int>(oidx);
  cready_ = true;
}

// The soft-control buffers of generate_ctl() and score(): a generator that never gets a soft call never
// allocates them, and they are in no arena, so no workspace size changes.
void Generator::soft_alloc() {
  if (gsoft_.tab) return;
  const size_t B = Bmax_, V = d_.V;
  for (SoftBufs* b : {&gsoft_, &ssoft_}) {
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&b->tab), (size_t)kSoftRows * V * 4));
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&b->idx), B * 4));
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&b->pres), B * 4));
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&b->freq), B * 4));
    HIP_CHECK(hipMemset(b->tab, 0, (size_t)kSoftRows * V * 4));
    HIP_CHECK(hipMemset(b->idx, 0, B * 4));
    HIP_CHECK(hipMemset(b->pres, 0, B * 4));
    HIP_CHECK(hipMemset(b->freq, 0, B * 4));
  }
}

void Generator::automaton_stage(const unsigned* tab, const unsigned short* next, int states, hipStream_t s) {
  const size_t B = Bmax_, V = d_.V;
  if (!astate_) {
    for (int** p : {&astart_, &astate_, &abstart_, &abstate_[0], &abstate_[1]}) {
      HIP_CHECK(hipMalloc(reinterpret_cast<void**>(p), B * 4));
      HIP_CHECK(hipMemset(*p, 0, B * 4));
    }
  }
  if (states > acap_) {   // grow: the recordings hold the old addresses
    HIP_CHECK(hipDeviceSynchronize());
    agraphs_.clear();
    asgraphs_.clear();
    abgraphs_.clear();
    adgraphs_.clear();
    aqgraphs_.clear();
    if (atab_) HIP_CHECK(hipFree(atab_));
    if (anxt_) HIP_CHECK(hipFree(anxt_));
    atab_ = nullptr; anxt_ = nullptr; acap_ = 0;
    int cap = 1024;
    while (cap < states) cap *= 2;
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&atab_), (size_t)cap * (V / 32) * 4));
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&anxt_), (size_t)cap * V * 2));
    acap_ = cap;
  }
  HIP_CHECK(hipMemcpyAsync(atab_, tab, (size_t)states * (V / 32) * 4, hipMemcpyDeviceToDevice, s));
  HIP_CHECK(hipMemcpyAsync(anxt_, next, (size_t)states * V * 2, hipMemcpyDeviceToDevice, s));
}

void Generator::generate_ctl(const float* rf, int N, const Ctl& c, unsigned char* out, hipStream_t s) {
  GK_TRACE("gk.generate_ctl");
  if (!d_.fp32) throw std::runtime_error("Generator::generate_ctl: sampling controls need precision fp32 or bf16x3");
  if (!c.inv_temp || !c.top_k || !c.top_p || !c.plen || !c.prefix)
    throw std::runtime_error("Generator::generate_ctl: every control array is required");
  const bool aut = c.allow_next != nullptr || c.allow_start != nullptr;
  if (aut && (!c.allow_next || !c.allow_start || !c.allow_tab || c.allow_idx || c.allow_rows < 1 ||
              c.allow_rows > kAutoStates || (d_.V != 256 && d_.V != 512)))
    throw std::runtime_error("Generator::generate_ctl: an automaton needs allow_tab, allow_next and allow_start, no "
                             "allow_idx, 1 <= allow_rows <= 65535 and a vocabulary of 256 or 512");
  const bool masked = c.allow_tab != nullptr;
  if (!aut && (masked != (c.allow_idx != nullptr) || (masked && (c.allow_rows < 1 || c.allow_rows > kAllowRows))))
    throw std::runtime_error("Generator::generate_ctl: constraints need allow_tab, allow_idx and 1 <= allow_rows <= 1024");
  const bool soft = c.soft_tab != nullptr;
  if (soft != (c.soft_idx != nullptr) || soft != (c.soft_pres != nullptr) || soft != (c.soft_freq != nullptr) ||
      (soft && (c.soft_rows < 1 || c.soft_rows > kSoftRows)))
    throw std::runtime_error("Generator::generate_ctl: soft controls need soft_tab, soft_idx, soft_pres, soft_freq and "
                             "1 <= soft_rows <= 256");
  if (N <= 0) return;
  const int ML = d_.max_len;
  const int sr = soft ? c.soft_rows : 0;
  const int cmode = aut ? kGenConAuto : masked ? kGenConMask : kGenConNone;
  // a batch that takes the constrained or the soft persistent launch reads the caller's tables in place: a
  // call made of such batches alone stages nothing and allocates nothing
  auto persist_batch = [&](int n) {
    if (soft) return uses_persist_soft(n, cmode);   // (opt-in: docs/DESIGN.md §4h)
    return masked ? uses_persist_con(n, aut) : uses_persist_ctl(n);   // (a constrained batch where the caller opted in: §4e)
  };
  bool graph_batch = false, soft_graph_batch = false;
  for (int start = 0; start < N; start += Bmax_) {
    const bool pb = persist_batch(std::min(Bmax_, N - start));
    if (soft ? !pb : !(masked && pb)) graph_batch = true;
    if (soft && !pb) soft_graph_batch = true;
  }
  // first soft call with a batch for the graph: allocates before the error word is cleared and anything is captured
  if (soft_graph_batch) soft_alloc();
  bool aut_staged = false;
  if (aut && graph_batch) {   // before the error word is cleared: growing the buffers synchronises
    ctl_alloc();
    automaton_stage(c.allow_tab, c.allow_next, c.allow_rows, s);
    aut_staged = true;
  }
  if (!err_clean_) HIP_CHECK(hipMemsetAsync(err_, 0, 16, s));   // the error word covers the whole call, as in generate()
  err_clean_ = false;
  bool tab_staged = false;
  bool soft_staged = false;
  if (soft_graph_batch) {   // the bias lines once per call
    HIP_CHECK(hipMemcpyAsync(gsoft_.tab, c.soft_tab, (size_t)sr * d_.V * 4, hipMemcpyDeviceToDevice, s));
    soft_staged = true;
  }
  for (int start = 0; start < N; start += Bmax_) {
    const int n = std::min(Bmax_, N - start);
    if (persist_batch(n)) {   // one launch on the caller's arrays at this batch's rows
      Ctl b;
      b.inv_temp = c.inv_temp + start; b.top_k = c.top_k + start; b.top_p = c.top_p + start; b.plen = c.plen + start;
      b.prefix = c.prefix + (size_t)start * ML;
      if (masked) {   // table and next by pointer; idx and start at the batch's rows
        b.allow_tab = c.allow_tab; b.allow_rows = c.allow_rows; b.allow_next = c.allow_next;
        if (aut) b.allow_start = c.allow_start + start;
        else b.allow_idx = c.allow_idx + (size_t)start * ML;
      }
      if (soft) {   // the bias table by pointer; lines and penalties at the batch's rows
        b.soft_tab = c.soft_tab; b.soft_rows = sr;
        b.soft_idx = c.soft_idx + start; b.soft_pres = c.soft_pres + start; b.soft_freq = c.soft_freq + start;
      }
      if (persist_launch(rf + (size_t)start * ML, n, &b, out + (size_t)start * (ML + 1), start + n >= N, s)) continue;
    }
    ctl_alloc();   // first batch on this path: allocates (and synchronises) before anything is captured
    if (aut && !aut_staged) {   // (a constrained persistent launch hit its spin limit: the graph after all)
      automaton_stage(c.allow_tab, c.allow_next, c.allow_rows, s);
      aut_staged = true;
    }
    if (soft && !soft_staged) {   // (a soft persistent launch hit its spin limit: the soft graph after all)
      soft_alloc();
      HIP_CHECK(hipMemcpyAsync(gsoft_.tab, c.soft_tab, (size_t)sr * d_.V * 4, hipMemcpyDeviceToDevice, s));
      soft_staged = true;
    }
    HIP_CHECK(hipMemcpyAsync(rf_, rf + (size_t)start * ML, (size_t)n * ML * 4, hipMemcpyDeviceToDevice, s));
    // this batch's slice of every control array: the graph reads rows 0 .. n - 1 of the buffers
    HIP_CHECK(hipMemcpyAsync(cinv_, c.inv_temp + start, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(ctopk_, c.top_k + start, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(ctopp_, c.top_p + start, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(cplen_, c.plen + start, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(cprefix_, c.prefix + (size_t)start * ML, (size_t)n * ML, hipMemcpyDeviceToDevice, s));
    const int ar = masked ? c.allow_rows : 0;
    if (soft) {   // this batch's lines and penalties
      HIP_CHECK(hipMemcpyAsync(gsoft_.idx, c.soft_idx + start, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
      HIP_CHECK(hipMemcpyAsync(gsoft_.pres, c.soft_pres + start, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
      HIP_CHECK(hipMemcpyAsync(gsoft_.freq, c.soft_freq + start, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    }
    if (aut) {   // the tables are staged: this batch's start states, then its graph
      HIP_CHECK(hipMemcpyAsync(astart_, c.allow_start + start, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
      if (use_graph_ && soft) {   // a soft recording, in the map of its own (the same cap)
        if (asgraphs_.size() >= kAutoGraphs && !asgraphs_.count(std::make_tuple(n, ar, sr))) {
          HIP_CHECK(hipStreamSynchronize(s));
          asgraphs_.clear();
        }
        auto& g = asgraphs_[std::make_tuple(n, ar, sr)];
        if (!g) {
          g.reset(new Graph());
          g->begin(cap_);
          record_steps_f32(n, cap_, true, ar, true, sr);
          g->end(cap_);
        }
        g->launch(s);
      } else if (use_graph_) {
        // every state count has a recording of its own, and a caller that grows an exclusion list call by
        // call never comes back to one: keep the latest few
        if (agraphs_.size() >= kAutoGraphs && !agraphs_.count(std::make_pair(n, ar))) {
          HIP_CHECK(hipStreamSynchronize(s));
          agraphs_.clear();
        }
        auto& g = agraphs_[std::make_pair(n, ar)];
        if (!g) {
          g.reset(new Graph());
          g->begin(cap_);
          record_steps_f32(n, cap_, true, ar, true);
          g->end(cap_);
        }
        g->launch(s);
      } else {
        record_steps_f32(n, s, true, ar, true, sr);
      }
      HIP_CHECK(hipMemcpyAsync(out + (size_t)start * (ML + 1), out_, (size_t)n * (ML + 1), hipMemcpyDeviceToDevice, s));
      continue;
    }
    if (masked) {   // the table once per call, this batch's lines
      if (!tab_staged) {
        HIP_CHECK(hipMemcpyAsync(ctab_, c.allow_tab, (size_t)ar * (d_.V / 32) * 4, hipMemcpyDeviceToDevice, s));
        tab_staged = true;
      }
      HIP_CHECK(hipMemcpyAsync(cidx_, c.allow_idx + (size_t)start * ML, (size_t)n * ML * 4, hipMemcpyDeviceToDevice, s));
    }
    if (use_graph_ && soft) {   // a soft recording: the bias table's line count is baked in as well
      auto& g = csgraphs_[std::make_tuple(n, ar, sr)];
      if (!g) {
        g.reset(new Graph());
        g->begin(cap_);
        record_steps_f32(n, cap_, true, ar, false, sr);
        g->end(cap_);
      }
      g->launch(s);
    } else if (use_graph_) {
      // the recording bakes the table's line count in (the sampler checks every entry against it),
      // so it is part of the key; 0 = the unconstrained graph, the only one an unconstrained call sees
      auto& g = cgraphs_[std::make_pair(n, ar)];
      if (!g) {
        g.reset(new Graph());
        g->begin(cap_);
        record_steps_f32(n, cap_, true, ar);
        g->end(cap_);
      }
      g->launch(s);
    } else {
      record_steps_f32(n, s, true, ar, false, sr);
    }
    HIP_CHECK(hipMemcpyAsync(out + (size_t)start * (ML + 1), out_, (size_t)n * (ML + 1), hipMemcpyDeviceToDevice, s));
  }
}

// ---------------------------------------------------------------------------------- scoring
// Buffers of the teacher-forced schedule, sized for Bmax_ names: a generator that never scores
// never allocates them.
void Generator::score_alloc() {
  if (sready_) return;
  const size_t V = d_.V, H = d_.H, ML = d_.max_len, B = Bmax_;
  const size_t slab_rows = std::max<size_t>(B, kF32SlabRows), all_rows = std::max<size_t>(ML * B, kF32SlabRows);
  const size_t orows = sarena_.reserve(B * (ML + 1)), on = sarena_.reserve(256);
  const size_t oids = sarena_.reserve(ML * B * 4), otgt = sarena_.reserve(ML * B * 4), ont = sarena_.reserve(B * 4);
  const size_t oh0 = sarena_.reserve(B * H * 4);
  std::vector<size_t> ohs;
  for (int l = 0; l < d_.L; ++l) ohs.push_back(sarena_.reserve(ML * B * H * 4));
  const size_t ogh = sarena_.reserve(slab_rows * 3 * H * 4);
  const size_t ogi = d_.L > 1 ? sarena_.reserve(ML * B * 3 * H * 4) : 0;
  const size_t olg = sarena_.reserve(all_rows * V * 4);
  const size_t otok = sarena_.reserve(B * ML * 4), ornk = sarena_.reserve(B * ML * 4);
  const size_t onm = sarena_.reserve(B * 4), onto = sarena_.reserve(B * 4);
  sarena_.commit();
  srows_ = sarena_.get<unsigned char>(orows); sn_ = sarena_.get<int>(on);
  sids_ = sarena_.get<int>(oids); stgt_ = sarena_.get<int>(otgt); sntok_ = sarena_.get<int>(ont);
  sh0_ = sarena_.get<float>(oh0);
  for (int l = 0; l < d_.L; ++l) shs_.push_back(sarena_.get<float>(ohs[l]));
  sgh_ = sarena_.get<float>(ogh); sgi_ = d_.L > 1 ? sarena_.get<float>(ogi) : nullptr;
  slogits_ = sarena_.get<float>(olg);
  stok_ = sarena_.get<float>(otok); srank_ = sarena_.get<int>(ornk);
  sname_ = sarena_.get<float>(onm); sntok_out_ = sarena_.get<int>(onto);
  sready_ = true;
}

// The current batch's controls, its constraint lines, the call's table and the staged n_kept, sized for
// Bmax_ names: a generator that never scores with controls never allocates them.
void Generator::score_ctl_alloc() {
  if (scready_) return;
  const size_t B = Bmax_, ML = d_.max_len;
  const size_t oi = scarena_.reserve(B * 4), ok = scarena_.reserve(B * 4), op = scarena_.reserve(B * 4);
  const size_t ol = scarena_.reserve(B * 4), opre = scarena_.reserve(B * ML);
  const size_t otab = scarena_.reserve((size_t)kAllowRows * (d_.V / 32) * 4), oidx = scarena_.reserve(B * ML * 4);
  const size_t onk = scarena_.reserve(B * ML * 4);
  scarena_.commit();
  scinv_ = scarena_.get<float>(oi); sctopk_ = scarena_.get<int>(ok); sctopp_ = scarena_.get<float>(op);
  scplen_ = scarena_.get<int>(ol); scprefix_ = scarena_.get<unsigned char>(opre);
  sctab_ = scarena_.get<unsigned>(otab); scidx_ = scarena_.get<int>(oidx); snkept_ = scarena_.get<int>(onk);
  scready_ = true;
}

// The schedule for a padded batch of Bp rows (the name count is read from sn_ by score_prep, so one
// recording serves every count that pads to Bp): 2 L ML + L + 2 launches, a single chain.
void Generator::record_score(int Bp, hipStream_t s, bool ctl, int allow_rows, int soft_rows) {
  const int H = d_.H, L = d_.L, V = d_.V, ML = d_.max_len;
  const int cap = std::max(Bmax_, kF32SlabRows);
  ScorePrepArgs p;
  p.rows = srows_; p.n_dev = sn_; p.ids = sids_; p.tgt = stgt_; p.ntok = sntok_; p.err = err_;
  p.Bp = Bp; p.ML = ML; p.V = V; p.sos = d_.sos; p.eos = d_.eos;
  score_prep(p, s);
  const long step = (long)Bp * H;   // one step's h rows
  for (int l = 0; l < L; ++l) {
    const std::string k = std::to_string(l);
    if (l > 0) {   // the layer's input projection for every step at once: Gi = h_below W_ih^T + b_ih
      GemmF32Args g;
      g.A = shs_[l - 1]; g.lda = H; g.B = P("weight_ih_l" + k); g.ldb = H; g.C = sgi_; g.ldc = 3 * H;
      g.bias = P("bias_ih_l" + k); g.M = ML * Bp; g.N = 3 * H; g.K = H;
      gemm_f32_nt(g, s);
    }
    for (int st = 0; st < ML; ++st) {
      const float* hprev = st == 0 ? sh0_ : shs_[l] + (st - 1) * step;
      GemmF32Args g;   // gh = h W_hh^T + b_hh (bias in slab 0; the gates sum the slabs in order)
      g.A = hprev; g.lda = H; g.B = P("weight_hh_l" + k); g.ldb = H; g.C = sgh_; g.ldc = 3 * H;
      g.bias = P("bias_hh_l" + k); g.M = Bp; g.N = 3 * H; g.K = H;
      g.splits = f32_splits(Bp, 3 * H, H, cap); g.slab = (long)Bp * 3 * H;
      gemm_f32_nt(g, s);
      GruGatesF32Args a;
      if (l == 0) { a.P = Ptab32_; a.ids = sids_ + (long)st * Bp; }
      else a.Gi = sgi_ + (long)st * Bp * 3 * H;
      a.Gh = sgh_; a.gh_splits = g.splits; a.gh_slab = g.slab;
      a.hprev = hprev; a.hout = shs_[l] + st * step;
      a.Bp = Bp; a.H = H; a.V = V; a.err = err_;
      gru_gates_f32(a, s);
    }
  }
  GemmF32Args g;   // every step's logits in one product
  g.A = shs_[L - 1]; g.lda = H; g.B = P("fc.weight"); g.ldb = H; g.C = slogits_; g.ldc = V;
  g.bias = P("fc.bias"); g.M = ML * Bp; g.N = V; g.K = H;
  g.splits = f32_splits(ML * Bp, V, H, std::max(ML * Bmax_, kF32SlabRows)); g.slab = (long)ML * Bp * V;
  gemm_f32_nt(g, s);
  ScoreLogprobArgs q;
  q.logits = slogits_; q.splits = g.splits; q.slab = g.slab; q.tgt = stgt_; q.ntok = sntok_;
  q.tok_logp = stok_; q.rank = srank_; q.name_logp = sname_; q.ntok_out = sntok_out_;
  q.Bp = Bp; q.V = V; q.ML = ML;
  if (ctl) {   // the controls of rows 0 .. Bp - 1 of the staging buffers (pad rows read none)
    ScoreCtlArgs c;
    c.s = q; c.inv_temp = scinv_; c.top_k = sctopk_; c.top_p = sctopp_; c.plen = scplen_; c.prefix = scprefix_;
    c.row0 = 0; c.err = err_; c.n_kept = snkept_;
    if (allow_rows > 0) { c.allow_tab = sctab_; c.allow_idx = scidx_; c.allow_rows = allow_rows; }
    if (soft_rows > 0) {
      c.soft_tab = ssoft_.tab; c.soft_idx = ssoft_.idx; c.soft_rows = soft_rows;
      c.soft_pres = ssoft_.pres; c.soft_freq = ssoft_.freq;
    }
    score_ctl_logprob_f32(c, s);
  } else {
    score_logprob_f32(q, s);
  }
  HIP_LAUNCH_CHECK();
}

void Generator::score(const unsigned char* rows, int N, float* tok_logp, int* rank, float* name_logp, int* n_tok,
                      hipStream_t s, const Ctl* c, int* n_kept) {
  GK_TRACE("gk.score");
  const bool masked = c && c->allow_tab != nullptr;
  const bool soft = c && c->soft_tab != nullptr;
  if (c) {
    if (soft != (c->soft_idx != nullptr) || soft != (c->soft_pres != nullptr) || soft != (c->soft_freq != nullptr) ||
        (soft && (c->soft_rows < 1 || c->soft_rows > kSoftRows)))
      throw std::runtime_error("Generator::score: soft controls need soft_tab, soft_idx, soft_pres, soft_freq and "
                               "1 <= soft_rows <= 256");
    if (!c->inv_temp || !c->top_k || !c->top_p || !c->plen || !c->prefix || !n_kept)
      throw std::runtime_error("Generator::score: a controlled score needs every control array and n_kept");
    if (masked != (c->allow_idx != nullptr) || (masked && (c->allow_rows < 1 || c->allow_rows > kAllowRows)))
      throw std::runtime_error("Generator::score: constraints need allow_tab, allow_idx and 1 <= allow_rows <= 1024");
    if (masked && 32 % (d_.V / 64))
      throw std::runtime_error("Generator::score: constraints need vocab / 64 in {1, 2, 4, 8}");
  }
  if (N <= 0) return;
  const int ML = d_.max_len;
  if (ML > 64 || d_.V > 512) throw std::runtime_error("Generator::score needs max_len <= 64 and vocab <= 512");
  score_alloc();   // first call: allocates (and synchronises) before anything is captured
  if (c) score_ctl_alloc();   // ... the first controlled one its control buffers
  if (soft) soft_alloc();     // ... the first soft one the soft-control buffers
  const int sr = soft ? c->soft_rows : 0;
  HIP_CHECK(hipMemsetAsync(err_, 0, 16, s));   // the error word covers the whole call, as in generate()
  err_clean_ = false;
  const int ar = masked ? c->allow_rows : 0;
  if (masked)   // the table once per call
    HIP_CHECK(hipMemcpyAsync(sctab_, c->allow_tab, (size_t)ar * (d_.V / 32) * 4, hipMemcpyDeviceToDevice, s));
  if (soft)     // the bias lines once per call
    HIP_CHECK(hipMemcpyAsync(ssoft_.tab, c->soft_tab, (size_t)sr * d_.V * 4, hipMemcpyDeviceToDevice, s));
  for (int start = 0; start < N; start += Bmax_) {
    const int n = std::min(Bmax_, N - start);
    const int Bp = rup(n, 64);
    score_set_count(sn_, n, s);
    HIP_CHECK(hipMemcpyAsync(srows_, rows + (size_t)start * (ML + 1), (size_t)n * (ML + 1), hipMemcpyDeviceToDevice, s));
    if (c) {   // this batch's slice of every control array: the recording reads rows 0 .. n - 1 of the buffers
      HIP_CHECK(hipMemcpyAsync(scinv_, c->inv_temp + start, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
      HIP_CHECK(hipMemcpyAsync(sctopk_, c->top_k + start, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
      HIP_CHECK(hipMemcpyAsync(sctopp_, c->top_p + start, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
      HIP_CHECK(hipMemcpyAsync(scplen_, c->plen + start, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
      HIP_CHECK(hipMemcpyAsync(scprefix_, c->prefix + (size_t)start * ML, (size_t)n * ML, hipMemcpyDeviceToDevice, s));
      if (masked)
        HIP_CHECK(hipMemcpyAsync(scidx_, c->allow_idx + (size_t)start * ML, (size_t)n * ML * 4, hipMemcpyDeviceToDevice, s));
      if (soft) {
        HIP_CHECK(hipMemcpyAsync(ssoft_.idx, c->soft_idx + start, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
        HIP_CHECK(hipMemcpyAsync(ssoft_.pres, c->soft_pres + start, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
        HIP_CHECK(hipMemcpyAsync(ssoft_.freq, c->soft_freq + start, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
      }
    }
    if (use_graph_ && soft) {   // a soft recording, in the map of its own
      auto& g = scsgraphs_[std::make_tuple(Bp, ar, sr)];
      if (!g) {
        g.reset(new Graph());
        g->begin(cap_);
        record_score(Bp, cap_, true, ar, sr);
        g->end(cap_);
      }
      g->launch(s);
    } else if (use_graph_) {
      // an uncontrolled call: the graphs it had.  A controlled recording bakes the table's line count in
      // (every entry is checked against it), so that is part of its key; 0 = unconstrained
      auto& g = c ? scgraphs_[std::make_pair(Bp, ar)] : sgraphs_[Bp];
      if (!g) {
        g.reset(new Graph());
        g->begin(cap_);
        record_score(Bp, cap_, c != nullptr, ar);
        g->end(cap_);
      }
      g->launch(s);
    } else {
      record_score(Bp, s, c != nullptr, ar, sr);
    }
    HIP_CHECK(hipMemcpyAsync(tok_logp + (size_t)start * ML, stok_, (size_t)n * ML * 4, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(rank + (size_t)start * ML, srank_, (size_t)n * ML * 4, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(name_logp + start, sname_, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(n_tok + start, sntok_out_, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    if (c) HIP_CHECK(hipMemcpyAsync(n_kept + (size_t)start * ML, snkept_, (size_t)n * ML * 4, hipMemcpyDeviceToDevice, s));
  }
}

// ------------------------------------------------------------------------------ beam search
// Buffers of the beam loop, sized for Bmax_ rows: a generator that never searches never allocates them.
void Generator::beam_alloc() {
  if (bready_) return;
  const size_t V = d_.V, H = d_.H, ML = d_.max_len, B = Bmax_;
  const size_t slab_rows = std::max<size_t>(B, kF32SlabRows);
  std::vector<size_t> oA, oB;
  for (int l = 0; l < d_.L; ++l) { oA.push_back(barena_.reserve(B * H * 4)); oB.push_back(barena_.reserve(B * H * 4)); }
  const size_t ogh = barena_.reserve(slab_rows * 3 * H * 4);
  const size_t ogi = d_.L > 1 ? barena_.reserve(slab_rows * 3 * H * 4) : 0;
  const size_t olg = barena_.reserve(slab_rows * V * 4);
  const size_t oids = barena_.reserve(B * 4);
  size_t osc[2], ost[2], oln[2], orw[2];
  for (int i = 0; i < 2; ++i) {
    osc[i] = barena_.reserve(B * 4); ost[i] = barena_.reserve(B * 4); oln[i] = barena_.reserve(B * 4);
    orw[i] = barena_.reserve(B * (ML + 1));
  }
  const size_t opa = barena_.reserve(B * 4), och = barena_.reserve(B * 4), onx = barena_.reserve(B * 4);
  const size_t onb = barena_.reserve(B * 4), opl = barena_.reserve(B * 4), opre = barena_.reserve(B * ML);
  const size_t otab = barena_.reserve((size_t)kAllowRows * (d_.V / 32) * 4), oidx = barena_.reserve(B * ML * 4);
  barena_.commit();
  for (int l = 0; l < d_.L; ++l) { bhA_.push_back(barena_.get<float>(oA[l])); bhB_.push_back(barena_.get<float>(oB[l])); }
  bgh_ = barena_.get<float>(ogh); bgi_ = d_.L > 1 ? barena_.get<float>(ogi) : nullptr;
  blogits_ = barena_.get<float>(olg); bids_ = barena_.get<int>(oids);
  for (int i = 0; i < 2; ++i) {
    bscore_[i] = barena_.get<float>(osc[i]); bstate_[i] = barena_.get<int>(ost[i]); blen_[i] = barena_.get<int>(oln[i]);
    brows_[i] = barena_.get<unsigned char>(orw[i]);
  }
  bparent_ = barena_.get<int>(opa); bchr_ = barena_.get<int>(och); bnext_ = barena_.get<int>(onx);
  bnb_ = barena_.get<int>(onb); bplen_ = barena_.get<int>(opl); bprefix_ = barena_.get<unsigned char>(opre);
  btab_ = barena_.get<unsigned>(otab); bidx_ = barena_.get<int>(oidx);
  bready_ = true;
}

// The beam loop for n names of W beams: 1 + ML (L products + L gates (+ L - 1 input products) + the
// logits product + select + reorder) launches, a single chain.  Every row runs record_steps_f32's
// exact-fp32 step (the master weights, f32_splits slabs summed in order by the consumer), but on
// fixed slots: the gates read bhA_ and write bhB_, the reorder gathers bhB_ -> bhA_.  Scores, states,
// lengths and output rows alternate between two sets by step parity; the result is in set ML & 1.
void Generator::record_beam(int n, int W, hipStream_t s, int allow_rows, bool automaton, BeamSelect sel) {
  const int H = d_.H, L = d_.L, V = d_.V, ML = d_.max_len;
  const int Bp = rup(n * W, 64);
  const int cap = std::max(Bmax_, kF32SlabRows);
  BeamResetArgs r;
  for (int l = 0; l < L; ++l) r.h[l] = bhA_[l];
  r.ids = bids_; r.score = bscore_[0]; r.state = bstate_[0]; r.len = blen_[0]; r.rows = brows_[0];
  r.N = n; r.W = W; r.L = L; r.Bp = Bp; r.H = H; r.max_len = ML; r.sos = d_.sos;
  if (automaton) { r.allow_state = abstate_[0]; r.allow_start = abstart_; }
  beam_reset(r, s);
  auto product = [&](const float* A, const float* Wt, const float* bias, int N, float* C) {
    GemmF32Args g;
    g.A = A; g.lda = H; g.B = Wt; g.ldb = H; g.C = C; g.ldc = N;
    g.bias = bias; g.M = Bp; g.N = N; g.K = H;
    g.splits = f32_splits(Bp, N, H, cap); g.slab = (long)Bp * N;
    gemm_f32_nt(g, s);
    return g.splits;
  };
  for (int st = 0; st < ML; ++st) {
    const int cur = st & 1, nxt = cur ^ 1;
    for (int l = 0; l < L; ++l) {
      const std::string k = std::to_string(l);
      const int sh = product(bhA_[l], P("weight_hh_l" + k), P("bias_hh_l" + k), 3 * H, bgh_);
      GruGatesF32Args a;
      if (l == 0) {
        a.P = Ptab32_; a.ids = bids_;
      } else {
        a.gi_splits = product(bhB_[l - 1], P("weight_ih_l" + k), P("bias_ih_l" + k), 3 * H, bgi_);
        a.Gi = bgi_; a.gi_slab = (long)Bp * 3 * H;
      }
      a.Gh = bgh_; a.gh_splits = sh; a.gh_slab = (long)Bp * 3 * H; a.hprev = bhA_[l]; a.hout = bhB_[l];
      a.Bp = Bp; a.H = H; a.V = V; a.err = err_;
      gru_gates_f32(a, s);
    }
    const int splits = product(bhB_[L - 1], P("fc.weight"), P("fc.bias"), V, blogits_);
    // what the three selections share: the logits, the states, the prefix, the outputs beam_reorder reads, the
    // shape and the constraint (an automaton's state buffers by step parity, or the per-position table)
    auto common = [&](auto& q) {
      q.logits = blogits_; q.splits = splits; q.slab = (long)Bp * V;
      q.state_in = bstate_[cur]; q.plen = bplen_; q.prefix = bprefix_;
      q.state_out = bstate_[nxt]; q.parent = bparent_; q.chr = bchr_; q.next_id = bnext_;
      q.err = err_; q.N = n; q.W = W; q.V = V; q.step = st; q.max_len = ML; q.sos = d_.sos; q.eos = d_.eos;
      if (automaton) {
        q.allow_tab = atab_; q.allow_next = anxt_; q.allow_rows = allow_rows;
        q.allow_state_in = abstate_[cur]; q.allow_state_out = abstate_[nxt];
      } else if (allow_rows > 0) {
        q.allow_tab = btab_; q.allow_idx = bidx_; q.allow_rows = allow_rows;
      }
    };
    if (sel == BeamSelect::kConditional) {   // §4j: the same loop, W weighted particles with resampling
      SmcSelectArgs q;
      common(q);
      q.logq_in = bscore_[cur]; q.logw_in = st == 0 ? bscore_[0] : qw_[cur];   // before step 0: logw = logq = 0 / -inf
      q.seed = qwords_; q.start = qwords_ + 1; q.thr = reinterpret_cast<const float*>(qwords_ + 2); q.inv_t = qinv_;
      q.logq_out = bscore_[nxt]; q.logw_out = qw_[nxt]; q.n_res = qres_;
      smc_select_f32(q, s);
    } else if (sel == BeamSelect::kDistinct) {   // §4i: the same loop, ranked by truncated Gumbel-perturbed log-probabilities
      SbsSelectArgs q;
      common(q);
      q.logq_in = bscore_[cur]; q.G_in = st == 0 ? bscore_[0] : dG_[cur];   // before step 0: G = logq = 0 / -inf
      q.seed = dwords_; q.start = dwords_ + 1; q.inv_t = dinv_;
      q.logq_out = bscore_[nxt]; q.G_out = dG_[nxt];
      sbs_select_f32(q, s);
    } else {
      BeamSelectArgs q;
      common(q);
      q.score_in = bscore_[cur]; q.score_out = bscore_[nxt];
      beam_select_f32(q, s);
    }
    BeamReorderArgs o;
    for (int l = 0; l < L; ++l) { o.h_src[l] = bhB_[l]; o.h_dst[l] = bhA_[l]; }
    o.parent = bparent_; o.chr = bchr_; o.next_id = bnext_;
    o.rows_src = brows_[cur]; o.rows_dst = brows_[nxt]; o.len_src = blen_[cur]; o.len_dst = blen_[nxt];
    o.ids = bids_; o.n_beams = bnb_;
    o.N = n; o.W = W; o.L = L; o.H = H; o.max_len = ML;
    beam_reorder(o, s);
    HIP_LAUNCH_CHECK();
  }
}

void Generator::beam(const int* plen, const unsigned char* prefix, int N, int W, unsigned char* rows, float* logp,
                     int* n_tok, int* n_beams, hipStream_t s, const unsigned* allow_tab, const int* allow_idx,
                     int allow_rows, const unsigned short* allow_next, const int* allow_start) {
  GK_TRACE("gk.beam");
  const int ML = d_.max_len;
  if (W < 1 || W > 32 || W > d_.V) throw std::runtime_error("Generator::beam needs 1 <= width <= min(32, vocab)");
  if (ML > 64 || d_.V > 512) throw std::runtime_error("Generator::beam needs max_len <= 64 and vocab <= 512");
  if (d_.max_batch < W) throw std::runtime_error("Generator::beam needs max_batch >= width");
  if (d_.L > 4) throw std::runtime_error("Generator::beam needs at most 4 layers");
  if (!plen || !prefix || !rows || !logp || !n_tok || !n_beams)
    throw std::runtime_error("Generator::beam: plen, prefix, rows, logp, n_tok and n_beams are required");
  const bool aut = allow_next != nullptr || allow_start != nullptr;
  if (aut && (!allow_next || !allow_start || !allow_tab || allow_idx || allow_rows < 1 || allow_rows > kAutoStates ||
              (d_.V != 256 && d_.V != 512)))
    throw std::runtime_error("Generator::beam: an automaton needs allow_tab, allow_next and allow_start, no allow_idx, "
                             "1 <= allow_rows <= 65535 and a vocabulary of 256 or 512");
  const bool masked = allow_tab != nullptr;
  if (!aut && (masked != (allow_idx != nullptr) || (masked && (allow_rows < 1 || allow_rows > kAllowRows))))
    throw std::runtime_error("Generator::beam: constraints need allow_tab, allow_idx and 1 <= allow_rows <= 1024");
  if (N <= 0) return;
  beam_alloc();   // first call: allocates (and synchronises) before anything is captured
  if (aut) automaton_stage(allow_tab, allow_next, allow_rows, s);   // the tables once per call
  HIP_CHECK(hipMemsetAsync(err_, 0, 16, s));   // the error word covers the whole call, as in generate()
  err_clean_ = false;
  const int nb = d_.max_batch / W, fin = ML & 1;
  const int ar = masked ? allow_rows : 0;
  if (masked && !aut)   // the table once per call
    HIP_CHECK(hipMemcpyAsync(btab_, allow_tab, (size_t)ar * (d_.V / 32) * 4, hipMemcpyDeviceToDevice, s));
  for (int start = 0; start < N; start += nb) {
    const int n = std::min(nb, N - start);
    HIP_CHECK(hipMemcpyAsync(bplen_, plen + start, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(bprefix_, prefix + (size_t)start * ML, (size_t)n * ML, hipMemcpyDeviceToDevice, s));
    if (aut)
      HIP_CHECK(hipMemcpyAsync(abstart_, allow_start + start, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    else if (masked)
      HIP_CHECK(hipMemcpyAsync(bidx_, allow_idx + (size_t)start * ML, (size_t)n * ML * 4, hipMemcpyDeviceToDevice, s));
    if (use_graph_) {
      // ar: baked into the recording, as in generate_ctl; the automaton recordings have a map of their own
      if (aut && abgraphs_.size() >= kAutoGraphs && !abgraphs_.count(std::make_tuple(n, W, ar))) {   // as in generate_ctl
        HIP_CHECK(hipStreamSynchronize(s));
        abgraphs_.clear();
      }
      auto& g = aut ? abgraphs_[std::make_tuple(n, W, ar)] : bgraphs_[std::make_tuple(n, W, ar)];
      if (!g) {
        g.reset(new Graph());
        g->begin(cap_);
        record_beam(n, W, cap_, ar, aut);
        g->end(cap_);
      }
      g->launch(s);
    } else {
      record_beam(n, W, s, ar, aut);
    }
    const size_t r0 = (size_t)start * W, nr = (size_t)n * W;
    HIP_CHECK(hipMemcpyAsync(rows + r0 * (ML + 1), brows_[fin], nr * (ML + 1), hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(logp + r0, bscore_[fin], nr * 4, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(n_tok + r0, blen_[fin], nr * 4, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(n_beams + start, bnb_, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  }
}

// ------------------------------------------------------------------------------ distinct names
void Generator::distinct_alloc() {
  if (dwords_) return;
  const size_t B = Bmax_;
  for (float** p : {&dG_[0], &dG_[1], &dinv_}) {
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(p), B * 4));
    HIP_CHECK(hipMemset(*p, 0, B * 4));
  }
  HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&dwords_), 16));
  HIP_CHECK(hipMemset(dwords_, 0, 16));
}

void Generator::distinct(const int* plen, const unsigned char* prefix, int N, int W, unsigned long long seed,
                         unsigned long long start, const float* inv_t, unsigned char* rows, float* logq, float* gumbel,
                         int* n_tok, int* n_found, hipStream_t s, const unsigned* allow_tab, const int* allow_idx,
                         int allow_rows, const unsigned short* allow_next, const int* allow_start) {
  GK_TRACE("gk.distinct");
  const int ML = d_.max_len;
  if (W < 1 || W > 32 || W > d_.V) throw std::runtime_error("Generator::distinct needs 1 <= width <= min(32, vocab)");
  if (ML > 64 || d_.V > 512) throw std::runtime_error("Generator::distinct needs max_len <= 64 and vocab <= 512");
  if (d_.max_batch < W) throw std::runtime_error("Generator::distinct needs max_batch >= width");
  if (d_.L > 4) throw std::runtime_error("Generator::distinct needs at most 4 layers");
  if (!plen || !prefix || !inv_t || !rows || !logq || !gumbel || !n_tok || !n_found)
    throw std::runtime_error("Generator::distinct: plen, prefix, inv_t, rows, logq, gumbel, n_tok and n_found are required");
  const bool aut = allow_next != nullptr || allow_start != nullptr;
  if (aut && (!allow_next || !allow_start || !allow_tab || allow_idx || allow_rows < 1 || allow_rows > kAutoStates ||
              (d_.V != 256 && d_.V != 512)))
    throw std::runtime_error("Generator::distinct: an automaton needs allow_tab, allow_next and allow_start, no allow_idx, "
                             "1 <= allow_rows <= 65535 and a vocabulary of 256 or 512");
  const bool masked = allow_tab != nullptr;
  if (!aut && (masked != (allow_idx != nullptr) || (masked && (allow_rows < 1 || allow_rows > kAllowRows))))
    throw std::runtime_error("Generator::distinct: constraints need allow_tab, allow_idx and 1 <= allow_rows <= 1024");
  if (N <= 0) return;
  beam_alloc();       // first call: allocates (and synchronises) before anything is captured
  distinct_alloc();
  if (aut) automaton_stage(allow_tab, allow_next, allow_rows, s);   // the tables once per call
  HIP_CHECK(hipMemsetAsync(err_, 0, 16, s));
  err_clean_ = false;
  const int nb = d_.max_batch / W, fin = ML & 1;
  const int ar = masked ? allow_rows : 0;
  if (masked && !aut)   // the table once per call
    HIP_CHECK(hipMemcpyAsync(btab_, allow_tab, (size_t)ar * (d_.V / 32) * 4, hipMemcpyDeviceToDevice, s));
  for (int b0 = 0; b0 < N; b0 += nb) {
    const int n = std::min(nb, N - b0);
    HIP_CHECK(hipMemcpyAsync(bplen_, plen + b0, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(bprefix_, prefix + (size_t)b0 * ML, (size_t)n * ML, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(dinv_, inv_t + b0, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    sbs_stage(dwords_, seed, dwords_ + 1, start + (unsigned long long)b0, s);
    HIP_LAUNCH_CHECK();
    if (aut)
      HIP_CHECK(hipMemcpyAsync(abstart_, allow_start + b0, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    else if (masked)
      HIP_CHECK(hipMemcpyAsync(bidx_, allow_idx + (size_t)b0 * ML, (size_t)n * ML * 4, hipMemcpyDeviceToDevice, s));
    if (use_graph_) {
      if (aut && adgraphs_.size() >= kAutoGraphs && !adgraphs_.count(std::make_tuple(n, W, ar))) {   // as in beam()
        HIP_CHECK(hipStreamSynchronize(s));
        adgraphs_.clear();
      }
      auto& g = aut ? adgraphs_[std::make_tuple(n, W, ar)] : dgraphs_[std::make_tuple(n, W, ar)];
      if (!g) {
        g.reset(new Graph());
        g->begin(cap_);
        record_beam(n, W, cap_, ar, aut, BeamSelect::kDistinct);
        g->end(cap_);
      }
      g->launch(s);
    } else {
      record_beam(n, W, s, ar, aut, BeamSelect::kDistinct);
    }
    const size_t r0 = (size_t)b0 * W, nr = (size_t)n * W;
    HIP_CHECK(hipMemcpyAsync(rows + r0 * (ML + 1), brows_[fin], nr * (ML + 1), hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(logq + r0, bscore_[fin], nr * 4, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(gumbel + r0, dG_[fin], nr * 4, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(n_tok + r0, blen_[fin], nr * 4, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(n_found + b0, bnb_, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  }
}

// ------------------------------------------------------------------------------ conditional names
void Generator::conditional_alloc() {
  if (qwords_) return;
  const size_t B = Bmax_;
  for (float** p : {&qw_[0], &qw_[1], &qinv_}) {
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(p), B * 4));
    HIP_CHECK(hipMemset(*p, 0, B * 4));
  }
  HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&qres_), B * 4));
  HIP_CHECK(hipMemset(qres_, 0, B * 4));
  HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&qwords_), 32));
  HIP_CHECK(hipMemset(qwords_, 0, 32));
}

void Generator::conditional(const int* plen, const unsigned char* prefix, int N, int W, unsigned long long seed,
                            unsigned long long start, float thr, const float* inv_t, unsigned char* rows, float* logw,
                            float* logq, int* n_tok, int* n_res, hipStream_t s, const unsigned* allow_tab,
                            const int* allow_idx, int allow_rows, const unsigned short* allow_next, const int* allow_start) {
  GK_TRACE("gk.conditional");
  const int ML = d_.max_len;
  if (W < 1 || W > 32 || W > d_.V) throw std::runtime_error("Generator::conditional needs 1 <= width <= min(32, vocab)");
  if (ML > 64 || d_.V > 512) throw std::runtime_error("Generator::conditional needs max_len <= 64 and vocab <= 512");
  if (d_.max_batch < W) throw std::runtime_error("Generator::conditional needs max_batch >= width");
  if (d_.L > 4) throw std::runtime_error("Generator::conditional needs at most 4 layers");
  if (!(thr >= 0.f && thr <= 1.f)) throw std::runtime_error("Generator::conditional needs 0 <= ess threshold <= 1");
  if (!plen || !prefix || !inv_t || !rows || !logw || !logq || !n_tok || !n_res)
    throw std::runtime_error("Generator::conditional: plen, prefix, inv_t, rows, logw, logq, n_tok and n_res are required");
  const bool aut = allow_next != nullptr || allow_start != nullptr;
  if (aut && (!allow_next || !allow_start || !allow_tab || allow_idx || allow_rows < 1 || allow_rows > kAutoStates ||
              (d_.V != 256 && d_.V != 512)))
    throw std::runtime_error("Generator::conditional: an automaton needs allow_tab, allow_next and allow_start, no "
                             "allow_idx, 1 <= allow_rows <= 65535 and a vocabulary of 256 or 512");
  const bool masked = allow_tab != nullptr;
  if (!aut && (masked != (allow_idx != nullptr) || (masked && (allow_rows < 1 || allow_rows > kAllowRows))))
    throw std::runtime_error("Generator::conditional: constraints need allow_tab, allow_idx and 1 <= allow_rows <= 1024");
  if (N <= 0) return;
  beam_alloc();       // first call: allocates (and synchronises) before anything is captured
  conditional_alloc();
  if (aut) automaton_stage(allow_tab, allow_next, allow_rows, s);   // the tables once per call
  HIP_CHECK(hipMemsetAsync(err_, 0, 16, s));
  err_clean_ = false;
  const int nb = d_.max_batch / W, fin = ML & 1;
  const int ar = masked ? allow_rows : 0;
  if (masked && !aut)   // the table once per call
    HIP_CHECK(hipMemcpyAsync(btab_, allow_tab, (size_t)ar * (d_.V / 32) * 4, hipMemcpyDeviceToDevice, s));
  for (int b0 = 0; b0 < N; b0 += nb) {
    const int n = std::min(nb, N - b0);
    HIP_CHECK(hipMemcpyAsync(bplen_, plen + b0, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(bprefix_, prefix + (size_t)b0 * ML, (size_t)n * ML, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(qinv_, inv_t + b0, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    smc_stage(qwords_, seed, start + (unsigned long long)b0, thr, s);
    HIP_LAUNCH_CHECK();
    if (aut)
      HIP_CHECK(hipMemcpyAsync(abstart_, allow_start + b0, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    else if (masked)
      HIP_CHECK(hipMemcpyAsync(bidx_, allow_idx + (size_t)b0 * ML, (size_t)n * ML * 4, hipMemcpyDeviceToDevice, s));
    if (use_graph_) {
      if (aut && aqgraphs_.size() >= kAutoGraphs && !aqgraphs_.count(std::make_tuple(n, W, ar))) {   // as in beam()
        HIP_CHECK(hipStreamSynchronize(s));
        aqgraphs_.clear();
      }
      auto& g = aut ? aqgraphs_[std::make_tuple(n, W, ar)] : qgraphs_[std::make_tuple(n, W, ar)];
      if (!g) {
        g.reset(new Graph());
        g->begin(cap_);
        record_beam(n, W, cap_, ar, aut, BeamSelect::kConditional);
        g->end(cap_);
      }
      g->launch(s);
    } else {
      record_beam(n, W, s, ar, aut, BeamSelect::kConditional);
    }
    const size_t r0 = (size_t)b0 * W, nr = (size_t)n * W;
    HIP_CHECK(hipMemcpyAsync(rows + r0 * (ML + 1), brows_[fin], nr * (ML + 1), hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(logq + r0, bscore_[fin], nr * 4, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(logw + r0, qw_[fin], nr * 4, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(n_tok + r0, blen_[fin], nr * 4, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(n_res + b0, qres_, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  }
}

unsigned Generator::read_error() {
  unsigned e[4] = {0, 0, 0, 0};
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpy(e, err_, 16, hipMemcpyDeviceToHost));
  // reporting is the caller's (HipGenerator / the C API raise or print it); the detail line is a debug aid
  const char* dbg = std::getenv("GK_GEN_DEBUG");
  if (e[0] && dbg && dbg[0] && dbg[0] != '0')
    std::fprintf(stderr, "[generator] error word %u: id %d (0x%08x) at row %u\n", e[0], (int)e[1], e[1], e[2]);
  return e[0];
}

}  // namespace gk

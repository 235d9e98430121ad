// Thin pybind11 layer over the native engine.  No torch headers: device memory is passed as
// integer addresses (tensor.data_ptr()) and streams as integer handles
// (torch.cuda.current_stream().cuda_stream), so this TU compiles in seconds and the
// extension binds to whichever libamdhip64 the process already loaded (torch's).
#include <pybind11/pybind11.h>
#include <pybind11/numpy.h>
#include <pybind11/stl.h>

#include "engine/trainer.h"
#include "engine/generator.h"
#include "comm/rccl_comm.h"
#include "comm/bootstrap.h"
#include "data/name_loader.h"

namespace py = pybind11;
using namespace gk;

static hipStream_t S(uintptr_t s) { return reinterpret_cast<hipStream_t>(s); }
template <class T> static T* Pp(uintptr_t p) { return reinterpret_cast<T*>(p); }

template <class T>
static T get(const py::dict& d, const char* k, T dflt) {
  if (!d.contains(k)) return dflt;
  return d[k].cast<T>();
}
#define GP(T, d, k) reinterpret_cast<T*>(get<uintptr_t>(d, k, 0))

// every OptimArgs field from a dict (raw optimiser kernels); `who` names the binding in errors
static OptimArgs optim_from(const py::dict& d, const std::string& who) {
  OptimArgs a;
  a.p = GP(float, d, "p"); a.g = GP(const float, d, "g"); a.m = GP(float, d, "m"); a.v = GP(float, d, "v");
  a.n = get<long>(d, "n", 0);
  a.step = GP(int, d, "step"); a.gscale = GP(const float, d, "gscale");
  a.err = GP(const unsigned, d, "err"); a.err_host = GP(unsigned, d, "err_host");
  a.lr = get<float>(d, "lr", a.lr); a.b1 = get<float>(d, "b1", a.b1); a.b2 = get<float>(d, "b2", a.b2);
  a.eps = get<float>(d, "eps", a.eps); a.wd = get<float>(d, "wd", a.wd); a.sgd = get<int>(d, "sgd", 0);
  a.sched = get<int>(d, "sched", 0); a.warmup = get<int>(d, "warmup", 0); a.total = get<int>(d, "total", 0);
  a.lr_min = get<float>(d, "lr_min", 0.f);
  a.keep_g = get<int>(d, "keep_g", 1);
  if (!a.p || !a.step || a.n < 0) throw std::runtime_error(who + ": p, step and n >= 0 required");
  if (!a.sgd && (!a.m || !a.v)) throw std::runtime_error(who + ": Adam needs m and v");
  if (a.sched < 0 || a.sched > 2) throw std::runtime_error(who + ": sched 0 (const), 1 (cosine) or 2 (linear)");
  return a;
}

// every GemmArgs field from a dict (raw GEMM kernels and their predicates); `who` names the binding in errors
static GemmArgs gemm_from(const py::dict& d, const std::string& who) {
  GemmArgs a;
  a.A = GP(const u16, d, "A"); a.lda = get<int>(d, "lda", 0);
  a.A32 = GP(const float, d, "A32"); a.a32_trans = get<int>(d, "a32_trans", 0);
  a.onehot_ids = GP(const int, d, "onehot_ids");
  a.B2 = GP(const u16, d, "B2"); a.b2_row = get<int>(d, "b2_row", 0);
  a.B = GP(const u16, d, "B"); a.ldb = get<int>(d, "ldb", 0);
  a.C = GP(float, d, "C"); a.ldc = get<int>(d, "ldc", 0);
  a.bias = GP(const float, d, "bias"); a.rowsumA = GP(float, d, "rowsumA");
  a.M = get<int>(d, "M", 0); a.N = get<int>(d, "N", 0); a.K = get<int>(d, "K", 0);
  a.splits = get<int>(d, "splits", 1); a.accumulate = get<int>(d, "accumulate", 0);
  a.raster = get<int>(d, "raster", 0);
  a.algo = get<int>(d, "algo", 0);
  if (a.M <= 0 || a.N <= 0 || a.K <= 0 || a.splits < 1 || a.K % a.splits)
    throw std::runtime_error(who + ": M, N, K > 0 and K a multiple of splits >= 1 required");
  if (a.raster != 0 && a.raster != 1) throw std::runtime_error(who + ": raster 0 (auto) or 1 (column-fast)");
  if (a.A32 && (a.A || a.onehot_ids)) throw std::runtime_error(who + ": A32 excludes A and onehot_ids");
  return a;
}

// what every generic kernel needs (the streaming one-hot kernel has its own, narrower column blocks)
static void gemm_tiles64(const GemmArgs& a, const std::string& who) {
  if (a.M % 64 || a.N % 64 || (a.K / a.splits) % 32)
    throw std::runtime_error(who + ": M, N must be multiples of 64 and K/splits a multiple of 32");
}

// PrepJob from a dict; rows up to Bp are read from a slot of Bmax rows (kernels.h prep_batch)
static PrepJob prep_from(const py::dict& d, const std::string& who) {
  PrepJob p;
  p.in = GP(const int, d, "in"); p.Bmax = get<int>(d, "Bmax", 0); p.T = get<int>(d, "T", 0); p.Bp = get<int>(d, "Bp", 0);
  p.ids = GP(int, d, "ids"); p.labels = GP(int, d, "labels"); p.inv_count = GP(float, d, "inv_count");
  if (!p.in || !p.ids || !p.labels || !p.inv_count || p.T < 1 || p.Bp < 1)
    throw std::runtime_error(who + ": in, ids, labels, inv_count and T, Bp >= 1 required");
  if (p.Bp > p.Bmax) throw std::runtime_error(who + ": Bp > Bmax would read past the staging slot");
  return p;
}

PYBIND11_MODULE(_C, m) {
  m.doc() = "gru_mpi_cuda_amd native engine (HIP/CDNA4 kernels, hipGraph executor, RCCL comm)";

  m.def("set_rank", [](int r) { global_rank() = r; });

  py::class_<NameLoader>(m, "NameLoader")
      .def(py::init([](py::dict d) {
        LoaderCfg c;
        c.B = get<int>(d, "B", 256); c.T = get<int>(d, "T", 32);
        c.sos = get<int>(d, "sos", 0); c.eos = get<int>(d, "eos", 0); c.max_len = get<int>(d, "max_len", 10);
        c.seed = get<uint64_t>(d, "seed", 0); c.prefetch = get<int>(d, "prefetch", 4);
        c.path = get<std::string>(d, "path", "");
        return new NameLoader(c);
      }))
      .def("next", [](NameLoader& L, int B, int T) {
        py::array_t<int32_t> x({B, T}), y({B, T});
        int32_t* px = x.mutable_data();
        int32_t* py_ = y.mutable_data();
        {
          py::gil_scoped_release nogil;   // the producer thread may still be filling the batch
          L.next(px, py_);
        }
        return py::make_tuple(x, y);
      })
      .def("batches", &NameLoader::batches)
      .def("epoch", &NameLoader::epoch)
      .def("names_in_file", &NameLoader::names_in_file);
  m.def("device_info", []() {
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    hipDeviceProp_t p;
    HIP_CHECK(hipGetDeviceProperties(&p, dev));
    py::dict d;
    d["name"] = std::string(p.name);
    d["arch"] = std::string(p.gcnArchName);
    d["cus"] = p.multiProcessorCount;
    d["lds_per_cu"] = (long)p.maxSharedMemoryPerMultiProcessor;
    d["hbm_bytes"] = (long)p.totalGlobalMem;
    return d;
  });
  m.def("device_synchronize", []() { HIP_CHECK(hipDeviceSynchronize()); });

  py::class_<Trainer>(m, "Trainer")
      .def(py::init([](py::dict dims, py::dict opt, uintptr_t params, uintptr_t grads, uintptr_t mm, uintptr_t vv,
                       long nflat, std::map<std::string, long> offsets) {
        Dims d;
        d.V = get<int>(dims, "V", 256); d.E = get<int>(dims, "E", 512); d.H = get<int>(dims, "H", 512);
        d.L = get<int>(dims, "L", 1); d.B = get<int>(dims, "B", 256); d.T = get<int>(dims, "T", 32);
        d.chunks = get<int>(dims, "chunks", 4); d.overlap = get<int>(dims, "overlap", 1);
        d.seed = get<uint64_t>(dims, "seed", 0);
        OptCfg o;
        o.lr = get<float>(opt, "lr", 1e-3f); o.b1 = get<float>(opt, "beta1", 0.9f); o.b2 = get<float>(opt, "beta2", 0.999f);
        o.eps = get<float>(opt, "eps", 1e-8f); o.wd = get<float>(opt, "weight_decay", 0.f);
        o.clip = get<float>(opt, "clip_norm", 0.f); o.sgd = get<int>(opt, "sgd", 0);
        o.sched = get<int>(opt, "lr_sched", 0); o.warmup = get<int>(opt, "warmup_steps", 0);
        o.total = get<int>(opt, "total_steps", 0); o.lr_min = get<float>(opt, "lr_min", 0.f);
        o.keep_grads = get<int>(opt, "keep_grads", 1);
        o.dropout = get<double>(opt, "dropout", 0.0);
        return new Trainer(d, o, Pp<float>(params), Pp<float>(grads), Pp<float>(mm), Pp<float>(vv), nflat, offsets);
      }))
      .def("refresh_weights", [](Trainer& t, uintptr_t s) { t.refresh_weights(S(s)); })
      .def("set_batch", [](Trainer& t, py::array_t<int, py::array::c_style | py::array::forcecast> x,
                           py::array_t<int, py::array::c_style | py::array::forcecast> y, uintptr_t s) {
        if (x.ndim() != 2 || y.ndim() != 2 || x.shape(0) != y.shape(0) || x.shape(1) != y.shape(1))
          throw std::runtime_error("set_batch: x and y must both be [B, T]");
        t.set_batch(x.data(), y.data(), (int)x.shape(0), S(s));
      })
      .def("set_batch_device", [](Trainer& t, uintptr_t x, uintptr_t y, int B, uintptr_t s) {
        t.set_batch_device(Pp<const int>(x), Pp<const int>(y), B, S(s));
      })
      .def("set_comm", [](Trainer& t, RcclComm* c, std::vector<std::pair<long, long>> buckets, long min_bucket) {
        t.set_comm(c, buckets, min_bucket);
      }, py::arg("comm"), py::arg("buckets"), py::arg("min_bucket_floats") = 2L << 20, py::keep_alive<1, 2>())
      .def("allreduce_log", &Trainer::allreduce_log)
      .def("step", [](Trainer& t, uintptr_t s) { t.step(S(s)); })
      .def("set_graph_steps", &Trainer::set_graph_steps)
      .def("graph_steps", &Trainer::graph_steps)
      .def("set_batches", [](Trainer& t, py::array_t<int, py::array::c_style | py::array::forcecast> x,
                             py::array_t<int, py::array::c_style | py::array::forcecast> y) {
        if (x.ndim() != 3 || y.ndim() != 3 || x.shape(0) != y.shape(0) || x.shape(1) != y.shape(1) ||
            x.shape(2) != y.shape(2))
          throw std::runtime_error("set_batches: x and y must both be [G, B, T]");
        t.set_batches(x.data(), y.data(), (int)x.shape(1), (int)x.shape(0));
      })
      .def("step_group", [](Trainer& t, uintptr_t s) { t.step_group(S(s)); })
      .def("forward_backward", [](Trainer& t, uintptr_t s) { t.forward_backward(S(s)); })
      .def("optimizer_step", [](Trainer& t, uintptr_t s) { t.optimizer_step(S(s)); })
      .def("read_loss", &Trainer::read_loss)
      .def("read_grad_norm", &Trainer::read_grad_norm)
      .def("get_step", &Trainer::get_step)
      .def("set_step", &Trainer::set_step)
      .def("set_lr", &Trainer::set_lr)
      .def("set_use_graph", &Trainer::set_use_graph)
      .def("set_carry", &Trainer::set_carry)
      .def("carry", &Trainer::carry)
      .def("reset_hidden", [](Trainer& t, uintptr_t s) { t.reset_hidden(S(s)); })
      .def("padded_batch", &Trainer::padded_batch)
      .def("workspace_bytes", &Trainer::workspace_bytes)
      .def("plan", &Trainer::plan)
      .def("uses_persistent", &Trainer::uses_persistent)
      .def("read_error", &Trainer::read_error)
      .def("enable_watchdog", &Trainer::enable_watchdog)
      .def("set_shard_optim", &Trainer::set_shard_optim)
      .def("set_dp_pipeline", &Trainer::set_dp_pipeline)
      .def("dp_pipeline", &Trainer::dp_pipeline)
      .def("dp_tail_recorded", &Trainer::dp_tail_recorded)
      .def("shard_optim", &Trainer::shard_optim)
      .def("shard_mode", &Trainer::shard_mode)
      .def("gather_params", [](Trainer& t, uintptr_t s) { t.gather_params(S(s)); })
      .def("shard_chunk", &Trainer::shard_chunk)
      .def("gather_opt_state", [](Trainer& t, uintptr_t s) { t.gather_opt_state(S(s)); })
      .def("inject_error", &Trainer::inject_error)
      .def("watchdog_status", &Trainer::watchdog_status)
      .def("watchdog_message", &Trainer::watchdog_message)
      .def("buffer", &Trainer::buffer);

  py::class_<Generator>(m, "Generator")
      .def(py::init([](py::dict dims, uintptr_t params, std::map<std::string, long> offsets) {
        GenDims d;
        d.V = get<int>(dims, "V", 256); d.E = get<int>(dims, "E", 512); d.H = get<int>(dims, "H", 1024);
        d.L = get<int>(dims, "L", 2); d.max_len = get<int>(dims, "max_len", 10); d.sos = get<int>(dims, "sos", 0);
        d.eos = get<int>(dims, "eos", 0); d.max_batch = get<int>(dims, "max_batch", 4096);
        d.fp32 = get<int>(dims, "fp32", 0);
        return new Generator(d, Pp<const float>(params), offsets);
      }))
      .def("refresh_weights", [](Generator& g, uintptr_t s) { g.refresh_weights(S(s)); })
      .def("generate", [](Generator& g, uintptr_t rf, int N, uintptr_t out, uintptr_t s) {
        g.generate(Pp<const float>(rf), N, Pp<unsigned char>(out), S(s));
      })
      .def("generate_ctl", [](Generator& g, uintptr_t rf, int N, uintptr_t inv_temp, uintptr_t top_k, uintptr_t top_p,
                              uintptr_t plen, uintptr_t prefix, uintptr_t out, uintptr_t s, uintptr_t allow_tab,
                              uintptr_t allow_idx, int allow_rows, uintptr_t allow_next, uintptr_t allow_start,
                              uintptr_t soft_tab, uintptr_t soft_idx, int soft_rows, uintptr_t soft_pres,
                              uintptr_t soft_freq) {
        Generator::Ctl c;
        c.soft_tab = Pp<const float>(soft_tab); c.soft_idx = Pp<const int>(soft_idx); c.soft_rows = soft_rows;
        c.soft_pres = Pp<const float>(soft_pres); c.soft_freq = Pp<const float>(soft_freq);
        c.allow_next = Pp<const unsigned short>(allow_next); c.allow_start = Pp<const int>(allow_start);
        c.inv_temp = Pp<const float>(inv_temp); c.top_k = Pp<const int>(top_k); c.top_p = Pp<const float>(top_p);
        c.plen = Pp<const int>(plen); c.prefix = Pp<const unsigned char>(prefix);
        c.allow_tab = Pp<const unsigned>(allow_tab); c.allow_idx = Pp<const int>(allow_idx); c.allow_rows = allow_rows;
        g.generate_ctl(Pp<const float>(rf), N, c, Pp<unsigned char>(out), S(s));
      }, py::arg("rf"), py::arg("N"), py::arg("inv_temp"), py::arg("top_k"), py::arg("top_p"), py::arg("plen"),
         py::arg("prefix"), py::arg("out"), py::arg("stream"), py::arg("allow_tab") = (uintptr_t)0,
         py::arg("allow_idx") = (uintptr_t)0, py::arg("allow_rows") = 0, py::arg("allow_next") = (uintptr_t)0,
         py::arg("allow_start") = (uintptr_t)0, py::arg("soft_tab") = (uintptr_t)0, py::arg("soft_idx") = (uintptr_t)0,
         py::arg("soft_rows") = 0, py::arg("soft_pres") = (uintptr_t)0, py::arg("soft_freq") = (uintptr_t)0)
      .def("soft_graphs", &Generator::soft_graphs)
      .def("automaton_graphs", &Generator::automaton_graphs)
      .def("ctl_workspace_bytes", &Generator::ctl_workspace_bytes)
      .def("ctl_graphs", &Generator::ctl_graphs)
      .def("score", [](Generator& g, uintptr_t rows, int N, uintptr_t tok_logp, uintptr_t rank, uintptr_t name_logp,
                       uintptr_t n_tok, uintptr_t s, uintptr_t inv_temp, uintptr_t top_k, uintptr_t top_p, uintptr_t plen,
                       uintptr_t prefix, uintptr_t n_kept, uintptr_t allow_tab, uintptr_t allow_idx, int allow_rows,
                       uintptr_t soft_tab, uintptr_t soft_idx, int soft_rows, uintptr_t soft_pres, uintptr_t soft_freq) {
        // inv_temp set: the controlled score (every control array and n_kept are then required)
        Generator::Ctl c;
        c.soft_tab = Pp<const float>(soft_tab); c.soft_idx = Pp<const int>(soft_idx); c.soft_rows = soft_rows;
        c.soft_pres = Pp<const float>(soft_pres); c.soft_freq = Pp<const float>(soft_freq);
        c.inv_temp = Pp<const float>(inv_temp); c.top_k = Pp<const int>(top_k); c.top_p = Pp<const float>(top_p);
        c.plen = Pp<const int>(plen); c.prefix = Pp<const unsigned char>(prefix);
        c.allow_tab = Pp<const unsigned>(allow_tab); c.allow_idx = Pp<const int>(allow_idx); c.allow_rows = allow_rows;
        const bool ctl = inv_temp || top_k || top_p || plen || prefix || n_kept || allow_tab || allow_idx || soft_tab ||
                         soft_idx || soft_pres || soft_freq;
        g.score(Pp<const unsigned char>(rows), N, Pp<float>(tok_logp), Pp<int>(rank), Pp<float>(name_logp),
                Pp<int>(n_tok), S(s), ctl ? &c : nullptr, Pp<int>(n_kept));
      }, py::arg("rows"), py::arg("N"), py::arg("tok_logp"), py::arg("rank"), py::arg("name_logp"), py::arg("n_tok"),
         py::arg("stream"), py::arg("inv_temp") = (uintptr_t)0, py::arg("top_k") = (uintptr_t)0,
         py::arg("top_p") = (uintptr_t)0, py::arg("plen") = (uintptr_t)0, py::arg("prefix") = (uintptr_t)0,
         py::arg("n_kept") = (uintptr_t)0, py::arg("allow_tab") = (uintptr_t)0, py::arg("allow_idx") = (uintptr_t)0,
         py::arg("allow_rows") = 0, py::arg("soft_tab") = (uintptr_t)0, py::arg("soft_idx") = (uintptr_t)0,
         py::arg("soft_rows") = 0, py::arg("soft_pres") = (uintptr_t)0, py::arg("soft_freq") = (uintptr_t)0)
      .def("score_workspace_bytes", &Generator::score_workspace_bytes)
      .def("score_graphs", &Generator::score_graphs)
      .def("beam", [](Generator& g, uintptr_t plen, uintptr_t prefix, int N, int W, uintptr_t rows, uintptr_t logp,
                      uintptr_t n_tok, uintptr_t n_beams, uintptr_t s, uintptr_t allow_tab, uintptr_t allow_idx,
                      int allow_rows, uintptr_t allow_next, uintptr_t allow_start) {
        g.beam(Pp<const int>(plen), Pp<const unsigned char>(prefix), N, W, Pp<unsigned char>(rows), Pp<float>(logp),
               Pp<int>(n_tok), Pp<int>(n_beams), S(s), Pp<const unsigned>(allow_tab), Pp<const int>(allow_idx), allow_rows,
               Pp<const unsigned short>(allow_next), Pp<const int>(allow_start));
      }, py::arg("plen"), py::arg("prefix"), py::arg("N"), py::arg("W"), py::arg("rows"), py::arg("logp"),
         py::arg("n_tok"), py::arg("n_beams"), py::arg("stream"), py::arg("allow_tab") = (uintptr_t)0,
         py::arg("allow_idx") = (uintptr_t)0, py::arg("allow_rows") = 0, py::arg("allow_next") = (uintptr_t)0,
         py::arg("allow_start") = (uintptr_t)0)
      .def("distinct", [](Generator& g, uintptr_t plen, uintptr_t prefix, int N, int W, unsigned long long seed,
                          unsigned long long start, uintptr_t inv_t, uintptr_t rows, uintptr_t logq, uintptr_t gumbel,
                          uintptr_t n_tok, uintptr_t n_found, uintptr_t s, uintptr_t allow_tab, uintptr_t allow_idx,
                          int allow_rows, uintptr_t allow_next, uintptr_t allow_start) {
        g.distinct(Pp<const int>(plen), Pp<const unsigned char>(prefix), N, W, seed, start, Pp<const float>(inv_t),
                   Pp<unsigned char>(rows), Pp<float>(logq), Pp<float>(gumbel), Pp<int>(n_tok), Pp<int>(n_found), S(s),
                   Pp<const unsigned>(allow_tab), Pp<const int>(allow_idx), allow_rows, Pp<const unsigned short>(allow_next),
                   Pp<const int>(allow_start));
      }, py::arg("plen"), py::arg("prefix"), py::arg("N"), py::arg("W"), py::arg("seed"), py::arg("start"),
         py::arg("inv_t"), py::arg("rows"), py::arg("logq"), py::arg("gumbel"), py::arg("n_tok"), py::arg("n_found"),
         py::arg("stream"), py::arg("allow_tab") = (uintptr_t)0, py::arg("allow_idx") = (uintptr_t)0,
         py::arg("allow_rows") = 0, py::arg("allow_next") = (uintptr_t)0, py::arg("allow_start") = (uintptr_t)0)
      .def("distinct_graphs", &Generator::distinct_graphs)
      .def("conditional", [](Generator& g, uintptr_t plen, uintptr_t prefix, int N, int W, unsigned long long seed,
                             unsigned long long start, float thr, uintptr_t inv_t, uintptr_t rows, uintptr_t logw,
                             uintptr_t logq, uintptr_t n_tok, uintptr_t n_res, uintptr_t s, uintptr_t allow_tab,
                             uintptr_t allow_idx, int allow_rows, uintptr_t allow_next, uintptr_t allow_start) {
        g.conditional(Pp<const int>(plen), Pp<const unsigned char>(prefix), N, W, seed, start, thr, Pp<const float>(inv_t),
                      Pp<unsigned char>(rows), Pp<float>(logw), Pp<float>(logq), Pp<int>(n_tok), Pp<int>(n_res), S(s),
                      Pp<const unsigned>(allow_tab), Pp<const int>(allow_idx), allow_rows,
                      Pp<const unsigned short>(allow_next), Pp<const int>(allow_start));
      }, py::arg("plen"), py::arg("prefix"), py::arg("N"), py::arg("W"), py::arg("seed"), py::arg("start"),
         py::arg("thr"), py::arg("inv_t"), py::arg("rows"), py::arg("logw"), py::arg("logq"), py::arg("n_tok"),
         py::arg("n_res"), py::arg("stream"), py::arg("allow_tab") = (uintptr_t)0, py::arg("allow_idx") = (uintptr_t)0,
         py::arg("allow_rows") = 0, py::arg("allow_next") = (uintptr_t)0, py::arg("allow_start") = (uintptr_t)0)
      .def("conditional_graphs", &Generator::conditional_graphs)
      .def("beam_workspace_bytes", &Generator::beam_workspace_bytes)
      .def("beam_graphs", &Generator::beam_graphs)
      .def("set_use_graph", &Generator::set_use_graph)
      .def("read_error", &Generator::read_error)
      .def("set_probe", [](Generator& g, uintptr_t p) { g.set_probe(Pp<float>(p)); })
      .def("set_persist", &Generator::set_persist)
      .def("set_persist_max", &Generator::set_persist_max)
      .def("set_persist_dbg", [](Generator& g, uintptr_t p) { g.set_persist_dbg(reinterpret_cast<unsigned long long*>(p)); })
      .def("uses_persist", &Generator::uses_persist)
      .def("uses_persist_ctl", &Generator::uses_persist_ctl)
      .def("set_persist_ctl_max", &Generator::set_persist_ctl_max)
      .def("uses_persist_con", &Generator::uses_persist_con)
      .def("set_persist_con_max", &Generator::set_persist_con_max)
      .def("persist_con_launches", &Generator::persist_con_launches)
      .def("uses_persist_soft", &Generator::uses_persist_soft)
      .def("set_persist_soft_max", &Generator::set_persist_soft_max)
      .def("persist_soft_launches", &Generator::persist_soft_launches)
      .def("set_global_names", &Generator::set_global_names)
      .def("inject_persist_error", &Generator::inject_persist_error)
      .def("dump_graph", &Generator::dump_graph);

  // ---------------------------------------------------------------- raw kernels (tests, bench)
  m.def("gemm_f32", [](py::dict d, uintptr_t s) {   // fp32 MFMA GEMM of the fp32 generation path
    GemmF32Args a;
    a.A = GP(const float, d, "A"); a.lda = get<int>(d, "lda", 0);
    a.B = GP(const float, d, "B"); a.ldb = get<int>(d, "ldb", 0);
    a.C = GP(float, d, "C"); a.ldc = get<int>(d, "ldc", 0);
    a.bias = GP(const float, d, "bias");
    a.M = get<int>(d, "M", 0); a.N = get<int>(d, "N", 0); a.K = get<int>(d, "K", 0);
    a.splits = get<int>(d, "splits", 1); a.slab = get<long>(d, "slab", 0);
    gemm_f32_nt(a, S(s));
  });
  m.def("gemm_nt", [](py::dict d, uintptr_t s) {
    const GemmArgs a = gemm_from(d, "gemm_nt");
    if (a.A32 && a.algo != 3) throw std::runtime_error("gemm_nt: A32 (fp32-staged A) is read by algo 3 (gemm_small) only");
    const bool stream = a.onehot_ids && (a.algo == 0 || a.algo == 2) && gemm_variants().onehot && onehot_dp_ok(a);
    if (!stream) gemm_tiles64(a, "gemm_nt");
    if (!a.onehot_ids && !a.A && !a.A32) throw std::runtime_error("gemm_nt: no A operand");
    if (!a.B || !a.C) throw std::runtime_error("gemm_nt: B and C required");
    gemm_nt(a, S(s));
    HIP_LAUNCH_CHECK();
  });
  // several products in one launch: kind "small" (gemm_small_group) or "lds" (gemm_lds_group), 1-4 jobs
  m.def("gemm_group", [](const std::string& kind, py::list jobs, uintptr_t s) {
    if (jobs.size() < 1 || jobs.size() > 4) throw std::runtime_error("gemm_group: 1..4 jobs");
    GemmArgs j[4];
    int n = 0;
    for (auto h : jobs) j[n++] = gemm_from(h.cast<py::dict>(), "gemm_group");
    if (kind == "small") {
      if (!gemm_small_group_depth(j, n)) throw std::runtime_error("gemm_group: the jobs share no small-kernel chunk depth");
      gemm_small_group(j, n, S(s));
    } else if (kind == "lds") {
      for (int k = 0; k < n; ++k)
        if (j[k].A32 || j[k].onehot_ids) throw std::runtime_error("gemm_group: lds jobs take a bf16 A only");
      gemm_lds_group(j, n, S(s));
    } else {
      throw std::runtime_error("gemm_group: kind is \"small\" or \"lds\"");
    }
    HIP_LAUNCH_CHECK();
  });
  // the layer-0 table product with the batch transpose on trailing blocks of the same launch
  m.def("gemm_with_prep", [](py::dict g, py::dict p, uintptr_t s) {
    const GemmArgs a = gemm_from(g, "gemm_with_prep");
    if (a.A32 || a.onehot_ids || !a.A || !a.B || !a.C) throw std::runtime_error("gemm_with_prep: a bf16 A, B and C only");
    gemm_tiles64(a, "gemm_with_prep");
    gemm_with_prep(a, prep_from(p, "gemm_with_prep"), S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("prep_batch", [](py::dict p, uintptr_t s) {
    const PrepJob j = prep_from(p, "prep_batch");
    prep_batch(j.in, j.Bmax, j.T, j.Bp, j.ids, j.labels, j.inv_count, S(s));
    HIP_LAUNCH_CHECK();
  });
  // training dropout (dropout.hip): the two mask kernels on raw buffers.  d: hsb / xd / xdT / ldT (forward)
  // or dy (backward), step (one device int), seed, thr, scale, layer, b0, T, Bp, H
  auto dropout_from = [](py::dict d) {
    DropoutArgs a;
    a.hsb = GP(const u16, d, "hsb"); a.xd = GP(u16, d, "xd"); a.xdT = GP(u16, d, "xdT");
    a.ldT = get<long>(d, "ldT", 0); a.dy = GP(float, d, "dy"); a.step = GP(const int, d, "step");
    a.seed = get<uint64_t>(d, "seed", 0); a.thr = get<uint32_t>(d, "thr", 0); a.scale = get<float>(d, "scale", 1.f);
    a.layer = get<int>(d, "layer", 0); a.b0 = get<int>(d, "b0", 0);
    a.T = get<int>(d, "T", 0); a.Bp = get<int>(d, "Bp", 0); a.H = get<int>(d, "H", 0);
    return a;
  };
  m.def("dropout_fwd_seq", [dropout_from](py::dict d, uintptr_t s) {
    dropout_fwd_seq(dropout_from(d), S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("dropout_bwd_seq", [dropout_from](py::dict d, uintptr_t s) {
    dropout_bwd_seq(dropout_from(d), S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("colsum", [](uintptr_t in, int R, int C, uintptr_t out, uintptr_t s) {
    if (!in || !out || R < 1 || C < 1) throw std::runtime_error("colsum: in, out and R, C >= 1 required");
    colsum(Pp<const float>(in), R, C, Pp<float>(out), S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("rowsum_bf16", [](uintptr_t A, int lda, int M, int K, uintptr_t out, uintptr_t s) {
    if (!A || !out || M < 1 || K < 8 || K % 8 || lda % 8 || lda < K || A % 16)
      throw std::runtime_error("rowsum_bf16: needs K % 8 == 0, lda % 8 == 0, lda >= K and a 16-B aligned A");
    rowsum_bf16(Pp<const u16>(A), lda, M, K, Pp<float>(out), S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("split_bf16x3", [](uintptr_t src, int R, int K, uintptr_t dst, uintptr_t s) {
    if (!src || !dst || R < 1 || K < 1) throw std::runtime_error("split_bf16x3: src, dst and R, K >= 1 required");
    split_bf16x3(Pp<const float>(src), R, K, Pp<u16>(dst), S(s));
    HIP_LAUNCH_CHECK();
  });
  // which kernel takes a product (the gemm_nt dict): tests assert support instead of skipping
  m.def("gemm_small_kblocks", [](py::dict d) { return gemm_small_kblocks(gemm_from(d, "gemm_small_kblocks")); });
  m.def("gemm_small_group_depth", [](py::list jobs) {
    if (jobs.size() < 1 || jobs.size() > 4) throw std::runtime_error("gemm_small_group_depth: 1..4 jobs");
    GemmArgs j[4];
    int n = 0;
    for (auto h : jobs) j[n++] = gemm_from(h.cast<py::dict>(), "gemm_small_group_depth");
    return gemm_small_group_depth(j, n);
  });
  m.def("gemm_lds_ok", [](py::dict d) { return gemm_lds_ok(gemm_from(d, "gemm_lds_ok")); });
  m.def("gemm256_ok", [](py::dict d) { return gemm256_ok(gemm_from(d, "gemm256_ok")); });
  m.def("gemm256_tile_rows", [](py::dict d) {
    const GemmArgs a = gemm_from(d, "gemm256_tile_rows");
    return gemm256_tile_rows(a.M, a.N, a.K, a.splits);
  });
  m.def("onehot_dp_ok", [](py::dict d) { return onehot_dp_ok(gemm_from(d, "onehot_dp_ok")); });
  m.def("onehot_dp_splits", [](py::dict d) {
    const GemmArgs a = gemm_from(d, "onehot_dp_splits");
    return onehot_dp_splits(a.N, a.K);
  });
  m.def("cast_multi", [](py::list jobs, uintptr_t s) {
    CastJobs j;
    if (jobs.size() > 24) throw std::runtime_error("cast_multi: at most 24 jobs");
    for (auto h : jobs) {
      py::dict d = h.cast<py::dict>();
      j.add(GP(const float, d, "src"), get<int>(d, "R", 0), get<int>(d, "C", 0), GP(u16, d, "dst"),
            GP(u16, d, "dstT"), GP(u16, d, "dstF"), GP(u16, d, "dstTF"));
    }
    cast_multi(j, S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("reduce_slabs_cast", [](py::dict d, uintptr_t s) {   // one slab-sum + cast job
    SlabJobs j;
    j.add_cast(GP(const float, d, "src"), get<int>(d, "splits", 1), get<int>(d, "R", 0), get<int>(d, "C", 0),
               GP(float, d, "dst"), GP(u16, d, "bf"), GP(u16, d, "bfT"));
    reduce_slabs_multi(j, S(s));
    HIP_LAUNCH_CHECK();
  });
  // the optimiser tail: fused Adam/SGD + bf16 refresh, the plain Adam kernel, global-norm clipping,
  // multi-job slab sums, the loss sum and the sharded optimiser's bias pack
  m.def("adam_cast_multi", [](py::dict o, py::list jobs, uintptr_t s) {
    const OptimArgs a = optim_from(o, "adam_cast_multi");
    OptCastJobs j;
    if (jobs.size() > 32) throw std::runtime_error("adam_cast_multi: at most 32 jobs");
    if (jobs.size() == 0) throw std::runtime_error("adam_cast_multi: no jobs");
    bool all_slabs = true;
    for (auto h : jobs) {
      py::dict d = h.cast<py::dict>();
      OptCastJob J{get<long>(d, "off", 0), get<int>(d, "R", 0), get<int>(d, "C", 0), GP(u16, d, "dst"), GP(u16, d, "dstT"),
                   GP(u16, d, "dstF"), GP(u16, d, "dstTF"), GP(const float, d, "gsl"), get<int>(d, "nsl", 0)};
      if (J.off < 0 || J.off % 4) throw std::runtime_error("adam_cast_multi: off must be a non-negative multiple of 4");
      if (J.R < 0 || J.C <= 0) throw std::runtime_error("adam_cast_multi: R >= 0 and C > 0 required");
      if (J.R == 0) {
        if (J.C % 4) throw std::runtime_error("adam_cast_multi: flat job needs C % 4 == 0");
        if (J.dstT || J.dstF || J.dstTF) throw std::runtime_error("adam_cast_multi: a flat job has only the dst copy");
      } else if (J.R % 64 || J.C % 64) {
        throw std::runtime_error("adam_cast_multi: matrix job needs R % 64 == 0 and C % 64 == 0");
      }
      if (J.off + (J.R ? (long)J.R * J.C : (long)J.C) > a.n) throw std::runtime_error("adam_cast_multi: job runs past n");
      if (J.gsl && J.nsl < 1) throw std::runtime_error("adam_cast_multi: gsl needs nsl >= 1");
      all_slabs = all_slabs && J.gsl;
      j.job[j.n++] = J;
    }
    if (!a.g && !(all_slabs && !a.keep_g)) throw std::runtime_error("adam_cast_multi: g required");
    adam_cast_multi(a, j, S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("adam_step", [](py::dict o, uintptr_t s) {   // the plain kernel (shapes off the 64-grid)
    const OptimArgs a = optim_from(o, "adam_step");
    if (!a.g) throw std::runtime_error("adam_step: g required");
    adam_step(a, S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("grad_clip_scale", [](py::dict d, uintptr_t s) {   // scale[0] = min(1, clip / (norm + 1e-6)), scale[1] = norm
    const float* x = GP(const float, d, "x");
    float* parts = GP(float, d, "parts");
    float* scale = GP(float, d, "scale");
    const long n = get<long>(d, "n", 0);
    const int nparts = get<int>(d, "nparts", 0);
    if (!x || !parts || !scale || n < 0 || nparts < 1 || nparts > 4096)
      throw std::runtime_error("grad_clip_scale: x, parts, scale, n >= 0 and 1 <= nparts <= 4096 required");
    sumsq_partials(x, n, parts, nparts, S(s));
    HIP_LAUNCH_CHECK();
    clip_scale_finalize(parts, nparts, get<float>(d, "clip", 0.f), scale, S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("reduce_slabs_multi", [](py::list jobs, uintptr_t bump, uintptr_t s) {
    SlabJobs j;
    if (jobs.size() > 24) throw std::runtime_error("reduce_slabs_multi: at most 24 jobs");
    if (jobs.size() == 0) throw std::runtime_error("reduce_slabs_multi: no jobs");
    for (auto h : jobs) {
      py::dict d = h.cast<py::dict>();
      const float* src = GP(const float, d, "src");
      const int splits = get<int>(d, "splits", 1);
      if (!src || splits < 1) throw std::runtime_error("reduce_slabs_multi: src and splits >= 1 required");
      if (d.contains("bf") || d.contains("bfT") || d.contains("R") || d.contains("C")) {
        const int R = get<int>(d, "R", 0), C = get<int>(d, "C", 0);
        if (!GP(u16, d, "bf") && !GP(u16, d, "bfT")) throw std::runtime_error("reduce_slabs_multi: cast job needs bf or bfT");
        if (R <= 0 || C <= 0) throw std::runtime_error("reduce_slabs_multi: cast job needs R, C > 0");
        j.add_cast(src, splits, R, C, GP(float, d, "dst"), GP(u16, d, "bf"), GP(u16, d, "bfT"));   // R % 16, C % 64: checked below
      } else {
        const long n = get<long>(d, "n", 0);
        if (n < 1 || !GP(float, d, "dst")) throw std::runtime_error("reduce_slabs_multi: plain job needs n >= 1 and dst");
        j.add(src, splits, n, GP(float, d, "dst"));
      }
    }
    j.bump = Pp<int>(bump);
    reduce_slabs_multi(j, S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("sum_partials", [](uintptr_t parts, int n, uintptr_t out, uintptr_t bump, uintptr_t s) {
    if (!parts || !out || n < 0) throw std::runtime_error("sum_partials: parts, out and n >= 0 required");
    sum_partials(Pp<const float>(parts), n, Pp<float>(out), S(s), Pp<int>(bump));
    HIP_LAUNCH_CHECK();
  });
  m.def("flat_pack_u32", [](uintptr_t p, uintptr_t pack, std::vector<std::pair<long, long>> ranges, long lo, long hi,
                            long tail, int unpack, uintptr_t s) {
    if (ranges.size() > 16) throw std::runtime_error("flat_pack_u32: at most 16 ranges");
    if (!p || !pack) throw std::runtime_error("flat_pack_u32: p and pack required");
    FlatRanges r;
    for (const auto& [off, n] : ranges) {
      if (off < 0 || n < 0 || n > (1L << 30)) throw std::runtime_error("flat_pack_u32: bad range");
      r.off[r.cnt] = off;
      r.n[r.cnt++] = (int)n;
    }
    flat_pack_u32(Pp<float>(p), Pp<unsigned>(pack), r, lo, hi, tail, unpack, S(s));
    HIP_LAUNCH_CHECK();
  });
  auto fwd_step_args = [](py::dict d) {
    FwdStepArgs a;
    a.hprev_bf = GP(const u16, d, "hprev_bf"); a.hprev_f = GP(const float, d, "hprev_f");
    a.Whh = GP(const u16, d, "Whh"); a.bhh = GP(const float, d, "bhh");
    a.P = GP(const float, d, "P"); a.ids = GP(const int, d, "ids"); a.Gi = GP(const float, d, "Gi");
    a.x_bf = GP(const u16, d, "x_bf"); a.Wih = GP(const u16, d, "Wih"); a.bih = GP(const float, d, "bih");
    a.Kin = get<int>(d, "Kin", 0);
    a.h_f = GP(float, d, "h_f"); a.h_bf = GP(u16, d, "h_bf"); a.hT = GP(u16, d, "hT");
    a.ldT = get<int>(d, "ldT", 0); a.colT = get<int>(d, "colT", 0);
    a.sr = GP(float, d, "sr"); a.sz = GP(float, d, "sz"); a.sn = GP(float, d, "sn"); a.sghn = GP(float, d, "sghn");
    a.s16 = GP(u16, d, "s16");
    a.Bp = get<int>(d, "Bp", 0); a.H = get<int>(d, "H", 0); a.algo = get<int>(d, "algo", 0);
    if (a.Bp % 32 || a.H % 64) throw std::runtime_error("fwd_step: Bp % 32 and H % 64 required");
    return a;
  };
  auto bwd_step_args = [](py::dict d) {
    BwdStepArgs a;
    a.dgh_next = GP(const u16, d, "dgh_next"); a.WhhT = GP(const u16, d, "WhhT");
    a.carry_in = GP(const float, d, "carry_in"); a.dy = GP(const float, d, "dy");
    a.r = GP(const float, d, "r"); a.z = GP(const float, d, "z"); a.n = GP(const float, d, "n");
    a.ghn = GP(const float, d, "ghn"); a.hprev = GP(const float, d, "hprev");
    a.carry_out = GP(float, d, "carry_out"); a.dgh = GP(u16, d, "dgh"); a.dghT = GP(u16, d, "dghT");
    a.dgiT = GP(u16, d, "dgiT"); a.dgi = GP(u16, d, "dgi");
    a.ldT = get<int>(d, "ldT", 0); a.colT = get<int>(d, "colT", 0);
    a.Bp = get<int>(d, "Bp", 0); a.H = get<int>(d, "H", 0); a.algo = get<int>(d, "algo", 0);
    a.sk_part = GP(float, d, "sk_part"); a.sk_part_floats = get<long>(d, "sk_part_floats", 0);
    a.sk_cnt = GP(unsigned, d, "sk_cnt"); a.sk_cnt_words = get<long>(d, "sk_cnt_words", 0);
    a.err = GP(unsigned, d, "err");
    a.dgiT_n_only = get<int>(d, "dgiT_n_only", 0);
    if (a.Bp % 32 || a.H % 64) throw std::runtime_error("bwd_step: Bp % 32 and H % 64 required");
    return a;
  };
  m.def("fwd_step", [fwd_step_args](py::dict d, uintptr_t s) {
    gru_fwd_step(fwd_step_args(d), S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("bwd_step", [bwd_step_args](py::dict d, uintptr_t s) {
    gru_bwd_step(bwd_step_args(d), S(s));
    HIP_LAUNCH_CHECK();
  });
  // the kernel fwd_step / bwd_step would launch for the same dict (the plan the launcher switches on)
  auto plan_dict = [](const StepPlan& p) {
    py::dict o;
    o["name"] = step_kernel_name(p.kernel);
    o["ks"] = p.ks; o["kb"] = p.kb; o["nks_i"] = p.nks_i; o["splits"] = p.splits; o["sk_map"] = p.sk_map;
    return o;
  };
  m.def("fwd_step_variant", [fwd_step_args, plan_dict](py::dict d) { return plan_dict(gru_fwd_step_plan(fwd_step_args(d))); });
  m.def("bwd_step_variant", [bwd_step_args, plan_dict](py::dict d) { return plan_dict(gru_bwd_step_plan(bwd_step_args(d))); });
  m.def("spin_delay", [](int us, uintptr_t s) { spin_delay(us, S(s)); HIP_LAUNCH_CHECK(); });
  // tests: copy an internal device buffer (Trainer::buffer) into a caller tensor
  m.def("copy_d2d", [](uintptr_t dst, uintptr_t src, size_t bytes) {
    HIP_CHECK(hipMemcpy(reinterpret_cast<void*>(dst), reinterpret_cast<const void*>(src), bytes, hipMemcpyDeviceToDevice));
  });
  m.def("graph_node_probe_detail", &graph_node_probe_detail);
  m.def("graph_node_probe", &graph_node_probe);
  m.def("block_cus", [](int nblocks, int us, uintptr_t s) { block_cus(nblocks, us, S(s)); });
  m.def("xcc_census", [](uintptr_t out, int nblocks, int threads, uintptr_t s) {
    xcc_census(Pp<unsigned>(out), nblocks, threads, S(s)); HIP_LAUNCH_CHECK(); });
  m.def("fwd_seq_supported", &gru_fwd_seq_supported);
  m.def("bwd_step_sk_splits", &gru_bwd_step_sk_splits);
  m.def("step_lds_variants", []() {
    const StepLdsVariants& v = step_lds_variants();
    py::dict d;
    d["fwd64"] = v.fwd64; d["bwd_sk_min_h"] = v.bwd_sk_min_h; d["dwfc_group"] = v.dwfc_group;
    d["bwd_big"] = v.bwd_big; d["bwd16"] = v.bwd16; d["bwd_xring"] = v.bwd_xring; d["fwd_xring"] = v.fwd_xring; d["fwd_fc"] = v.fwd_fc; d["fc_flash"] = v.fc_flash; d["fc_tail"] = v.fc_tail; d["bwd_tail"] = v.bwd_tail; d["fb_one"] = v.fb_one; d["save16"] = v.save16; d["big_dy"] = v.big_dy; d["ld_pad"] = v.ld_pad;
    return d;
  });
  m.def("set_step_lds_variants", [](py::dict d) {
    StepLdsVariants& v = step_lds_variants();
    for (auto kv : d) {
      const std::string k = py::str(kv.first);
      const int x = kv.second.cast<int>();
      if (k == "fwd64") v.fwd64 = x;
      else if (k == "bwd_sk_min_h") v.bwd_sk_min_h = x;
      else if (k == "dwfc_group") v.dwfc_group = x;
      else if (k == "bwd_big") v.bwd_big = x;
      else if (k == "bwd16") v.bwd16 = x;
      else if (k == "bwd_xring") v.bwd_xring = x;
      else if (k == "fwd_xring") v.fwd_xring = x;
      else if (k == "fwd_fc") v.fwd_fc = x;
      else if (k == "fc_flash") v.fc_flash = x;
      else if (k == "fc_tail") v.fc_tail = x;
      else if (k == "bwd_tail") v.bwd_tail = x;
      else if (k == "fb_one") v.fb_one = x;
      else if (k == "big_dy") v.big_dy = x;
      else if (k == "ld_pad") v.ld_pad = x;
      else if (k == "save16") v.save16 = x;
      else throw std::runtime_error("set_step_lds_variants: unknown field " + k);
    }
  });
  m.def("gemm_variants", []() {
    const GemmVariants& v = gemm_variants();
    py::dict d;
    d["mfma"] = v.mfma; d["phased"] = v.phased; d["sched"] = v.sched; d["groupm"] = v.groupm; d["onehot"] = v.onehot;
    d["small_ring"] = v.small_ring;
    return d;
  });
  m.def("set_gemm_variants", [](py::dict d) {
    GemmVariants& v = gemm_variants();
    for (auto kv : d) {
      const std::string k = py::str(kv.first);
      const int x = kv.second.cast<int>();
      if (k == "mfma") v.mfma = x;
      else if (k == "phased") v.phased = x;
      else if (k == "sched") v.sched = x;
      else if (k == "groupm") v.groupm = x;
      else if (k == "onehot") v.onehot = x;
      else if (k == "small_ring") {
        if (x != 0 && x != 3 && x != 4) throw std::runtime_error("set_gemm_variants: small_ring is 0, 3 or 4");
        v.small_ring = x;
      }
      else throw std::runtime_error("set_gemm_variants: unknown field " + k);
    }
  });
  m.def("bwd_seq_supported", &gru_bwd_seq_supported);
  m.def("fwd_seq2", [](py::dict lo, py::dict hi, uintptr_t Wih, uintptr_t bih, uintptr_t s) {
    auto parse = [](py::dict d) {
      SeqFwdArgs a;
      a.HSb = GP(u16, d, "HSb"); a.HSf = GP(float, d, "HSf"); a.HT = GP(u16, d, "HT"); a.ldT = get<int>(d, "ldT", 0);
      a.HF = GP(u16, d, "HF"); a.xch = GP(u16, d, "xch");
      a.sr = GP(float, d, "sr"); a.sz = GP(float, d, "sz"); a.sn = GP(float, d, "sn"); a.sghn = GP(float, d, "sghn");
      a.Whh = GP(const u16, d, "Whh"); a.bhh = GP(const float, d, "bhh");
      a.P = GP(const float, d, "P"); a.ids = GP(const int, d, "ids"); a.Gi = GP(const float, d, "Gi");
      a.h0 = GP(const float, d, "h0");
      a.cnt = GP(unsigned, d, "cnt"); a.err = GP(unsigned, d, "err");
      a.dbg = GP(unsigned long long, d, "dbg"); a.allow_local = get<int>(d, "allow_local", 1);
      a.xring = get<int>(d, "xring", 0);
      a.s16 = GP(u16, d, "s16");
      a.zero_next = GP(unsigned, d, "zero_next"); a.zero_words = get<long>(d, "zero_words", 0);
      a.T = get<int>(d, "T", 0); a.Bp = get<int>(d, "Bp", 0); a.H = get<int>(d, "H", 0);
      if (!a.xch || !a.cnt || !a.HSb || !a.HSf || !a.Whh || !a.bhh) throw std::runtime_error("fwd_seq2: HSb/HSf/xch/cnt/Whh/bhh required");
      return a;
    };
    SeqFwd2Args a;
    a.lo = parse(lo); a.hi = parse(hi);
    a.Wih = reinterpret_cast<const u16*>(Wih); a.bih = reinterpret_cast<const float*>(bih);
    if (!a.lo.ids == !a.lo.Gi) throw std::runtime_error("fwd_seq2: lo needs exactly one of P+ids / Gi");
    if (!gru_fwd_seq2_supported(a.lo.H, a.lo.Bp)) throw std::runtime_error("fwd_seq2: shape not supported");
    gru_fwd_seq2(a, S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("fwd_seq2_supported", &gru_fwd_seq2_supported);
  m.def("fwd_seq_fc_supported", &gru_fwd_seq_fc_supported);
  m.def("fwd_seq_fc", [](py::dict d, py::dict fd, uintptr_t s) {
    SeqFwdArgs a;
    a.HSb = GP(u16, d, "HSb"); a.HSf = GP(float, d, "HSf"); a.HT = GP(u16, d, "HT"); a.ldT = get<int>(d, "ldT", 0);
    a.HF = GP(u16, d, "HF"); a.xch = GP(u16, d, "xch");
    a.sr = GP(float, d, "sr"); a.sz = GP(float, d, "sz"); a.sn = GP(float, d, "sn"); a.sghn = GP(float, d, "sghn");
    a.Whh = GP(const u16, d, "Whh"); a.bhh = GP(const float, d, "bhh");
    a.P = GP(const float, d, "P"); a.ids = GP(const int, d, "ids"); a.Gi = GP(const float, d, "Gi");
    a.h0 = GP(const float, d, "h0");
    a.cnt = GP(unsigned, d, "cnt"); a.err = GP(unsigned, d, "err");
    a.dbg = GP(unsigned long long, d, "dbg"); a.allow_local = get<int>(d, "allow_local", 1);
    a.xring = get<int>(d, "xring", 0);
    a.T = get<int>(d, "T", 0); a.Bp = get<int>(d, "Bp", 0); a.H = get<int>(d, "H", 0);
    SeqFcArgs f;
    f.Wf = GP(const u16, fd, "Wf"); f.WTf = GP(const u16, fd, "WTf"); f.b = GP(const float, fd, "b");
    f.labels = GP(const int, fd, "labels"); f.inv_count = GP(const float, fd, "inv_count");
    f.dy = GP(float, fd, "dy"); f.dlF = GP(u16, fd, "dlF"); f.loss_part = GP(float, fd, "loss_part");
    f.dW = GP(float, fd, "dW"); f.db = GP(float, fd, "db"); f.V = get<int>(fd, "V", 0);
    f.probe = get<int>(fd, "probe", 0);
    if (!a.xch || !a.cnt || !a.HSb || !a.HSf || !a.Whh || !a.bhh) throw std::runtime_error("fwd_seq_fc: HSb/HSf/xch/cnt/Whh/bhh required");
    if (!gru_fwd_seq_fc_supported(a.H, a.Bp, f.V)) throw std::runtime_error("fwd_seq_fc: shape not supported");
    gru_fwd_seq_fc(a, f, S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("fwd_seq", [](py::dict d, uintptr_t s) {
    SeqFwdArgs a;
    a.HSb = GP(u16, d, "HSb"); a.HSf = GP(float, d, "HSf"); a.HT = GP(u16, d, "HT"); a.ldT = get<int>(d, "ldT", 0);
    a.HF = GP(u16, d, "HF");
    a.xch = GP(u16, d, "xch");
    if (!a.xch) throw std::runtime_error("fwd_seq: exchange buffer xch [T][Bp][H] bf16 required");
    a.sr = GP(float, d, "sr"); a.sz = GP(float, d, "sz"); a.sn = GP(float, d, "sn"); a.sghn = GP(float, d, "sghn");
    a.Whh = GP(const u16, d, "Whh"); a.bhh = GP(const float, d, "bhh");
    a.P = GP(const float, d, "P"); a.ids = GP(const int, d, "ids"); a.Gi = GP(const float, d, "Gi");
    a.h0 = GP(const float, d, "h0");
    a.cnt = GP(unsigned, d, "cnt"); a.err = GP(unsigned, d, "err");
    a.dbg = GP(unsigned long long, d, "dbg"); a.allow_local = get<int>(d, "allow_local", 1);
    a.xring = get<int>(d, "xring", 0);
    a.s16 = GP(u16, d, "s16");
    a.zero_next = GP(unsigned, d, "zero_next"); a.zero_words = get<long>(d, "zero_words", 0);
    a.T = get<int>(d, "T", 0); a.Bp = get<int>(d, "Bp", 0); a.H = get<int>(d, "H", 0);
    if (!gru_fwd_seq_supported(a.H, a.Bp)) throw std::runtime_error("fwd_seq: shape not supported");
    gru_fwd_seq(a, S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("bwd_seq_big_supported", &gru_bwd_seq_big_supported);
  m.def("bwd_seq_big_part_floats", &gru_bwd_seq_big_part_floats);
  m.def("bwd_seq16_supported", &gru_bwd_seq16_supported);
  m.def("seq_flag_words", &seq_flag_words);
  m.def("bwd_seq", [](py::dict d, uintptr_t s) {
    SeqBwdArgs a;
    a.dy = GP(const float, d, "dy");
    a.sr = GP(const float, d, "sr"); a.sz = GP(const float, d, "sz"); a.sn = GP(const float, d, "sn");
    a.sghn = GP(const float, d, "sghn"); a.HSf = GP(const float, d, "HSf");
    a.HT = GP(const u16, d, "HT"); a.ldT = get<int>(d, "ldT", 0); a.WhhT = GP(const u16, d, "WhhT");
    a.HF = GP(const u16, d, "HF");
    a.xbuf = GP(u16, d, "xbuf"); a.dghT = GP(u16, d, "dghT"); a.dgiT = GP(u16, d, "dgiT");
    a.ldG = get<int>(d, "ldG", 0); a.dgi = GP(u16, d, "dgi");
    a.dWhh_part = GP(float, d, "dWhh_part"); a.dbhh_part = GP(float, d, "dbhh_part");
    a.dbih_part = GP(float, d, "dbih_part"); a.ids = GP(const int, d, "ids");
    a.dP_part = GP(float, d, "dP_part"); a.V = get<int>(d, "V", 0);
    a.cnt = GP(unsigned, d, "cnt"); a.err = GP(unsigned, d, "err"); a.dbg = GP(unsigned long long, d, "dbg");
    a.allow_local = get<int>(d, "allow_local", 1); a.xring = get<int>(d, "xring", 0);
    a.s16 = GP(const u16, d, "s16"); a.part = GP(float, d, "part");
    a.dl = GP(const u16, d, "dl"); a.WfcT = GP(const u16, d, "WfcT");
    a.dgiT_n_only = get<int>(d, "dgiT_n_only", 0);
    a.zero_next = GP(unsigned, d, "zero_next"); a.zero_words = get<long>(d, "zero_words", 0);
    a.T = get<int>(d, "T", 0); a.Bp = get<int>(d, "Bp", 0); a.H = get<int>(d, "H", 0);
    if (get<int>(d, "big", 0)) {   // the large-H split-K backward (gru_seq_big.hip): its own argument checks throw
      gru_bwd_seq_big(a, S(s));
      HIP_LAUNCH_CHECK();
      return;
    }
    // "unchecked": skip the co-residency query and go straight to the dispatch table (tests its
    // unmatched-variant error without launching anything)
    if (get<int>(d, "rows16", 0)) {   // the 16-row-block backward (gru_seq16.hip)
      if (!gru_bwd_seq16_supported(a.H, a.Bp, a.dP_part != nullptr)) throw std::runtime_error("bwd_seq(rows16): shape not supported");
      gru_bwd_seq16(a, S(s));
      HIP_LAUNCH_CHECK();
      return;
    }
    if (!get<int>(d, "unchecked", 0) &&
        !gru_bwd_seq_supported(a.H, a.Bp, a.dWhh_part != nullptr, a.dP_part != nullptr))
      throw std::runtime_error("bwd_seq: shape not supported");
    gru_bwd_seq(a, S(s));
    HIP_LAUNCH_CHECK();
  });
  auto fc_xent_args = [](const py::dict& d) {
    FcXentArgs a;
    a.X = GP(const u16, d, "X"); a.W = GP(const u16, d, "W"); a.b = GP(const float, d, "b");
    a.labels = GP(const int, d, "labels"); a.inv_count = GP(const float, d, "inv_count");
    a.dl = GP(u16, d, "dl"); a.dlT = GP(u16, d, "dlT"); a.loss_part = GP(float, d, "loss_part");
    a.M = get<int>(d, "M", 0); a.H = get<int>(d, "H", 0); a.V = get<int>(d, "V", 0);
    a.ldT = get<int>(d, "ldT", 0); a.colT = get<int>(d, "colT", 0);
    a.WT = GP(const u16, d, "WT"); a.dy = GP(float, d, "dy");
    a.dbg = GP(unsigned long long, d, "dbg");
    a.Wf = GP(const u16, d, "Wf"); a.WTf = GP(const u16, d, "WTf");
    return a;
  };
  m.def("fc_xent", [fc_xent_args](py::dict d, uintptr_t s) {
    const FcXentArgs a = fc_xent_args(d);
    if (a.M % 32 || a.V % 64 || a.V > 512 || a.H % 32 || a.ldT % 8 || a.colT % 8)
      throw std::runtime_error("fc_xent: bad shape");
    fc_xent(a, S(s));
    HIP_LAUNCH_CHECK();
  });
  // the one-layer persistent forward with the fused FC head as its tail: the fwd_seq dict and the fc_xent
  // dict (X = HSb + Bp * H, M = T * Bp, fused dH); scripts/probe_seq.py TAIL=1
  m.def("fwd_seq_tail_supported", &gru_fwd_seq_tail_supported);
  m.def("fwd_seq_tail", [fc_xent_args](py::dict d, py::dict fd, uintptr_t s) {
    SeqFwdArgs a;
    a.HSb = GP(u16, d, "HSb"); a.HSf = GP(float, d, "HSf"); a.HT = GP(u16, d, "HT"); a.ldT = get<int>(d, "ldT", 0);
    a.HF = GP(u16, d, "HF"); a.xch = GP(u16, d, "xch");
    a.sr = GP(float, d, "sr"); a.sz = GP(float, d, "sz"); a.sn = GP(float, d, "sn"); a.sghn = GP(float, d, "sghn");
    a.Whh = GP(const u16, d, "Whh"); a.bhh = GP(const float, d, "bhh");
    a.P = GP(const float, d, "P"); a.ids = GP(const int, d, "ids"); a.Gi = GP(const float, d, "Gi");
    a.h0 = GP(const float, d, "h0");
    a.cnt = GP(unsigned, d, "cnt"); a.err = GP(unsigned, d, "err");
    a.dbg = GP(unsigned long long, d, "dbg"); a.allow_local = get<int>(d, "allow_local", 1);
    a.xring = get<int>(d, "xring", 0);
    a.s16 = GP(u16, d, "s16");
    a.zero_next = GP(unsigned, d, "zero_next"); a.zero_words = get<long>(d, "zero_words", 0);
    a.T = get<int>(d, "T", 0); a.Bp = get<int>(d, "Bp", 0); a.H = get<int>(d, "H", 0);
    const FcXentArgs f = fc_xent_args(fd);
    if (!a.xch || !a.cnt || !a.HSb || !a.HSf || !a.Whh || !a.bhh) throw std::runtime_error("fwd_seq_tail: HSb/HSf/xch/cnt/Whh/bhh required");
    if (!gru_fwd_seq_tail_supported(a.H, a.Bp, f.V)) throw std::runtime_error("fwd_seq_tail: shape not supported");
    gru_fwd_seq_tail(a, f, S(s));
    HIP_LAUNCH_CHECK();
  });
  // the row-wise softmax-xent of the large-H plans on caller-made fp32 logits [M][V]: the fc_xent dict
  // without X / W / b / H; softmax_xent itself throws on a shape it does not serve
  m.def("softmax_xent", [fc_xent_args](uintptr_t logits, py::dict d, uintptr_t s) {
    const FcXentArgs a = fc_xent_args(d);
    if (!logits || !a.labels || !a.inv_count || !a.dlT || !a.loss_part || a.M <= 0 || a.V <= 0 ||
        a.ldT < a.colT + a.M)
      throw std::runtime_error("softmax_xent: logits, labels, inv_count, dlT, loss_part and ldT >= colT + M required");
    softmax_xent(reinterpret_cast<const float*>(logits), a, S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("fc_sample", [](py::dict d, uintptr_t s) {
    FcSampleArgs a;
    a.X = GP(const u16, d, "X"); a.W = GP(const u16, d, "W"); a.b = GP(const float, d, "b");
    a.Wf = GP(const u16, d, "Wf");
    a.rf = GP(const float, d, "rf"); a.ids = GP(int, d, "ids"); a.out = GP(unsigned char, d, "out");
    a.alive = GP(int, d, "alive"); a.probs = GP(float, d, "probs");
    a.N = get<int>(d, "N", 0); a.Bp = get<int>(d, "Bp", 0); a.H = get<int>(d, "H", 0); a.V = get<int>(d, "V", 0);
    a.step = get<int>(d, "step", 0); a.max_len = get<int>(d, "max_len", 0); a.eos = get<int>(d, "eos", 0);
    if (a.Bp % 32 || a.V % 64 || a.V > 512 || a.H % 32) throw std::runtime_error("fc_sample: bad shape");
    fc_sample(a, S(s));
    HIP_LAUNCH_CHECK();
  });
  // the fp32 path's samplers on caller-made logits: sample_f32, and sample_ctl with the per-row controls
  auto sample_args = [](const py::dict& d) {
    SampleF32Args a;
    a.logits = GP(const float, d, "logits"); a.splits = get<int>(d, "splits", 1); a.slab = get<long>(d, "slab", 0);
    a.bias = GP(const float, d, "bias"); a.rf = GP(const float, d, "rf"); a.ids = GP(int, d, "ids");
    a.out = GP(unsigned char, d, "out"); a.alive = GP(int, d, "alive"); a.probs = GP(float, d, "probs");
    a.N = get<int>(d, "N", 0); a.V = get<int>(d, "V", 0); a.step = get<int>(d, "step", 0);
    a.max_len = get<int>(d, "max_len", 0); a.eos = get<int>(d, "eos", 0);
    if (!a.logits || !a.rf || !a.ids || !a.out || !a.alive || a.N < 0 || a.splits < 1 || a.step < 0 ||
        a.step >= a.max_len || (a.splits > 1 && a.slab < (long)a.N * a.V))
      throw std::runtime_error("sample: logits, rf, ids, out, alive, 0 <= step < max_len and slab >= N * V required");
    return a;
  };
  m.def("sample_f32", [sample_args](py::dict d, uintptr_t s) {
    sample_f32(sample_args(d), S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("sample_ctl", [sample_args](py::dict d, uintptr_t s) {
    SampleCtlArgs c;
    c.s = sample_args(d);
    c.inv_temp = GP(const float, d, "inv_temp"); c.top_k = GP(const int, d, "top_k");
    c.top_p = GP(const float, d, "top_p"); c.plen = GP(const int, d, "plen");
    c.prefix = GP(const unsigned char, d, "prefix"); c.row0 = get<int>(d, "row0", 0); c.err = GP(unsigned, d, "err");
    c.allow_tab = GP(const unsigned, d, "allow_tab"); c.allow_idx = GP(const int, d, "allow_idx");
    c.allow_rows = get<int>(d, "allow_rows", 0);
    c.allow_state = GP(int, d, "allow_state"); c.allow_next = GP(const unsigned short, d, "allow_next");
    c.soft_tab = GP(const float, d, "soft_tab"); c.soft_idx = GP(const int, d, "soft_idx");
    c.soft_rows = get<int>(d, "soft_rows", 0);
    c.soft_pres = GP(const float, d, "soft_pres"); c.soft_freq = GP(const float, d, "soft_freq");
    sample_ctl_f32(c, S(s));
    HIP_LAUNCH_CHECK();
  });
  // the generation path's kernels on caller-owned buffers (tests/test_gen_gpu.py): the persistent
  // launch with its workspace (layout: kernels.h, GenPersistArgs::ws), the fp32 gates, the batch
  // reset and the scorer's two kernels
  m.def("gen_persist_supported", &gen_persist_supported);
  m.def("gen_persist_ctl_supported", &gen_persist_ctl_supported);
  m.def("gen_persist_con_supported", &gen_persist_con_supported);
  m.def("gen_persist_soft_supported", &gen_persist_soft_supported);
  m.def("gen_persist_con_bytes", []() { return (long)sizeof(GenPersistCon); });
  m.def("gen_persist_ws_floats", &gen_persist_ws_floats);
  m.def("gen_persist_sync_words", &gen_persist_sync_words);
  m.def("gen_persist_fill_ws", [](uintptr_t ws, int H, int L, int V, int ML, uintptr_t s) {
    if (!ws) throw std::runtime_error("gen_persist_fill_ws: ws required");
    gen_persist_fill_ws(Pp<float>(ws), H, L, V, ML, S(s));
  });
  m.def("gen_persist", [](py::dict d, uintptr_t s) {
    GenPersistArgs a;
    a.N = get<int>(d, "N", 0); a.H = get<int>(d, "H", 0); a.L = get<int>(d, "L", 0); a.V = get<int>(d, "V", 0);
    a.ML = get<int>(d, "ML", 0); a.sos = get<int>(d, "sos", 0); a.eos = get<int>(d, "eos", 0);
    a.par = get<int>(d, "par", 0);
    if (a.L < 1 || a.L > 4) throw std::runtime_error("gen_persist: 1 <= L <= 4");
    if (a.sos < 0 || a.sos >= a.V) throw std::runtime_error("gen_persist: 0 <= sos < V");
    auto ptrs = [&](const char* k, const float* (&dst)[4], int first) {
      const auto v = get<std::vector<uintptr_t>>(d, k, {});
      if ((int)v.size() != a.L) throw std::runtime_error(std::string("gen_persist: ") + k + " needs L pointers");
      for (int l = first; l < a.L; ++l) dst[l] = Pp<const float>(v[l]);
    };
    ptrs("Whh", a.Whh, 0); ptrs("bhh", a.bhh, 0); ptrs("Wih", a.Wih, 1); ptrs("bih", a.bih, 1);
    a.Wfc = GP(const float, d, "Wfc"); a.bfc = GP(const float, d, "bfc"); a.P = GP(const float, d, "P");
    a.rf = GP(const float, d, "rf"); a.out = GP(unsigned char, d, "out"); a.probs = GP(float, d, "probs");
    a.ws = GP(float, d, "ws"); a.sync = GP(unsigned, d, "sync"); a.err = GP(unsigned, d, "err");
    // sampling controls (all five or none: gen_persist_f32 throws on a mixture)
    a.inv_temp = GP(const float, d, "inv_temp"); a.top_k = GP(const int, d, "top_k");
    a.top_p = GP(const float, d, "top_p"); a.plen = GP(const int, d, "plen");
    a.prefix = GP(const unsigned char, d, "prefix");
    // constraints (SampleCtlArgs' fields and rules: gen_persist_con_mode throws on an inconsistent set):
    // stored into the caller's device struct `con` (gen_persist_con_bytes) in stream order, then the launch
    GenPersistCon h;
    h.allow_tab = GP(const unsigned, d, "allow_tab"); h.allow_idx = GP(const int, d, "allow_idx");
    h.allow_next = GP(const unsigned short, d, "allow_next"); h.allow_start = GP(const int, d, "allow_start");
    h.allow_state = GP(int, d, "allow_state"); h.allow_rows = get<int>(d, "allow_rows", 0);
    // soft controls (SampleCtlArgs' five keys; gen_persist_soft_check throws on an inconsistent set): further
    // fields of the same struct
    h.soft_tab = GP(const float, d, "soft_tab"); h.soft_idx = GP(const int, d, "soft_idx");
    h.soft_rows = get<int>(d, "soft_rows", 0);
    h.soft_pres = GP(const float, d, "soft_pres"); h.soft_freq = GP(const float, d, "soft_freq");
    a.con_mode = gen_persist_con_mode(h);
    a.soft = gen_persist_soft_check(h) ? 1 : 0;
    if (a.con_mode != kGenConNone || a.soft) {
      GenPersistCon* dev = GP(GenPersistCon, d, "con");
      if (!dev) throw std::runtime_error("gen_persist: a constrained or soft launch needs `con`, gen_persist_con_bytes() of device memory");
      if (!a.inv_temp || !a.top_k || !a.top_p || !a.plen || !a.prefix)
        throw std::runtime_error("gen_persist: constraints and soft controls go with the five sampling controls");
      gen_persist_con_store(dev, h, S(s));
      a.con = dev;
    }
    gen_persist_f32(a, S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("gru_gates_f32", [](py::dict d, uintptr_t s) {
    GruGatesF32Args a;
    a.P = GP(const float, d, "P"); a.ids = GP(const int, d, "ids"); a.Gi = GP(const float, d, "Gi");
    a.Gh = GP(const float, d, "Gh");
    a.gi_splits = get<int>(d, "gi_splits", 1); a.gh_splits = get<int>(d, "gh_splits", 1);
    a.gi_slab = get<long>(d, "gi_slab", 0); a.gh_slab = get<long>(d, "gh_slab", 0);
    a.hprev = GP(const float, d, "hprev"); a.hout = GP(float, d, "hout");
    a.Bp = get<int>(d, "Bp", 0); a.H = get<int>(d, "H", 0); a.V = get<int>(d, "V", 0);
    a.err = GP(unsigned, d, "err"); a.bgh = GP(const float, d, "bgh"); a.bgi = GP(const float, d, "bgi");
    a.hsplit = GP(unsigned short, d, "hsplit");
    const long row = 3L * a.H * a.Bp;
    if (a.Bp <= 0 || a.H <= 0 || !a.Gh || !a.hprev || !a.hout || (a.P ? !a.ids || a.V <= 0 : !a.Gi) ||
        a.gi_splits < 1 || a.gh_splits < 1 || (a.gh_splits > 1 && a.gh_slab < row) ||
        (!a.P && a.gi_splits > 1 && a.gi_slab < row))
      throw std::runtime_error("gru_gates_f32: Gh, hprev, hout, (P, ids, V) or Gi, and slabs >= Bp * 3H required");
    gru_gates_f32(a, S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("gen_reset", [](py::dict d, uintptr_t s) {
    GenResetArgs a;
    a.L = get<int>(d, "L", 0); a.Bp = get<int>(d, "Bp", 0); a.H = get<int>(d, "H", 0); a.ML = get<int>(d, "ML", 0);
    a.sos = get<int>(d, "sos", 0); a.hb_cols = get<int>(d, "hb_cols", 0);
    const auto hf = get<std::vector<uintptr_t>>(d, "hf", {}), hb = get<std::vector<uintptr_t>>(d, "hb", {});
    if (a.L < 1 || a.L > 4 || (int)hf.size() != a.L || (!hb.empty() && (int)hb.size() != a.L))
      throw std::runtime_error("gen_reset: 1 <= L <= 4, L hf pointers and no or L hb pointers");
    for (int l = 0; l < a.L; ++l) {
      a.hf[l] = Pp<float>(hf[l]);
      if (!hb.empty()) a.hb[l] = Pp<unsigned short>(hb[l]);
      if (!a.hf[l]) throw std::runtime_error("gen_reset: null hf");
    }
    a.ids = GP(int, d, "ids"); a.alive = GP(int, d, "alive"); a.out = GP(unsigned char, d, "out");
    if (!a.ids || !a.alive || !a.out || a.Bp <= 0 || a.H <= 0 || a.ML <= 0)
      throw std::runtime_error("gen_reset: ids, alive, out, Bp, H, ML required");
    gen_reset(a, S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("score_set_count", [](uintptr_t n_dev, int n, uintptr_t s) {
    if (!n_dev) throw std::runtime_error("score_set_count: n_dev required");
    score_set_count(Pp<int>(n_dev), n, S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("score_prep", [](py::dict d, uintptr_t s) {
    ScorePrepArgs a;
    a.rows = GP(const unsigned char, d, "rows"); a.n_dev = GP(const int, d, "n_dev");
    a.ids = GP(int, d, "ids"); a.tgt = GP(int, d, "tgt"); a.ntok = GP(int, d, "ntok"); a.err = GP(unsigned, d, "err");
    a.N = get<int>(d, "N", 0); a.Bp = get<int>(d, "Bp", 0); a.ML = get<int>(d, "ML", 0); a.V = get<int>(d, "V", 0);
    a.sos = get<int>(d, "sos", 0); a.eos = get<int>(d, "eos", 0);
    if (!a.rows || !a.ids || !a.tgt || !a.ntok || a.N < 0 || a.N > a.Bp)
      throw std::runtime_error("score_prep: rows, ids, tgt, ntok and 0 <= N <= Bp required");
    score_prep(a, S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("score_logprob", [](py::dict d, uintptr_t s) {
    ScoreLogprobArgs a;
    a.logits = GP(const float, d, "logits"); a.splits = get<int>(d, "splits", 1); a.slab = get<long>(d, "slab", 0);
    a.bias = GP(const float, d, "bias"); a.tgt = GP(const int, d, "tgt"); a.ntok = GP(const int, d, "ntok");
    a.tok_logp = GP(float, d, "tok_logp"); a.rank = GP(int, d, "rank"); a.name_logp = GP(float, d, "name_logp");
    a.ntok_out = GP(int, d, "ntok_out");
    a.Bp = get<int>(d, "Bp", 0); a.V = get<int>(d, "V", 0); a.ML = get<int>(d, "ML", 0);
    if (!a.logits || !a.tgt || !a.ntok || !a.tok_logp || !a.rank || !a.name_logp || !a.ntok_out)
      throw std::runtime_error("score_logprob: logits, tgt, ntok, tok_logp, rank, name_logp, ntok_out required");
    score_logprob_f32(a, S(s));
    HIP_LAUNCH_CHECK();
  });
  // score_logprob under the sampler's controls and constraints (tests/test_score_ctl_gpu.py)
  m.def("score_ctl_logprob", [](py::dict d, uintptr_t s) {
    ScoreCtlArgs c;
    ScoreLogprobArgs& a = c.s;
    a.logits = GP(const float, d, "logits"); a.splits = get<int>(d, "splits", 1); a.slab = get<long>(d, "slab", 0);
    a.bias = GP(const float, d, "bias"); a.tgt = GP(const int, d, "tgt"); a.ntok = GP(const int, d, "ntok");
    a.tok_logp = GP(float, d, "tok_logp"); a.rank = GP(int, d, "rank"); a.name_logp = GP(float, d, "name_logp");
    a.ntok_out = GP(int, d, "ntok_out");
    a.Bp = get<int>(d, "Bp", 0); a.V = get<int>(d, "V", 0); a.ML = get<int>(d, "ML", 0);
    if (!a.logits || !a.tgt || !a.ntok || !a.tok_logp || !a.rank || !a.name_logp || !a.ntok_out)
      throw std::runtime_error("score_ctl_logprob: logits, tgt, ntok, tok_logp, rank, name_logp, ntok_out required");
    c.inv_temp = GP(const float, d, "inv_temp"); c.top_k = GP(const int, d, "top_k");
    c.top_p = GP(const float, d, "top_p"); c.plen = GP(const int, d, "plen");
    c.prefix = GP(const unsigned char, d, "prefix"); c.row0 = get<int>(d, "row0", 0); c.err = GP(unsigned, d, "err");
    c.allow_tab = GP(const unsigned, d, "allow_tab"); c.allow_idx = GP(const int, d, "allow_idx");
    c.allow_rows = get<int>(d, "allow_rows", 0); c.n_kept = GP(int, d, "n_kept");
    c.soft_tab = GP(const float, d, "soft_tab"); c.soft_idx = GP(const int, d, "soft_idx");
    c.soft_rows = get<int>(d, "soft_rows", 0);
    c.soft_pres = GP(const float, d, "soft_pres"); c.soft_freq = GP(const float, d, "soft_freq");
    score_ctl_logprob_f32(c, S(s));
    HIP_LAUNCH_CHECK();
  });
  // the beam search's kernels on caller-owned buffers (tests/test_beam_gpu.py)
  m.def("beam_select", [](py::dict d, uintptr_t s) {
    BeamSelectArgs a;
    a.logits = GP(const float, d, "logits"); a.splits = get<int>(d, "splits", 1); a.slab = get<long>(d, "slab", 0);
    a.bias = GP(const float, d, "bias"); a.score_in = GP(const float, d, "score_in"); a.state_in = GP(const int, d, "state_in");
    a.plen = GP(const int, d, "plen"); a.prefix = GP(const unsigned char, d, "prefix");
    a.score_out = GP(float, d, "score_out"); a.parent = GP(int, d, "parent"); a.chr = GP(int, d, "chr");
    a.state_out = GP(int, d, "state_out"); a.next_id = GP(int, d, "next_id");
    a.lp = GP(float, d, "lp"); a.sel = GP(int, d, "sel"); a.err = GP(unsigned, d, "err");
    a.N = get<int>(d, "N", 0); a.W = get<int>(d, "W", 0); a.V = get<int>(d, "V", 0); a.step = get<int>(d, "step", 0);
    a.max_len = get<int>(d, "max_len", 0); a.sos = get<int>(d, "sos", 0); a.eos = get<int>(d, "eos", 0);
    a.allow_tab = GP(const unsigned, d, "allow_tab"); a.allow_idx = GP(const int, d, "allow_idx");
    a.allow_rows = get<int>(d, "allow_rows", 0);
    a.allow_state_in = GP(const int, d, "allow_state_in"); a.allow_state_out = GP(int, d, "allow_state_out");
    a.allow_next = GP(const unsigned short, d, "allow_next");
    beam_select_f32(a, S(s));
    HIP_LAUNCH_CHECK();
  });
  // the stochastic beam search's selection on caller-owned buffers (tests/test_sbs_gpu.py)
  m.def("sbs_select", [](py::dict d, uintptr_t s) {
    SbsSelectArgs a;
    a.logits = GP(const float, d, "logits"); a.splits = get<int>(d, "splits", 1); a.slab = get<long>(d, "slab", 0);
    a.bias = GP(const float, d, "bias"); a.logq_in = GP(const float, d, "logq_in"); a.G_in = GP(const float, d, "G_in");
    a.state_in = GP(const int, d, "state_in"); a.plen = GP(const int, d, "plen");
    a.prefix = GP(const unsigned char, d, "prefix");
    a.seed = GP(const unsigned long long, d, "seed"); a.start = GP(const unsigned long long, d, "start");
    a.inv_t = GP(const float, d, "inv_t");
    a.logq_out = GP(float, d, "logq_out"); a.G_out = GP(float, d, "G_out"); a.parent = GP(int, d, "parent");
    a.chr = GP(int, d, "chr"); a.state_out = GP(int, d, "state_out"); a.next_id = GP(int, d, "next_id");
    a.lq = GP(float, d, "lq"); a.gt = GP(float, d, "gt"); a.zmax = GP(float, d, "zmax"); a.sel = GP(int, d, "sel");
    a.err = GP(unsigned, d, "err");
    a.N = get<int>(d, "N", 0); a.W = get<int>(d, "W", 0); a.V = get<int>(d, "V", 0); a.step = get<int>(d, "step", 0);
    a.max_len = get<int>(d, "max_len", 0); a.sos = get<int>(d, "sos", 0); a.eos = get<int>(d, "eos", 0);
    a.allow_tab = GP(const unsigned, d, "allow_tab"); a.allow_idx = GP(const int, d, "allow_idx");
    a.allow_rows = get<int>(d, "allow_rows", 0);
    a.allow_state_in = GP(const int, d, "allow_state_in"); a.allow_state_out = GP(int, d, "allow_state_out");
    a.allow_next = GP(const unsigned short, d, "allow_next");
    sbs_select_f32(a, S(s));
    HIP_LAUNCH_CHECK();
  });
  // the sequential Monte Carlo selection on caller-owned buffers (tests/test_smc_gpu.py)
  m.def("smc_select", [](py::dict d, uintptr_t s) {
    SmcSelectArgs a;
    a.logits = GP(const float, d, "logits"); a.splits = get<int>(d, "splits", 1); a.slab = get<long>(d, "slab", 0);
    a.bias = GP(const float, d, "bias"); a.logw_in = GP(const float, d, "logw_in"); a.logq_in = GP(const float, d, "logq_in");
    a.state_in = GP(const int, d, "state_in"); a.plen = GP(const int, d, "plen");
    a.prefix = GP(const unsigned char, d, "prefix");
    a.seed = GP(const unsigned long long, d, "seed"); a.start = GP(const unsigned long long, d, "start");
    a.thr = GP(const float, d, "thr"); a.inv_t = GP(const float, d, "inv_t");
    a.logw_out = GP(float, d, "logw_out"); a.logq_out = GP(float, d, "logq_out"); a.parent = GP(int, d, "parent");
    a.chr = GP(int, d, "chr"); a.state_out = GP(int, d, "state_out"); a.next_id = GP(int, d, "next_id");
    a.n_res = GP(int, d, "n_res"); a.logm = GP(float, d, "logm"); a.lq = GP(float, d, "lq"); a.ess = GP(float, d, "ess");
    a.err = GP(unsigned, d, "err");
    a.N = get<int>(d, "N", 0); a.W = get<int>(d, "W", 0); a.V = get<int>(d, "V", 0); a.step = get<int>(d, "step", 0);
    a.max_len = get<int>(d, "max_len", 0); a.sos = get<int>(d, "sos", 0); a.eos = get<int>(d, "eos", 0);
    a.allow_tab = GP(const unsigned, d, "allow_tab"); a.allow_idx = GP(const int, d, "allow_idx");
    a.allow_rows = get<int>(d, "allow_rows", 0);
    a.allow_state_in = GP(const int, d, "allow_state_in"); a.allow_state_out = GP(int, d, "allow_state_out");
    a.allow_next = GP(const unsigned short, d, "allow_next");
    smc_select_f32(a, S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("beam_reorder", [](py::dict d, uintptr_t s) {
    BeamReorderArgs a;
    a.N = get<int>(d, "N", 0); a.W = get<int>(d, "W", 0); a.L = get<int>(d, "L", 0); a.H = get<int>(d, "H", 0);
    a.max_len = get<int>(d, "max_len", 0);
    const auto hs = get<std::vector<uintptr_t>>(d, "h_src", {}), hd = get<std::vector<uintptr_t>>(d, "h_dst", {});
    if (a.L < 1 || a.L > 4 || (int)hs.size() != a.L || (int)hd.size() != a.L)
      throw std::runtime_error("beam_reorder: 1 <= L <= 4, L h_src and L h_dst pointers");
    for (int l = 0; l < a.L; ++l) { a.h_src[l] = Pp<const float>(hs[l]); a.h_dst[l] = Pp<float>(hd[l]); }
    a.parent = GP(const int, d, "parent"); a.chr = GP(const int, d, "chr"); a.next_id = GP(const int, d, "next_id");
    a.rows_src = GP(const unsigned char, d, "rows_src"); a.rows_dst = GP(unsigned char, d, "rows_dst");
    a.len_src = GP(const int, d, "len_src"); a.len_dst = GP(int, d, "len_dst");
    a.ids = GP(int, d, "ids"); a.n_beams = GP(int, d, "n_beams");
    beam_reorder(a, S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("beam_reset", [](py::dict d, uintptr_t s) {
    BeamResetArgs a;
    a.N = get<int>(d, "N", 0); a.W = get<int>(d, "W", 0); a.L = get<int>(d, "L", 0); a.Bp = get<int>(d, "Bp", 0);
    a.H = get<int>(d, "H", 0); a.max_len = get<int>(d, "max_len", 0); a.sos = get<int>(d, "sos", 0);
    const auto h = get<std::vector<uintptr_t>>(d, "h", {});
    if (a.L < 1 || a.L > 4 || (int)h.size() != a.L) throw std::runtime_error("beam_reset: 1 <= L <= 4 and L h pointers");
    for (int l = 0; l < a.L; ++l) a.h[l] = Pp<float>(h[l]);
    a.ids = GP(int, d, "ids"); a.score = GP(float, d, "score"); a.state = GP(int, d, "state"); a.len = GP(int, d, "len");
    a.rows = GP(unsigned char, d, "rows");
    a.allow_state = GP(int, d, "allow_state"); a.allow_start = GP(const int, d, "allow_start");
    beam_reset(a, S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("reduce_slabs", [](uintptr_t src, int splits, long n, uintptr_t dst, uintptr_t s) {
    reduce_slabs(Pp<const float>(src), splits, n, Pp<float>(dst), S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("cast_bf16", [](uintptr_t in, long n, uintptr_t out, uintptr_t s) {
    cast_bf16(Pp<const float>(in), n, Pp<u16>(out), S(s));
    HIP_LAUNCH_CHECK();
  });
  m.def("transpose_bf16", [](uintptr_t in, int R, int C, uintptr_t out, uintptr_t s) {
    transpose_bf16(Pp<const float>(in), R, C, Pp<u16>(out), S(s));
    HIP_LAUNCH_CHECK();
  });

  // ---------------------------------------------------------------- RCCL communicator
  m.def("bootstrap_key", &bootstrap_key);
  m.def("launch_env", [] {
    const LaunchEnv e = launch_env();
    py::dict d;
    d["rank"] = e.rank; d["world"] = e.world; d["local"] = e.local; d["launcher"] = e.launcher;
    return d;
  });
  m.def("bootstrap_path", &bootstrap_path);
  m.def("file_exchange_uid", [](int rank, const std::string& path, const std::string& key, py::bytes uid,
                                int timeout_ms) {
    std::string u = uid;
    py::gil_scoped_release nogil;
    return py::bytes(file_exchange_uid(rank, path, key, u, timeout_ms));
  });
  py::class_<RcclComm>(m, "RcclComm")
      .def(py::init([](py::bytes uid, int rank, int world) {
        std::string s = uid;
        return new RcclComm(s, rank, world);
      }))
      .def_static("unique_id", []() { return py::bytes(RcclComm::unique_id()); })
      .def("allreduce_avg_f32", [](RcclComm& c, uintptr_t p, long n, uintptr_t s) {
        c.allreduce_avg_f32(Pp<float>(p), n, S(s));
      })
      .def("allreduce_sum_f32", [](RcclComm& c, uintptr_t p, long n, uintptr_t s) {
        c.allreduce_sum_f32(Pp<float>(p), n, S(s));
      })
      .def("allreduce_max_u32", [](RcclComm& c, uintptr_t p, long n, uintptr_t s) {
        c.allreduce_max_u32(Pp<unsigned>(p), n, S(s));
      })
      .def("broadcast_f32", [](RcclComm& c, uintptr_t p, long n, int root, uintptr_t s) {
        c.broadcast_f32(Pp<float>(p), n, root, S(s));
      })
      .def("allgather_u8", [](RcclComm& c, uintptr_t send, uintptr_t recv, long n, uintptr_t s) {
        c.allgather_u8(Pp<const unsigned char>(send), Pp<unsigned char>(recv), n, S(s));
      })
      .def("reduce_scatter_avg_f32", [](RcclComm& c, uintptr_t send, uintptr_t recv, long n, uintptr_t s) {
        c.reduce_scatter_avg_f32(Pp<const float>(send), Pp<float>(recv), n, S(s));
      })
      .def("allgather_f32", [](RcclComm& c, uintptr_t send, uintptr_t recv, long n, uintptr_t s) {
        c.allgather_f32(Pp<const float>(send), Pp<float>(recv), n, S(s));
      })
      .def("count", &RcclComm::count)
      .def("check_async_error", &RcclComm::check_async_error)
      .def("abort", &RcclComm::abort)
      .def("aborted", &RcclComm::aborted)
      .def("rank", &RcclComm::rank)
      .def("world", &RcclComm::world);
}

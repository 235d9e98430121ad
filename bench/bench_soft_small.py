#!/usr/bin/env python3
"""Soft preferences on small batches: the soft persistent launch against the per-char soft graph it
replaces, on the reference's model (preset ``ref``), fp32, with top_k = 40, top_p = 0.95, T = 0.8.

docs/DESIGN.md §4h's bench values: one bias line ("xqz" -2, EOS -1, "ae" +0.5), presence 0.5 and frequency
0.5 for every name.  Sides, per name count (1, 8, 16, 32, 64):
  (a) ``generate_ctl`` with the soft values and ``set_persist_soft_max(64)`` -- one soft persistent launch;
  (b) the same call with ``set_persist_soft_max(0)`` -- the per-char soft graph, the path such a call took
      before the switch existed and the comparator;
  (c) the same call without the soft values -- the controlled persistent launch;
  (d) (a) with both penalties 0 (the bias only): the history walk is skipped, so (a) - (d) is what it costs.

Same process, one generator, alternating rounds (a, b, c, d, a, ...); per side the median, the minimum and
the spread (max - min) over the rounds of ``reps`` calls, launch and error read-back included.
Device-resident uniforms, controls, tables and outputs; host transfer excluded (the form of
bench_constrained_small.py).  One JSON line per name count, appended to --out as well; ``persist_wins`` is
(a)'s median below (b)'s by more than (b)'s spread.

    python bench/bench_soft_small.py [--names 1,8,16,32,64] [--preset ref] [--reps 10] [--rounds 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="ref")
    ap.add_argument("--names", default="1,8,16,32,64", help="comma list: one JSON line per count")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--top-k", dest="top_k", type=int, default=40)
    ap.add_argument("--top-p", dest="top_p", type=float, default=0.95)
    ap.add_argument("--temperature", type=float, default=0.8)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "soft_persist_bench.jsonl"))
    args = ap.parse_args()

    from gru_mpi_cuda_amd.config import preset
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    from gru_mpi_cuda_amd.models import cpu_ref
    from gru_mpi_cuda_amd.models.params import init_params

    cfg = preset(args.preset)
    dev = torch.device("cuda", 0)
    params = init_params(cfg)
    ML = cfg.max_len
    bias = {"xqz": -2.0, int(cfg.eos): -1.0, "ae": 0.5}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.reps

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for n in [int(x) for x in args.names.split(",")]:
        gen = HipGenerator(cfg, params, max_batch=max(n, 64), device=dev, precision="fp32")
        g = gen.g
        g.set_persist_ctl_max(64)      # the sides choose the path themselves, whatever the defaults are
        rf = torch.from_numpy(np.random.default_rng(7).random((n, ML), dtype=np.float32)).to(dev)
        c = cpu_ref.make_controls(cfg, n, args.temperature, args.top_k, args.top_p)
        ctl = [torch.from_numpy(a).to(dev) for a in (c.inv_temp, c.top_k, c.top_p, c.plen, c.prefix)]
        s = gen._s()
        held = gen._soft_tensors(cpu_ref.make_soft(cfg, n, bias, 0.5, 0.5))
        held0 = gen._soft_tensors(cpu_ref.make_soft(cfg, n, bias, 0.0, 0.0))
        outs = {k: torch.empty(n, ML + 1, dtype=torch.uint8, device=dev) for k in "abcd"}

        def call(out, soft_max, skw):
            def fn():
                g.set_persist_soft_max(soft_max)
                g.generate_ctl(rf.data_ptr(), n, *[t.data_ptr() for t in ctl], out.data_ptr(), s, **skw)
            return fn

        arms = {"a": call(outs["a"], 64, gen._soft_kwargs(held)), "b": call(outs["b"], 0, gen._soft_kwargs(held)),
                "c": call(outs["c"], 0, {}), "d": call(outs["d"], 64, gen._soft_kwargs(held0))}
        on_persist = bool((g.set_persist_soft_max(64), g.uses_persist_soft(n, 0))[1])
        before = g.persist_soft_launches()
        for _ in range(2):             # warm-up: the workspace filled, the graph captured
            for fn in arms.values():
                fn()
        ts = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():
                ts[k].append(timed(fn))
        torch.cuda.synchronize()
        launches = g.persist_soft_launches() - before

        def side(k):
            med = statistics.median(ts[k])
            return {"s_median": round(med, 7), "s_min": round(min(ts[k]), 7), "s_spread": round(max(ts[k]) - min(ts[k]), 7),
                    "us_per_char_step": round(med / ML * 1e6, 2), "chars": int((outs[k] != 0).sum())}

        ma, mb, mc, md = (statistics.median(ts[k]) for k in "abcd")
        spread_b = max(ts["b"]) - min(ts["b"])
        res = {"preset": args.preset, "model": f"GRU L={cfg.layers} H={cfg.hidden} E={cfg.embed} V={cfg.vocab}",
               "max_len": ML, "names": n, "reps": args.reps, "rounds": args.rounds,
               "data": "random-init weights, seeded uniforms",
               "soft": {"logit_bias": {str(k): v for k, v in bias.items()}, "presence_penalty": 0.5, "frequency_penalty": 0.5},
               "controls": {"top_k": args.top_k, "top_p": args.top_p, "temperature": args.temperature},
               "a_soft_persistent": side("a"), "b_soft_per_char_graph": side("b"), "c_ctl_persistent": side("c"),
               "d_soft_persistent_bias_only": side("d"),
               "side_a_on_persistent_launch": on_persist,
               "side_ad_persistent_launches": int(launches), "side_ad_calls": 2 * (2 + args.rounds * args.reps),
               "a_rows_equal_b_rows": bool((outs["a"] == outs["b"]).all()),
               "a_rows_differ_from_c_rows": bool((outs["a"] != outs["c"]).any()),
               "a_vs_b_time": round(ma / mb, 3), "persist_wins": bool(mb - ma > spread_b),
               "soft_extra_us_per_char_step_vs_ctl": round((ma - mc) / ML * 1e6, 2),
               "history_walk_us_per_char_step": round((ma - md) / ML * 1e6, 2),
               "error_word": int(g.read_error())}
        line = json.dumps(res)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        del gen
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Conditional names on small calls: the persistent launch (docs/DESIGN.md §4j, ``set_persist_conditional_max``)
against the recorded per-char graph it replaces, on the reference's model (preset ``ref``).

Shapes (systems x width): 1 x 4, 1 x 8, 1 x 16 and 16 x 4, every prefix "Mar", under two rules: the regex
``[A-Z][a-z]{3,6}`` (an automaton, a line per slot) and §4e's per-position rule (a line per step).  Sides:
  (a) ``Generator.conditional`` with ``set_persist_conditional_max(64)`` -- one persistent launch per call;
  (b) the same call with ``set_persist_conditional_max(0)`` -- the recorded graph, the path every call takes by
      default and the comparator.

Same process, one generator, alternating rounds (a, b, a, ...); per side the median, the minimum and the
spread (max - min) over the rounds of ``reps`` calls, launch and the error word's read-back included.
Device-resident prefixes, tables and outputs; host transfer and the Python-side validation excluded (the form
of bench_distinct_small.py).  One JSON line per (rule, shape), appended to --out as well; ``persist_wins`` is
(a)'s median below (b)'s by more than (b)'s spread.

    python bench/bench_conditional_small.py [--shapes 1x4,1x8,1x16,16x4] [--preset ref] [--reps 200] [--rounds 7]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import string
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="ref")
    ap.add_argument("--shapes", default="1x4,1x8,1x16,16x4", help="comma list of systems x width: one JSON line each")
    ap.add_argument("--prefix", default="Mar")
    ap.add_argument("--max-len", dest="max_len", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--ess-threshold", dest="thr", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=200, help="calls per timed window (a call is about a millisecond)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "conditional_persist_bench.jsonl"))
    args = ap.parse_args()

    from gru_mpi_cuda_amd.config import preset
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    from gru_mpi_cuda_amd.models import cpu_ref
    from gru_mpi_cuda_amd.models.params import init_params

    cfg = preset(args.preset).replace(max_len=args.max_len)
    dev = torch.device("cuda", 0)
    params = init_params(cfg)
    ML = cfg.max_len
    hi = min(7, ML)
    rules = {"regex": dict(regex="[A-Z][a-z]{3,%d}" % (hi - 1)),
             "per_position": dict(pattern="[A-Z]", charset=string.ascii_letters, min_len=4, max_len=hi)}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.reps

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    gen = HipGenerator(cfg, params, max_batch=64, device=dev, precision="fp32")
    g, s = gen.g, gen._s()
    for rule, rkw in rules.items():
        for shape in args.shapes.split(","):
            N, W = (int(x) for x in shape.split("x"))
            pre, plen, inv, seed, start, thr, _, _ = cpu_ref.conditional_inputs(cfg, [args.prefix[:ML]] * N, W, None, 1,
                                                                                args.seed, 0, None, args.thr)
            cons = cpu_ref.make_constraints(cfg, N, **rkw)
            cpu_ref.check_prefix_allowed(cons, pre, plen)
            held = gen._constraint_tensors(cons)
            extra = gen._constraint_args(held)
            p, l, it = (torch.from_numpy(x).to(dev) for x in (pre, plen, inv))
            # rows, log_weight, logq, n_tok, n_resampled per side
            outs = {k: (torch.empty(N, W, ML + 1, dtype=torch.uint8, device=dev), torch.empty(N, W, dtype=torch.float32, device=dev),
                        torch.empty(N, W, dtype=torch.float32, device=dev), torch.empty(N, W, dtype=torch.int32, device=dev),
                        torch.empty(N, dtype=torch.int32, device=dev)) for k in "ab"}
            err = {"a": 0, "b": 0}
            took = {}

            def call(k, rows_max):
                def fn():
                    g.set_persist_conditional_max(rows_max)
                    g.conditional(l.data_ptr(), p.data_ptr(), N, W, seed, start, thr, it.data_ptr(),
                                  *[t.data_ptr() for t in outs[k]], s, *extra)
                    err[k] |= int(g.read_error())
                    took[k] = bool(g.conditional_last_persist())
                return fn

            arms = {"a": call("a", 64), "b": call("b", 0)}
            before = g.persist_conditional_launches()
            for _ in range(2):             # warm-up: the buffers allocated, the graph captured
                for fn in arms.values():
                    fn()
            ts = {k: [] for k in arms}
            for _ in range(args.rounds):
                for k, fn in arms.items():
                    ts[k].append(timed(fn))
            torch.cuda.synchronize()
            launches = g.persist_conditional_launches() - before

            def side(k):
                med = statistics.median(ts[k])
                return {"s_median": round(med, 7), "s_min": round(min(ts[k]), 7), "s_spread": round(max(ts[k]) - min(ts[k]), 7),
                        "us_per_char_step": round(med / ML * 1e6, 2), "resamples": int(outs[k][4].sum())}

            def diff(i):
                xa, xb = (outs[k][i].cpu().numpy().astype(np.float64) for k in "ab")
                return float(np.abs(xa - xb).max())

            ma, mb = (statistics.median(ts[k]) for k in "ab")
            res = {"preset": args.preset, "model": f"GRU L={cfg.layers} H={cfg.hidden} E={cfg.embed} V={cfg.vocab}",
                   "max_len": ML, "rule": rule, "constraints": {k: str(v) for k, v in rkw.items()}, "systems": N, "width": W,
                   "rows": N * W, "prefix": args.prefix[:ML], "seed": args.seed, "ess_threshold": args.thr,
                   "reps": args.reps, "rounds": args.rounds, "data": "random-init weights",
                   "a_persistent": side("a"), "b_recorded_graph": side("b"),
                   "side_a_on_persistent_launch": took["a"], "side_b_on_persistent_launch": took["b"],
                   "side_a_persistent_launches": int(launches), "side_a_calls": (2 + args.rounds * args.reps),
                   "a_rows_equal_b_rows": bool((outs["a"][0] == outs["b"][0]).all()),
                   "a_resamples_equal_b": bool((outs["a"][4] == outs["b"][4]).all()),
                   "a_vs_b_max_logw_diff": diff(1), "a_vs_b_max_logq_diff": diff(2),
                   "a_vs_b_time": round(ma / mb, 3), "persist_wins": bool(mb - ma > max(ts["b"]) - min(ts["b"])),
                   "error_word": err["a"] | err["b"]}
            line = json.dumps(res)
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

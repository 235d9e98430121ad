#!/usr/bin/env python3
"""Constrained beam and distinct searches on small calls: the constrained persistent launches (docs/DESIGN.md §4d /
§4i, "Constraints inside the launch") against the recorded per-char graph they replace, on the reference's model
(preset ``ref``).

Commands: ``beam`` and ``distinct``.  Shapes (prefixes x width): 1 x 4, 1 x 8, 1 x 16 and 16 x 4, every prefix
"Mar".  Rules: ``regex`` = ``[A-Z][a-z]{3,6}`` (an automaton, a state per row) and ``pos`` = §4e's per-position
rule (letters only, exactly six chars).  Sides, with ``persist_beam`` / ``persist_distinct`` at 64 throughout:
  (a) ``set_persist_con_max(64)`` -- one constrained persistent launch per call;
  (b) ``set_persist_con_max(0)`` -- the recorded graph, the path every constrained call takes by default and the
      comparator.

Same process, one generator, alternating rounds (a, b, a, ...); per side the median, the minimum and the spread
(max - min) over the rounds of ``reps`` calls, launch and the error word's read-back included.  Device-resident
inputs, tables and outputs; host transfer and the Python-side validation excluded (the form of
bench_beam_small.py).  One JSON line per command, rule and shape, appended to --out as well; ``persist_wins`` is
(a)'s median below (b)'s by more than (b)'s spread.

    python bench/bench_search_con_small.py [--commands beam,distinct] [--rules regex,pos] [--shapes 1x4,1x8,1x16,16x4]
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

LETTERS = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"
RULES = {"regex": dict(regex="[A-Z][a-z]{3,6}"), "pos": dict(charset=LETTERS, min_len=6, max_len=6)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="ref")
    ap.add_argument("--commands", default="beam,distinct")
    ap.add_argument("--rules", default="regex,pos")
    ap.add_argument("--shapes", default="1x4,1x8,1x16,16x4", help="comma list of prefixes x width: one JSON line each")
    ap.add_argument("--prefix", default="Mar")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "search_con_persist_bench.jsonl"))
    args = ap.parse_args()

    from gru_mpi_cuda_amd.config import preset
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    from gru_mpi_cuda_amd.models import cpu_ref
    from gru_mpi_cuda_amd.models.params import init_params

    cfg = preset(args.preset)
    dev = torch.device("cuda", 0)
    params = init_params(cfg)
    ML = cfg.max_len

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.reps

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    gen = HipGenerator(cfg, params, max_batch=64, device=dev, precision="fp32", persist_beam=64, persist_distinct=64)
    g, s = gen.g, gen._s()
    for cmd in args.commands.split(","):
        beam = cmd == "beam"
        for rule in args.rules.split(","):
            for shape in args.shapes.split(","):
                N, W = (int(x) for x in shape.split("x"))
                prefixes = [args.prefix[:ML]] * N
                if beam:
                    pre, plen = cpu_ref.beam_inputs(cfg, prefixes, W)
                    lead = ()
                else:
                    pre, plen, inv, seed, start = cpu_ref.distinct_inputs(cfg, prefixes, W, None, 1, 0, None)
                    it = torch.from_numpy(inv).to(dev)
                    lead = (seed, start, it.data_ptr())
                cons = cpu_ref.as_constraints(cfg, N, RULES[rule])
                cpu_ref.check_prefix_allowed(cons, pre, plen)
                held = gen._constraint_tensors(cons)
                extra = gen._constraint_args(held)
                p, l = torch.from_numpy(pre).to(dev), torch.from_numpy(plen).to(dev)
                nf32 = 1 if beam else 2   # logp | logq, gumbel
                outs = {k: ([torch.empty(N, W, ML + 1, dtype=torch.uint8, device=dev)] +
                            [torch.empty(N, W, dtype=torch.float32, device=dev) for _ in range(nf32)] +
                            [torch.empty(N, W, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)])
                        for k in "ab"}
                err = {"a": 0, "b": 0}
                took = {}

                def call(k, rows_max):
                    def fn():
                        g.set_persist_con_max(rows_max)
                        if beam:
                            g.beam(l.data_ptr(), p.data_ptr(), N, W, *[t.data_ptr() for t in outs[k]], s, *extra)
                            took[k] = bool(g.beam_last_persist())
                        else:
                            g.distinct(l.data_ptr(), p.data_ptr(), N, W, *lead, *[t.data_ptr() for t in outs[k]], s, *extra)
                            took[k] = bool(g.distinct_last_persist())
                        err[k] |= int(g.read_error())
                    return fn

                arms = {"a": call("a", 64), "b": call("b", 0)}
                for _ in range(2):             # warm-up: the arena committed, the graph captured
                    for fn in arms.values():
                        fn()
                ts = {k: [] for k in arms}
                for _ in range(args.rounds):
                    for k, fn in arms.items():
                        ts[k].append(timed(fn))
                torch.cuda.synchronize()

                def side(k):
                    med = statistics.median(ts[k])
                    return {"s_median": round(med, 7), "s_min": round(min(ts[k]), 7),
                            "s_spread": round(max(ts[k]) - min(ts[k]), 7), "us_per_char_step": round(med / ML * 1e6, 2),
                            "rows_found": int(outs[k][-1].sum())}

                ma, mb = (statistics.median(ts[k]) for k in "ab")
                la, lb = (outs[k][1].cpu().numpy().astype(np.float64) for k in "ab")
                live = np.isfinite(lb)
                same = bool((np.isfinite(la) == live).all())
                res = {"command": cmd, "rule": rule, "constraints": RULES[rule], "preset": args.preset,
                       "model": f"GRU L={cfg.layers} H={cfg.hidden} E={cfg.embed} V={cfg.vocab}", "max_len": ML, "prefixes": N,
                       "width": W, "rows": N * W, "prefix": args.prefix[:ML], "reps": args.reps, "rounds": args.rounds,
                       "data": "random-init weights", "a_persistent": side("a"), "b_recorded_graph": side("b"),
                       "side_a_on_persistent_launch": took["a"], "side_b_on_persistent_launch": took["b"],
                       "a_rows_equal_b_rows": bool((outs["a"][0] == outs["b"][0]).all()),
                       "a_vs_b_max_score_diff": float(np.abs(la[live] - lb[live]).max()) if live.any() and same else None,
                       "a_vs_b_time": round(ma / mb, 3), "persist_wins": bool(mb - ma > max(ts["b"]) - min(ts["b"])),
                       "error_word": err["a"] | err["b"]}
                line = json.dumps(res)
                print(line, flush=True)
                with open(args.out, "a") as f:
                    f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

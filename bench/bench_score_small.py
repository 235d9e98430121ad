#!/usr/bin/env python3
"""Scoring small batches: the persistent launch (docs/DESIGN.md §4a, ``set_persist_score_max``) against the
recorded graph it replaces, on the reference's model (preset ``ref``).

Batches of 1 / 8 / 16 / 32 / 64 rows of max_len non-EOS chars (seeded), so every row has max_len tokens.  Sides:
  (a) ``Generator.score`` with ``set_persist_score_max(64)`` -- one persistent launch per call;
  (b) the same call with ``set_persist_score_max(0)`` -- the recorded graph, the path every call takes by
      default and the comparator.

Same process, one generator, alternating rounds (a, b, a, ...); per side the median, the minimum and the
spread (max - min) over the rounds of ``reps`` calls, launch and the error word's read-back included.
Device-resident rows and outputs; host transfer and the Python-side validation excluded (the form of
bench_beam_small.py).  One JSON line per batch size, appended to --out as well; ``persist_wins`` is (a)'s
median below (b)'s by more than (b)'s spread.

    python bench/bench_score_small.py [--names 1,8,16,32,64] [--preset ref] [--reps 200] [--rounds 5]
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
    ap.add_argument("--names", default="1,8,16,32,64", help="comma list of batch sizes: one JSON line each")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "score_persist_bench.jsonl"))
    args = ap.parse_args()

    from gru_mpi_cuda_amd.config import preset
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
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
    gen = HipGenerator(cfg, params, max_batch=64, device=dev, precision="fp32")
    g, s = gen.g, gen._s()
    for N in (int(x) for x in args.names.split(",")):
        rows = np.random.default_rng(1).integers(0, cfg.vocab - 1, size=(N, ML + 1), dtype=np.uint8)
        rows[rows >= cfg.eos] += 1          # no EOS among the chars: max_len tokens per row
        rows[:, ML] = 0
        r = torch.from_numpy(rows).to(dev)
        outs = {k: (torch.empty(N, ML, dtype=torch.float32, device=dev), torch.empty(N, ML, dtype=torch.int32, device=dev),
                    torch.empty(N, dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)) for k in "ab"}
        err = {"a": 0, "b": 0}
        took = {}

        def call(k, names_max):
            def fn():
                g.set_persist_score_max(names_max)
                g.score(r.data_ptr(), N, *[t.data_ptr() for t in outs[k]], s)
                err[k] |= int(g.read_error())
                took[k] = bool(g.score_last_persist())
            return fn

        arms = {"a": call("a", 64), "b": call("b", 0)}
        before = g.persist_score_launches()
        for _ in range(3):             # warm-up: the workspaces allocated, the graph captured
            for fn in arms.values():
                fn()
        ts = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():
                ts[k].append(timed(fn))
        torch.cuda.synchronize()
        launches = g.persist_score_launches() - before

        def side(k):
            med = statistics.median(ts[k])
            return {"s_median": round(med, 7), "s_min": round(min(ts[k]), 7), "s_spread": round(max(ts[k]) - min(ts[k]), 7),
                    "us_per_char_step": round(med / ML * 1e6, 2), "tokens": int(outs[k][3].sum())}

        ma, mb = (statistics.median(ts[k]) for k in "ab")
        ta, tb = (outs[k][0].cpu().numpy().astype(np.float64) for k in "ab")
        res = {"preset": args.preset, "model": f"GRU L={cfg.layers} H={cfg.hidden} E={cfg.embed} V={cfg.vocab}",
               "max_len": ML, "names": N, "reps": args.reps, "rounds": args.rounds, "data": "random-init weights",
               "a_persistent": side("a"), "b_recorded_graph": side("b"),
               "side_a_on_persistent_launch": took["a"], "side_b_on_persistent_launch": took["b"],
               "side_a_persistent_launches": int(launches), "side_a_calls": (3 + args.rounds * args.reps),
               "a_ranks_equal_b_ranks": bool((outs["a"][1] == outs["b"][1]).all()),
               "a_vs_b_max_tok_logp_diff": float(np.abs(ta - tb).max()),
               "a_vs_b_time": round(ma / mb, 3), "persist_wins": bool(mb - ma > max(ts["b"]) - min(ts["b"])),
               "error_word": err["a"] | err["b"]}
        line = json.dumps(res)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Conditional-names benchmark: ``Generator.conditional`` (sequential Monte Carlo, docs/DESIGN.md §4j) against
``Generator.distinct`` for the same N prefixes of W rows under §4g's bench regex, on the reference's model
(preset ``ref``).

Both sides run the same graph shape -- per char the exact-fp32 step on N W rows, one selection launch and
beam_reorder -- and differ in the selection alone: smc_select_f32 reads a row twice (its mass in phase (a),
the ancestor's row again in phase (c)) and has one barrier, where sbs_select_f32 ranks W V candidates in W
rounds.  The difference per char step is the difference of the two selections; neither is timed on its own.

Same process, same generator, alternating rounds (distinct, conditional, distinct, ...); per side the median
and the minimum over the rounds.  Device-resident prefixes and outputs; host transfer and the Python-side
validation excluded.  One JSON line per (prefixes, width), appended to profiles/conditional_bench.jsonl.

    python bench/bench_conditional.py [--prefixes 1,16,256] [--widths 4,8,16] [--preset ref] [--reps 10] [--rounds 5] [--out f]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="ref")
    ap.add_argument("--prefixes", default="1,16,256", help="comma list of prefix counts")
    ap.add_argument("--widths", default="4,8,16", help="comma list of widths")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ess-threshold", dest="thr", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conditional_bench.jsonl"),
                    help="append the JSON lines to this file")
    args = ap.parse_args()

    from gru_mpi_cuda_amd.config import preset
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    from gru_mpi_cuda_amd.models import cpu_ref
    from gru_mpi_cuda_amd.models.params import init_params

    cfg = preset(args.preset)
    dev = torch.device("cuda", 0)
    params = init_params(cfg)
    ML = cfg.max_len
    rx = "[A-Z][a-z]{3,%d}" % (min(7, ML) - 1)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.reps

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for n in [int(x) for x in args.prefixes.split(",")]:
        for W in [int(x) for x in args.widths.split(",")]:
            R = n * W
            gen = HipGenerator(cfg, params, max_batch=max(R, 64), device=dev, precision="fp32")
            aut = cpu_ref.make_constraints(cfg, n, regex=rx)
            held = gen._constraint_tensors(aut)
            extra = gen._constraint_args(held)
            plen = torch.zeros(n, dtype=torch.int32, device=dev)      # empty prefixes: every step free
            pre = torch.zeros(n, ML, dtype=torch.uint8, device=dev)
            inv = torch.ones(n, dtype=torch.float32, device=dev)
            rows = torch.empty(n, W, ML + 1, dtype=torch.uint8, device=dev)
            logq = torch.empty(n, W, dtype=torch.float32, device=dev)
            aux = torch.empty(n, W, dtype=torch.float32, device=dev)      # gumbel / log_weight
            ntok = torch.empty(n, W, dtype=torch.int32, device=dev)
            cnt = torch.empty(n, dtype=torch.int32, device=dev)           # n_found / n_resampled
            s = gen._s()
            calls = [0]

            def distinct():
                calls[0] += 1      # a new seed per call: the recordings read it from memory
                gen.g.distinct(plen.data_ptr(), pre.data_ptr(), n, W, calls[0], 0, inv.data_ptr(), rows.data_ptr(),
                               logq.data_ptr(), aux.data_ptr(), ntok.data_ptr(), cnt.data_ptr(), s, *extra)

            def conditional():
                calls[0] += 1
                gen.g.conditional(plen.data_ptr(), pre.data_ptr(), n, W, calls[0], 0, args.thr, inv.data_ptr(),
                                  rows.data_ptr(), aux.data_ptr(), logq.data_ptr(), ntok.data_ptr(), cnt.data_ptr(), s, *extra)

            distinct(); conditional()              # warm-up: both graphs captured
            distinct(); conditional()
            td, tc = [], []
            for _ in range(args.rounds):
                td.append(timed(distinct))
                tc.append(timed(conditional))
            torch.cuda.synchronize()
            lw = aux.double().cpu().numpy()        # the last call was conditional's
            log_z = float((lw.max(1) + np.log(np.exp(lw - lw.max(1, keepdims=True)).mean(1))).mean())

            def side(ts):
                med = statistics.median(ts)
                return {"ms_per_call": round(med * 1e3, 4), "ms_min": round(min(ts) * 1e3, 4),
                        "us_per_char_step": round(med / ML * 1e6, 2)}

            md, mc = statistics.median(td), statistics.median(tc)
            res = {"bench": "conditional", "preset": args.preset,
                   "model": f"GRU L={cfg.layers} H={cfg.hidden} E={cfg.embed} V={cfg.vocab}", "max_len": ML,
                   "prefixes": n, "width": W, "rows": R, "reps": args.reps, "rounds": args.rounds,
                   "data": "random-init weights, empty prefixes, temperature 1", "language": rx, "states": aut.states,
                   "ess_threshold": args.thr,
                   "conditional": side(tc), "distinct_same_rows": side(td),
                   "conditional_vs_distinct_time": round(mc / md, 3),
                   "extra_us_per_char_step": round((mc - md) / ML * 1e6, 2),
                   "mean_log_z": round(log_z, 4), "mean_resamples": round(float(cnt.double().mean()), 3),
                   "conditional_graphs": int(gen.g.conditional_graphs()), "distinct_graphs": int(gen.g.distinct_graphs()),
                   "error_word": int(gen.g.read_error())}
            line = json.dumps(res)
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
            del gen
    return 0


if __name__ == "__main__":
    sys.exit(main())

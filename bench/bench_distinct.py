#!/usr/bin/env python3
"""Distinct-names benchmark: ``Generator.distinct`` (stochastic beam search, docs/DESIGN.md §4i) against
``Generator.beam`` for the same N prefixes of W rows, on the reference's model (preset ``ref``).

Both sides run the same graph shape -- per char the exact-fp32 step on N W rows, one selection launch and
beam_reorder -- and differ in the selection alone: sbs_select_f32 adds the renormalisation, one or two
Philox calls and the Gumbel truncation per lane and row to beam_select_f32.  The difference per char step
is that extra cost.

Same process, same generator, alternating rounds (beam, distinct, beam, ...); per side the median and the
minimum over the rounds.  Device-resident prefixes and outputs; host transfer and the Python-side
validation excluded.  One JSON line per (prefixes, width), appended to profiles/distinct_bench.jsonl.

    python bench/bench_distinct.py [--prefixes 1,16,256] [--widths 4,8,16] [--preset ref] [--reps 10] [--rounds 5] [--out f]
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

import torch


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="ref")
    ap.add_argument("--prefixes", default="1,16,256", help="comma list of prefix counts")
    ap.add_argument("--widths", default="4,8,16", help="comma list of widths")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distinct_bench.jsonl"),
                    help="append the JSON lines to this file")
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

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for n in [int(x) for x in args.prefixes.split(",")]:
        for W in [int(x) for x in args.widths.split(",")]:
            R = n * W
            gen = HipGenerator(cfg, params, max_batch=max(R, 64), device=dev, precision="fp32")
            plen = torch.zeros(n, dtype=torch.int32, device=dev)      # empty prefixes: every step free
            pre = torch.zeros(n, ML, dtype=torch.uint8, device=dev)
            inv = torch.ones(n, dtype=torch.float32, device=dev)
            rows = torch.empty(n, W, ML + 1, dtype=torch.uint8, device=dev)
            logp = torch.empty(n, W, dtype=torch.float32, device=dev)
            gum = torch.empty(n, W, dtype=torch.float32, device=dev)
            ntok = torch.empty(n, W, dtype=torch.int32, device=dev)
            nb = torch.empty(n, dtype=torch.int32, device=dev)
            s = gen._s()
            calls = [0]

            def beam():
                gen.g.beam(plen.data_ptr(), pre.data_ptr(), n, W, rows.data_ptr(), logp.data_ptr(), ntok.data_ptr(),
                           nb.data_ptr(), s)

            def distinct():
                calls[0] += 1      # a new seed per call: the recording reads it from memory
                gen.g.distinct(plen.data_ptr(), pre.data_ptr(), n, W, calls[0], 0, inv.data_ptr(), rows.data_ptr(),
                               logp.data_ptr(), gum.data_ptr(), ntok.data_ptr(), nb.data_ptr(), s)

            beam(); distinct()              # warm-up: both graphs captured
            beam(); distinct()
            tb, td = [], []
            for _ in range(args.rounds):
                tb.append(timed(beam))
                td.append(timed(distinct))
            torch.cuda.synchronize()

            def side(ts):
                med = statistics.median(ts)
                return {"ms_per_call": round(med * 1e3, 4), "ms_min": round(min(ts) * 1e3, 4),
                        "us_per_char_step": round(med / ML * 1e6, 2)}

            mb, md = statistics.median(tb), statistics.median(td)
            res = {"bench": "distinct", "preset": args.preset,
                   "model": f"GRU L={cfg.layers} H={cfg.hidden} E={cfg.embed} V={cfg.vocab}", "max_len": ML,
                   "prefixes": n, "width": W, "rows": R, "reps": args.reps, "rounds": args.rounds,
                   "data": "random-init weights, empty prefixes, temperature 1",
                   "distinct": side(td), "beam_same_rows": side(tb),
                   "distinct_vs_beam_time": round(md / mb, 3),
                   "extra_us_per_char_step": round((md - mb) / ML * 1e6, 2),
                   "rows_found": int(nb.sum()), "distinct_graphs": int(gen.g.distinct_graphs()),
                   "beam_graphs": int(gen.g.beam_graphs()), "error_word": int(gen.g.read_error())}
            line = json.dumps(res)
            print(line, flush=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
            del gen
    return 0


if __name__ == "__main__":
    sys.exit(main())

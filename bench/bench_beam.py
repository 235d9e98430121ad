#!/usr/bin/env python3
"""Beam search benchmark: ``Generator.beam`` for N prefixes of W beams against greedy generation
(``generate_ctl`` with temperature 0) of the same number of rows (N W) on the per-char controlled
fp32 graph with the persistent path off, on the reference's model (preset ``ref``).

Both sides run the same exact-fp32 step per row and char (products on the master weights, IEEE
gates, the logits product); greedy ends a char with one sampler launch, the beam search with its two
(beam_select_f32, beam_reorder).  The difference is then those two launches per step.

Same process, same generator, alternating rounds (greedy, beam, greedy, ...); per side the median and
the minimum over the rounds.  Device-resident prefixes, controls and outputs; host transfer and the
Python-side validation excluded.  One JSON line per (prefixes, width).

    python bench/bench_beam.py [--prefixes 1,16,256] [--widths 4,8,16] [--preset ref] [--reps 10] [--rounds 5] [--out f]
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
    ap.add_argument("--prefixes", default="1,16,256", help="comma list of prefix counts")
    ap.add_argument("--widths", default="4,8,16", help="comma list of beam widths")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
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

    for n in [int(x) for x in args.prefixes.split(",")]:
        for W in [int(x) for x in args.widths.split(",")]:
            R = n * W
            gen = HipGenerator(cfg, params, max_batch=max(R, 64), device=dev, precision="fp32")
            gen.g.set_persist(False)      # the comparator is the per-char controlled graph
            rf = torch.from_numpy(np.random.default_rng(7).random((R, ML), dtype=np.float32)).to(dev)
            c = cpu_ref.make_controls(cfg, R, 0.0, None, None)      # greedy, no prefix
            ctl = [torch.from_numpy(a).to(dev) for a in (c.inv_temp, c.top_k, c.top_p, c.plen, c.prefix)]
            plen = torch.zeros(n, dtype=torch.int32, device=dev)      # empty prefixes: every step free
            pre = torch.zeros(n, ML, dtype=torch.uint8, device=dev)
            out_g = torch.empty(R, ML + 1, dtype=torch.uint8, device=dev)
            rows = torch.empty(n, W, ML + 1, dtype=torch.uint8, device=dev)
            logp = torch.empty(n, W, dtype=torch.float32, device=dev)
            ntok = torch.empty(n, W, dtype=torch.int32, device=dev)
            nb = torch.empty(n, dtype=torch.int32, device=dev)
            s = gen._s()

            def greedy():
                gen.g.generate_ctl(rf.data_ptr(), R, *[t.data_ptr() for t in ctl], out_g.data_ptr(), s)

            def beam():
                gen.g.beam(plen.data_ptr(), pre.data_ptr(), n, W, rows.data_ptr(), logp.data_ptr(), ntok.data_ptr(),
                           nb.data_ptr(), s)

            greedy(); beam()              # warm-up: both graphs captured
            greedy(); beam()
            assert not gen.g.uses_persist_ctl(R)
            tg, tb = [], []
            for _ in range(args.rounds):
                tg.append(timed(greedy))
                tb.append(timed(beam))
            torch.cuda.synchronize()

            def side(ts):
                med = statistics.median(ts)
                return {"ms_per_call": round(med * 1e3, 4), "ms_min": round(min(ts) * 1e3, 4),
                        "us_per_char_step": round(med / ML * 1e6, 2)}

            mg, mb = statistics.median(tg), statistics.median(tb)
            res = {"bench": "beam", "preset": args.preset,
                   "model": f"GRU L={cfg.layers} H={cfg.hidden} E={cfg.embed} V={cfg.vocab}", "max_len": ML,
                   "prefixes": n, "width": W, "rows": R, "reps": args.reps, "rounds": args.rounds,
                   "data": "random-init weights, empty prefixes",
                   "beam": side(tb), "greedy_ctl_graph_same_rows": side(tg),
                   "beam_vs_greedy_time": round(mb / mg, 3),
                   "extra_us_per_char_step": round((mb - mg) / ML * 1e6, 2),
                   "beams_found": int(nb.sum()), "beam_workspace_mb": round(gen.g.beam_workspace_bytes() / 2 ** 20, 1),
                   "error_word": int(gen.g.read_error())}
            line = json.dumps(res)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            del gen
    return 0


if __name__ == "__main__":
    sys.exit(main())

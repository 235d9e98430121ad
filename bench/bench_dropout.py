#!/usr/bin/env python3
"""Training-dropout benchmark (docs/DESIGN.md §3.5): what ``dropout > 0`` costs per training step.

Two trainers of one preset in one process -- ``dropout = 0`` (the headline plan) and ``dropout = p`` (the
unfused head, one ``dropout_fwd_seq`` and one ``dropout_bwd_seq`` launch per layer) -- stepping the same
pool of batches in alternating rounds (off, on, off, ...): per side the median and the minimum ms/step over
the rounds, and the plan strings.  A round is ``--steps`` steps as ``steps()`` groups of ``--group`` steps
per graph launch (``--group 1``: one graph per step).  One JSON line.  No threshold: a measurement.

    python bench/bench_dropout.py [--preset h512] [--dropout 0.2] [--steps 200] [--group 20] [--rounds 6]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="h512")
    ap.add_argument("--dropout", type=float, default=0.2)
    ap.add_argument("--steps", type=int, default=200, help="steps per timed round")
    ap.add_argument("--group", type=int, default=20, help="steps per graph launch (1 .. 32)")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=200)
    args = ap.parse_args()
    if not (0.0 < args.dropout < 1.0) or args.group < 1 or args.group > 32 or args.steps % args.group:
        ap.error("need 0 < --dropout < 1, 1 <= --group <= 32 and --steps a multiple of --group")

    from gru_mpi_cuda_amd.config import preset
    from gru_mpi_cuda_amd.engine.trainer import HipTrainer
    from gru_mpi_cuda_amd.models.params import init_params
    from gru_mpi_cuda_amd.utils.data import NameStream

    cfg = preset(args.preset)
    stream = NameStream(cfg.batch, cfg.seq, cfg.sos, cfg.eos, seed=1000, max_len=cfg.max_len)
    pool = [stream.next() for _ in range(8)]
    sides = {"off": HipTrainer(cfg, params=init_params(cfg)),
             "on": HipTrainer(cfg.replace(dropout=args.dropout), params=init_params(cfg))}

    def run(tr, n):
        i = 0
        while i < n:
            if args.group == 1:
                tr.step(*pool[i % len(pool)])
            else:
                tr.steps([pool[(i + j) % len(pool)] for j in range(args.group)])
            i += args.group

    def timed(tr):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(tr, args.steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    for tr in sides.values():            # graphs captured, clocks up
        run(tr, max(args.warmup, args.group))
    ms = {k: [] for k in sides}
    for _ in range(args.rounds):
        for k, tr in sides.items():
            ms[k].append(timed(tr))

    def side(k):
        tr = sides[k]
        return {"ms_per_step_median": round(statistics.median(ms[k]), 4), "ms_per_step_min": round(min(ms[k]), 4),
                "ms_per_step_rounds": [round(v, 4) for v in ms[k]], "plan": tr.t.plan(),
                "workspace_mb": round(tr.t.workspace_bytes() / 2 ** 20, 1), "final_loss": round(tr.loss(), 4),
                "error_word": int(tr.t.read_error())}

    off, on = side("off"), side("on")
    print(json.dumps({"bench": "train_dropout", "preset": args.preset, "dropout": args.dropout,
                      "model": f"GRU L={cfg.layers} H={cfg.hidden} E={cfg.embed} V={cfg.vocab}",
                      "global_batch": cfg.batch, "seq_len": cfg.seq, "steps_per_round": args.steps,
                      "graph_steps": args.group, "rounds": args.rounds,
                      "data": "synthetic name sequences (seeded syllable generator), random-init weights",
                      "off": off, "on": on,
                      "on_vs_off_time": round(on["ms_per_step_median"] / off["ms_per_step_median"], 4),
                      "extra_us_per_step": round((on["ms_per_step_median"] - off["ms_per_step_median"]) * 1e3, 2)}),
          flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

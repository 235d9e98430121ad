#!/usr/bin/env python3
"""Scoring under the sampler (docs/DESIGN.md §4f): what the controls and the mask cost.

``Generator::score`` three ways on the same rows at 32 / 256 / 4096 names of the reference model: plain,
with controls (top_k = 40, top_p = 0.95, T = 0.8) and with controls plus the §4e bench constraint ("a
capital, then letters, 4 to 7 chars").  The three share score_prep, the products and the gates; only the
last launch differs (score_logprob_f32 / score_ctl_logprob_f32 without and with MASK), plus the copies
of the batch's controls, of the table and of the idx slice.

Same process, same generator, alternating rounds (plain, controlled, constrained, plain, ...); per side
the median and the minimum over the rounds.  Device-resident inputs and outputs; host transfer and the
Python-side validation excluded (as bench_constrained.py).  One JSON line per name count, printed and
written to ``--out``.  No threshold: these are the first measurements.

    python bench/bench_score_ctl.py [--names 32,256,4096] [--reps 10] [--rounds 5] [--out profiles/score_ctl_bench.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import string
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="ref")
    ap.add_argument("--names", default="32,256,4096", help="comma list: one JSON line per count")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--top-k", dest="top_k", type=int, default=40)
    ap.add_argument("--top-p", dest="top_p", type=float, default=0.95)
    ap.add_argument("--temperature", type=float, default=0.8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_ctl_bench.jsonl"))
    args = ap.parse_args()

    from gru_mpi_cuda_amd.config import preset
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    from gru_mpi_cuda_amd.models import cpu_ref
    from gru_mpi_cuda_amd.models.params import init_params

    cfg = preset(args.preset)
    dev = torch.device("cuda", 0)
    params = init_params(cfg)
    ML = cfg.max_len
    rule = dict(pattern="[A-Z]", charset=string.ascii_letters, min_len=4, max_len=min(7, ML))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.reps

    def side(ts, n):
        med = statistics.median(ts)
        return {"s_median": round(med, 6), "s_min": round(min(ts), 6), "names_per_s": round(n / med, 1)}

    base = {"bench": "score_ctl", "preset": args.preset,
            "model": f"GRU L={cfg.layers} H={cfg.hidden} E={cfg.embed} V={cfg.vocab}", "max_len": ML, "reps": args.reps,
            "rounds": args.rounds, "data": "random-init weights, rows from generate() with seeded uniforms",
            "controls": {"top_k": args.top_k, "top_p": args.top_p, "temperature": args.temperature},
            "constraint": dict(rule)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    lines_out = []
    for n in [int(x) for x in args.names.split(",")]:
        gen = HipGenerator(cfg, params, max_batch=max(64, n), device=dev, precision="fp32")
        s = gen._s()
        rows = torch.from_numpy(gen.generate(np.random.default_rng(7).random(n * ML, dtype=np.float32))).to(dev)
        c = cpu_ref.make_controls(cfg, n, args.temperature, args.top_k, args.top_p)
        ctl = [torch.from_numpy(a).to(dev) for a in (c.inv_temp, c.top_k, c.top_p, c.plen, c.prefix)]
        tab, idx, lines = gen._constraint_tensors(cpu_ref.make_constraints(cfg, n, **rule))
        outs = [(torch.empty(n, ML, dtype=torch.float32, device=dev), torch.empty(n, ML, dtype=torch.int32, device=dev),
                 torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
                for _ in range(3)]
        nk = [torch.empty(n, ML, dtype=torch.int32, device=dev) for _ in range(2)]

        def plain():
            gen.g.score(rows.data_ptr(), n, *[t.data_ptr() for t in outs[0]], s)

        def controlled():
            gen.g.score(rows.data_ptr(), n, *[t.data_ptr() for t in outs[1]], s, *[t.data_ptr() for t in ctl], nk[0].data_ptr())

        def constrained():
            gen.g.score(rows.data_ptr(), n, *[t.data_ptr() for t in outs[2]], s, *[t.data_ptr() for t in ctl], nk[1].data_ptr(),
                        tab.data_ptr(), idx.data_ptr(), lines)

        fns = (plain, controlled, constrained)
        for _ in range(2):           # warm-up: the three graphs captured
            for fn in fns:
                fn()
        ts = ([], [], [])
        for _ in range(args.rounds):
            for fn, acc in zip(fns, ts):
                acc.append(timed(fn))
        torch.cuda.synchronize()
        med = [statistics.median(a) for a in ts]
        kept = nk[0].cpu().numpy()
        rec = dict(base, names=n, plain=side(ts[0], n), controlled=side(ts[1], n), constrained=side(ts[2], n),
                   controlled_vs_plain_time=round(med[1] / med[0], 3), constrained_vs_plain_time=round(med[2] / med[0], 3),
                   extra_us_controlled=round((med[1] - med[0]) * 1e6, 2), extra_us_constrained=round((med[2] - med[0]) * 1e6, 2),
                   table_lines=lines, mean_n_kept=round(float(kept[kept >= 0].mean()), 2),
                   impossible={"controlled": int(torch.isneginf(outs[1][2]).sum()), "constrained": int(torch.isneginf(outs[2][2]).sum())},
                   score_graphs=int(gen.g.score_graphs()), error_word=int(gen.g.read_error()))
        print(json.dumps(rec), flush=True)
        lines_out.append(json.dumps(rec))
        del gen
    with open(args.out, "w") as f:
        f.write("\n".join(lines_out) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Soft-preference benchmark (docs/DESIGN.md §4h): what the logit bias and the two penalties cost.

* ``generate_ctl`` (top_k = 40, top_p = 0.95, T = 0.8) with and without soft controls -- the same per-char
  graph with the SOFT instantiation of ``sample_ctl_f32`` as its sampler node, plus the copy of the bias
  table and of the batch's idx / presence / frequency slices -- at 256 and 4096 names (persistent path
  off: both sides on the per-char graph);
* ``score`` with the same controls, with and without soft controls, on the rows the soft call generated.

The soft controls are one bias line ("xqz" -2, EOS -1, "ae" +0.5), presence 0.5 and frequency 0.5 for every
name.  Same process, same generator, alternating rounds (plain, soft, plain, ...); per side the median and
the minimum over the rounds.  Device-resident inputs and outputs; host transfer and the Python-side
validation excluded (as bench_constrained.py).  One JSON line per measurement, with the ratio against
the call without soft controls of the same run and the microseconds per char step.  No threshold: these
are the first measurements.

    python bench/bench_soft_ctl.py [--names 256,4096] [--reps 10] [--rounds 5]
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
    ap.add_argument("--names", default="256,4096", help="comma list: two JSON lines per count")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--top-k", dest="top_k", type=int, default=40)
    ap.add_argument("--top-p", dest="top_p", type=float, default=0.95)
    ap.add_argument("--temperature", type=float, default=0.8)
    args = ap.parse_args()

    from gru_mpi_cuda_amd.config import preset
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    from gru_mpi_cuda_amd.models import cpu_ref
    from gru_mpi_cuda_amd.models.params import init_params

    cfg = preset(args.preset)
    dev = torch.device("cuda", 0)
    params = init_params(cfg)
    ML = cfg.max_len
    rule = dict(logit_bias={"xqz": -2.0, cfg.eos: -1.0, "ae": 0.5}, presence_penalty=0.5, frequency_penalty=0.5)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.reps

    def side(ts, n):
        med = statistics.median(ts)
        return {"s_median": round(med, 6), "s_min": round(min(ts), 6), "names_per_s": round(n / med, 1),
                "us_per_char_step": round(med / ML * 1e6, 2)}

    def rounds(plain, soft):
        plain(); soft()              # warm-up: both graphs captured
        plain(); soft()
        tp, tm = [], []
        for _ in range(args.rounds):
            tp.append(timed(plain))
            tm.append(timed(soft))
        torch.cuda.synchronize()
        return tp, tm

    base = {"preset": args.preset, "model": f"GRU L={cfg.layers} H={cfg.hidden} E={cfg.embed} V={cfg.vocab}",
            "max_len": ML, "reps": args.reps, "rounds": args.rounds, "data": "random-init weights, seeded uniforms",
            "controls": {"top_k": args.top_k, "top_p": args.top_p, "temperature": args.temperature},
            "soft_controls": {"logit_bias": {str(k): v for k, v in rule["logit_bias"].items()},
                              "presence_penalty": rule["presence_penalty"],
                              "frequency_penalty": rule["frequency_penalty"]}}

    for n in [int(x) for x in args.names.split(",")]:
        gen = HipGenerator(cfg, params, max_batch=n, device=dev, precision="fp32")
        gen.g.set_persist(False)
        s = gen._s()
        rf = torch.from_numpy(np.random.default_rng(7).random((n, ML), dtype=np.float32)).to(dev)
        c = cpu_ref.make_controls(cfg, n, args.temperature, args.top_k, args.top_p)
        ctl = [torch.from_numpy(a).to(dev) for a in (c.inv_temp, c.top_k, c.top_p, c.plen, c.prefix)]
        held = gen._soft_tensors(cpu_ref.make_soft(cfg, n, **rule))
        skw = gen._soft_kwargs(held)
        out_p = torch.empty(n, ML + 1, dtype=torch.uint8, device=dev)
        out_m = torch.empty(n, ML + 1, dtype=torch.uint8, device=dev)

        def plain():
            gen.g.generate_ctl(rf.data_ptr(), n, *[t.data_ptr() for t in ctl], out_p.data_ptr(), s)

        def soft():
            gen.g.generate_ctl(rf.data_ptr(), n, *[t.data_ptr() for t in ctl], out_m.data_ptr(), s, **skw)

        tp, tm = rounds(plain, soft)
        mp, mm = statistics.median(tp), statistics.median(tm)
        differ = float((out_p != out_m).any(1).float().mean())
        print(json.dumps(dict(base, bench="generate_ctl", names=n, plain=side(tp, n), soft=side(tm, n),
                              soft_vs_plain_time=round(mm / mp, 3), extra_us_per_char_step=round((mm - mp) / ML * 1e6, 2),
                              names_changed_by_soft=round(differ, 4), soft_graphs=int(gen.g.soft_graphs()),
                              error_word=int(gen.g.read_error()))), flush=True)

        # score the soft call's rows under both settings
        tok = [torch.empty(n, ML, dtype=torch.float32, device=dev) for _ in range(2)]
        rank = [torch.empty(n, ML, dtype=torch.int32, device=dev) for _ in range(2)]
        name = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2)]
        nt = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2)]
        nk = [torch.empty(n, ML, dtype=torch.int32, device=dev) for _ in range(2)]

        def score(o, kw):
            return lambda: gen.g.score(out_m.data_ptr(), n, tok[o].data_ptr(), rank[o].data_ptr(), name[o].data_ptr(),
                                       nt[o].data_ptr(), s, *[t.data_ptr() for t in ctl], nk[o].data_ptr(), **kw)

        tp, tm = rounds(score(0, {}), score(1, skw))
        mp, mm = statistics.median(tp), statistics.median(tm)
        print(json.dumps(dict(base, bench="score", names=n, plain=side(tp, n), soft=side(tm, n),
                              soft_vs_plain_time=round(mm / mp, 3), extra_us_per_char_step=round((mm - mp) / ML * 1e6, 2),
                              finite_under_soft=round(float(torch.isfinite(name[1]).float().mean()), 4),
                              finite_under_plain=round(float(torch.isfinite(name[0]).float().mean()), 4),
                              error_word=int(gen.g.read_error()))), flush=True)
        del gen
    return 0


if __name__ == "__main__":
    sys.exit(main())

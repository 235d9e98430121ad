#!/usr/bin/env python3
"""Constrained generation benchmark (docs/DESIGN.md §4e): what the mask costs.

* ``generate_ctl`` (top_k = 40, top_p = 0.95, T = 0.8) with and without a constraint -- the same
  per-char graph with the MASK instantiation of ``sample_ctl_f32`` as its sampler node, plus the copy
  of the table and of the batch's idx slice -- at 256 and 4096 names (persistent path off: both sides on
  the per-char graph);
* ``beam`` at 16 prefixes x W = 8 with and without a constraint.

The constraint is "a capital, then letters, 4 to 7 chars".  Same process, same generator, alternating
rounds (unmasked, masked, unmasked, ...); per side the median and the minimum over the rounds.
Device-resident inputs and outputs; host transfer and the Python-side validation excluded (as
bench_sample_ctl.py).  One JSON line per measurement, with the ratio against the unmasked call of the
same run and the microseconds per char step.  No threshold: these are the first measurements.

    python bench/bench_constrained.py [--names 256,4096] [--prefixes 16] [--width 8] [--reps 10] [--rounds 5]
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
    ap.add_argument("--names", default="256,4096", help="comma list: one JSON line per count")
    ap.add_argument("--prefixes", type=int, default=16)
    ap.add_argument("--width", type=int, default=8)
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
        return {"s_median": round(med, 6), "s_min": round(min(ts), 6), "names_per_s": round(n / med, 1),
                "us_per_char_step": round(med / ML * 1e6, 2)}

    def rounds(plain, masked):
        plain(); masked()            # warm-up: both graphs captured
        plain(); masked()
        tp, tm = [], []
        for _ in range(args.rounds):
            tp.append(timed(plain))
            tm.append(timed(masked))
        torch.cuda.synchronize()
        return tp, tm

    base = {"preset": args.preset, "model": f"GRU L={cfg.layers} H={cfg.hidden} E={cfg.embed} V={cfg.vocab}",
            "max_len": ML, "reps": args.reps, "rounds": args.rounds, "data": "random-init weights, seeded uniforms",
            "constraint": {k: v for k, v in rule.items()}}

    for n in [int(x) for x in args.names.split(",")]:
        gen = HipGenerator(cfg, params, max_batch=n, device=dev, precision="fp32")
        gen.g.set_persist(False)
        s = gen._s()
        rf = torch.from_numpy(np.random.default_rng(7).random((n, ML), dtype=np.float32)).to(dev)
        c = cpu_ref.make_controls(cfg, n, args.temperature, args.top_k, args.top_p)
        ctl = [torch.from_numpy(a).to(dev) for a in (c.inv_temp, c.top_k, c.top_p, c.plen, c.prefix)]
        cons = cpu_ref.make_constraints(cfg, n, **rule)
        tab, idx, lines = gen._constraint_tensors(cons)
        out_p = torch.empty(n, ML + 1, dtype=torch.uint8, device=dev)
        out_m = torch.empty(n, ML + 1, dtype=torch.uint8, device=dev)

        def plain():
            gen.g.generate_ctl(rf.data_ptr(), n, *[t.data_ptr() for t in ctl], out_p.data_ptr(), s)

        def masked():
            gen.g.generate_ctl(rf.data_ptr(), n, *[t.data_ptr() for t in ctl], out_m.data_ptr(), s,
                               tab.data_ptr(), idx.data_ptr(), lines)

        tp, tm = rounds(plain, masked)
        rows = out_m.cpu().numpy()
        A = cons.allowed()
        obey = all(all(A[i, l, ch] for l, ch in enumerate(r[:ML]) if l == 0 or r[l - 1] != cfg.eos) for i, r in enumerate(rows[:256]))
        mp, mm = statistics.median(tp), statistics.median(tm)
        print(json.dumps(dict(base, bench="generate_ctl", names=n,
                              controls={"top_k": args.top_k, "top_p": args.top_p, "temperature": args.temperature},
                              unmasked=side(tp, n), masked=side(tm, n), masked_vs_unmasked_time=round(mm / mp, 3),
                              extra_us_per_char_step=round((mm - mp) / ML * 1e6, 2), table_lines=lines,
                              first_256_rows_obey=bool(obey), error_word=int(gen.g.read_error()))), flush=True)
        del gen

    N, W = args.prefixes, args.width
    gen = HipGenerator(cfg, params, max_batch=max(64, N * W), device=dev, precision="fp32")
    s = gen._s()
    pre, plen = cpu_ref.beam_inputs(cfg, [chr(65 + i % 26) for i in range(N)], W)
    p, l = torch.from_numpy(pre).to(dev), torch.from_numpy(plen).to(dev)
    cons = cpu_ref.make_constraints(cfg, N, **rule)
    tab, idx, lines = gen._constraint_tensors(cons)
    outs = [(torch.empty(N, W, ML + 1, dtype=torch.uint8, device=dev), torch.empty(N, W, dtype=torch.float32, device=dev),
             torch.empty(N, W, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)) for _ in range(2)]

    def beam(o, extra=()):
        return lambda: gen.g.beam(l.data_ptr(), p.data_ptr(), N, W, *[t.data_ptr() for t in outs[o]], s, *extra)

    tp, tm = rounds(beam(0), beam(1, (tab.data_ptr(), idx.data_ptr(), lines)))
    mp, mm = statistics.median(tp), statistics.median(tm)
    print(json.dumps(dict(base, bench="beam", prefixes=N, width=W, unmasked=side(tp, N), masked=side(tm, N),
                          masked_vs_unmasked_time=round(mm / mp, 3), extra_us_per_char_step=round((mm - mp) / ML * 1e6, 2),
                          table_lines=lines, beams_found={"unmasked": int(outs[0][3].sum()), "masked": int(outs[1][3].sum())},
                          error_word=int(gen.g.read_error()))), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Controlled sampling benchmark: ``Generator.generate_ctl`` (top_k = 40, top_p = 0.95, T = 0.8) against
plain fp32 ``generate()`` with the persistent path off, i.e. the same per-char graph with
``sample_f32`` in place of ``sample_ctl_f32``, on the reference's model (preset ``ref``).

Same process, same generator, alternating rounds (plain, controlled, plain, ...); per side the median
and the minimum over the rounds.  Device-resident uniforms, controls and outputs, host transfer and
the Python-side validation excluded (as bench_score.py times ``score``).  A char is an emitted
non-NUL byte of that side's own output.  One JSON line per name count.

    python bench/bench_sample_ctl.py [--names 256,4096] [--preset ref] [--reps 10] [--rounds 5]
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
    ap.add_argument("--names", default="256,4096", help="comma list: one JSON line per count")
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

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.reps

    for n in [int(x) for x in args.names.split(",")]:
        gen = HipGenerator(cfg, params, max_batch=n, device=dev, precision="fp32")
        gen.g.set_persist(False)
        rf = torch.from_numpy(np.random.default_rng(7).random((n, ML), dtype=np.float32)).to(dev)

        def controls(T, k, p):
            c = cpu_ref.make_controls(cfg, n, T, k, p)
            return [torch.from_numpy(a).to(dev) for a in (c.inv_temp, c.top_k, c.top_p, c.plen, c.prefix)]

        ctl = controls(args.temperature, args.top_k, args.top_p)
        # where the extra time goes: the same graph with neither search (the extra loads and branches
        # alone), with the top-k bisection only, with the top-p bisection only
        parts = {"neutral": controls(1.0, 0, 1.0), "top_k_only": controls(1.0, args.top_k, 1.0),
                 "top_p_only": controls(1.0, 0, args.top_p)}
        out_p = torch.empty(n, ML + 1, dtype=torch.uint8, device=dev)
        out_c = torch.empty(n, ML + 1, dtype=torch.uint8, device=dev)
        out_x = torch.empty(n, ML + 1, dtype=torch.uint8, device=dev)
        s = gen._s()

        def plain():
            gen.g.generate(rf.data_ptr(), n, out_p.data_ptr(), s)

        def controlled():
            gen.g.generate_ctl(rf.data_ptr(), n, *[t.data_ptr() for t in ctl], out_c.data_ptr(), s)

        def part(name):
            return lambda: gen.g.generate_ctl(rf.data_ptr(), n, *[t.data_ptr() for t in parts[name]], out_x.data_ptr(), s)

        plain(); controlled()            # warm-up: both graphs captured
        plain(); controlled()
        tp, tc, tx = [], [], {k: [] for k in parts}
        for _ in range(args.rounds):
            tp.append(timed(plain))
            tc.append(timed(controlled))
            for k in parts:
                tx[k].append(timed(part(k)))
        torch.cuda.synchronize()
        cp, cc = int((out_p != 0).sum()), int((out_c != 0).sum())

        def side(ts, chars):
            med = statistics.median(ts)
            return {"s_median": round(med, 6), "s_min": round(min(ts), 6), "names_per_s": round(n / med, 1),
                    "chars": chars, "chars_per_s": round(chars / med, 1), "us_per_char_step": round(med / ML * 1e6, 2)}

        mp, mc = statistics.median(tp), statistics.median(tc)
        res = {"preset": args.preset, "model": f"GRU L={cfg.layers} H={cfg.hidden} E={cfg.embed} V={cfg.vocab}",
               "max_len": ML, "names": n, "reps": args.reps, "rounds": args.rounds,
               "data": "random-init weights, seeded uniforms",
               "controls": {"top_k": args.top_k, "top_p": args.top_p, "temperature": args.temperature},
               "plain_fp32_graph": side(tp, cp), "controlled": side(tc, cc),
               "controlled_vs_plain_time": round(mc / mp, 3),
               "extra_us_per_char_step": round((mc - mp) / ML * 1e6, 2),
               "extra_us_per_char_step_by_part": {k: round((statistics.median(v) - mp) / ML * 1e6, 2)
                                                  for k, v in tx.items()},
               "ctl_workspace_kb": round(gen.g.ctl_workspace_bytes() / 1024, 1),
               "error_word": int(gen.g.read_error())}
        print(json.dumps(res), flush=True)
        del gen
    return 0


if __name__ == "__main__":
    sys.exit(main())

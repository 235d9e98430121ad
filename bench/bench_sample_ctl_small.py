#!/usr/bin/env python3
"""Controlled sampling on small batches: the controlled persistent launch against the per-char
controlled graph it replaces, on the reference's model (preset ``ref``), fp32.

Arms, per name count (1, 8, 16, 32, 64):
  (a) ``generate_ctl`` with top_k = 40, top_p = 0.95, T = 0.8 -- one controlled persistent launch;
  (b) the same call with ``set_persist(False)`` -- the per-char controlled graph, the comparator that
      decides the default of GK_GEN_PERSIST_CTL_MAX;
  (c) plain ``generate()`` -- the plain persistent launch;
  (d) (a)'s path with a 3-char prefix and no other control.

Same process, one generator, alternating rounds (a, b, c, d, a, ...); per arm the median, the minimum
and the spread (max - min) over the rounds of ``reps`` calls.  Device-resident uniforms, controls and
outputs; host transfer and the Python-side validation excluded (the form of bench_sample_ctl.py).  One
JSON line per name count; ``persist_wins`` is (a)'s median below (b)'s by more than (b)'s spread.

    python bench/bench_sample_ctl_small.py [--names 1,8,16,32,64] [--preset ref] [--reps 10] [--rounds 5]
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
    ap.add_argument("--names", default="1,8,16,32,64", help="comma list: one JSON line per count")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--top-k", dest="top_k", type=int, default=40)
    ap.add_argument("--top-p", dest="top_p", type=float, default=0.95)
    ap.add_argument("--temperature", type=float, default=0.8)
    ap.add_argument("--prefix", default="Mar")
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
        gen = HipGenerator(cfg, params, max_batch=max(n, 64), device=dev, precision="fp32")
        g = gen.g
        g.set_persist_ctl_max(64)      # the arms choose the path themselves, whatever the default is
        rf = torch.from_numpy(np.random.default_rng(7).random((n, ML), dtype=np.float32)).to(dev)

        def controls(T, k, p, prefix=None):
            c = cpu_ref.make_controls(cfg, n, T, k, p, prefix)
            return [torch.from_numpy(a).to(dev) for a in (c.inv_temp, c.top_k, c.top_p, c.plen, c.prefix)]

        ctl = controls(args.temperature, args.top_k, args.top_p)
        pre = controls(None, None, None, args.prefix)
        outs = {k: torch.empty(n, ML + 1, dtype=torch.uint8, device=dev) for k in "abcd"}
        s = gen._s()

        def call_ctl(arrays, out, persist):
            def fn():
                g.set_persist(persist)
                g.generate_ctl(rf.data_ptr(), n, *[t.data_ptr() for t in arrays], out.data_ptr(), s)
            return fn

        def plain():
            g.set_persist(True)
            g.generate(rf.data_ptr(), n, outs["c"].data_ptr(), s)

        arms = {"a": call_ctl(ctl, outs["a"], True), "b": call_ctl(ctl, outs["b"], False), "c": plain,
                "d": call_ctl(pre, outs["d"], True)}
        g.set_persist(True)
        on_persist = bool(g.uses_persist_ctl(n))
        for _ in range(2):             # warm-up: the workspace filled, the graph captured
            for fn in arms.values():
                fn()
        ts = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():
                ts[k].append(timed(fn))
        torch.cuda.synchronize()
        g.set_persist(True)
        same_rows = bool((outs["a"] == outs["b"]).all())

        def side(k):
            med = statistics.median(ts[k])
            return {"s_median": round(med, 7), "s_min": round(min(ts[k]), 7), "s_spread": round(max(ts[k]) - min(ts[k]), 7),
                    "us_per_char_step": round(med / ML * 1e6, 2), "chars": int((outs[k] != 0).sum())}

        ma, mb = statistics.median(ts["a"]), statistics.median(ts["b"])
        spread_b = max(ts["b"]) - min(ts["b"])
        res = {"preset": args.preset, "model": f"GRU L={cfg.layers} H={cfg.hidden} E={cfg.embed} V={cfg.vocab}",
               "max_len": ML, "names": n, "reps": args.reps, "rounds": args.rounds,
               "data": "random-init weights, seeded uniforms",
               "controls": {"top_k": args.top_k, "top_p": args.top_p, "temperature": args.temperature, "prefix_arm_d": args.prefix},
               "a_ctl_persistent": side("a"), "b_ctl_per_char_graph": side("b"), "c_plain_persistent": side("c"),
               "d_prefix_only_persistent": side("d"),
               "arm_a_on_persistent_launch": on_persist, "a_rows_equal_b_rows": same_rows,
               "a_vs_b_time": round(ma / mb, 3), "persist_wins": bool(mb - ma > spread_b),
               "ctl_extra_us_per_char_step_vs_plain": round((ma - statistics.median(ts["c"])) / ML * 1e6, 2),
               "error_word": int(g.read_error())}
        print(json.dumps(res), flush=True)
        del gen
    return 0


if __name__ == "__main__":
    sys.exit(main())

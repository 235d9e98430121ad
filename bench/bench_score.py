#!/usr/bin/env python3
"""Scoring benchmark: ``HipGenerator.score`` (teacher-forced log-likelihood, layer-major schedule,
exact fp32) on the reference's model (preset ``ref``), with fp32 ``generate()`` of the same name
counts in the same process for comparison.

Rows to score are the generator's own fp32 output for seeded uniforms, so both sides walk the same
names.  Metrics: names/s and chars/s, where a char is a scored token for ``score`` (every char incl.
the EOS, a cut-off name's max_len chars) and an emitted char for ``generate`` (every non-NUL byte, as
bench_generate.py counts them); device-resident inputs and outputs, host transfer excluded.  One JSON
line per name count.

    python bench/bench_score.py [--names 32,256,4096] [--preset ref] [--reps 10]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="ref")
    ap.add_argument("--names", default="32,256,4096", help="comma list: one JSON line per count")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()

    from gru_mpi_cuda_amd.config import preset
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    from gru_mpi_cuda_amd.models.params import init_params

    cfg = preset(args.preset)
    dev = torch.device("cuda", 0)
    params = init_params(cfg)
    ML = cfg.max_len

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.reps

    for n in [int(x) for x in args.names.split(",")]:
        gen = HipGenerator(cfg, params, max_batch=n, device=dev, precision="fp32")
        rf = torch.from_numpy(np.random.default_rng(7).random((n, ML), dtype=np.float32)).to(dev)
        rows = gen.generate_device(rf, n)
        emitted = int((rows != 0).sum())
        s = gen._s()
        tok = torch.empty(n, ML, dtype=torch.float32, device=dev)
        rank = torch.empty(n, ML, dtype=torch.int32, device=dev)
        name = torch.empty(n, dtype=torch.float32, device=dev)
        nt = torch.empty(n, dtype=torch.int32, device=dev)

        def score():
            gen.g.score(rows.data_ptr(), n, tok.data_ptr(), rank.data_ptr(), name.data_ptr(), nt.data_ptr(), s)

        dt_s = timed(score)
        tokens = int(nt.sum())
        dt_g = timed(lambda: gen.generate_device(rf, n))
        res = {"preset": args.preset, "model": f"GRU L={cfg.layers} H={cfg.hidden} E={cfg.embed} V={cfg.vocab}",
               "max_len": ML, "names": n, "reps": args.reps, "data": "random-init weights, seeded uniforms",
               "score": {"s": round(dt_s, 6), "names_per_s": round(n / dt_s, 1), "tokens": tokens,
                         "chars_per_s": round(tokens / dt_s, 1),
                         "emitted_chars_per_s": round(emitted / dt_s, 1),   # generate's count of the same rows
                         "workspace_mb": round(gen.g.score_workspace_bytes() / 2 ** 20, 1)},
               "generate_fp32": {"s": round(dt_g, 6), "names_per_s": round(n / dt_g, 1), "chars": emitted,
                                 "chars_per_s": round(emitted / dt_g, 1),
                                 "persistent": bool(gen.g.uses_persist(n))},
               "score_vs_generate_time": round(dt_g / dt_s, 2), "error_word": int(gen.g.read_error())}
        print(json.dumps(res), flush=True)
        del gen
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Fast bf16 scoring benchmark: ``HipGenerator.score(fast=True)``'s native call (``score_fast``: bf16 MFMA steps
and the fused ``score_head_bf16``) against the exact-fp32 ``score`` of the same rows on the same bf16
generator, in one process, on the reference's model (preset ``ref``).

Rows are the generator's own output for seeded uniforms.  The two paths alternate over ``--rounds`` rounds of
``--reps`` calls each (both warmed first: the warm-up records their graphs); a round's time is a host clock
around work that ends in a device synchronise.  Per path the record holds every round, their median and their
spread (max - min); ``fast_beats_fp32_spread`` says whether the medians differ by more than the fp32 path's
own spread.  A char is a scored token.  Device-resident inputs and outputs, host transfer excluded.  One JSON
line per name count, appended to ``--out`` when given.

    python bench/bench_score_fast.py [--names 256,4096,32768] [--rounds 7] [--reps 10] [--out profiles/score_fast_bench.jsonl]
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
    ap.add_argument("--names", default="256,4096,32768", help="comma list: one JSON line per count")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from gru_mpi_cuda_amd.config import preset
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    from gru_mpi_cuda_amd.models.params import init_params

    cfg = preset(args.preset)
    dev = torch.device("cuda", 0)
    params = init_params(cfg)
    ML = cfg.max_len

    for n in [int(x) for x in args.names.split(",")]:
        gen = HipGenerator(cfg, params, max_batch=min(n, 4096), device=dev, precision="bf16")
        rf = torch.from_numpy(np.random.default_rng(7).random((n, ML), dtype=np.float32)).to(dev)
        rows = gen.generate_device(rf, n)
        s = gen._s()
        out = {k: (torch.empty(n, ML, dtype=torch.float32, device=dev), torch.empty(n, ML, dtype=torch.int32, device=dev),
                   torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
               for k in ("fast", "fp32")}
        call = {k: (lambda f=getattr(gen.g, m), o=out[k]: f(rows.data_ptr(), n, *[t.data_ptr() for t in o], s))
                for k, m in (("fast", "score_fast"), ("fp32", "score"))}
        times = {"fast": [], "fp32": []}
        for k in call:
            call[k]()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for k in ("fp32", "fast"):
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    call[k]()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / args.reps)
        tokens = int(out["fast"][3].sum())
        mask = torch.arange(ML, device=dev)[None, :] < out["fp32"][3][:, None]
        diff = (out["fast"][0] - out["fp32"][0]).abs()[mask]
        rec = {"preset": args.preset, "model": f"GRU L={cfg.layers} H={cfg.hidden} E={cfg.embed} V={cfg.vocab}",
               "max_len": ML, "names": n, "rounds": args.rounds, "reps": args.reps, "tokens": tokens,
               "data": "random-init weights, seeded uniforms"}
        for k in times:
            med = float(np.median(times[k]))
            rec[k] = {"s_rounds": [round(t, 6) for t in times[k]], "s_median": round(med, 6),
                      "s_spread": round(max(times[k]) - min(times[k]), 6), "chars_per_s": round(tokens / med, 1)}
        rec["fp32_over_fast"] = round(rec["fp32"]["s_median"] / rec["fast"]["s_median"], 2)
        rec["fast_beats_fp32_spread"] = bool(rec["fp32"]["s_median"] - rec["fast"]["s_median"] > rec["fp32"]["s_spread"])
        rec["n_tok_equal"] = bool(torch.equal(out["fast"][3], out["fp32"][3]))
        rec["max_abs_tok_logp_diff"] = float(diff.max())
        rec["rank_equal_share"] = round(float((out["fast"][1] == out["fp32"][1])[mask].float().mean()), 4)
        rec["workspace_mb"] = round(gen.g.score_workspace_bytes() / 2 ** 20, 1)
        rec["error_word"] = int(gen.g.read_error())
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
        del gen
    return 0


if __name__ == "__main__":
    sys.exit(main())

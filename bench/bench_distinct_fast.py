#!/usr/bin/env python3
"""Fast bf16 distinct names benchmark: ``HipGenerator.sample_distinct(fast=True)``'s native call (``distinct_fast``:
bf16 MFMA steps, the fused ``sbs_head_bf16``, ``sbs_merge``, ``beam_reorder_bf16``) on a bf16 generator against
the exact-fp32 ``distinct`` of the same prefixes on an fp32 generator with the same weights, in one process, on
the reference's model (preset ``ref``).

Prefixes are seeded letters of length 0 .. 3.  The two paths alternate over ``--rounds`` rounds of ``--reps`` calls
each (both warmed first: the warm-up records their graphs); a round's time is a host clock around work that ends
in a device synchronise.  Per path the record holds every round, their median and their spread (max - min);
``fast_beats_both_spreads`` says whether the medians differ by more than the sum of the two spreads.
Device-resident inputs and outputs, host transfer excluded.  One JSON line per (prefixes, width), appended to
``--out`` when given.

    python bench/bench_distinct_fast.py [--prefixes 16,256,2048] [--widths 4,8,16] [--rounds 7] [--reps 5] [--out profiles/distinct_fast_bench.jsonl]
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
    ap.add_argument("--prefixes", default="16,256,2048", help="comma list of prefix counts")
    ap.add_argument("--widths", default="4,8,16")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from gru_mpi_cuda_amd.config import preset
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    from gru_mpi_cuda_amd.models import cpu_ref
    from gru_mpi_cuda_amd.models.params import init_params

    cfg = preset(args.preset)
    dev = torch.device("cuda", 0)
    params = init_params(cfg)
    ML = cfg.max_len
    gens = {"fast": HipGenerator(cfg, params, max_batch=4096, device=dev, precision="bf16"),
            "fp32": HipGenerator(cfg, params, max_batch=4096, device=dev, precision="fp32")}
    method = {"fast": "distinct_fast", "fp32": "distinct"}

    for n in [int(x) for x in args.prefixes.split(",")]:
        rng = np.random.default_rng(7)
        words = ["".join(chr(97 + int(c)) for c in rng.integers(0, 26, int(ln))) for ln in rng.integers(0, 4, n)]
        pre, plen, inv, seed, start = cpu_ref.distinct_inputs(cfg, words, 4, None, 1, 0, None)
        p, l, it = torch.from_numpy(pre).to(dev), torch.from_numpy(plen).to(dev), torch.from_numpy(inv).to(dev)
        for W in [int(x) for x in args.widths.split(",")]:
            out = {k: (torch.empty(n, W, ML + 1, dtype=torch.uint8, device=dev), torch.empty(n, W, dtype=torch.float32, device=dev),
                       torch.empty(n, W, dtype=torch.float32, device=dev), torch.empty(n, W, dtype=torch.int32, device=dev),
                       torch.empty(n, dtype=torch.int32, device=dev)) for k in gens}
            call = {k: (lambda f=getattr(gens[k].g, method[k]), o=out[k], s=gens[k]._s():
                        f(l.data_ptr(), p.data_ptr(), n, W, seed, start, it.data_ptr(), *[t.data_ptr() for t in o], s))
                    for k in gens}
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
            same = (out["fast"][0] == out["fp32"][0]).all(-1)
            both = torch.isfinite(out["fast"][1]) & torch.isfinite(out["fp32"][1]) & same
            rec = {"preset": args.preset, "model": f"GRU L={cfg.layers} H={cfg.hidden} E={cfg.embed} V={cfg.vocab}",
                   "max_len": ML, "prefixes": n, "width": W, "rows": n * W, "rounds": args.rounds, "reps": args.reps,
                   "data": "random-init weights, seeded prefixes of 0-3 letters, search seed 1, temperature 1"}
            for k in times:
                med = float(np.median(times[k]))
                rec[k] = {"s_rounds": [round(t, 6) for t in times[k]], "s_median": round(med, 6),
                          "s_spread": round(max(times[k]) - min(times[k]), 6),
                          "us_per_char_step": round(med / ML * 1e6, 2)}
            rec["fp32_over_fast"] = round(rec["fp32"]["s_median"] / rec["fast"]["s_median"], 2)
            rec["fast_beats_both_spreads"] = bool(rec["fp32"]["s_median"] - rec["fast"]["s_median"] >
                                                  rec["fp32"]["s_spread"] + rec["fast"]["s_spread"])
            rec["same_row_share"] = round(float(same.float().mean()), 4)
            rec["max_abs_logq_diff_same_rows"] = float((out["fast"][1] - out["fp32"][1]).abs()[both].max()) if bool(both.any()) else None
            rec["n_found_equal"] = bool(torch.equal(out["fast"][4], out["fp32"][4]))
            rec["workspace_mb"] = round(gens["fast"].g.beam_workspace_bytes() / 2 ** 20, 1)
            rec["error_word"] = int(gens["fast"].g.read_error()) | int(gens["fp32"].g.read_error())
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

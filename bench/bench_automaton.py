#!/usr/bin/env python3
"""Automaton-constrained generation benchmark (docs/DESIGN.md §4g): what the state costs against the
per-position mask of §4e.

The language is "a capital, then 3 to 6 lower-case letters", written twice: as ``regex`` (an automaton:
the sampler reads its line from a per-row state and stores the successor, one 2-byte load and one 4-byte
store per row and step) and as ``pattern`` + ``charset`` + ``min_len`` + ``max_len`` (a line per position).

* ``generate_ctl`` (top_k = 40, top_p = 0.95, T = 0.8) at 256 and 4096 names, persistent path off: both
  sides on the per-char controlled graph;
* ``beam`` at 16 prefixes x W = 8;
* one ``generate_ctl`` run of the regex with a 5000-name exclusion list drawn from the language (the host-side
  build time of the tables is reported apart).

Same process, same generator, alternating rounds (pattern, regex, pattern, ...); per side the median and the
minimum over the rounds.  Device-resident inputs and outputs; host transfer and the Python-side compilation
excluded (as bench_constrained.py).  One JSON line per measurement, appended to --out as well.  No
threshold: these are the first measurements.

    python bench/bench_automaton.py [--names 256,4096] [--prefixes 16] [--width 8] [--reps 10] [--rounds 5]
"""
from __future__ import annotations

import argparse
import json
import os
import re
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
    ap.add_argument("--exclude", type=int, default=5000, help="names in the exclusion list of the last run")
    ap.add_argument("--top-k", dest="top_k", type=int, default=40)
    ap.add_argument("--top-p", dest="top_p", type=float, default=0.95)
    ap.add_argument("--temperature", type=float, default=0.8)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "automaton_bench.jsonl"))
    args = ap.parse_args()

    from gru_mpi_cuda_amd.config import preset
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    from gru_mpi_cuda_amd.models import cpu_ref
    from gru_mpi_cuda_amd.models.params import init_params

    cfg = preset(args.preset)
    dev = torch.device("cuda", 0)
    params = init_params(cfg)
    ML = cfg.max_len
    hi = min(7, ML)
    rx = "[A-Z][a-z]{3,%d}" % (hi - 1)
    as_regex = dict(regex=rx)
    as_pattern = dict(pattern="[A-Z]", charset=string.ascii_lowercase, min_len=4, max_len=hi)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

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

    def rounds(a, b):
        a(); b()            # warm-up: both graphs captured
        a(); b()
        ta, tb = [], []
        for _ in range(args.rounds):
            ta.append(timed(a))
            tb.append(timed(b))
        torch.cuda.synchronize()
        return ta, tb

    def in_language(rows, banned=()):
        names = [bytes(r[:ML]).split(bytes([cfg.eos]))[0].decode("latin-1") for r in rows]
        return all(re.fullmatch(rx, nm) and nm not in banned for nm in names)

    base = {"preset": args.preset, "model": f"GRU L={cfg.layers} H={cfg.hidden} E={cfg.embed} V={cfg.vocab}",
            "max_len": ML, "reps": args.reps, "rounds": args.rounds, "data": "random-init weights, seeded uniforms",
            "language": rx, "controls": {"top_k": args.top_k, "top_p": args.top_p, "temperature": args.temperature}}

    def ctl_call(gen, n, rf, ctl, out, held):
        extra = gen._constraint_args(held)
        return lambda: gen.g.generate_ctl(rf.data_ptr(), n, *[t.data_ptr() for t in ctl], out.data_ptr(), gen._s(), *extra)

    for n in [int(x) for x in args.names.split(",")]:
        gen = HipGenerator(cfg, params, max_batch=n, device=dev, precision="fp32")
        gen.g.set_persist(False)
        rf = torch.from_numpy(np.random.default_rng(7).random((n, ML), dtype=np.float32)).to(dev)
        c = cpu_ref.make_controls(cfg, n, args.temperature, args.top_k, args.top_p)
        ctl = [torch.from_numpy(a).to(dev) for a in (c.inv_temp, c.top_k, c.top_p, c.plen, c.prefix)]
        pos = gen._constraint_tensors(cpu_ref.make_constraints(cfg, n, **as_pattern))
        aut_h = cpu_ref.make_constraints(cfg, n, **as_regex)
        aut = gen._constraint_tensors(aut_h)
        out_p = torch.empty(n, ML + 1, dtype=torch.uint8, device=dev)
        out_a = torch.empty(n, ML + 1, dtype=torch.uint8, device=dev)
        tp, ta = rounds(ctl_call(gen, n, rf, ctl, out_p, pos), ctl_call(gen, n, rf, ctl, out_a, aut))
        mp, ma = statistics.median(tp), statistics.median(ta)
        emit(dict(base, bench="generate_ctl", names=n, pattern=side(tp, n), regex=side(ta, n),
                  regex_vs_pattern_time=round(ma / mp, 3), extra_us_per_char_step=round((ma - mp) / ML * 1e6, 2),
                  states=aut_h.states, table_lines=pos[2], rows_identical=bool(torch.equal(out_p, out_a)),
                  rows_in_language=bool(in_language(out_a.cpu().numpy()[:256])), error_word=int(gen.g.read_error())))
        if n == max(int(x) for x in args.names.split(",")) and args.exclude > 0:
            # the exclusion list: names of the language itself, so that the trie survives the intersection
            rng = np.random.default_rng(11)
            banned = sorted({chr(65 + int(rng.integers(26))) + "".join(string.ascii_lowercase[int(v)] for v in rng.integers(0, 26, int(rng.integers(3, hi))))
                             for _ in range(args.exclude)})
            t0 = time.perf_counter()
            ex_h = cpu_ref.make_constraints(cfg, n, regex=rx, exclude=banned)
            build_s = time.perf_counter() - t0
            ex = gen._constraint_tensors(ex_h)
            out_e = torch.empty(n, ML + 1, dtype=torch.uint8, device=dev)
            tp, te = rounds(ctl_call(gen, n, rf, ctl, out_p, pos), ctl_call(gen, n, rf, ctl, out_e, ex))
            mp, me = statistics.median(tp), statistics.median(te)
            emit(dict(base, bench="generate_ctl+exclude", names=n, excluded=len(banned), pattern=side(tp, n), regex_exclude=side(te, n),
                      regex_exclude_vs_pattern_time=round(me / mp, 3), extra_us_per_char_step=round((me - mp) / ML * 1e6, 2),
                      states=ex_h.states, table_bytes=int(ex_h.tab.nbytes + ex_h.nxt.nbytes), host_build_s=round(build_s, 3),
                      rows_in_language=bool(in_language(out_e.cpu().numpy()[:256], set(banned))),
                      error_word=int(gen.g.read_error())))
        del gen

    N, W = args.prefixes, args.width
    gen = HipGenerator(cfg, params, max_batch=max(64, N * W), device=dev, precision="fp32")
    s = gen._s()
    pre, plen = cpu_ref.beam_inputs(cfg, [chr(65 + i % 26) for i in range(N)], W)
    p, l = torch.from_numpy(pre).to(dev), torch.from_numpy(plen).to(dev)
    pos = gen._constraint_tensors(cpu_ref.make_constraints(cfg, N, **as_pattern))
    aut_h = cpu_ref.make_constraints(cfg, N, **as_regex)
    aut = gen._constraint_tensors(aut_h)
    outs = [(torch.empty(N, W, ML + 1, dtype=torch.uint8, device=dev), torch.empty(N, W, dtype=torch.float32, device=dev),
             torch.empty(N, W, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)) for _ in range(2)]

    def beam(o, held):
        extra = gen._constraint_args(held)
        return lambda: gen.g.beam(l.data_ptr(), p.data_ptr(), N, W, *[t.data_ptr() for t in outs[o]], s, *extra)

    tp, ta = rounds(beam(0, pos), beam(1, aut))
    mp, ma = statistics.median(tp), statistics.median(ta)
    emit(dict(base, bench="beam", prefixes=N, width=W, pattern=side(tp, N), regex=side(ta, N),
              regex_vs_pattern_time=round(ma / mp, 3), extra_us_per_char_step=round((ma - mp) / ML * 1e6, 2),
              states=aut_h.states, table_lines=pos[2],
              results_identical=bool(all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))),
              error_word=int(gen.g.read_error())))
    return 0


if __name__ == "__main__":
    sys.exit(main())

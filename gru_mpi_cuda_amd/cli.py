"""Command-line entry point.

    python -m gru_mpi_cuda_amd.cli train    --preset h512 --steps 200 --ckpt out/model.bin
    python -m gru_mpi_cuda_amd.cli generate --ckpt out/model.bin -n 20 --seed 1
    python -m gru_mpi_cuda_amd.cli generate --ckpt out/model.bin -n 20 --prefix Mar --temperature 0.8 --top-k 40 --top-p 0.95
    python -m gru_mpi_cuda_amd.cli score    --ckpt out/model.bin --names heldout.txt
    python -m gru_mpi_cuda_amd.cli score    --ckpt out/model.bin --names heldout.txt --temperature 0.8 --top-k 40 --pattern '[A-Z]'
    python -m gru_mpi_cuda_amd.cli beam     --ckpt out/model.bin --width 5 --prefix Mar
    python -m gru_mpi_cuda_amd.cli generate --ckpt out/model.bin -n 200 --regex '.*son' --exclude-file train.txt --exclude-emitted
    python -m gru_mpi_cuda_amd.cli distinct --ckpt out/model.bin --width 20 --prefix Mar --seed 1
    python -m gru_mpi_cuda_amd.cli conditional --ckpt out/model.bin --regex '.*son' --width 16 --runs 8
    python -m gru_mpi_cuda_amd.cli info
    python -m gru_mpi_cuda_amd.cli bench    [bench.py args]

Multi-GPU: launch with ``python -m torch.distributed.run --nproc-per-node N ...`` (one process
per GPU; RANK / WORLD_SIZE / LOCAL_RANK from the launcher).  The reference's own driver
(main.cpp, missing from the repo) called namegen_initialize / namegen /
namegen_finalize -- ``generate`` does exactly that; the native equivalent without Python is
``gru_mpi_cuda_amd/bin/namegen``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from typing import Optional

import numpy as np


def _add_model_args(ap: argparse.ArgumentParser, skip=()) -> None:
    for name, typ in (("vocab", int), ("embed", int), ("hidden", int), ("layers", int), ("batch", int),
                      ("seq", int), ("lr", float), ("max_len", int), ("sos", int), ("eos", int),
                      ("clip_norm", float), ("seed", int), ("bucket_mb", float), ("time_chunks", int),
                      ("warmup_steps", int), ("total_steps", int), ("lr_min", float)):
        if name in skip:
            continue
        ap.add_argument("--" + name.replace("_", "-"), dest=name, type=typ, default=None)
    ap.add_argument("--optimizer", choices=["adam", "sgd"], default=None)
    ap.add_argument("--lr-sched", dest="lr_sched", choices=["const", "cosine", "linear"], default=None,
                    help="learning-rate decay after --warmup-steps, down to --lr-min at --total-steps")
    ap.add_argument("--shard-optim", dest="shard_optim", type=int, nargs="?", const=1, default=None, choices=[0, 1, 2],
                    help="data-parallel: sharded optimiser step (reduce-scatter, Adam on 1/world, all-gather of "
                         "the fp32 masters (1) or of the bf16 working copies (2))")
    ap.add_argument("--carry-hidden", dest="carry_hidden", action="store_const", const=True, default=None,
                    help="truncated BPTT: carry each step's final hidden state into the next step")


def _cfg_from(args):
    from .config import preset
    cfg = preset(args.preset)
    over = {k: v for k, v in vars(args).items()
            if k in cfg.__dataclass_fields__ and v is not None}
    return cfg.replace(**over)


def save_checkpoint(tr, path: str, fmt: str = "gen") -> None:
    """Weights (reference or generalised layout) + Adam state + step counter (rank 0 writes)."""
    import torch
    from .utils import ckpt
    # optimiser state first, on EVERY rank: with a sharded optimiser it is a collective (the moment
    # slices other ranks own are all-gathered); only then do the non-writing ranks leave
    if hasattr(tr, "t"):                    # HipTrainer
        (m, v), step = tr.opt_state(), tr.t.get_step()
    else:
        m, v, step = tr.opt_state()
    if getattr(tr, "ctx", None) is not None and not tr.ctx.is_main:
        return
    cfg = tr.cfg
    params = tr.state_dict()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    ckpt.save(path, cfg, params, fmt=fmt,
              opt_state={"m": m, "v": v, "step": torch.tensor([step], dtype=torch.int64)})


def _read_checkpoint(tr, path: Optional[str]):
    """(params dict, opt-state dict or None).  Data-parallel: only rank 0 opens the file; the
    flat weights, Adam moments and step go to the other ranks by broadcast (SURVEY §5.4 -- the
    reference has every rank read the blob, namegensf.cu:368-372, §2.7 item 4), so ranks > 0
    need neither the file nor a shared filesystem."""
    import torch
    from .models.params import flat_layout, from_flat, to_flat
    from .utils import ckpt
    ctx = getattr(tr, "ctx", None)
    if ctx is None or ctx.world <= 1:
        _, params = ckpt.load(path, tr.cfg)
        return params, ckpt.load_opt_state(path)
    import torch.distributed as dist
    dev = ctx.device if ctx.backend == "nccl" else torch.device("cpu")
    n = flat_layout(tr.cfg).total
    hdr = torch.zeros(2, dtype=torch.int64, device=dev)   # [has optimiser state, step]
    flat = torch.zeros(3 * n, dtype=torch.float32, device=dev)
    if ctx.is_main:
        _, params = ckpt.load(path, tr.cfg)
        st = ckpt.load_opt_state(path)
        flat[:n] = to_flat(tr.cfg, params).to(dev)
        if st is not None:
            flat[n:2 * n] = st["m"].float().to(dev)
            flat[2 * n:] = st["v"].float().to(dev)
            hdr[0], hdr[1] = 1, int(st["step"][0])
    dist.broadcast(hdr, 0)
    dist.broadcast(flat, 0)
    flat, hdr = flat.cpu(), hdr.cpu()
    params = from_flat(tr.cfg, flat[:n])
    st = None
    if int(hdr[0]):
        st = {"m": flat[n:2 * n].clone(), "v": flat[2 * n:].clone(),
              "step": torch.tensor([int(hdr[1])], dtype=torch.int64)}
    return params, st


def load_checkpoint(tr, path: Optional[str]) -> int:
    """Restore weights (+ optimiser state when present) into a trainer; returns the step.
    ``path`` is only read on rank 0 (may be None elsewhere)."""
    params, st = _read_checkpoint(tr, path)
    if hasattr(tr, "t"):
        tr.load_state(params)
        if st is not None:
            tr.load_opt_state(st["m"], st["v"])
            tr.t.set_step(int(st["step"][0]))
    else:
        for k in tr.params:
            tr.params[k].copy_(params[k])
        if st is not None:
            tr.load_opt_state(st["m"], st["v"], int(st["step"][0]))
    return int(st["step"][0]) if st is not None else 0


def cmd_train(args) -> int:
    import torch
    from .parallel import dist as gdist
    from .parallel.rccl import make_comm
    from .engine.trainer import make_trainer
    from .utils.data import make_stream
    from .utils.metrics import MetricsWriter, StepTimer, log
    ctx = gdist.init(use_gpu=torch.cuda.is_available() and not args.cpu, verbose=True)
    cfg = _cfg_from(args)
    if cfg.lr_sched != "const" and cfg.total_steps <= 0:
        if args.resume:
            # the resumed run restores the step counter: a default of --steps would put the whole run
            # past the end of the schedule (at lr_min, warm-up skipped)
            raise SystemExit("--resume with --lr-sched cosine/linear needs --total-steps (the schedule's "
                             "length across restarts)")
        cfg = cfg.replace(total_steps=args.steps)   # decay over this run
    comm = make_comm(ctx) if ctx.device.type == "cuda" else None
    tr = make_trainer(cfg, ctx, comm=comm)
    start = load_checkpoint(tr, args.resume) if args.resume else 0
    if hasattr(tr, "t"):
        log(f"plan: {tr.t.plan()}, workspace {tr.t.workspace_bytes() / 2**20:.1f} MiB")
    data = make_stream(cfg.batch // ctx.world, cfg.seq, cfg.sos, cfg.eos, seed=cfg.seed * 1000 + ctx.rank + start,
                       max_len=cfg.max_len, path=args.data)
    mw = MetricsWriter(args.metrics)
    evaluate = _Evaluator(args.eval_data, cfg, ctx.device.type == "cuda") if args.eval_data else None
    timer = StepTimer()
    for it in range(start, start + args.steps):
        tr.step(*data.next())
        timer.tick()
        last = it + 1 == start + args.steps
        do_eval = evaluate is not None and (last or (args.eval_every > 0 and (it + 1) % args.eval_every == 0))
        if (it + 1) % args.log_every == 0 or last or do_eval:
            loss = tr.loss()                # synchronises
            r = timer.rate()
            tok_s = r["steps_per_s"] * cfg.batch * cfg.seq
            rec = dict(step=it + 1, loss=loss, tokens_per_s=tok_s, world=ctx.world,
                       ms_per_step=1e3 / r["steps_per_s"] if r["steps_per_s"] else None)
            if ctx.device.type == "cuda":
                free, total = torch.cuda.mem_get_info(ctx.device)
                rec["hbm_used_gb"] = (total - free) / 2 ** 30
                if hasattr(tr, "t"):
                    rec["workspace_mb"] = tr.t.workspace_bytes() / 2 ** 20
                if hasattr(tr, "comm_stats"):
                    cs = tr.comm_stats()
                    rec.update(cs)
                    if cs and rec["ms_per_step"]:
                        # upper bound of the step share the collectives take if none of it overlaps
                        rec["allreduce_step_fraction_max"] = cs["allreduce_ms_standalone"] / rec["ms_per_step"]
                timer.rate()                # the probe above is not training time
            ev = ""
            if do_eval:
                rec.update(evaluate(tr))
                ev = f" eval nll {rec['eval_nll']:.4f} ppl {rec['eval_ppl']:.2f} top1 {rec['eval_top1']:.3f}"
                timer.rate()                # nor is the evaluation
            log(f"step {it + 1} loss {loss:.4f} {tok_s / 1e6:.2f} M char-tokens/s{ev}")
            mw.write(**rec)
        if args.ckpt and args.save_every and (it + 1) % args.save_every == 0:
            save_checkpoint(tr, args.ckpt, args.fmt)
    if args.ckpt:
        save_checkpoint(tr, args.ckpt, args.fmt)
        log(f"saved {args.ckpt} ({args.fmt})")
    mw.close()
    gdist.shutdown()
    return 0


def _constraint_args(p) -> None:
    p.add_argument("--pattern", default=None,
                   help="one item per position: a char, \\char, . (any char of --charset), [abc], [a-z], [^...]")
    p.add_argument("--charset", default=None, help="the chars a name may use (default: all)")
    p.add_argument("--min-len", dest="min_len", type=int, default=None, help="no name shorter than this")
    p.add_argument("--max-name-len", dest="max_name_len", type=int, default=None,
                   help="no name longer than this (<= the model's max_len)")
    p.add_argument("--regex", default=None,
                   help="the whole name matches this: --pattern's items, groups ( ), |, and * + ? {m} {m,} {m,n} "
                        "(not with --pattern; docs/DESIGN.md §4g)")
    p.add_argument("--exclude-file", dest="exclude_file", default=None,
                   help="one name per line: none of them is generated (novel names: pass the training file)")


def _constraints_from(args):
    """The make_constraints keywords of --pattern / --charset / --min-len / --max-name-len / --regex /
    --exclude-file (None: none given)."""
    kw = {k: v for k, v in (("pattern", args.pattern), ("charset", args.charset), ("min_len", args.min_len),
                            ("max_len", args.max_name_len), ("regex", args.regex)) if v is not None}
    if args.exclude_file is not None:
        kw["exclude"] = _read_names(args.exclude_file)
    if "pattern" in kw and ("regex" in kw or "exclude" in kw):
        raise SystemExit("--pattern cannot be combined with --regex / --exclude-file (write the pattern as a regex)")
    return kw or None


def _bias_item(text: str):
    """--logit-bias CHARS=VALUE -> (bytes, float); CHARS literal latin-1 (the last '=' splits)."""
    chars, sep, val = text.rpartition("=")
    try:
        if not sep or not chars:
            raise ValueError
        return chars.encode("latin-1"), float(val)
    except ValueError:   # (UnicodeEncodeError is one)
        raise argparse.ArgumentTypeError(f"CHARS=VALUE expected (CHARS latin-1, VALUE a number), got {text!r}")


def _soft_args(p) -> None:
    p.add_argument("--logit-bias", dest="logit_bias", type=_bias_item, action="append", default=None,
                   metavar="CHARS=VALUE", help="add VALUE to the logit of every char in CHARS (repeatable; soft "
                                               "preferences: docs/DESIGN.md §4h)")
    p.add_argument("--eos-bias", dest="eos_bias", type=float, default=None, metavar="X",
                   help="add X to the end-of-name char's logit (negative: longer names)")
    p.add_argument("--presence-penalty", dest="presence_penalty", type=float, default=None, metavar="X",
                   help="deduct X from the logit of every char the name already holds")
    p.add_argument("--frequency-penalty", dest="frequency_penalty", type=float, default=None, metavar="X",
                   help="deduct X per earlier occurrence of a char in the name")


def _soft_from(args, eos: int) -> dict:
    """The soft-control keywords of --logit-bias / --eos-bias / --presence-penalty / --frequency-penalty
    (empty: none given).  Values for the same char add up."""
    kw = {}
    if args.logit_bias is not None or args.eos_bias is not None:
        bias = {}
        for chars, val in args.logit_bias or []:
            for c in chars:
                bias[c] = bias.get(c, 0.0) + val
        if args.eos_bias is not None:
            bias[int(eos)] = bias.get(int(eos), 0.0) + args.eos_bias
        kw["logit_bias"] = bias
    for key in ("presence_penalty", "frequency_penalty"):
        if getattr(args, key) is not None:
            kw[key] = getattr(args, key)
    return kw


def cmd_generate(args) -> int:
    from .engine import generator as G
    from .utils.data import random_floats
    from .utils import ckpt
    fmt = args.fmt
    if fmt == "auto":
        fmt = "gen" if os.path.exists(args.ckpt + ".json") else "ref"
    cfg = _cfg_from(args) if fmt == "ref" else None
    N = args.n
    ml = args.max_len if args.max_len is not None else (
        cfg.max_len if fmt == "ref" else ckpt.load(args.ckpt, None, "gen")[0].max_len)
    rf = random_floats(N, ml, seed=args.seed)
    ctl = {}
    for key in ("temperature", "top_k", "top_p"):
        if getattr(args, key) is not None:
            ctl[key] = getattr(args, key)
    if args.prefix is not None and args.prefix_file is not None:
        raise SystemExit("--prefix and --prefix-file exclude each other")
    if args.prefix is not None:
        ctl["prefix"] = args.prefix
    elif args.prefix_file is not None:
        pres = _read_names(args.prefix_file)
        if not pres:
            raise SystemExit(f"{args.prefix_file}: no prefixes")
        ctl["prefix"] = [pres[i % len(pres)] for i in range(N)]   # cycled over the names
    if _constraints_from(args) is not None:
        ctl["constraints"] = _constraints_from(args)
    if args.persist_constraints is not None:
        if args.persist_constraints < 0:
            raise SystemExit("--persist-constraints needs a count >= 0")
        ctl["persist_constraints"] = args.persist_constraints
    if args.persist_soft is not None:
        if args.persist_soft < 0:
            raise SystemExit("--persist-soft needs a count >= 0")
        ctl["persist_soft"] = args.persist_soft
    ctx = None
    if args.cpu:
        from .parallel.dist import DistCtx
        ctx = DistCtx()
    t0 = time.perf_counter()
    G.namegen_initialize(N, args.seed, args.ckpt, cfg, fmt, ctx=ctx, precision=args.precision)
    out = np.zeros(N * (ml + 1), dtype=np.uint8)
    ctl.update(_soft_from(args, G._S.cfg.eos))   # (the EOS id is the checkpoint's)
    t1 = time.perf_counter()
    if args.exclude_emitted:
        _generate_distinct(G, args, N, ml, ctl, out)
    else:
        G.namegen(N, rf, out, **ctl)
    t2 = time.perf_counter()
    rank = int(os.environ.get("RANK", "0"))
    if rank == 0:
        # raw bytes of an untrained model can be control chars: escape them for text output
        names = ["".join(c if c.isprintable() else f"\\x{ord(c):02x}" for c in nm)
                 for nm in G.decode_names(out, N, ml)]
        if args.raw_out:
            out.tofile(args.raw_out)        # the reference's N x (MAX_LEN+1) byte layout
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(names) + "\n")
        else:
            print("\n".join(names))
        print(json.dumps({"names": N, "init_s": round(t1 - t0, 4), "generate_s": round(t2 - t1, 4),
                          "names_per_s": round(N / max(t2 - t1, 1e-9), 1)}), file=sys.stderr)
    G.namegen_finalize()
    return 0


def _generate_distinct(G, args, N: int, ml: int, ctl: dict, out: np.ndarray) -> None:
    """--exclude-emitted: N distinct names.  Batches of --emit-batch names; every batch's names join the
    exclusion list (docs/DESIGN.md §4g) before the next one, and of the names that one batch holds twice
    the later ones are dropped and drawn again.  Batch r draws the uniforms of seed + r."""
    from .utils.data import random_floats
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("--exclude-emitted runs on one rank")
    cons = dict(ctl.get("constraints") or {})
    if "pattern" in cons:
        raise SystemExit("--exclude-emitted cannot be combined with --pattern (write the pattern as a regex)")
    seen = set(cons.get("exclude") or [])
    rows = out.reshape(N, ml + 1)
    done = r = 0
    while done < N:
        n = min(args.emit_batch, N - done)
        prefix = ctl.get("prefix")
        if isinstance(prefix, list):
            prefix = prefix[done:done + n]
        kw = {k: v for k, v in ctl.items() if k not in ("constraints", "prefix")}
        if prefix is not None:
            kw["prefix"] = prefix
        buf = np.zeros(n * (ml + 1), dtype=np.uint8)
        try:
            G.namegen(n, random_floats(n, ml, seed=args.seed + r), buf, constraints=dict(cons, exclude=sorted(seen)), **kw)
        except ValueError as e:
            raise SystemExit(f"--exclude-emitted: {done} of {N} names generated, then: {e}")
        r += 1
        eos = bytes([G._S.cfg.eos])
        for row in buf.reshape(n, ml + 1):
            name = bytes(row[:ml]).split(eos, 1)[0]
            if name in seen:
                continue
            seen.add(name)
            rows[done] = row
            done += 1


def _escape(name: str) -> str:
    return "".join(c if c.isprintable() else f"\\x{ord(c):02x}" for c in name)


def _read_names(path: str) -> list:
    """One name per line, bytes kept as they are (latin-1); an empty line is the empty name."""
    with open(path, "rb") as f:
        lines = f.read().split(b"\n")
    if lines and not lines[-1]:
        lines.pop()                         # the file's final newline
    return [ln[:-1] if ln.endswith(b"\r") else ln for ln in lines]


def cmd_score(args) -> int:
    """Teacher-forced log-likelihood of names under a checkpoint: one `name<TAB>logp<TAB>n_tok` line
    per name, a JSON summary on stderr.  With any of `generate`'s sampling flags logp is the
    log-probability that `generate` with the same flags emits the name: `-inf` for a name it cannot
    emit, counted as `impossible` in the summary (docs/DESIGN.md §4f)."""
    import torch
    from .engine import generator as G
    from .models import cpu_ref
    from .utils import ckpt
    fmt = args.fmt
    if fmt == "auto":
        fmt = "gen" if os.path.exists(args.ckpt + ".json") else "ref"
    cfg, params = ckpt.load(args.ckpt, _cfg_from(args) if fmt == "ref" else None, fmt)
    over = {k: getattr(args, k) for k in ("max_len", "sos", "eos") if getattr(args, k) is not None}
    cfg = cfg.replace(**over)
    ML = cfg.max_len
    if args.raw:
        raw = np.fromfile(args.raw, dtype=np.uint8)
        if raw.size % (ML + 1):
            raise SystemExit(f"{args.raw}: {raw.size} bytes is not a whole number of {ML + 1}-byte rows")
        rows = raw.reshape(-1, ML + 1)
    else:
        rows = G.encode_names(_read_names(args.names), cfg)
    # the sampler's settings (generate's flags): the rows are scored under the distribution it draws from
    ctl = {key: getattr(args, key) for key in ("temperature", "top_k", "top_p") if getattr(args, key) is not None}
    if args.prefix is not None and args.prefix_file is not None:
        raise SystemExit("--prefix and --prefix-file exclude each other")
    if args.prefix is not None:
        ctl["prefix"] = args.prefix
    elif args.prefix_file is not None:
        pres = _read_names(args.prefix_file)
        if not pres:
            raise SystemExit(f"{args.prefix_file}: no prefixes")
        ctl["prefix"] = [pres[i % len(pres)] for i in range(rows.shape[0])]   # cycled over the rows, as generate does
    if _constraints_from(args) is not None:
        ctl["constraints"] = _constraints_from(args)
    ctl.update(_soft_from(args, cfg.eos))
    t0 = time.perf_counter()
    if args.cpu or not torch.cuda.is_available():
        out = cpu_ref.score({k: v.float() for k, v in params.items()}, cfg, rows, **ctl)
        res = G.ScoreResult(out[0], out[3], out[1], out[2], out[4] if ctl else None)
    else:
        res = G.HipGenerator(cfg, params, max_batch=max(64, min(4096, rows.shape[0]))).score(rows, **ctl)
    dt = time.perf_counter() - t0
    lines = []
    for r, lp, nt in zip(rows, res.name_logp, res.n_tok):
        # the scored chars without the EOS (a row cut off at max_len has none)
        k = int(nt) - 1 if r[int(nt) - 1] == cfg.eos else int(nt)
        lines.append(f"{_escape(bytes(r[:k]).decode('latin-1'))}\t{float(lp):.6f}\t{int(nt)}")
    text = "\n".join(lines) + ("\n" if lines else "")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    print(json.dumps({"names": int(rows.shape[0]), "tokens": res.tokens, "nll_per_char": res.nll_per_char,
                      "perplexity": res.perplexity, "top1": res.top1, "impossible": res.impossible,
                      "seconds": round(dt, 4)}), file=sys.stderr)
    return 0


def cmd_beam(args) -> int:
    """The `width` most probable names per prefix: one `prefix<TAB>rank<TAB>name<TAB>logp` line per beam
    (rank from 0, dead slots left out)."""
    import torch
    from .engine import generator as G
    from .models import cpu_ref
    from .utils import ckpt
    fmt = args.fmt
    if fmt == "auto":
        fmt = "gen" if os.path.exists(args.ckpt + ".json") else "ref"
    cfg, params = ckpt.load(args.ckpt, _cfg_from(args) if fmt == "ref" else None, fmt)
    over = {k: getattr(args, k) for k in ("max_len", "sos", "eos") if getattr(args, k) is not None}
    cfg = cfg.replace(**over)
    if args.prefix_file:
        prefixes = [b.decode("latin-1") for b in _read_names(args.prefix_file)]
    else:
        prefixes = [args.prefix or ""]
    if args.cpu or not torch.cuda.is_available():
        res = cpu_ref.beam_search({k: v.float() for k, v in params.items()}, cfg, prefixes, args.width,
                                  constraints=_constraints_from(args))
    else:
        gen = G.HipGenerator(cfg, params, max_batch=max(64, min(4096, len(prefixes) * args.width)))
        res = gen.beam_search(prefixes, args.width, constraints=_constraints_from(args))
    lines = []
    for pre, names, lps in zip(prefixes, res.names(), res.logp):
        for k, nm in enumerate(names):
            lines.append(f"{_escape(pre)}\t{k}\t{_escape(nm)}\t{float(lps[k]):.6f}")
    text = "\n".join(lines) + ("\n" if lines else "")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    return 0


def cmd_distinct(args) -> int:
    """`width` distinct names per prefix, sampled without replacement in draw order with the model's
    probabilities (stochastic beam search, docs/DESIGN.md §4i): one `prefix<TAB>draw<TAB>name<TAB>logq` line
    per row (draw from 0, dead slots left out; logq: the name's log-probability under the sampler)."""
    import torch
    from .engine import generator as G
    from .models import cpu_ref
    from .utils import ckpt
    fmt = args.fmt
    if fmt == "auto":
        fmt = "gen" if os.path.exists(args.ckpt + ".json") else "ref"
    cfg, params = ckpt.load(args.ckpt, _cfg_from(args) if fmt == "ref" else None, fmt)
    over = {k: getattr(args, k) for k in ("max_len", "sos", "eos") if getattr(args, k) is not None}
    cfg = cfg.replace(**over)
    if args.prefix is not None and args.prefix_file is not None:
        raise SystemExit("--prefix and --prefix-file exclude each other")
    if args.prefix_file:
        prefixes = [b.decode("latin-1") for b in _read_names(args.prefix_file)]
    else:
        prefixes = [args.prefix or ""]
    kw = dict(seed=args.noise_seed, temperature=args.temperature, constraints=_constraints_from(args))
    if args.cpu or not torch.cuda.is_available():
        res = cpu_ref.sample_distinct({k: v.float() for k, v in params.items()}, cfg, prefixes, args.width, **kw)
    else:
        gen = G.HipGenerator(cfg, params, max_batch=max(64, min(4096, len(prefixes) * args.width)))
        res = gen.sample_distinct(prefixes, args.width, **kw)
    lines = []
    for pre, names, lqs in zip(prefixes, res.names(), res.logq):
        for k, nm in enumerate(names):
            lines.append(f"{_escape(pre)}\t{k}\t{_escape(nm)}\t{float(lqs[k]):.6f}")
    text = "\n".join(lines) + ("\n" if lines else "")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    return 0


def cmd_conditional(args) -> int:
    """Weighted names from the model's own distribution over the names that satisfy the constraints, and the
    probability of the constraints under the model (sequential Monte Carlo, docs/DESIGN.md §4j): one
    `prefix<TAB>i<TAB>name<TAB>weight` line per particle (weights normalised per prefix), or per draw with
    --draw; one JSON summary per prefix on stderr (log_z, probability, z_stderr, ess, resamples)."""
    import json
    import torch
    from .engine import generator as G
    from .models import cpu_ref
    from .utils import ckpt
    fmt = args.fmt
    if fmt == "auto":
        fmt = "gen" if os.path.exists(args.ckpt + ".json") else "ref"
    cfg, params = ckpt.load(args.ckpt, _cfg_from(args) if fmt == "ref" else None, fmt)
    over = {k: getattr(args, k) for k in ("max_len", "sos", "eos") if getattr(args, k) is not None}
    cfg = cfg.replace(**over)
    if args.prefix is not None and args.prefix_file is not None:
        raise SystemExit("--prefix and --prefix-file exclude each other")
    if args.prefix_file:
        prefixes = [b.decode("latin-1") for b in _read_names(args.prefix_file)]
    else:
        prefixes = [args.prefix or ""]
    if args.draw is not None and args.draw < 1:
        raise SystemExit("--draw needs a count >= 1")
    kw = dict(runs=args.runs, seed=args.noise_seed, temperature=args.temperature, constraints=_constraints_from(args),
              ess_threshold=args.ess_threshold, top_k=args.top_k, top_p=args.top_p, logit_bias=args.logit_bias,
              presence_penalty=args.presence_penalty, frequency_penalty=args.frequency_penalty)
    try:
        if args.cpu or not torch.cuda.is_available():
            res = cpu_ref.sample_conditional({k: v.float() for k, v in params.items()}, cfg, prefixes, args.width, **kw)
        else:
            gen = G.HipGenerator(cfg, params, max_batch=max(64, min(4096, len(prefixes) * args.runs * args.width)))
            res = gen.sample_conditional(prefixes, args.width, **kw)
    except ValueError as e:
        raise SystemExit(f"conditional: {e}")
    lines = []
    names, w = res.names(), res.weights()
    drawn = res.draw(args.draw, args.noise_seed) if args.draw is not None else None
    for n, pre in enumerate(prefixes):
        if drawn is not None:
            for k, nm in enumerate(drawn[n]):
                lines.append(f"{_escape(pre)}\t{k}\t{_escape(nm)}\t{1.0 / len(drawn[n]):.6f}")
        else:
            for k, nm in enumerate(names[n]):
                lines.append(f"{_escape(pre)}\t{k}\t{_escape(nm)}\t{float(w[n, k]):.6f}")
        se = float(res.z_stderr[n])
        sys.stderr.write(json.dumps(dict(prefix=pre, log_z=float(res.log_z[n]), probability=float(np.exp(res.log_z[n])),
                                         z_stderr=None if se != se else se, ess=float(res.ess[n]),
                                         resamples=[int(v) for v in res.n_resampled[n]])) + "\n")
    text = "\n".join(lines) + ("\n" if lines else "")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    return 0


class _Evaluator:
    """Held-out evaluation for `train --eval-data`: the file is read once; every call scores the
    trainer's current weights on all of it (each rank the whole file: no collective of its own)."""

    def __init__(self, path: str, cfg, on_gpu: bool):
        from .engine import generator as G
        self.G, self.cfg, self.gen = G, cfg, None
        self.rows = G.encode_names(_read_names(path), cfg)
        self.on_gpu = on_gpu

    def __call__(self, tr) -> dict:
        from .models import cpu_ref
        params = tr.state_dict()           # collective with shard_optim=2: every rank calls it
        if self.on_gpu:
            if self.gen is None:
                self.gen = self.G.HipGenerator(self.cfg, params, max_batch=max(64, min(4096, self.rows.shape[0])))
            else:
                self.gen.load_state(params)
            res = self.gen.score(self.rows)
        else:
            tok, name, n_tok, rank = cpu_ref.score({k: v.float() for k, v in params.items()}, self.cfg, self.rows)
            res = self.G.ScoreResult(tok, rank, name, n_tok)
        return dict(eval_nll=res.nll_per_char, eval_ppl=res.perplexity, eval_top1=res.top1,
                    eval_names=int(self.rows.shape[0]))


def cmd_info(args) -> int:
    import torch
    info = {"torch": torch.__version__, "hip": torch.version.hip, "gpu": torch.cuda.is_available()}
    if torch.cuda.is_available():
        from .ops import load_ext
        info["device"] = load_ext().device_info()
    print(json.dumps(info, indent=1))
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="gru_mpi_cuda_amd")
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("train", help="train on synthetic names (one process per GPU)")
    t.add_argument("--preset", default="h512")
    t.add_argument("--steps", type=int, default=100)
    t.add_argument("--log-every", type=int, default=10)
    t.add_argument("--ckpt", default=None)
    t.add_argument("--fmt", choices=["gen", "ref"], default="gen")
    t.add_argument("--save-every", type=int, default=0)
    t.add_argument("--resume", default=None)
    t.add_argument("--metrics", default=None, help="JSONL metrics file (rank 0)")
    t.add_argument("--cpu", action="store_true", help="force the CPU reference path")
    t.add_argument("--data", default=None,
                   help="names file, one per line (default: synthetic names); read by the native loader")
    t.add_argument("--eval-data", dest="eval_data", default=None,
                   help="held-out names file, one per line: scored every --eval-every steps and at the end "
                        "(eval_nll / eval_ppl / eval_top1 in the log line and the metrics record)")
    t.add_argument("--eval-every", dest="eval_every", type=int, default=0)
    _add_model_args(t)
    t.add_argument("--dropout", type=float, default=None, metavar="P",
                   help="training dropout on the non-recurrent connections, 0 <= P < 1 (default 0: off)")
    sc = sub.add_parser("score", help="teacher-forced log-likelihood of names under a checkpoint")
    sc.add_argument("--ckpt", required=True)
    sc.add_argument("--fmt", choices=["auto", "gen", "ref"], default="auto")
    src = sc.add_mutually_exclusive_group(required=True)
    src.add_argument("--names", default=None, help="names file, one per line")
    src.add_argument("--raw", default=None, help="raw N x (MAX_LEN+1) bytes, as `generate --raw-out` writes")
    sc.add_argument("--out", default=None, help="name, log-prob and token count per line, tab-separated")
    sc.add_argument("--cpu", action="store_true", help="cpu_ref.score in fp32 instead of the HIP generator")
    sc.add_argument("--temperature", type=float, default=None,
                    help="score under the sampler: `generate`'s temperature T >= 0 (0: greedy).  With any of these "
                         "flags logp is the log-probability that `generate` with the same flags emits the name "
                         "(-inf: it cannot)")
    sc.add_argument("--top-k", dest="top_k", type=int, default=None, help="`generate`'s --top-k (0: off)")
    sc.add_argument("--top-p", dest="top_p", type=float, default=None, help="`generate`'s --top-p, in (0, 1] (1: off)")
    sc.add_argument("--prefix", default=None, help="`generate`'s --prefix: every name is forced to start with these chars")
    sc.add_argument("--prefix-file", dest="prefix_file", default=None, help="one prefix per line, cycled over the names")
    _constraint_args(sc)
    _soft_args(sc)
    sc.add_argument("--preset", default="ref", help="dims for --fmt ref (headerless blob)")
    _add_model_args(sc)
    g = sub.add_parser("generate", help="namegen_initialize / namegen / namegen_finalize")
    g.add_argument("--ckpt", required=True)
    g.add_argument("--fmt", choices=["auto", "gen", "ref"], default="auto")
    g.add_argument("-n", type=int, default=10)
    g.add_argument("--out", default=None, help="names, one per line (non-printables escaped)")
    g.add_argument("--raw-out", default=None, help="raw N x (MAX_LEN+1) output bytes")
    g.add_argument("--precision", choices=["fp32", "bf16", "bf16x3"], default="fp32",
                   help="fp32 (default): the reference's fp32 arithmetic (fp32 MFMA products); "
                        "bf16x3: fp32 arithmetic on split-bf16 MFMA products (~2^-16 relative error per "
                        "product, ~2x faster; parity with fp32 unpinned on near-tie samples); "
                        "bf16: MFMA fast mode")
    g.add_argument("--temperature", type=float, default=None,
                   help="sampling temperature T >= 0 (0: greedy); any sampling control takes the controlled "
                        "per-char path (fp32 / bf16x3)")
    g.add_argument("--top-k", dest="top_k", type=int, default=None, help="keep the k most likely chars (0: off)")
    g.add_argument("--top-p", dest="top_p", type=float, default=None,
                   help="keep the smallest top set whose mass reaches p, in (0, 1] (1: off)")
    g.add_argument("--prefix", default=None, help="every name starts with these chars")
    g.add_argument("--prefix-file", dest="prefix_file", default=None,
                   help="one prefix per line, cycled over the names")
    _constraint_args(g)
    _soft_args(g)
    g.add_argument("--persist-constraints", dest="persist_constraints", type=int, nargs="?", const=64, default=None,
                   metavar="N", help="constrained batches of up to N names (bare flag: 64) run as one constrained "
                                     "persistent launch instead of the per-char graph (opt-in; docs/DESIGN.md §4e)")
    g.add_argument("--persist-soft", dest="persist_soft", type=int, nargs="?", const=64, default=None,
                   metavar="N", help="soft batches (--logit-bias / --presence-penalty / --frequency-penalty) of up "
                                     "to N names (bare flag: 64) run as one soft persistent launch instead of the "
                                     "per-char graph (opt-in; docs/DESIGN.md §4h)")
    g.add_argument("--exclude-emitted", dest="exclude_emitted", action="store_true",
                   help="distinct names: every batch's names are excluded from the later batches")
    g.add_argument("--emit-batch", dest="emit_batch", type=int, default=256,
                   help="names per batch of --exclude-emitted")
    g.add_argument("--cpu", action="store_true", help="force the CPU reference path (single process)")
    g.add_argument("--preset", default="ref", help="dims for --fmt ref (headerless blob)")
    _add_model_args(g)
    g.set_defaults(seed=0)
    bm = sub.add_parser("beam", help="beam search: the most probable names per prefix")
    bm.add_argument("--ckpt", required=True)
    bm.add_argument("--fmt", choices=["auto", "gen", "ref"], default="auto")
    bm.add_argument("--width", type=int, default=4, help="beams per prefix, 1 .. min(32, vocab)")
    bm.add_argument("--prefix", default=None, help="the names start with these chars (default: the empty prefix)")
    bm.add_argument("--prefix-file", dest="prefix_file", default=None, help="one prefix per line")
    _constraint_args(bm)
    bm.add_argument("--out", default=None, help="prefix, rank, name and log-prob per line, tab-separated")
    bm.add_argument("--cpu", action="store_true", help="cpu_ref.beam_search in fp32 instead of the HIP generator")
    bm.add_argument("--preset", default="ref", help="dims for --fmt ref (headerless blob)")
    _add_model_args(bm)
    ds = sub.add_parser("distinct", help="distinct names per prefix: sampling without replacement (stochastic beam search)")
    ds.add_argument("--ckpt", required=True)
    ds.add_argument("--fmt", choices=["auto", "gen", "ref"], default="auto")
    ds.add_argument("--width", type=int, default=4, help="distinct names per prefix, 1 .. min(32, vocab)")
    ds.add_argument("--prefix", default=None, help="the names start with these chars (default: the empty prefix)")
    ds.add_argument("--prefix-file", dest="prefix_file", default=None, help="one prefix per line")
    ds.add_argument("--temperature", type=float, default=None, help="softmax temperature, > 0 (default 1)")
    _constraint_args(ds)
    ds.add_argument("--out", default=None, help="prefix, draw, name and log-prob per line, tab-separated")
    ds.add_argument("--cpu", action="store_true", help="cpu_ref.sample_distinct in fp32 instead of the HIP generator")
    ds.add_argument("--seed", dest="noise_seed", type=int, default=0,
                    help="the sampler's seed: the same seed gives the same names (default 0)")
    ds.add_argument("--preset", default="ref", help="dims for --fmt ref (headerless blob)")
    _add_model_args(ds, skip=("seed",))      # --seed is the sampler's here, not the config's
    cd = sub.add_parser("conditional", help="weighted names from the model's distribution given the constraints, and "
                                            "the constraints' probability (sequential Monte Carlo)")
    cd.add_argument("--ckpt", required=True)
    cd.add_argument("--fmt", choices=["auto", "gen", "ref"], default="auto")
    cd.add_argument("--width", type=int, default=16, help="particles per system, 1 .. min(32, vocab)")
    cd.add_argument("--runs", type=int, default=1, help="independent systems per prefix, pooled (default 1)")
    cd.add_argument("--prefix", default=None, help="the names start with these chars (default: the empty prefix)")
    cd.add_argument("--prefix-file", dest="prefix_file", default=None, help="one prefix per line")
    cd.add_argument("--temperature", type=float, default=None, help="softmax temperature, > 0 (default 1)")
    cd.add_argument("--ess-threshold", dest="ess_threshold", type=float, default=0.5,
                    help="resample when the effective sample size falls below this fraction of the width (0: never)")
    _constraint_args(cd)
    cd.add_argument("--draw", type=int, default=None, help="print K names per prefix drawn from the weighted pool instead")
    cd.add_argument("--out", default=None, help="prefix, index, name and weight per line, tab-separated")
    cd.add_argument("--cpu", action="store_true", help="cpu_ref.sample_conditional in fp32 instead of the HIP generator")
    cd.add_argument("--seed", dest="noise_seed", type=int, default=0,
                    help="the sampler's seed: the same seed gives the same particles (default 0)")
    # not carried by the rule: given, they are an error before anything runs
    cd.add_argument("--top-k", dest="top_k", type=int, default=None, help=argparse.SUPPRESS)
    cd.add_argument("--top-p", dest="top_p", type=float, default=None, help=argparse.SUPPRESS)
    cd.add_argument("--logit-bias", dest="logit_bias", default=None, help=argparse.SUPPRESS)
    cd.add_argument("--presence-penalty", dest="presence_penalty", type=float, default=None, help=argparse.SUPPRESS)
    cd.add_argument("--frequency-penalty", dest="frequency_penalty", type=float, default=None, help=argparse.SUPPRESS)
    cd.add_argument("--preset", default="ref", help="dims for --fmt ref (headerless blob)")
    _add_model_args(cd, skip=("seed",))      # --seed is the sampler's here, not the config's
    sub.add_parser("info", help="device / build info")
    b = sub.add_parser("bench", help="run bench.py", add_help=False)
    args, rest = ap.parse_known_args(argv)
    if args.cmd == "bench":
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        import bench
        sys.argv = ["bench.py"] + rest
        return bench.main()
    if rest:
        ap.error(f"unrecognized arguments: {rest}")
    return {"train": cmd_train, "generate": cmd_generate, "score": cmd_score, "beam": cmd_beam, "distinct": cmd_distinct,
            "conditional": cmd_conditional, "info": cmd_info}[args.cmd](args)


if __name__ == "__main__":
    sys.exit(main())

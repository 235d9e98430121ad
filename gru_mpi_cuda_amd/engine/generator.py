"""Generation engines + the reference's 3-call API.

``HipGenerator`` drives the native device-resident generator (csrc/engine/generator.cpp).
``namegen_initialize / namegen / namegen_finalize`` keep the reference's signatures and
semantics (/root/reference/namegensf.cu:359, 627, 897):

* every rank generates a contiguous slice of the N names (remainder spread over the first
  ranks instead of dropped), each name n consuming the *global*
  ``random_floats[n*MAX_LEN + l]`` at step l, so the output is independent of world size
  (the §3.2 invariant);
* rank 0 ends with ``output[N*(MAX_LEN+1)]``: each name's chars, the EOS char written before
  stopping, NUL padding;
* only rank 0 reads the parameter file; weights are broadcast.

Collectives: RCCL all-gather of the fixed-size per-rank output slabs on device (replaces
MPI_Scatter of the randoms + MPI_Gather of the names, namegensf.cu:636,889); the randoms
are not scattered at all -- every rank reads only its own slice of the caller's array.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch

from ..config import GRUConfig
from ..models import cpu_ref
from ..models.params import flat_layout, pad_config, pad_params, to_flat
from ..parallel.dist import DistCtx, shard


PRECISIONS = ("fp32", "bf16", "bf16x3")
_MODE = {"bf16": 0, "fp32": 1, "bf16x3": 2}   # GenDims::fp32


class HipGenerator:
    """precision "fp32" (default): the reference's arithmetic (namegensf.cu:233-242, 294-333) --
    fp32 MFMA GEMMs on the fp32 master weights, IEEE gates and softmax;
    "bf16x3": the same with its products as bf16 MFMA GEMMs over split operands (x = hi + lo,
    hi*hi + hi*lo + lo*hi in fp32: ~2^-16 relative error per product, 1.9x the fp32 speed at 4096
    names).  Opt-in: 2400 names (profiles/r3_gen_default_decision.jsonl) matched the fp64 oracle
    as often as fp32, but that sample cannot separate a 2^-16 product error from fp32 on near-tie
    samples (parity unpinned);
    "bf16": bf16 MFMA fast mode (fused step kernels, bf16 weight copies).
    Small batches run the exact fp32 persistent kernel in both fp32 modes.
    ``persist_constraints`` = N (opt-in, default 0; docs/DESIGN.md §4e): constrained batches of up to N
    names (at most 64) run as one constrained persistent launch instead of the per-char graph.
    ``persist_soft`` = N (opt-in, default 0; docs/DESIGN.md §4h): soft batches (``logit_bias`` /
    ``presence_penalty`` / ``frequency_penalty``) of up to N names (at most 64) run as one soft persistent
    launch instead of the per-char graph, where the shape has a variant (vocab 256, max_len <= 64); a soft
    batch with constraints needs ``persist_constraints`` to cover it as well."""

    def __init__(self, cfg: GRUConfig, params: Dict[str, torch.Tensor], max_batch: int = 4096,
                 device: Optional[torch.device] = None, flat: Optional[torch.Tensor] = None,
                 precision: str = "fp32", persist_constraints: int = 0, persist_soft: int = 0):
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {PRECISIONS}")
        self.precision = precision
        from ..ops import load_ext
        self.C = load_ext()
        self.cfg = cfg
        self.dev = device or torch.device("cuda", torch.cuda.current_device())
        # E, H off the 64-grid: the exactly equivalent zero-padded model (models/params.py).  The
        # vocabulary is not padded: the sampler's fallback index is V - 1 (namegensf.cu:333)
        if cfg.vocab % 64:
            raise ValueError(f"HIP generator needs vocab % 64 == 0 (got {cfg.vocab})")
        icfg = pad_config(cfg).replace(vocab=cfg.vocab)
        if icfg != cfg:
            if flat is not None:
                raise ValueError("a shared flat buffer needs embed and hidden to be multiples of 64")
            params = pad_params(params, cfg, icfg)
        self.layout = flat_layout(icfg)
        self.flat = flat if flat is not None else to_flat(icfg, params).to(self.dev)
        offsets = {s.name: s.offset for s in self.layout.segments}
        dims = dict(V=cfg.vocab, E=icfg.embed, H=icfg.hidden, L=cfg.layers, max_len=cfg.max_len,
                    sos=cfg.sos, eos=cfg.eos, max_batch=max_batch, fp32=_MODE[precision])
        self.g = self.C.Generator(dims, self.flat.data_ptr(), offsets)
        self.g.refresh_weights(self._s())
        self.set_persist_constraints(persist_constraints)
        self.set_persist_soft(persist_soft)

    def set_persist_constraints(self, n: int) -> None:
        """Constrained batches of up to ``n`` names take the constrained persistent launch where the
        shape has one (``g.uses_persist_con``); 0 turns it off (the default)."""
        n = int(n)
        if n < 0:
            raise ValueError(f"persist_constraints must be >= 0, got {n}")
        self.g.set_persist_con_max(n)

    def set_persist_soft(self, n: int) -> None:
        """Soft batches of up to ``n`` names take the soft persistent launch where the shape has one
        (``g.uses_persist_soft``); 0 turns it off (the default)."""
        n = int(n)
        if n < 0:
            raise ValueError(f"persist_soft must be >= 0, got {n}")
        self.g.set_persist_soft_max(n)

    def _s(self) -> int:
        return torch.cuda.current_stream(self.dev).cuda_stream

    def _constraint_tensors(self, cons):
        """A Constraints object's arrays on the device: (tab, idx, lines); an Automaton's (docs/DESIGN.md
        §4g): (tab, None, states, nxt, start).  The tuple holds the tensors alive; ``_constraint_args``
        turns it into the native call's trailing arguments."""
        if isinstance(cons, cpu_ref.Automaton):
            if self.cfg.vocab not in (256, 512):
                raise ValueError(f"regex / exclude constraints need vocab 256 or 512 on the device, got {self.cfg.vocab}")
            tab = torch.from_numpy(cons.tab.view(np.int32)).to(self.dev)
            nxt = torch.from_numpy(np.ascontiguousarray(cons.nxt, dtype=np.uint16).view(np.int16)).to(self.dev)
            start = torch.from_numpy(np.ascontiguousarray(cons.start, dtype=np.int32)).to(self.dev)
            return tab, None, cons.states, nxt, start
        if self.cfg.vocab // 64 not in (1, 2, 4, 8):
            raise ValueError(f"constraints need vocab in (64, 128, 256, 512), got {self.cfg.vocab}")
        tab = torch.from_numpy(cons.tab.view(np.int32)).to(self.dev)
        idx = torch.from_numpy(np.ascontiguousarray(cons.idx, dtype=np.int32)).to(self.dev)
        return tab, idx, cons.rows

    @staticmethod
    def _constraint_args(t) -> tuple:
        return tuple(0 if v is None else (v if isinstance(v, int) else v.data_ptr()) for v in t)

    def _soft_tensors(self, soft):
        """A Soft object's arrays on the device (docs/DESIGN.md §4h): the tuple holds the tensors alive;
        ``_soft_kwargs`` turns it into the native call's keywords."""
        return (torch.from_numpy(np.ascontiguousarray(soft.tab, dtype=np.float32)).to(self.dev),
                torch.from_numpy(np.ascontiguousarray(soft.idx, dtype=np.int32)).to(self.dev), soft.rows,
                torch.from_numpy(np.ascontiguousarray(soft.presence, dtype=np.float32)).to(self.dev),
                torch.from_numpy(np.ascontiguousarray(soft.frequency, dtype=np.float32)).to(self.dev))

    @staticmethod
    def _soft_kwargs(t) -> dict:
        return dict(soft_tab=t[0].data_ptr(), soft_idx=t[1].data_ptr(), soft_rows=t[2], soft_pres=t[3].data_ptr(),
                    soft_freq=t[4].data_ptr())

    def generate_device(self, rf_dev: torch.Tensor, n: int, *, temperature=None, top_k=None, top_p=None,
                        prefix=None, constraints=None, logit_bias=None, presence_penalty=None,
                        frequency_penalty=None) -> torch.Tensor:
        """``temperature`` / ``top_k`` / ``top_p`` / ``prefix`` (scalars or one value per name; semantics:
        cpu_ref.make_controls, docs/DESIGN.md §4b): any that is not None -- a neutral value too -- takes
        the controlled path (fp32 / bf16x3 only): per batch one controlled persistent launch where
        ``g.uses_persist_ctl(batch)`` says so (small batches), else the controlled per-char graph.
        ``constraints`` (a cpu_ref.Constraints for the ``n`` names, or a dict of cpu_ref.make_constraints
        keywords; docs/DESIGN.md §4e): every name samples inside its per-position allowed sets, on the
        controlled per-char graph, or -- batches of up to ``persist_constraints`` names -- in one
        constrained persistent launch.  With ``regex`` / ``exclude`` among the keywords, or a
        cpu_ref.Automaton (docs/DESIGN.md §4g), the sets follow what the name has emitted so far: the same
        graph with a per-row state that the sampler advances.
        ``logit_bias`` / ``presence_penalty`` / ``frequency_penalty`` (cpu_ref.make_soft's arguments;
        docs/DESIGN.md §4h): soft preferences -- a per-char additive bias (a dict {chars: value}, V values, or
        one of those per name), a deduction for every char the name already holds and one per earlier
        occurrence.  Any that is not None takes the controlled per-char graph, whatever the batch size -- or,
        batches of up to ``persist_soft`` names, one soft persistent launch -- and combines with every control
        and constraint above.  Bad values raise ValueError before anything
        is launched."""
        ML = self.cfg.max_len
        ctl = None
        cons = cpu_ref.as_constraints(self.cfg, max(n, 0), constraints)
        soft = cpu_ref.as_soft(self.cfg, max(n, 0), None, logit_bias, presence_penalty, frequency_penalty)
        if cons is not None or soft is not None or any(v is not None for v in (temperature, top_k, top_p, prefix)):
            if self.precision == "bf16":
                raise ValueError('sampling controls and constraints need precision "fp32" or "bf16x3" (the bf16 '
                                 "mode samples inside its fused FC kernel)")
            ctl = cpu_ref.make_controls(self.cfg, max(n, 0), temperature, top_k, top_p, prefix)
            cpu_ref.check_prefix_allowed(cons, ctl.prefix, ctl.plen)
        out = torch.empty(max(n, 1), ML + 1, dtype=torch.uint8, device=self.dev)   # every row written
        if n > 0 and ctl is None:
            self.g.generate(rf_dev.data_ptr(), n, out.data_ptr(), self._s())
        elif n > 0:
            dev = [torch.from_numpy(a).to(self.dev) for a in (ctl.inv_temp, ctl.top_k, ctl.top_p, ctl.plen, ctl.prefix)]
            extra = ()
            if cons is not None:
                held = self._constraint_tensors(cons)
                extra = self._constraint_args(held)
            skw = {}
            if soft is not None:
                sheld = self._soft_tensors(soft)
                skw = self._soft_kwargs(sheld)
            self.g.generate_ctl(rf_dev.data_ptr(), n, *[t.data_ptr() for t in dev], out.data_ptr(), self._s(), *extra,
                                **skw)
            err = self.g.read_error()   # synchronises: the control tensors stay alive until the call is done
            if err:
                raise RuntimeError(f"HipGenerator.generate: device error word {err}")
        return out[:n]

    def generate(self, rfloats: np.ndarray, start: int = 0, count: Optional[int] = None, *, temperature=None,
                 top_k=None, top_p=None, prefix=None, constraints=None, logit_bias=None, presence_penalty=None,
                 frequency_penalty=None) -> np.ndarray:
        """Names ``start .. start+count-1`` of the job.  The controls, constraints and soft controls are
        generate_device's; per-name values are indexed by the generated names (``count`` entries)."""
        ML = self.cfg.max_len
        N = (rfloats.size // ML - start) if count is None else count
        rf = torch.from_numpy(np.ascontiguousarray(rfloats[start * ML:(start + N) * ML], dtype=np.float32))
        rf = rf.to(self.dev)
        return self.generate_device(rf, N, temperature=temperature, top_k=top_k, top_p=top_p,
                                    prefix=prefix, constraints=constraints, logit_bias=logit_bias,
                                    presence_penalty=presence_penalty,
                                    frequency_penalty=frequency_penalty).cpu().numpy()

    def load_state(self, params: Dict[str, torch.Tensor]) -> None:
        """New weights (cfg-shaped tensors) into the flat buffer; every derived copy and table follows."""
        icfg = pad_config(self.cfg).replace(vocab=self.cfg.vocab)
        if icfg != self.cfg:
            params = pad_params(params, self.cfg, icfg)
        self.flat.copy_(to_flat(icfg, params).to(self.dev))
        self.g.refresh_weights(self._s())

    def score(self, rows: np.ndarray, *, temperature=None, top_k=None, top_p=None, prefix=None,
              constraints=None, logit_bias=None, presence_penalty=None, frequency_penalty=None) -> "ScoreResult":
        """Teacher-forced log-likelihood of output rows ([N, MAX_LEN+1] or flat uint8, the format
        ``generate`` writes; semantics: cpu_ref.score_inputs).  Always exact fp32 arithmetic, whatever
        ``precision`` this generator samples with.  A byte >= vocab at a scored position raises
        ValueError before anything is launched.
        ``temperature`` / ``top_k`` / ``top_p`` / ``prefix`` / ``constraints`` (``generate``'s keywords, scalars
        or one value per row; the rule: cpu_ref.score, docs/DESIGN.md §4f): any that is not None -- a neutral
        value too -- scores the rows under the distribution ``generate`` samples from with these settings:
        exp(name_logp) is the probability that it emits exactly that row, -inf marks a row it cannot emit,
        and the result carries n_kept.  ``logit_bias`` / ``presence_penalty`` / ``frequency_penalty``
        (``generate``'s soft controls, docs/DESIGN.md §4h) do the same; their counts are those of the scored
        row's bytes before the position.  Every precision mode takes them all.  Bad values raise ValueError
        before anything is launched."""
        ML = self.cfg.max_len
        ctl = cons = soft = None
        soft_given = any(v is not None for v in (logit_bias, presence_penalty, frequency_penalty))
        if constraints is not None or soft_given or any(v is not None for v in (temperature, top_k, top_p, prefix)):
            count = np.ascontiguousarray(rows, dtype=np.uint8).size // (ML + 1)
            soft = cpu_ref.as_soft(self.cfg, count, None, logit_bias, presence_penalty, frequency_penalty)
            cons = cpu_ref.as_constraints(self.cfg, count, constraints)
            ctl = cpu_ref.make_controls(self.cfg, count, temperature, top_k, top_p, prefix)
            cpu_ref.check_prefix_allowed(cons, ctl.prefix, ctl.plen)
            if isinstance(cons, cpu_ref.Automaton):   # the rows are known: the host walks them into per-step lines
                cons = cons.for_rows(self.cfg, rows)
            if cons is not None and self.cfg.vocab // 64 not in (1, 2, 4, 8):
                raise ValueError(f"constraints need vocab in (64, 128, 256, 512), got {self.cfg.vocab}")
        rows, n_tok, _, _ = cpu_ref.score_inputs(self.cfg, rows)
        N = rows.shape[0]
        if N == 0:
            return ScoreResult(np.zeros((0, ML), np.float32), np.zeros((0, ML), np.int32),
                               np.zeros(0, np.float32), np.zeros(0, np.int32),
                               None if ctl is None else np.zeros((0, ML), np.int32))
        r = torch.from_numpy(rows).to(self.dev)
        tok = torch.empty(N, ML, dtype=torch.float32, device=self.dev)
        rank = torch.empty(N, ML, dtype=torch.int32, device=self.dev)
        name = torch.empty(N, dtype=torch.float32, device=self.dev)
        nt = torch.empty(N, dtype=torch.int32, device=self.dev)
        nk = None
        if ctl is None:
            self.g.score(r.data_ptr(), N, tok.data_ptr(), rank.data_ptr(), name.data_ptr(), nt.data_ptr(), self._s())
        else:
            dev = [torch.from_numpy(a).to(self.dev) for a in (ctl.inv_temp, ctl.top_k, ctl.top_p, ctl.plen, ctl.prefix)]
            nk = torch.empty(N, ML, dtype=torch.int32, device=self.dev)
            extra = ()
            if cons is not None:
                held = self._constraint_tensors(cons)
                extra = self._constraint_args(held)
            skw = {}
            if soft is not None:
                sheld = self._soft_tensors(soft)
                skw = self._soft_kwargs(sheld)
            self.g.score(r.data_ptr(), N, tok.data_ptr(), rank.data_ptr(), name.data_ptr(), nt.data_ptr(), self._s(),
                         *[t.data_ptr() for t in dev], nk.data_ptr(), *extra, **skw)
        err = self.g.read_error()   # synchronises: the control tensors stay alive until the call is done
        if err:
            raise RuntimeError(f"HipGenerator.score: device error word {err}")
        res = ScoreResult(tok.cpu().numpy(), rank.cpu().numpy(), name.cpu().numpy(), nt.cpu().numpy(),
                          None if nk is None else nk.cpu().numpy())
        if not np.array_equal(res.n_tok, n_tok):
            raise RuntimeError("HipGenerator.score: device token counts differ from the host's")
        return res

    def beam_search(self, prefix=None, width: int = 4, count: Optional[int] = None, constraints=None) -> "BeamResult":
        """The ``width`` most probable output rows per prefix, in order (the rule: cpu_ref.beam_search,
        docs/DESIGN.md §4d).  ``prefix``: a string, a list of strings, or None for ``count`` (default 1)
        empty prefixes.  Always exact fp32 arithmetic, whatever ``precision`` this generator samples
        with.  ``constraints`` (a cpu_ref.Constraints for the prefixes, or a dict of
        cpu_ref.make_constraints keywords; docs/DESIGN.md §4e; ``regex`` / ``exclude`` or a cpu_ref.Automaton:
        §4g, a state per beam): the ``width`` most probable rows that satisfy them.  A width outside [1, min(32, vocab)], a bad prefix or constraint and max_len > 64
        raise ValueError before anything is launched."""
        pre, plen = cpu_ref.beam_inputs(self.cfg, prefix, width, count)
        N, W, ML = pre.shape[0], int(width), self.cfg.max_len
        cons = cpu_ref.as_constraints(self.cfg, N, constraints)
        cpu_ref.check_prefix_allowed(cons, pre, plen)
        if N == 0:
            return BeamResult(np.zeros((0, W, ML + 1), np.uint8), np.zeros((0, W), np.float32),
                              np.zeros((0, W), np.int32), np.zeros(0, np.int32), self.cfg.eos)
        p, l = torch.from_numpy(pre).to(self.dev), torch.from_numpy(plen).to(self.dev)
        rows = torch.empty(N, W, ML + 1, dtype=torch.uint8, device=self.dev)
        logp = torch.empty(N, W, dtype=torch.float32, device=self.dev)
        nt = torch.empty(N, W, dtype=torch.int32, device=self.dev)
        nb = torch.empty(N, dtype=torch.int32, device=self.dev)
        extra = ()
        if cons is not None:
            held = self._constraint_tensors(cons)
            extra = self._constraint_args(held)
        self.g.beam(l.data_ptr(), p.data_ptr(), N, W, rows.data_ptr(), logp.data_ptr(), nt.data_ptr(), nb.data_ptr(),
                    self._s(), *extra)
        err = self.g.read_error()   # synchronises: the prefix tensors stay alive until the call is done
        if err:
            raise RuntimeError(f"HipGenerator.beam_search: device error word {err}")
        return BeamResult(rows.cpu().numpy(), logp.cpu().numpy(), nt.cpu().numpy(), nb.cpu().numpy(), self.cfg.eos)


    def sample_distinct(self, prefix=None, width: int = 4, count: Optional[int] = None, *, seed: int = 0, start: int = 0,
                        temperature=None, constraints=None, **excluded) -> "DistinctResult":
        """``width`` distinct output rows per prefix, an exact sample without replacement in draw order from
        the distribution ``generate`` samples from with the same ``temperature`` / ``prefix`` / ``constraints``
        -- stochastic beam search (the rule: cpu_ref.sample_distinct, docs/DESIGN.md §4i).  ``logq`` is what
        ``score(rows, temperature=, prefix=, constraints=).name_logp`` returns for the rows; ``gumbel`` the
        final perturbed values.  Name n of the call draws its noise at the global index ``start + n`` under
        ``seed``, so the result does not depend on how a job is cut into calls or batches.  Always exact fp32
        arithmetic; precision "bf16" is refused (ValueError), as are top_k, top_p, temperature 0 and the soft
        controls, before anything is launched."""
        if self.precision == "bf16":
            raise ValueError('sample_distinct needs precision "fp32" or "bf16x3" (it runs exact fp32; the bf16 mode '
                             "samples from another distribution)")
        pre, plen, inv, seed, start = cpu_ref.distinct_inputs(self.cfg, prefix, width, count, seed, start, temperature,
                                                              **excluded)
        N, W, ML = pre.shape[0], int(width), self.cfg.max_len
        cons = cpu_ref.as_constraints(self.cfg, N, constraints)
        cpu_ref.check_prefix_allowed(cons, pre, plen)
        if N == 0:
            return DistinctResult(np.zeros((0, W, ML + 1), np.uint8), np.zeros((0, W), np.float32),
                                  np.zeros((0, W), np.float32), np.zeros((0, W), np.int32), np.zeros(0, np.int32),
                                  self.cfg.eos)
        p, l = torch.from_numpy(pre).to(self.dev), torch.from_numpy(plen).to(self.dev)
        it = torch.from_numpy(inv).to(self.dev)
        rows = torch.empty(N, W, ML + 1, dtype=torch.uint8, device=self.dev)
        logq = torch.empty(N, W, dtype=torch.float32, device=self.dev)
        gum = torch.empty(N, W, dtype=torch.float32, device=self.dev)
        nt = torch.empty(N, W, dtype=torch.int32, device=self.dev)
        nf = torch.empty(N, dtype=torch.int32, device=self.dev)
        extra = ()
        if cons is not None:
            held = self._constraint_tensors(cons)
            extra = self._constraint_args(held)
        self.g.distinct(l.data_ptr(), p.data_ptr(), N, W, seed, start, it.data_ptr(), rows.data_ptr(), logq.data_ptr(),
                        gum.data_ptr(), nt.data_ptr(), nf.data_ptr(), self._s(), *extra)
        err = self.g.read_error()   # synchronises: the input tensors stay alive until the call is done
        if err:
            raise RuntimeError(f"HipGenerator.sample_distinct: device error word {err}")
        return DistinctResult(rows.cpu().numpy(), logq.cpu().numpy(), gum.cpu().numpy(), nt.cpu().numpy(),
                              nf.cpu().numpy(), self.cfg.eos)

    def sample_conditional(self, prefix=None, width: int = 16, count: Optional[int] = None, *, runs: int = 1, seed: int = 0,
                           start: int = 0, temperature=None, constraints=None, ess_threshold: float = 0.5,
                           **excluded) -> "ConditionalResult":
        """Weighted names from the MODEL's distribution conditioned on ``constraints`` (and ``prefix``), and the
        probability of the rule under the model -- sequential Monte Carlo over the constrained sampler (the
        rule: cpu_ref.sample_conditional, docs/DESIGN.md §4j).  ``generate(constraints=...)`` renormalises the
        allowed chars at every step, so each of its names satisfies the rule but a name is favoured by the
        mass that was forbidden along its way; here every particle carries that mass as its importance weight
        and the particles are resampled when ESS < ``ess_threshold`` x width (0: plain importance sampling).

        ``runs`` independent systems of ``width`` <= 32 particles per prefix are pooled (run r of prefix n draws
        its noise at the global index ``start + n * runs + r`` under ``seed``: the result does not depend on
        how a job is cut into calls or batches).  ``exp(result.log_z)`` is an unbiased estimate of P(rule |
        prefix) at any width; ``weights`` / ``expectation`` / ``draw`` are self-normalised: consistent, with a
        bias of order 1 / particles.  Always exact fp32 arithmetic; precision "bf16" is refused (ValueError),
        as are top_k, top_p, temperature 0 and the soft controls, before anything is launched."""
        if self.precision == "bf16":
            raise ValueError('sample_conditional needs precision "fp32" or "bf16x3" (it runs exact fp32; the bf16 mode '
                             "samples from another distribution)")
        pre, plen, inv, seed, start, thr, N, R = cpu_ref.conditional_inputs(self.cfg, prefix, width, count, runs, seed, start,
                                                                            temperature, ess_threshold, **excluded)
        M, W, ML = N * R, int(width), self.cfg.max_len
        cons = cpu_ref.conditional_constraints(self.cfg, N, R, constraints)
        cpu_ref.check_prefix_allowed(cons, pre, plen)
        if M == 0:
            return cpu_ref.pool_conditional(np.zeros((0, W, ML + 1), np.uint8), np.zeros((0, W), np.float32),
                                            np.zeros((0, W), np.float32), np.zeros((0, W), np.int32), np.zeros(0, np.int32),
                                            N, R, W, self.cfg.eos)
        p, l = torch.from_numpy(pre).to(self.dev), torch.from_numpy(plen).to(self.dev)
        it = torch.from_numpy(inv).to(self.dev)
        rows = torch.empty(M, W, ML + 1, dtype=torch.uint8, device=self.dev)
        logw = torch.empty(M, W, dtype=torch.float32, device=self.dev)
        logq = torch.empty(M, W, dtype=torch.float32, device=self.dev)
        nt = torch.empty(M, W, dtype=torch.int32, device=self.dev)
        nr = torch.empty(M, dtype=torch.int32, device=self.dev)
        extra = ()
        if cons is not None:
            held = self._constraint_tensors(cons)
            extra = self._constraint_args(held)
        self.g.conditional(l.data_ptr(), p.data_ptr(), M, W, seed, start, thr, it.data_ptr(), rows.data_ptr(),
                           logw.data_ptr(), logq.data_ptr(), nt.data_ptr(), nr.data_ptr(), self._s(), *extra)
        err = self.g.read_error()   # synchronises: the input tensors stay alive until the call is done
        if err:
            raise RuntimeError(f"HipGenerator.sample_conditional: device error word {err}")
        return cpu_ref.pool_conditional(rows.cpu().numpy(), logw.cpu().numpy(), logq.cpu().numpy(), nt.cpu().numpy(),
                                        nr.cpu().numpy(), N, R, W, self.cfg.eos)


BeamResult = cpu_ref.BeamResult
DistinctResult = cpu_ref.DistinctResult
ConditionalResult = cpu_ref.ConditionalResult


@dataclass
class ScoreResult:
    """``HipGenerator.score`` / ``cpu_ref.score`` output.  tok_logp [N, ML] (masked positions 0),
    rank [N, ML] int32 (masked -1), name_logp [N], n_tok [N] int32; the summaries are computed in
    float64 from tok_logp.  A score with sampling controls or constraints (docs/DESIGN.md §4f) also has
    n_kept [N, ML] int32, the size of each step's kept set (masked -1; None for a plain score), and may
    hold -inf: ``impossible`` counts the names the sampler cannot emit, and with one of them
    nll_per_char and perplexity are inf (top1 is the model's, unchanged)."""
    tok_logp: np.ndarray
    rank: np.ndarray
    name_logp: np.ndarray
    n_tok: np.ndarray
    n_kept: Optional[np.ndarray] = None

    @property
    def tokens(self) -> int:
        return int(self.n_tok.sum())

    @property
    def impossible(self) -> int:
        return int(np.isneginf(self.name_logp).sum())

    @property
    def nll_per_char(self) -> float:
        return float(-self.tok_logp.astype(np.float64).sum() / max(self.tokens, 1))

    @property
    def perplexity(self) -> float:
        return float(np.exp(self.nll_per_char))

    @property
    def top1(self) -> float:
        return float((self.rank == 0).sum() / max(self.tokens, 1))


encode_prefixes = cpu_ref.encode_prefixes   # (rows [N, MAX_LEN] uint8, plen [N] int32), validated


def encode_names(names, cfg: GRUConfig) -> np.ndarray:
    """Names (bytes, or str taken as latin-1) -> rows [N, MAX_LEN+1] uint8 in the ``generate`` format:
    the chars, the EOS byte when the name is shorter than MAX_LEN (a name of exactly MAX_LEN chars has
    none, as a generated one that was cut off), NUL padding.  Longer names, chars outside the
    vocabulary and names that contain the EOS byte raise ValueError."""
    ML = cfg.max_len
    rows = np.zeros((len(names), ML + 1), dtype=np.uint8)
    for i, nm in enumerate(names):
        try:
            b = nm.encode("latin-1") if isinstance(nm, str) else bytes(nm)
        except UnicodeEncodeError as e:
            raise ValueError(f"name {i} ({nm!r}) is not latin-1") from e
        if len(b) > ML:
            raise ValueError(f"name {i} ({nm!r}) has {len(b)} chars, more than max_len = {ML}")
        a = np.frombuffer(b, dtype=np.uint8)
        if (a >= cfg.vocab).any():
            raise ValueError(f"name {i} ({nm!r}) holds a byte >= vocab ({cfg.vocab})")
        if (a == cfg.eos).any():
            raise ValueError(f"name {i} ({nm!r}) contains the EOS byte {cfg.eos}")
        rows[i, :len(b)] = a
        if len(b) < ML:
            if cfg.eos >= cfg.vocab:
                raise ValueError(f"eos {cfg.eos} outside the vocabulary of {cfg.vocab}")
            rows[i, len(b)] = cfg.eos
    return rows


# --------------------------------------------------------------------------- 3-call API
class _State:
    cfg: GRUConfig
    ctx: DistCtx
    gen = None            # HipGenerator or None (CPU path)
    params = None
    comm = None


_S: Optional[_State] = None


def namegen_initialize(N: int, rng_seed: int, parameter_fname: str, cfg: Optional[GRUConfig] = None,
                       fmt: str = "auto", ctx: Optional[DistCtx] = None, precision: str = "fp32") -> None:
    """namegensf.cu:359-618.  ``rng_seed`` is accepted and unused, as in the reference.
    ``precision``: "fp32" (default), "bf16x3" (split-bf16 products) or "bf16" (fast mode) on the GPU
    path (see HipGenerator); the CPU path is the fp32 oracle."""
    global _S
    from ..parallel import dist as gdist
    from ..utils import ckpt
    s = _State()
    s.ctx = ctx or gdist.init(verbose=True)
    if s.ctx.is_main:
        s.cfg, params = ckpt.load(parameter_fname, cfg, fmt)
    else:
        s.cfg, params = (cfg or GRUConfig()), None
    if s.ctx.world > 1:   # dims + weights from rank 0
        import torch.distributed as dist
        box = [s.cfg]
        dist.broadcast_object_list(box, 0)
        s.cfg = box[0]
    if s.ctx.device.type == "cuda":
        from ..parallel.rccl import make_comm
        s.comm = make_comm(s.ctx)
        lay = flat_layout(s.cfg)
        flat = (to_flat(s.cfg, params) if params is not None
                else torch.zeros(lay.total)).to(s.ctx.device)
        if s.comm is not None:
            s.comm.broadcast_f32(flat.data_ptr(), lay.total, 0, torch.cuda.current_stream().cuda_stream)
        # E / H off the 64-grid: the generator pads the parameters itself, so it takes them as views of
        # the (broadcast) buffer instead of sharing it
        off_grid = pad_config(s.cfg).replace(vocab=s.cfg.vocab) != s.cfg
        s.gen = HipGenerator(s.cfg, lay.views(flat.cpu()) if off_grid else {}, device=s.ctx.device,
                             flat=None if off_grid else flat,
                             max_batch=max(64, min(8192, N // max(1, s.ctx.world) + 1)), precision=precision)
    else:
        lay = flat_layout(s.cfg)
        flat = to_flat(s.cfg, params) if params is not None else torch.zeros(lay.total)
        if s.ctx.world > 1:
            import torch.distributed as dist
            dist.broadcast(flat, 0)
        s.params = {k: v.clone() for k, v in lay.views(flat).items()}
    gdist.barrier()
    _S = s


def _slice_control(v, N: int, start: int, count: int):
    """This rank's part of a control given for the N names of the job (scalars and a single str / bytes
    prefix apply to every name)."""
    if v is None or isinstance(v, (str, bytes)) or np.ndim(v) == 0:
        return v
    if len(v) != N:
        raise ValueError(f"a per-name control needs {N} entries, got {len(v)}")
    return v[start:start + count]


def _slice_logit_bias(v, N: int, start: int, count: int):
    """This rank's part of ``logit_bias``: one row (a dict or V values) applies to every name, a list of N
    rows is sliced by global name index."""
    if cpu_ref._soft_is_single(v):
        return v
    if len(v) != N:
        raise ValueError(f"logit_bias: one row or {N} rows expected, got {len(v)}")
    return v[start:start + count]


def _slice_constraints(cfg: GRUConfig, constraints, N: int, start: int, count: int):
    """This rank's part of the job's constraints: a Constraints object's idx rows by global name index
    (the table is shared), a keyword dict's per-name values like any control."""
    if constraints is None:
        return None
    if isinstance(constraints, cpu_ref.Constraints):
        if constraints.idx.shape[0] != N:
            raise ValueError(f"constraints for {N} names expected, got {constraints.idx.shape[0]}")
        return constraints.slice(start, count)
    if isinstance(constraints, cpu_ref.Automaton):
        if constraints.start.shape[0] != N:
            raise ValueError(f"constraints for {N} names expected, got {constraints.start.shape[0]}")
        return constraints.slice(start, count)
    def one_list(k, v):   # exclude = one list of names for every name of the job, not a per-name value
        return k == "exclude" and v is not None and all(isinstance(x, (str, bytes)) for x in v)
    return {k: v if one_list(k, v) else _slice_control(v, N, start, count) for k, v in dict(constraints).items()}


def namegen(N: int, random_floats: np.ndarray, output: np.ndarray, *, temperature=None, top_k=None, top_p=None,
            prefix=None, constraints=None, persist_constraints=None, logit_bias=None, presence_penalty=None,
            frequency_penalty=None, persist_soft=None) -> None:
    """namegensf.cu:627-890.  ``output`` (rank 0): uint8 [N*(MAX_LEN+1)] filled in place.
    ``temperature`` / ``top_k`` / ``top_p`` / ``prefix``: sampling controls (HipGenerator.generate_device),
    scalars or one value per name of the job; every rank takes its names' slice.  ``constraints``: a
    cpu_ref.Constraints / cpu_ref.Automaton for the N names or a dict of make_constraints keywords
    (docs/DESIGN.md §4e, §4g: ``regex`` / ``exclude``), sliced by global name index like the prefixes.
    ``persist_constraints``: HipGenerator.set_persist_constraints for this and later calls (None: as it
    is); the CPU path ignores it.  ``logit_bias`` / ``presence_penalty`` / ``frequency_penalty``: the soft
    controls (docs/DESIGN.md §4h), one value for every name or one per name of the job, sliced likewise.
    ``persist_soft``: HipGenerator.set_persist_soft for this and later calls (None: as it is); the CPU path
    ignores it."""
    assert _S is not None, "call namegen_initialize first"
    cfg, ctx = _S.cfg, _S.ctx
    ML = cfg.max_len
    start, count = shard(N, ctx.rank, ctx.world)
    per = -(-N // ctx.world)          # ceil: fixed slab size for the all-gather
    ctl = {k: _slice_control(v, N, start, count) for k, v in
           (("temperature", temperature), ("top_k", top_k), ("top_p", top_p), ("prefix", prefix)) if v is not None}
    if constraints is not None:
        ctl["constraints"] = _slice_constraints(cfg, constraints, N, start, count)
    if logit_bias is not None:
        ctl["logit_bias"] = _slice_logit_bias(logit_bias, N, start, count)
    for k, v in (("presence_penalty", presence_penalty), ("frequency_penalty", frequency_penalty)):
        if v is not None:
            ctl[k] = _slice_control(v, N, start, count)
    if _S.gen is not None:
        if persist_constraints is not None:
            _S.gen.set_persist_constraints(persist_constraints)
        if persist_soft is not None:
            _S.gen.set_persist_soft(persist_soft)
        _S.gen.g.set_global_names(N)   # bf16 mode: the same arithmetic path at every world size
        mine = _S.gen.generate(random_floats, start, count, **ctl)
        if ctx.world > 1:
            dev = ctx.device
            slab = torch.zeros(per, ML + 1, dtype=torch.uint8, device=dev)
            slab[:count] = torch.from_numpy(mine).to(dev)
            allv = torch.empty(ctx.world, per, ML + 1, dtype=torch.uint8, device=dev)
            _S.comm.allgather_u8(slab.data_ptr(), allv.data_ptr(), slab.numel(),
                                 torch.cuda.current_stream().cuda_stream)
            allv = allv.cpu().numpy()
        else:
            allv = mine[None]
    else:
        mine = cpu_ref.generate(_S.params, cfg, random_floats, start, count, **ctl)
        if ctx.world > 1:
            import torch.distributed as dist
            slab = torch.zeros(per, ML + 1, dtype=torch.uint8)
            slab[:count] = torch.from_numpy(mine)
            bufs = [torch.empty_like(slab) for _ in range(ctx.world)]
            dist.all_gather(bufs, slab)
            allv = torch.stack(bufs).numpy()
        else:
            allv = mine[None]
    if ctx.is_main:
        res = np.zeros((N, ML + 1), dtype=np.uint8)
        for r in range(ctx.world):
            s0, c0 = shard(N, r, ctx.world)
            res[s0:s0 + c0] = allv[r][:c0]
        output.reshape(-1)[: N * (ML + 1)] = res.reshape(-1)


def namegen_finalize() -> None:
    """namegensf.cu:897-1033 (frees everything; no MPI_Finalize here either)."""
    global _S
    _S = None
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def decode_names(output: np.ndarray, N: int, max_len: int) -> list:
    rows = np.asarray(output, dtype=np.uint8).reshape(-1)[: N * (max_len + 1)].reshape(N, max_len + 1)
    return [bytes(r).split(b"\0", 1)[0].decode("latin-1") for r in rows]

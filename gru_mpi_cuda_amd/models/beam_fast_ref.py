"""Reference of the bf16 fast beam search (csrc/kernels/beam_fast.hip, Generator::beam_fast; docs/DESIGN.md
§4d "Fast bf16 beam search"; the rule: cpu_ref.beam_search(round_operands=True)).

* ``twin``: the float64 trajectory with bf16-rounded operands -- beam_ref's ``_run`` on params whose matrices are
  bf16-exact, every h rounded where a product reads it -- with beam_ref's per-step clearance.
* ``rows_D``: D, the largest |twin - exact| float64 ``name_logp`` (cpu_ref.score with and without
  ``round_operands``) over the twin's rows.  The device rounds fp32-accumulated states where the twin rounds
  float64 ones: single roundings can flip, the effect has the same size, hence the guard 2 D (§4a's form).
* ``logp_bound``: per row, the sum over its tokens of 2 D + 1e-5 + 2e-7 exp(-ref_tok) (tests/test_score_fast_gpu.py's
  token bound, summed), against cpu_ref.score(rows, round_operands=True) in float64.
* A prefix is *settled* when its smallest clearance is at least 2 D: only then are the rows and their order
  compared with the twin's; every prefix keeps beam_ref.check_result's invariants.

At that guard beam_ref.TRAJ_CASES are unusable (D ~ 8e-3 on the x8-sharpened models, 5 - 7 of 8 prefixes
unsettled), so the cases here run mostly long prefixes (0 - 2 free steps) beside a few short ones, W <= 8, and
seeds picked on the CPU from the twin alone: in every case at most half of the prefixes are unsettled
(tests/test_beam_fast_ref.py asserts it; it is a condition of the GPU test).
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple

import numpy as np

from . import beam_ref, cpu_ref
from ..config import GRUConfig
from .params import init_params
from .seq_ref import bf16_round

Out = Dict[str, object]


class FastCase(NamedTuple):
    name: str
    V: int
    E: int
    H: int
    L: int
    ML: int
    eos: int
    W: int
    prefixes: tuple
    seed: int
    sharp: float
    compare: bool = True      # False: the shape cannot meet the cap below; it keeps the invariants only


def _prefixes(V: int, ML: int, eos: int) -> tuple:
    """Eight long prefixes (0 .. 2 free steps, beam_ref._long) and two short ones."""
    ok = [c for c in beam_ref._alpha(V) if ord(c) != eos]
    return beam_ref._long(V, ML, eos, 8) + ("", ok[3] + ok[11])


# The first seed from 4 at which the case meets the cap (python -m gru_mpi_cuda_amd.models.beam_fast_ref reprints
# every case's D and unsettled count).  V = 256 with W = 8 meets it at no seed from 4 to 21 (6 - 7 of 10
# unsettled at L = 1 and at L = 2: nine candidates per free step, 2 D ~ 1e-2 apart): those two cases keep the
# invariants and the logp bound, and the kernel-level test carries the order.
_SEEDS: Dict[str, int] = {"L1-V64-W8": 11}
_NO_CAP = ("L1-V256-W8", "L2-V256-W8")
SHARP = 8.0


def _cases() -> List[FastCase]:
    out = []
    for L in (1, 2):
        for V, E, H, ML in ((64, 64, 64, 6), (256, 128, 256, 10)):
            for W in (1, 3, 8):
                name = f"L{L}-V{V}-W{W}"
                out.append(FastCase(name, V, E, H, L, ML, 0, W, _prefixes(V, ML, 0), _SEEDS.get(name, 4), SHARP,
                                    name not in _NO_CAP))
    return out


CASES = _cases()
_models: Dict[tuple, tuple] = {}
_twins: Dict[tuple, Out] = {}


def case_model(c: FastCase):
    """(cfg, fp32 params) of a case: beam_ref's sharpened init, every tensor rounded to bf16 -- the device's bf16
    copies then hold the same values as the fp32 masters.  Shared, never modified."""
    key = (c.V, c.E, c.H, c.L, c.ML, c.eos, c.seed, c.sharp)
    if key not in _models:
        cfg = GRUConfig(vocab=c.V, embed=c.E, hidden=c.H, layers=c.L, max_len=c.ML, sos=0, eos=c.eos, seed=c.seed)
        p = init_params(cfg)
        p["fc.weight"] = p["fc.weight"] * c.sharp
        _models[key] = (cfg, {k: bf16_round(v) for k, v in p.items()})
    return _models[key]


def score64(params, cfg: GRUConfig, rows: np.ndarray, round_operands: bool):
    """float64 cpu_ref.score of [N][W][ML + 1] rows: (tok_logp [N W][ML], name_logp [N][W], n_tok [N W])."""
    N, W = rows.shape[:2]
    p64 = {k: v.double() for k, v in params.items()}
    tok, name, nt, _ = cpu_ref.score(p64, cfg, rows.reshape(N * W, -1), round_operands=round_operands)
    return tok, name.reshape(N, W), nt


def rows_D(params, cfg: GRUConfig, rows: np.ndarray, n_beams: np.ndarray) -> float:
    """The largest |twin - exact| float64 name_logp over the live rows."""
    a, b = score64(params, cfg, rows, True)[1], score64(params, cfg, rows, False)[1]
    live = np.arange(rows.shape[1])[None, :] < np.asarray(n_beams)[:, None]
    return float(np.abs(a - b)[live].max())


def twin(c: FastCase) -> Out:
    """A case's float64 twin trajectory with ``D`` and ``settled`` (every step's clearance at least 2 D),
    computed once and shared (never modified)."""
    key = tuple(c)
    if key not in _twins:
        cfg, p = case_model(c)
        pre, plen = cpu_ref.beam_inputs(cfg, list(c.prefixes), c.W)
        out = beam_ref._run(p, cfg, pre, plen, c.W, True, rnd=bf16_round)
        out["D"] = rows_D(p, cfg, out["rows"], out["n_beams"])
        out["settled"] = out["clear"].min(1) >= 2 * out["D"]
        _twins[key] = out
    return _twins[key]


def logp_bound(params, cfg: GRUConfig, rows: np.ndarray, D: float):
    """(ref, bound) [N][W]: the rows' float64 log-probability with rounded operands, and per row the sum over its
    tokens of 2 D + 1e-5 + 2e-7 exp(-ref_tok)."""
    tok, name, nt = score64(params, cfg, rows, True)
    mask = np.arange(cfg.max_len)[None, :] < nt[:, None]
    per = np.where(mask, 2 * D + 1e-5 + 2e-7 * np.exp(-tok), 0.0).sum(1)
    return name, per.reshape(name.shape)


if __name__ == "__main__":
    for case in CASES:
        t = twin(case)
        print(f"{case.name}: seed {case.seed}, D {t['D']:.3e}, unsettled {int((~t['settled']).sum())} of {len(case.prefixes)}",
              flush=True)

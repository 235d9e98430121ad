"""Per-element reference of the stochastic beam search (csrc/kernels/sbs.hip, Generator::distinct; the
rule: docs/DESIGN.md §4i, cpu_ref.sample_distinct / cpu_ref.sbs_step).

* ``philox4x32`` / ``sbs_uniform``: the numpy twin of the device's counter-based noise (cpu_ref's).
* ``step_inputs``: one launch of sbs_select_f32 on planted inputs -- logits on exact grids (the parts a
  kernel sums back are exact in fp32, as beam_ref's), logq on a 2^-7 grid, G = logq + a multiple of 2^-5 in
  [-2, 3], every slot state, forced / free / mixed steps, a per-position mask or an automaton state buffer,
  1 / T in {1, 1.25}, seeds and start indices above 2^32, a duplicated slot (exact ties in Gt).
* ``select_ref`` / ``select_emulate``: cpu_ref.sbs_step in float64 from the given fp32 inputs, and in
  float32 with a ``mut`` hook: one function, the dtype switched.  In float32 every operation of the kernel is
  done in its order and rounded once, the row sum as the kernel's lane sums and neighbour tree; expf, logf,
  log1pf and expm1f are taken as correctly rounded, which the device's are not (an ulp or two), so the
  emulator bounds the kernel's deviation, it does not reproduce its bits.
* ``oracle`` / ``emulate``: the whole trajectory on a model, float64 / float32.  The oracle also returns the
  clearance of every (name, step).
* ``check_step`` / ``check_result``: what the tests assert; every entry of MUTATIONS must fail them.

The truncation Gt = -log(e^-G_b - e^-Z + e^-g) is ill-conditioned where the parent's G_b lies above its
children's maximum Z: an error in g is amplified by dGt/dg = exp(Gt - g), up to exp(G_b - Z) for a child
next to the row's best one (dGt/dZ = -exp(Gt - Z) and dGt/dG_b = exp(Gt - G_b) are no larger).  The row
figure exp(G_b - Z) is about 1 / q_b -- G stays O(1) along a search while logq falls with every char -- so as
a unit it reaches 10^5 .. 10^7 after four chars and no pair of candidates would ever clear a guard scaled
by it; the unit used here is the candidate's own factor, scale = max(1, exp(Gt - g)), never larger than the
row's, and 1 for a row's best child (Gt == G_b bitwise) and for a carry.  A Gt deviation is measured in
units of its scale, the tolerance of a candidate is ATOL times that scale, and the clearance of a (name,
step) is the smallest neighbour gap in Gt among the first W + 1 candidates, each gap divided by the larger
scale of the two (bitwise-equal ties are resolved by j in both precisions and not
counted).  A name whose smallest clearance is below GUARD is *unsettled*: fp32 may order two candidates
the other way, so only its invariants are checked, not its bytes.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from . import cpu_ref
from ..config import GRUConfig
from .params import init_params
from .cpu_ref import philox4x32, sbs_uniform   # noqa: F401  (the numpy Philox lives beside the rule)

Out = Dict[str, object]
DEAD, LIVE, FIN = cpu_ref.BEAM_DEAD, cpu_ref.BEAM_LIVE, cpu_ref.BEAM_FIN

# Deviation of the float32 emulator from float64, the largest over STEP_CASES x seeds 0, 1, 2 and over
# TRAJ_CASES, rounded up to three digits:
#   lq   : an entry of a row's renormalised log-softmax
#   Gt   : a candidate's truncated perturbed value in units of its scale (a row's Z: scale 1; a returned
#          row's final perturbed value: in units of the largest scale its name met)
#   logq : a new slot's / a returned row's log-probability
# Measured, not chosen: ``python -m gru_mpi_cuda_amd.models.sbs_ref`` reprints them.
MEASURED_DEV = {
    "lq": 1.99e-06,
    "Gt": 4.62e-06,
    "logq": 4.26e-06,
}
GUARD = 8.0 * MEASURED_DEV["Gt"]
ATOL = {k: 4.0 * v for k, v in MEASURED_DEV.items()}


# ------------------------------------------------------------------------------ one step
class StepCase(NamedTuple):
    V: int
    W: int
    N: int
    splits: int = 1
    bias: bool = False
    mode: str = "free"            # free | forced | mixed (odd names forced)
    states: str = "mix"           # mix | live | fin | step0 (all but slot 0 dead)
    mask: str = "none"            # none | pos (a line per name and step) | auto (a line per slot)
    eos: int = 5
    big: bool = False             # seed and start above 2^32
    optional: bool = True         # with the lq / gt / zmax / sel outputs


def _step_cases() -> List[StepCase]:
    out = []
    modes, states = ("free", "forced", "mixed"), ("mix", "live", "fin", "step0")
    i = 0
    for V in (64, 256, 512):
        for W in (1, 4, 16, 17, 32):
            for N in (1, 3):
                mask = ("none", "pos", "auto")[(i // 2) % 3]
                if mask == "auto" and V == 64:
                    mask = "pos"
                out.append(StepCase(V, W, N, 1 + i % 2, i % 3 == 1, modes[i % 3], states[(i // 3) % 4], mask, (5, 0)[i % 2],
                                    i % 2 == 1, i % 4 != 3))
                i += 1
    return out


STEP_CASES = _step_cases()
SOS = 1
LINES = 6     # lines of a planted constraint table / states of a planted automaton


def step_inputs(c: StepCase, seed: int = 0) -> Out:
    """Planted inputs of one sbs_select_f32 launch (the docstring above).  Pad rows up to the 64-row granule
    hold NaN: the kernel never reads them."""
    V, W, N = c.V, c.W, c.N
    rng = np.random.default_rng(1000 * seed + 7 * V + 131 * W + N + 17 * c.splits)
    R = N * W
    Rp = (R + 63) // 64 * 64
    x = np.stack([(0.05 * rng.permutation(V)).astype(np.float32) for _ in range(R)])
    if c.splits > 1 or c.bias:
        x = (np.round(x.astype(np.float64) * 4096) / 4096).astype(np.float32)
    logq = (-rng.integers(0, 1025, R) / 128.0).astype(np.float32)
    G = (logq + rng.integers(-64, 97, R) / 32.0).astype(np.float32)
    if c.states == "live":
        state = np.full(R, LIVE, np.int32)
    elif c.states == "fin":
        state = np.full(R, FIN, np.int32)
    elif c.states == "step0":
        state = np.where(np.arange(R) % W == 0, LIVE, DEAD).astype(np.int32)
    else:
        state = rng.integers(0, 3, R).astype(np.int32)
        state[::W] = np.where(np.arange(N) % 3 == 2, FIN, LIVE)      # slot 0: never dead
    logq[state == DEAD] = -np.inf
    G[state == DEAD] = -np.inf
    if W >= 3:     # slot 2: a bitwise copy of slot 0 -- its best child ties with slot 0's in Gt
        for n in range(N):
            x[n * W + 2], logq[n * W + 2], G[n * W + 2], state[n * W + 2] = x[n * W], logq[n * W], G[n * W], state[n * W]
    bias = (0.25 * rng.integers(-4, 5, V)).astype(np.float32) if c.bias else None
    buf = np.full((c.splits, Rp, V), np.nan, np.float32)
    buf[:, :R] = 0
    buf[0, :R] = x - bias if c.bias else x
    if c.splits == 2:
        buf[1, :R] = (0.25 * rng.integers(-8, 9, (R, V))).astype(np.float32)
        buf[0, :R] = buf[0, :R] - buf[1, :R]
    back = buf[0, :R].copy()
    if c.splits == 2:
        back = back + buf[1, :R]
    if c.bias:
        back = back + bias
    assert back.dtype == np.float32 and (back == x).all()
    ML, step = 6, 2
    plen = np.zeros(N, np.int32)
    if c.mode == "forced":
        plen[:] = ML
    elif c.mode == "mixed":
        plen[1::2] = step + 1
    prefix = rng.integers(0, min(V, 256), (N, ML)).astype(np.uint8)
    prefix[prefix == c.eos] = 7
    inv_t = np.where(np.arange(N) % 2 == 0, 1.0, 1.25).astype(np.float32)
    d = dict(case=c, V=V, W=W, N=N, R=R, Rp=Rp, splits=c.splits, logits=buf, bias=bias, logq=logq, G=G, state=state,
             plen=plen, prefix=prefix, step=step, ML=ML, sos=SOS, eos=c.eos, inv_t=inv_t,
             seed=(0x9E3779B97F4A7C15 * (seed + 1)) % 2 ** 64 if c.big else 12345 + seed,
             start=2 ** 33 + 5 + seed if c.big else 3 + seed,
             tab=None, idx=None, astate=None, nxt=None, allowed=None)
    if c.mask != "none":     # line 0: everything; the others: about half the chars
        bits = rng.random((LINES, V)) < 0.5
        bits[0] = True
        d["tab"] = np.ascontiguousarray(cpu_ref._pack_lines(bits, V))
        if c.mask == "pos":
            d["idx"] = rng.integers(0, LINES, (N, ML)).astype(np.int32)
            d["allowed"] = bits[d["idx"][:, step]]
        else:
            ast = rng.integers(0, LINES, R).astype(np.int32)
            ast[state != LIVE] = 0        # a carried or dead slot sits in the free state
            if W >= 3:
                ast.reshape(N, W)[:, 2] = ast.reshape(N, W)[:, 0]
            d["astate"] = ast
            d["nxt"] = rng.integers(0, LINES, (LINES, V)).astype(np.uint16)
            d["allowed"] = bits[ast].reshape(N, W, V)
    return d


def _x_of(d: Out, dt) -> np.ndarray:
    R = d["R"]
    x = d["logits"][0, :R].astype(dt)
    for s in range(1, d["splits"]):
        x = x + d["logits"][s, :R].astype(dt)
    if d["bias"] is not None:
        x = x + d["bias"].astype(dt)
    return x


def _clearance(s: Out, unit: str = "top_scale") -> np.ndarray:
    """[N]: the smallest scaled neighbour gap among each name's first W + 1 candidates (inf with fewer than
    two, bitwise ties not counted).  ``unit``: "top_scale", the candidates' own factors, or "top_row_scale",
    their rows' supremum exp(G_b - Z) (``row_unit_counts``)."""
    gt, sc = s["top_gt"].astype(np.float64), s[unit]
    with np.errstate(invalid="ignore"):
        gap = (gt[:, :-1] - gt[:, 1:]) / np.maximum(sc[:, :-1], sc[:, 1:])
    gap = np.where(np.isnan(gap) | (gap == 0), np.inf, gap)
    return gap.min(1) if gap.shape[1] else np.full(gt.shape[0], np.inf)


def _select_all(d: Out, f64: bool, mut: Optional[str] = None) -> Out:
    V, W, N = d["V"], d["W"], d["N"]
    dt = np.float64 if f64 else np.float32
    x = _x_of(d, dt).reshape(N, W, V)
    forced = np.full(N, -1, np.int64)
    for n in range(N):
        if d["step"] < d["plen"][n]:
            f = int(d["prefix"][n, d["step"]])
            forced[n] = f if f < V else 0
    g = np.arange(N, dtype=np.uint64) + np.uint64(0 if mut == "counter_local_index" else d["start"])
    u = sbs_uniform(d["seed"], g, 0 if mut == "counter_without_step" else d["step"], W, V)
    s = cpu_ref.sbs_step(x, d["logq"].astype(dt).reshape(N, W), d["G"].astype(dt).reshape(N, W), d["state"].reshape(N, W),
                         forced, d["allowed"], d["inv_t"], u, d["eos"], d["sos"], mut)
    out: Out = {k: s[k].reshape(N * W) for k in ("parent", "chr", "state", "logq", "G", "next_id", "sel", "zmax")}
    out.update(lq=s["lq"].reshape(N * W, V), gt=s["gt"].reshape(N * W, V), scale=s["scale"].reshape(N * W, V),
               wscale=np.where(np.isnan(s["top_scale"][:, :W]), 1.0, s["top_scale"][:, :W]).reshape(N * W),
               clear=_clearance(s))
    if d["astate"] is not None:    # the children's automaton states
        q = d["astate"].reshape(N, W)[np.arange(N)[:, None], np.maximum(s["parent"], 0)]
        out["astate"] = np.where(s["chr"] >= 0, d["nxt"][q, np.maximum(s["chr"], 0)], 0).astype(np.int32).reshape(-1)
    return out


def select_ref(d: Out) -> Out:
    return _select_all(d, True)


def select_emulate(d: Out, mut: Optional[str] = None) -> Out:
    assert mut is None or mut in MUTATIONS, mut
    return _select_all(d, False, mut)


def settled_inputs(c: StepCase, seed: int = 0) -> Out:
    """The first ``step_inputs(c, seed + 100 k)``, k = 0, 1, ..., in which every name clears the guard."""
    for k in range(32):
        d = step_inputs(c, seed + 100 * k)
        if (select_ref(d)["clear"] >= GUARD).all():
            return d
    raise AssertionError(f"{c}: no planted input clears the guard")


def _dev(got, ref, unit=None) -> float:
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ok = np.isfinite(ref) & np.isfinite(got)
    if not ok.any():
        return 0.0
    with np.errstate(invalid="ignore"):
        e = np.abs(got - ref)
    if unit is not None:
        e = e / np.broadcast_to(unit, e.shape)
    return float(e[ok].max())


def _same_pattern(got, ref) -> bool:
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return bool(np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
                and np.array_equal(np.sign(got[np.isinf(got)]), np.sign(ref[np.isinf(ref)])))


def check_step(d: Out, ref: Out, got: Out) -> List[str]:
    """The failures of one launch's outputs (float32) against the float64 rule (empty: passed).  ``got``:
    parent, chr, state, next_id, logq, G and optionally sel, astate, lq, gt, zmax."""
    N, W, V = d["N"], d["W"], d["V"]
    bad = []
    settled = np.repeat(ref["clear"] >= GUARD, W)
    for k in ("parent", "chr", "state", "next_id", "sel", "astate"):
        if got.get(k) is None or k not in ref:
            continue
        g = np.asarray(got[k], np.int64)
        if not np.array_equal(g[settled], ref[k].astype(np.int64)[settled]):
            bad.append(f"{k}: differs at {np.flatnonzero((g != ref[k]) & settled)[:8].tolist()}")
    par = np.maximum(np.asarray(got["parent"], np.int64), 0) + np.repeat(np.arange(N) * W, W)
    for k, unit in (("logq", None), ("G", ref["wscale"])):
        if not _same_pattern(np.asarray(got[k])[settled], ref[k][settled]):
            bad.append(f"{k}: the dead slots differ")
        else:
            dev = _dev(np.asarray(got[k])[settled], ref[k][settled], None if unit is None else unit[settled])
            if not dev <= ATOL["Gt" if k == "G" else k]:
                bad.append(f"{k}: deviation {dev:.3e} > {ATOL['Gt' if k == 'G' else k]:.3e}")
    Gin = d["G"].astype(np.float32)
    gG = np.asarray(got["G"], np.float32)
    if not (gG.reshape(N, W)[:, 1:] <= gG.reshape(N, W)[:, :-1]).all():
        bad.append("G: not non-increasing along the slots")
    chosen = np.asarray(got["parent"], np.int64) >= 0
    if (gG[chosen] > Gin[par][chosen]).any():
        bad.append("G: a child above its parent")
    for k, unit in (("lq", None), ("gt", ref["scale"]), ("zmax", None)):
        if got.get(k) is None:
            continue
        if not _same_pattern(got[k], ref[k]):
            bad.append(f"{k}: the NaN / inf pattern differs")
            continue
        dev = _dev(got[k], ref[k], unit)
        a = ATOL["lq" if k == "lq" else "Gt"]
        if not dev <= a:
            bad.append(f"{k}: deviation {dev:.3e} > {a:.3e}")
    if got.get("gt") is not None:     # bitwise: a live parent's best child keeps G_b, no child lies above it
        gt = np.asarray(got["gt"], np.float32)
        rows = np.flatnonzero((d["state"] == LIVE) & ~np.isnan(gt).all(1))
        if len(rows):
            best = np.nanmax(gt[rows], 1)
            if not np.array_equal(best, Gin[rows]):
                bad.append(f"gt: the best child of rows {rows[best != Gin[rows]][:8].tolist()} is not G_b bitwise")
    if got.get("lq") is not None:     # bitwise: a child's logq is psi = logq_b + lq[c] (0 on a forced step)
        lq = np.asarray(got["lq"], np.float32)
        ch = np.asarray(got["chr"], np.int64)
        kid = ch >= 0
        forced = np.repeat(d["step"] < d["plen"], W)
        add = np.where(forced, np.float32(0), lq[par, np.maximum(ch, 0)]).astype(np.float32)
        psi = (d["logq"].astype(np.float32)[par] + add).astype(np.float32)
        if not np.array_equal(np.asarray(got["logq"], np.float32)[kid], psi[kid]):
            bad.append("logq: a child's value is not logq_b + lq[c] bitwise")
    return bad


# ------------------------------------------------------------------------------ the trajectory
class TrajCase(NamedTuple):
    name: str
    V: int
    E: int
    H: int
    L: int
    ML: int
    eos: int
    W: int
    prefixes: tuple
    seed: int = 4                 # the model's
    noise: int = 1                # the search's seed
    start: int = 0
    temperature: Optional[float] = None
    constraints: Optional[dict] = None
    preset: Optional[str] = None


def _alpha(V: int) -> str:
    return "".join(chr(c) for c in range(33, min(V, 127)))


def _mixture(V: int, ML: int, eos: int, n: int) -> tuple:
    """n prefixes: empty, short, of length ML and lengths in between, chars inside the vocabulary, no EOS."""
    ok = [c for c in _alpha(V) if ord(c) != eos]
    out = []
    for i in range(n):
        ln = min((0, 1, ML, 2, 0, ML // 2, 1, 3)[i % 8], ML)
        out.append("".join(ok[(5 * i + 3 * j + i // 8) % len(ok)] for j in range(ln)))
    return tuple(out)


def _traj_cases() -> List[TrajCase]:
    out = []

    def add(name, V, E, H, L, ML, eos, W, prefixes, **kw):
        out.append(TrajCase(name, V, E, H, L, ML, eos, W, prefixes, **kw))

    i = 0
    for H, L in ((64, 1), (128, 2)):
        for npre in (1, 3, 9):
            for W in (1, 4, 17, 32):
                ML = (5, 3, 4)[i % 3]
                add(f"h{H}-L{L}-n{npre}-W{W}", 64, 64, H, L, ML, (5, 0)[i % 2], W, _mixture(64, ML, (5, 0)[i % 2], npre),
                    start=(0, 2 ** 33 + 7)[i % 2])
                i += 1
    add("pattern", 64, 64, 64, 1, 4, 0, 4, ("12", "", "7"), constraints=dict(charset="0123456789", min_len=2))
    add("temperature", 64, 64, 128, 2, 4, 5, 4, _mixture(64, 4, 5, 3), temperature=0.7)
    add("regex3", 256, 64, 64, 1, 4, 0, 4, ("", "a"), constraints=dict(regex="a(b|c|d)"))
    add("ref", 0, 0, 0, 0, 0, 0, 4, ("Ma", ""), preset="ref", temperature=0.7)
    return out


TRAJ_CASES = _traj_cases()
_models: Dict[tuple, tuple] = {}


def case_model(c: TrajCase):
    """(cfg, fp32 params) of a case: init_params with fc.weight x 8 (a sharper model, as beam_ref's), or the
    ``ref`` preset's configuration with fresh parameters.  Shared, never modified."""
    key = (c.preset, c.V, c.E, c.H, c.L, c.ML, c.eos, c.seed)
    if key not in _models:
        if c.preset is not None:
            from ..config import PRESETS
            cfg = PRESETS[c.preset].replace(seed=c.seed)
        else:
            cfg = GRUConfig(vocab=c.V, embed=c.E, hidden=c.H, layers=c.L, max_len=c.ML, sos=0, eos=c.eos, seed=c.seed)
        p = init_params(cfg)
        p["fc.weight"] = p["fc.weight"] * 8.0
        _models[key] = (cfg, p)
    return _models[key]


def case_kwargs(c: TrajCase) -> dict:
    """The keywords of ``sample_distinct`` for a case (beside prefix and width)."""
    return dict(seed=c.noise, start=c.start, temperature=c.temperature, constraints=c.constraints)


def _run(params, cfg: GRUConfig, prefixes, W: int, f64: bool, seed=0, start=0, temperature=None, constraints=None,
         mut: Optional[str] = None, unit: str = "top_scale") -> Out:
    pre, plen, inv, seed, start = cpu_ref.distinct_inputs(cfg, list(prefixes), W, None, seed, start, temperature)
    cons = cpu_ref.as_constraints(cfg, pre.shape[0], constraints)
    cpu_ref.check_prefix_allowed(cons, pre, plen)
    p = {k: v.to(torch.float64 if f64 else torch.float32) for k, v in params.items()}
    trace: list = []
    r = cpu_ref.sample_distinct_rule(p, cfg, pre, plen, W, seed, start, inv, cons, mut, trace)
    clear = np.stack([_clearance(s, unit) for s in trace], 1)
    scale = np.stack([np.nanmax(np.where(np.isnan(s["top_scale"][:, :W]), 1.0, s["top_scale"][:, :W]), 1) for s in trace], 1)
    return dict(rows=r.rows, logq=r.logq, gumbel=r.gumbel, n_tok=r.n_tok, n_found=r.n_found, clear=clear,
                scale=scale.max(1), tops=[(s["sel"], s["G"], s["logq"]) for s in trace])


def oracle(params, cfg: GRUConfig, prefixes, W: int, **kw) -> Out:
    """The float64 trajectory: rows, logq, gumbel, n_tok, n_found, ``clear`` [N][ML], ``scale`` [N] (the largest
    scale among the winners' rows along the way) and ``settled`` [N] (every step's clearance at least GUARD)."""
    out = _run(params, cfg, prefixes, W, True, **kw)
    out["settled"] = out["clear"].min(1) >= GUARD
    return out


def emulate(params, cfg: GRUConfig, prefixes, W: int, mut: Optional[str] = None, **kw) -> Out:
    assert mut is None or mut in MUTATIONS, mut
    return _run(params, cfg, prefixes, W, False, mut=mut, **kw)


_oracles: Dict[str, Out] = {}


def case_oracle(c: TrajCase) -> Out:
    """A case's float64 trajectory, computed once and shared (never modified)."""
    if c.name not in _oracles:
        cfg, p = case_model(c)
        _oracles[c.name] = oracle(p, cfg, c.prefixes, c.W, **case_kwargs(c))
    return _oracles[c.name]


def score64_of(params, cfg: GRUConfig, prefixes, got, temperature=None, constraints=None) -> np.ndarray:
    """float64 cpu_ref.score (name_logp, under the sampler: the same keywords) of a result's rows, [N][W]; NaN for
    a dead slot."""
    rows = got["rows"] if isinstance(got, dict) else got.rows
    nf = got["n_found"] if isinstance(got, dict) else got.n_found
    N, W = rows.shape[:2]
    p64 = {k: v.double() for k, v in params.items()}
    out = np.full((N, W), np.nan)
    for n in range(N):      # per prefix: its rows share the prefix and the constraint
        k = int(nf[n])
        if k:
            cons = None if constraints is None else cpu_ref.as_constraints(cfg, k, dict(constraints))
            out[n, :k] = cpu_ref.score(p64, cfg, rows[n, :k], temperature=1.0 if temperature is None else temperature,
                                       prefix=[prefixes[n]] * k, constraints=cons)[1]
    return out


def check_result(cfg: GRUConfig, prefixes, orc: Out, got, score64: Optional[np.ndarray] = None) -> List[str]:
    """The failures of a result (a DistinctResult or a dict) against the oracle: bytes and counts of the
    settled prefixes, their logq and gumbel within ATOL, and for every prefix the invariants (distinct rows,
    gumbel non-increasing, rows start with the prefix, NUL after the name, dead slots as specified, logq
    equal to ``score64`` -- float64 cpu_ref.score of the returned rows under the same keywords -- within ATOL)."""
    g = got if isinstance(got, dict) else dict(rows=got.rows, logq=got.logq, gumbel=got.gumbel, n_tok=got.n_tok,
                                               n_found=got.n_found)
    pre, plen = cpu_ref.encode_prefixes(list(prefixes), cfg)
    N, W = g["logq"].shape
    ML = cfg.max_len
    bad = []
    for n in range(N):
        nb = int(g["n_found"][n])
        rows, lq, gm, nt = g["rows"][n], np.asarray(g["logq"][n], np.float64), np.asarray(g["gumbel"][n], np.float64), g["n_tok"][n]
        if orc["settled"][n]:
            if not (np.array_equal(rows, orc["rows"][n]) and np.array_equal(nt, orc["n_tok"][n]) and nb == orc["n_found"][n]):
                bad.append(f"prefix {n}: rows / n_tok / n_found differ from the oracle's")
            elif nb:
                dq = float(np.abs(lq[:nb] - orc["logq"][n, :nb]).max())
                dg = float(np.abs(gm[:nb] - orc["gumbel"][n, :nb]).max()) / float(orc["scale"][n])
                if not dq <= ATOL["logq"]:
                    bad.append(f"prefix {n}: logq deviates {dq:.3e}")
                if not dg <= ATOL["Gt"]:
                    bad.append(f"prefix {n}: gumbel deviates {dg:.3e} (in units of the scale {float(orc['scale'][n]):.3g})")
        if not (0 <= nb <= W) or (nb == 0 and W > 0):
            bad.append(f"prefix {n}: n_found {nb}")
            continue
        if not (np.isneginf(lq[nb:]).all() and np.isneginf(gm[nb:]).all() and (rows[nb:] == 0).all() and (nt[nb:] == 0).all()
                and np.isfinite(lq[:nb]).all() and np.isfinite(gm[:nb]).all()):
            bad.append(f"prefix {n}: dead slots not as specified")
        if (np.diff(gm[:nb]) > 0).any():
            bad.append(f"prefix {n}: gumbel increases")
        if gm[0] != 0:
            bad.append(f"prefix {n}: the first draw's gumbel is not the root's 0")
        if len({bytes(r) for r in rows[:nb]}) != nb:
            bad.append(f"prefix {n}: rows not distinct")
        for k in range(nb):
            t = int(nt[k])
            if not (plen[n] <= t <= ML and (rows[k, :plen[n]] == pre[n, :plen[n]]).all() and (rows[k, t:] == 0).all()):
                bad.append(f"prefix {n} draw {k}: prefix / padding")
            if (rows[k, :max(t - 1, 0)] == cfg.eos).any() or (t < ML and rows[k, t - 1] != cfg.eos):
                bad.append(f"prefix {n} draw {k}: EOS placement")
        if score64 is not None and nb:
            ds = float(np.abs(lq[:nb] - score64[n, :nb]).max())
            if not ds <= ATOL["logq"]:
                bad.append(f"prefix {n}: logq is not the rows' log-probability under the sampler ({ds:.3e})")
    return bad


# planted defects -> where the checks must catch them: "step" (some applicable STEP_CASES entry) or a
# TRAJ_CASES name
MUTATIONS = {
    "g_as_key": ("step", None),                 # the untruncated g used as the key
    "z_over_masked": ("step", None),            # Z taken over masked chars too
    "lq_not_renormalised": ("step", None),      # lq over the whole vocabulary under a mask
    "forced_adds_lp": ("step", None),           # a forced char adding its log-prob
    "naive_truncation": ("step", None),         # -log(e^-G - e^-Z + e^-g) in fp32
    "counter_without_step": ("step", None),     # the Philox counter without the step
    "counter_local_index": ("step", None),      # ... with the batch-local instead of the global name index
    "carry_reperturbed": ("step", None),        # a finished slot's carry perturbed afresh
    "logq_from_key": ("step", None),            # logq rebuilt from the key: Gt - gum
}


def mutation_applies(mut: str, c: StepCase) -> bool:
    """Whether a step case exercises the branch a mutation breaks."""
    live = c.states in ("live", "mix", "step0")
    if mut in ("z_over_masked", "lq_not_renormalised"):
        return c.mask != "none" and live and c.mode == "free"
    if mut == "forced_adds_lp":
        return c.mode == "forced" and live and c.mask == "none"
    if mut == "carry_reperturbed":
        return c.states == "fin"
    if mut in ("g_as_key", "naive_truncation", "logq_from_key"):
        return c.states == "live" and c.mode == "free"
    return live and c.mode == "free"     # the counters (a forced step's one child keeps G_b whatever its noise)


# ------------------------------------------------------------------------------ measurement
def step_deviation(c: StepCase, seed: int = 0) -> Dict[str, float]:
    d = step_inputs(c, seed)
    ref, emu = select_ref(d), select_emulate(d)
    out = dict(lq=_dev(emu["lq"], ref["lq"]),
               Gt=max(_dev(emu["gt"], ref["gt"], ref["scale"]), _dev(emu["zmax"], ref["zmax"])), logq=0.0)
    ok = np.repeat(ref["clear"] >= GUARD, c.W) if GUARD > 0 else np.repeat(np.array_equal(ref["sel"], emu["sel"]), c.N * c.W)
    ok = ok & (ref["sel"] == emu["sel"])
    out["logq"] = _dev(emu["logq"][ok], ref["logq"][ok])
    return out


def traj_deviation(c: TrajCase) -> Dict[str, float]:
    cfg, p = case_model(c)
    orc = case_oracle(c)
    emu = emulate(p, cfg, c.prefixes, c.W, **case_kwargs(c))
    logq = G = 0.0
    for n in range(len(c.prefixes)):
        if not np.array_equal(emu["rows"][n], orc["rows"][n]):
            assert GUARD == 0 or not orc["settled"][n], f"{c.name}: settled prefix {n} differs in the emulator"
            continue
        nb = int(orc["n_found"][n])
        if nb:
            logq = max(logq, _dev(emu["logq"][n, :nb], orc["logq"][n, :nb]))
            G = max(G, _dev(emu["gumbel"][n, :nb], orc["gumbel"][n, :nb]) / float(orc["scale"][n]))
    return dict(logq=logq, G=G, unsettled=float((~orc["settled"]).sum()), names=float(len(c.prefixes)))


def measure_deviations(seeds=(0, 1, 2), verbose: bool = False) -> Dict[str, float]:
    out = {k: 0.0 for k in MEASURED_DEV}
    for c in STEP_CASES:
        for seed in seeds:
            dev = step_deviation(c, seed)
            for k in dev:
                out[k] = max(out[k], dev[k])
    if verbose:
        print("steps", {k: f"{v:.3e}" for k, v in out.items()}, flush=True)
    for c in TRAJ_CASES:
        dev = traj_deviation(c)
        if verbose:
            print(c.name, {k: f"{v:.3e}" for k, v in dev.items()}, flush=True)
        out["logq"] = max(out["logq"], dev["logq"])
        out["Gt"] = max(out["Gt"], dev["G"])
    return out


def row_unit_counts(seeds=range(1, 9), sharps=(8.0, 64.0)) -> Dict[str, Dict[tuple, int]]:
    """Why the unit is the candidate's factor and not its row's exp(G_b - Z): per TRAJ_CASES entry the
    unsettled prefixes when the guard is scaled by the row figure, for each (fc.weight factor, noise seed).
    ``python -m gru_mpi_cuda_amd.models.sbs_ref --row-unit`` prints them beside the case's prefix count
    and the cap (one prefix in eight)."""
    out: Dict[str, Dict[tuple, int]] = {}
    for c in TRAJ_CASES:
        cfg, p = case_model(c)
        out[c.name] = {}
        for sharp in sharps:
            p2 = dict(p)
            p2["fc.weight"] = p["fc.weight"] * (sharp / 8.0)
            for noise in seeds:
                kw = dict(case_kwargs(c), seed=noise)
                o = oracle(p2, cfg, c.prefixes, c.W, unit="top_row_scale", **kw)
                out[c.name][(sharp, noise)] = int((~o["settled"]).sum())
    return out


if __name__ == "__main__":
    import sys
    if "--row-unit" in sys.argv[1:]:
        for name, res in row_unit_counts().items():
            n = len(next(c for c in TRAJ_CASES if c.name == name).prefixes)
            ok = [k for k, v in res.items() if v * 8 <= n]
            print(f"{name}: {n} prefixes, unsettled per (fc.weight x, seed) {res}; within the cap at {ok or 'none'}")
        sys.exit(0)
    res = measure_deviations(verbose=True)
    for k in MEASURED_DEV:
        print(f'    "{k}": {res[k]:.3e},')

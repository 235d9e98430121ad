"""Per-element reference of the sequential Monte Carlo sampler (csrc/kernels/smc.hip, Generator::conditional;
the rule: docs/DESIGN.md §4j, cpu_ref.sample_conditional / cpu_ref.smc_step).

* ``step_inputs``: one launch of smc_select_f32 on planted inputs -- logits on exact grids (the parts a kernel
  sums back are exact in fp32, as sbs_ref's), logw and logq on a 2^-7 grid, live and finished slots, step 0
  (the fan-out), forced / free / mixed steps, a per-position mask or an automaton state buffer, a line with
  one char, all weight on the last slot, both thresholds 0 and 1 on the same inputs, 1 / T in {1, 1.25},
  seeds and start indices above 2^32.
* ``select_ref`` / ``select_emulate``: cpu_ref.smc_step in float64 from the given fp32 inputs, and in float32
  with a ``mut`` hook: one function, the dtype switched.  In float32 every operation of the kernel is done in
  its order and rounded once (the row sums as the kernel's lane sums and neighbour tree; the running sums one
  addition at a time where the kernel scans); expf and logf are taken as correctly rounded, which the
  device's are not (an ulp or two), so the emulator bounds the kernel's deviation, it does not reproduce its
  bits.
* ``oracle`` / ``emulate``: the whole trajectory on a model, float64 / float32.  The oracle also returns the
  clearance of every (name, step).
* ``check_step`` / ``check_result``: what the tests assert; every entry of MUTATIONS must fail them, or the
  law test of tests/test_smc_ref.py.

A step takes three kinds of discrete decisions from rounded numbers: whether to resample (ESS against
thr W), every new slot's ancestor (t_i against the running sums of e) and every drawn char (r_i times the
total against the running sums of the row).  The *clearance* of a (name, step) is the smallest of
|ESS - thr W| / W, the gaps between any t_i and the running-sum boundaries over S, and the gaps between
r_i total and the two running sums around the chosen char over the total.  (Where every weight of a name is
bitwise equal -- one slot, the step after a resampling when it is forced or unconstrained -- e = 1 and
S = sum e e = the slot count exactly, so ESS is exact in either precision and its term is left out: at
thr = 1 it would otherwise be 0 by construction.)  A name whose smallest clearance
is below GUARD is *unsettled*: fp32 may decide the other way, so only its invariants are checked, not its
bytes.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from . import cpu_ref
from ..config import GRUConfig
from .params import init_params
from .cpu_ref import philox4x32, smc_uniform   # noqa: F401  (the numpy Philox lives beside the rule)

Out = Dict[str, object]
DEAD, LIVE, FIN = cpu_ref.BEAM_DEAD, cpu_ref.BEAM_LIVE, cpu_ref.BEAM_FIN

# Deviation of the float32 emulator from float64, the largest over STEP_CASES x seeds 0, 1, 2 and over
# TRAJ_CASES, rounded up to three digits:
#   decide : the three quantities a decision is taken from -- ESS / W, (running sum_b - t_i) / S,
#            (running sum - r_i total) / total around the chosen char
#   logm   : a slot's log allowed mass
#   logw   : a new slot's / a returned row's log importance weight
#   logq   : a new slot's / a returned row's log-probability under the sampler
# Measured, not chosen: ``python -m gru_mpi_cuda_amd.models.smc_ref`` reprints them.
MEASURED_DEV = {
    "decide": 6.46e-07,
    "logm": 2.99e-06,
    "logw": 2.99e-06,
    "logq": 3.27e-06,
}
GUARD = 8.0 * MEASURED_DEV["decide"]
ATOL = {k: 4.0 * v for k, v in MEASURED_DEV.items()}


# ------------------------------------------------------------------------------ one step
class StepCase(NamedTuple):
    V: int
    W: int
    N: int
    splits: int = 1
    bias: bool = False
    mode: str = "free"            # free | forced | mixed (odd names forced)
    states: str = "mix"           # mix (live and finished) | live | fin | step0 (the fan-out: all but slot 0 dead)
    mask: str = "none"            # none | pos (a line per name and step) | auto (a line per slot)
    eos: int = 5
    big: bool = False             # seed and start above 2^32
    thr: float = 0.5              # the ESS threshold: 0 never resamples, 1 does whenever the weights differ
    weights: str = "rand"         # rand | last (all weight on the last slot)
    single: bool = False          # masked: name 0's line / slot 1's state allows one char only
    optional: bool = True         # with the logm / lq / ess outputs


def _step_cases() -> List[StepCase]:
    out = []
    modes, states = ("free", "forced", "mixed"), ("mix", "live", "fin", "step0")
    i = 0
    for V in (64, 256, 512):
        for W in (1, 2, 4, 16, 17, 32):
            for N in (1, 3):
                mask = ("none", "pos", "auto")[(i // 2) % 3]
                if mask == "auto" and V == 64:
                    mask = "pos"
                out.append(StepCase(V, W, N, 1 + i % 2, i % 3 == 1, modes[i % 3], states[(i // 3) % 4], mask, (5, 0)[i % 2],
                                    i % 2 == 1, (0.5, 1.0, 0.0)[(i // 2) % 3], "rand", False, i % 4 != 3))
                i += 1
    for V, W, mask in ((64, 4, "none"), (256, 17, "auto"), (512, 32, "pos"), (256, 16, "pos")):
        for thr in (0.0, 1.0):      # the same inputs: one resamples, one does not
            out.append(StepCase(V, W, 3, mode="free", states="live", mask=mask, thr=thr))
            out.append(StepCase(V, W, 2, mode="free", states="mix", mask=mask, thr=thr, weights="last"))
        if mask != "none":
            out.append(StepCase(V, W, 2, mode="free", states="live", mask=mask, thr=1.0, single=True))
    # finished slots under a line of their own: their weight must not move
    out.append(StepCase(64, 4, 3, mode="free", states="mix", mask="pos", thr=0.0))
    out.append(StepCase(512, 16, 3, splits=2, mode="free", states="mix", mask="pos", thr=0.5, big=True))
    out.append(StepCase(256, 2, 3, mode="free", states="fin", mask="pos", thr=1.0))
    return out


STEP_CASES = _step_cases()
SOS = 1
LINES = 6     # lines of a planted constraint table / states of a planted automaton


def step_inputs(c: StepCase, seed: int = 0) -> Out:
    """Planted inputs of one smc_select_f32 launch (the docstring above).  Pad rows up to the 64-row granule
    hold NaN: the kernel never reads them."""
    V, W, N = c.V, c.W, c.N
    rng = np.random.default_rng(1000 * seed + 7 * V + 131 * W + N + 17 * c.splits)
    R = N * W
    Rp = (R + 63) // 64 * 64
    x = np.stack([(0.05 * rng.permutation(V)).astype(np.float32) for _ in range(R)])
    if c.splits > 1 or c.bias:
        x = (np.round(x.astype(np.float64) * 4096) / 4096).astype(np.float32)
    logq = (-rng.integers(0, 1025, R) / 128.0).astype(np.float32)
    logw = (-rng.integers(0, 513, R) / 128.0).astype(np.float32)
    step = 2
    if c.states == "live":
        state = np.full(R, LIVE, np.int32)
    elif c.states == "fin":
        state = np.full(R, FIN, np.int32)
    elif c.states == "step0":
        state = np.where(np.arange(R) % W == 0, LIVE, DEAD).astype(np.int32)
        step = 0
    else:
        state = rng.integers(1, 3, R).astype(np.int32)
        state[::W] = np.where(np.arange(N) % 3 == 2, FIN, LIVE)
    logq[state == DEAD] = -np.inf
    logw[state == DEAD] = -np.inf
    if c.weights == "last":
        logw.reshape(N, W)[:, :-1] = -np.inf
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
    ML = 6
    plen = np.zeros(N, np.int32)
    if c.mode == "forced":
        plen[:] = ML
    elif c.mode == "mixed":
        plen[1::2] = step + 1
    prefix = rng.integers(0, min(V, 256), (N, ML)).astype(np.uint8)
    prefix[prefix == c.eos] = 7
    inv_t = np.where(np.arange(N) % 2 == 0, 1.0, 1.25).astype(np.float32)
    d = dict(case=c, V=V, W=W, N=N, R=R, Rp=Rp, splits=c.splits, logits=buf, bias=bias, logw=logw, logq=logq, state=state,
             plen=plen, prefix=prefix, step=step, ML=ML, sos=SOS, eos=c.eos, inv_t=inv_t, thr=float(c.thr),
             seed=(0x9E3779B97F4A7C15 * (seed + 1)) % 2 ** 64 if c.big else 12345 + seed,
             start=2 ** 33 + 5 + seed if c.big else 3 + seed,
             tab=None, idx=None, astate=None, nxt=None, allowed=None)
    if c.mask != "none":     # line 0: everything; line 1: one char if asked for; the others: about half the chars
        bits = rng.random((LINES, V)) < 0.5
        bits[0] = True
        if c.single:
            bits[1] = False
            bits[1, int(rng.integers(0, V))] = True
        d["tab"] = np.ascontiguousarray(cpu_ref._pack_lines(bits, V))
        if c.mask == "pos":
            d["idx"] = rng.integers(0, LINES, (N, ML)).astype(np.int32)
            if c.single:
                d["idx"][0, step] = 1
            d["allowed"] = bits[d["idx"][:, step]]
        else:
            ast = rng.integers(0, LINES, R).astype(np.int32)
            if c.single:
                ast.reshape(N, W)[:, min(1, W - 1)] = 1
            ast[state != LIVE] = 0        # a carried or dead slot sits in the free state
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
    noise = smc_uniform(d["seed"], g, 0 if mut == "counter_without_step" else d["step"], W)
    s = cpu_ref.smc_step(x, d["logw"].astype(dt).reshape(N, W), d["logq"].astype(dt).reshape(N, W), d["state"].reshape(N, W),
                         forced, d["allowed"], d["inv_t"], noise, d["thr"], d["step"], d["eos"], d["sos"], mut)
    out: Out = {k: s[k].reshape(N * W) for k in ("parent", "chr", "state", "logw", "logq", "next_id", "logm")}
    out.update(lq=s["lq"].reshape(N * W, V), ess=s["ess"], resampled=s["resampled"], clear=s["clear"], q_ess=s["q_ess"],
               q_t=s["q_t"], q_r=s["q_r"])
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


def _dev(got, ref) -> float:
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ok = np.isfinite(ref) & np.isfinite(got)
    if not ok.any():
        return 0.0
    return float(np.abs(got[ok] - ref[ok]).max())


def _same_pattern(got, ref) -> bool:
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return bool(np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
                and np.array_equal(np.sign(got[np.isinf(got)]), np.sign(ref[np.isinf(ref)])))


def check_step(d: Out, ref: Out, got: Out) -> List[str]:
    """The failures of one launch's outputs (float32) against the float64 rule (empty: passed).  ``got``:
    parent, chr, state, next_id, logw, logq, resampled (the launch's increment of n_res) and optionally
    astate, logm, lq, ess."""
    N, W = d["N"], d["W"]
    bad = []
    settled = np.repeat(ref["clear"] >= GUARD, W)
    for k in ("parent", "chr", "state", "next_id", "astate"):
        if got.get(k) is None or k not in ref:
            continue
        g = np.asarray(got[k], np.int64)
        if not np.array_equal(g[settled], ref[k].astype(np.int64)[settled]):
            bad.append(f"{k}: differs at {np.flatnonzero((g != ref[k]) & settled)[:8].tolist()}")
    sn = ref["clear"] >= GUARD
    if not np.array_equal(np.asarray(got["resampled"], bool)[sn], np.asarray(ref["resampled"], bool)[sn]):
        bad.append("resampled: the count differs")
    for k in ("logw", "logq"):
        if not _same_pattern(np.asarray(got[k])[settled], ref[k][settled]):
            bad.append(f"{k}: the -inf pattern differs")
        else:
            dev = _dev(np.asarray(got[k])[settled], ref[k][settled])
            if not dev <= ATOL[k]:
                bad.append(f"{k}: deviation {dev:.3e} > {ATOL[k]:.3e}")
    # invariants, settled or not
    gw = np.asarray(got["logw"], np.float32).reshape(N, W)
    gs = np.asarray(got["state"]).reshape(N, W)
    par = np.asarray(got["parent"], np.int64).reshape(N, W)
    res = np.asarray(got["resampled"], bool)
    if d["step"] == 0 and res.any():
        bad.append("resampled: the fan-out counted")
    for n in range(N):
        alive = gs[n] != DEAD
        if (res[n] or d["step"] == 0) and alive.any() and len(set(gw[n][alive].tobytes()[i:i + 4] for i in range(0, 4 * int(alive.sum()), 4))) != 1:
            bad.append(f"name {n}: logw not equal across the slots after a resampling step")
        if not res[n] and d["step"] > 0 and not np.array_equal(par[n][alive], np.arange(W)[alive]):
            bad.append(f"name {n}: ancestors moved without resampling")
        if (np.diff(par[n][alive]) < 0).any():
            bad.append(f"name {n}: systematic resampling keeps the ancestors in order")
    flat_par = np.maximum(par.reshape(-1), 0) + np.repeat(np.arange(N) * W, W)
    if got.get("logm") is not None:
        if not _same_pattern(got["logm"], ref["logm"]):
            bad.append("logm: the NaN / inf pattern differs")
        elif not _dev(got["logm"], ref["logm"]) <= ATOL["logm"]:
            bad.append(f"logm: deviation {_dev(got['logm'], ref['logm']):.3e} > {ATOL['logm']:.3e}")
        lm = np.asarray(got["logm"], np.float32)
        zero = np.repeat(d["step"] < d["plen"], W) | (d["state"] == FIN)
        if d["allowed"] is None:
            zero = zero | (d["state"] == LIVE)
        if (lm[zero & (d["state"] != DEAD)] != 0).any():
            bad.append("logm: not exactly 0 on a forced step / for a finished slot / without a constraint")
        if (lm[d["state"] != DEAD] > 0).any():
            bad.append("logm: above 0")
        # bitwise: without resampling a slot's new weight is logw + logm
        keep = np.repeat(~res & (d["step"] > 0), W) & (np.asarray(got["parent"]) >= 0)
        u = (d["logw"].astype(np.float32) + lm).astype(np.float32)
        if not np.array_equal(gw.reshape(-1)[keep], u[keep]):
            bad.append("logw: not logw + logm bitwise without resampling")
    if got.get("lq") is not None:
        if not _same_pattern(got["lq"], ref["lq"]):
            bad.append("lq: the NaN / inf pattern differs")
        elif not _dev(got["lq"], ref["lq"]) <= ATOL["logq"]:
            bad.append(f"lq: deviation {_dev(got['lq'], ref['lq']):.3e} > {ATOL['logq']:.3e}")
        lq = np.asarray(got["lq"], np.float32)
        ch = np.asarray(got["chr"], np.int64)
        kid = ch >= 0
        forced = np.repeat(d["step"] < d["plen"], W)
        add = np.where(forced, np.float32(0), lq[flat_par, np.maximum(ch, 0)]).astype(np.float32)
        want = (d["logq"].astype(np.float32)[flat_par] + add).astype(np.float32)
        if not np.array_equal(np.asarray(got["logq"], np.float32)[kid], want[kid]):
            bad.append("logq: a child's value is not logq_a + lq_a[c] bitwise")
        if np.isnan(lq[flat_par, np.maximum(ch, 0)][kid & ~forced]).any():
            bad.append("chr: a char outside the allowed set")
    carried = (np.asarray(got["parent"]) >= 0) & (np.asarray(got["chr"]) < 0)
    if not np.array_equal(np.asarray(got["logq"], np.float32)[carried], d["logq"].astype(np.float32)[flat_par][carried]):
        bad.append("logq: a carried slot's value changed")
    if got.get("ess") is not None and d["step"] > 0:
        de = _dev(np.asarray(got["ess"], np.float64) / W, ref["q_ess"])
        if not de <= ATOL["decide"]:
            bad.append(f"ess: deviation {de:.3e} > {ATOL['decide']:.3e} (in units of W)")
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
    noise: int = 1                # the sampler's seed
    start: int = 0
    temperature: Optional[float] = None
    constraints: Optional[dict] = None
    preset: Optional[str] = None
    thr: float = 0.5


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


DIGITS = dict(charset="0123456789")     # the H x L x prefixes x W grid runs under it: without a rule nothing is weighted


def _traj_cases() -> List[TrajCase]:
    out = []

    def add(name, V, E, H, L, ML, eos, W, prefixes, **kw):
        out.append(TrajCase(name, V, E, H, L, ML, eos, W, prefixes, **kw))

    i = 0
    for H, L in ((64, 1), (128, 2)):
        for npre in (1, 3, 9):
            for W in (1, 4, 17, 32):
                ML = (5, 3, 4)[i % 3]
                pre = tuple("".join("0123456789"[(ord(ch) + k) % 10] for k, ch in enumerate(p)) for p in _mixture(64, ML, 5, npre))
                add(f"h{H}-L{L}-n{npre}-W{W}", 64, 64, H, L, ML, 5, W, pre, start=(0, 2 ** 33 + 7)[i % 2],
                    constraints=DIGITS, thr=(0.5, 1.0, 0.0)[i % 3])
                i += 1
    add("plain", 64, 64, 64, 1, 4, 5, 4, _mixture(64, 4, 5, 3))
    add("pattern", 64, 64, 64, 1, 4, 0, 4, ("12", "", "7"), constraints=dict(charset="0123456789", min_len=2))
    add("temperature", 64, 64, 128, 2, 4, 5, 4, ("", "3", "12"), temperature=0.7, constraints=DIGITS, thr=1.0)
    add("regex3", 256, 64, 64, 1, 4, 0, 4, ("", "a"), constraints=dict(regex="a(b|c|d)"))
    add("ref", 0, 0, 0, 0, 0, 0, 4, ("Ma", ""), preset="ref", temperature=0.7, constraints=dict(regex=".*son"))
    return out


TRAJ_CASES = _traj_cases()
_models: Dict[tuple, tuple] = {}


def case_model(c: TrajCase):
    """(cfg, fp32 params) of a case: init_params with fc.weight x 8 (a sharper model, as sbs_ref's), or the
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
    """The keywords of ``sample_conditional`` for a case (beside prefix and width)."""
    return dict(seed=c.noise, start=c.start, temperature=c.temperature, constraints=c.constraints, ess_threshold=c.thr)


def _run(params, cfg: GRUConfig, prefixes, W: int, f64: bool, seed=0, start=0, temperature=None, constraints=None,
         ess_threshold=0.5, mut: Optional[str] = None) -> Out:
    pre, plen, inv, seed, start, thr, N, R = cpu_ref.conditional_inputs(cfg, list(prefixes), W, None, 1, seed, start,
                                                                        temperature, ess_threshold)
    cons = cpu_ref.conditional_constraints(cfg, N, 1, constraints)
    cpu_ref.check_prefix_allowed(cons, pre, plen)
    p = {k: v.to(torch.float64 if f64 else torch.float32) for k, v in params.items()}
    trace: list = []
    rows, logw, logq, ntok, nres = cpu_ref.sample_conditional_rule(p, cfg, pre, plen, W, seed, start, inv, thr, cons, mut, trace)
    return dict(rows=rows, log_weight=logw, logq=logq, n_tok=ntok, n_resampled=nres,
                clear=np.stack([s["clear"] for s in trace], 1), resampled=np.stack([s["resampled"] for s in trace], 1),
                trace=trace)


def oracle(params, cfg: GRUConfig, prefixes, W: int, **kw) -> Out:
    """The float64 trajectory: rows, log_weight, logq, n_tok, n_resampled, ``clear`` [N][ML], ``resampled``
    [N][ML] and ``settled`` [N] (every step's clearance at least GUARD)."""
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


def score64_of(params, cfg: GRUConfig, prefixes, got, temperature=None, constraints=None):
    """float64 cpu_ref.score name_logp of a result's rows, [N][P] each: under the constrained sampler (the same
    keywords) and under the model at the temperature given the prefix (no constraints)."""
    rows = got["rows"] if isinstance(got, dict) else got.rows
    N, P = rows.shape[:2]
    p64 = {k: v.double() for k, v in params.items()}
    T = 1.0 if temperature is None else temperature
    lq, lp = np.zeros((N, P)), np.zeros((N, P))
    for n in range(N):      # per prefix: its rows share the prefix and the constraint
        cons = None if constraints is None else cpu_ref.as_constraints(cfg, P, dict(constraints))
        lq[n] = cpu_ref.score(p64, cfg, rows[n], temperature=T, prefix=[prefixes[n]] * P, constraints=cons)[1]
        lp[n] = cpu_ref.score(p64, cfg, rows[n], temperature=T, prefix=[prefixes[n]] * P)[1]
    return lq, lp


def check_result(cfg: GRUConfig, prefixes, orc: Out, got, score64=None, thr: Optional[float] = None) -> List[str]:
    """The failures of a one-run result (a ConditionalResult or a dict) against the oracle: bytes and counts of
    the settled prefixes, their log_weight and logq within ATOL, and for every prefix the invariants (rows start
    with the prefix, NUL after the name, no dead slot, log_weight <= 0, log_weight equal across a name whose
    last step resampled -- read from the oracle where settled -- and, with ``score64`` = ``score64_of``'s pair,
    finite constrained scores (the rule holds), logq equal to the constrained score and at ``thr`` 0 log_weight
    equal to model score - constrained score, within ATOL)."""
    g = got if isinstance(got, dict) else dict(rows=got.rows, log_weight=got.log_weight, logq=got.logq, n_tok=got.n_tok,
                                               n_resampled=got.n_resampled.reshape(-1))
    pre, plen = cpu_ref.encode_prefixes(list(prefixes), cfg)
    N, W = g["logq"].shape
    ML = cfg.max_len
    bad = []
    for n in range(N):
        rows, lw, lq, nt = g["rows"][n], np.asarray(g["log_weight"][n], np.float64), np.asarray(g["logq"][n], np.float64), g["n_tok"][n]
        if orc["settled"][n]:
            if not (np.array_equal(rows, orc["rows"][n]) and np.array_equal(nt, orc["n_tok"][n])):
                bad.append(f"prefix {n}: rows / n_tok differ from the oracle's")
            else:
                dw, dq = float(np.abs(lw - orc["log_weight"][n]).max()), float(np.abs(lq - orc["logq"][n]).max())
                if not dw <= ATOL["logw"]:
                    bad.append(f"prefix {n}: log_weight deviates {dw:.3e}")
                if not dq <= ATOL["logq"]:
                    bad.append(f"prefix {n}: logq deviates {dq:.3e}")
            if int(g["n_resampled"][n]) != int(orc["n_resampled"][n]):
                bad.append(f"prefix {n}: n_resampled {int(g['n_resampled'][n])}, the oracle's {int(orc['n_resampled'][n])}")
            if orc["resampled"][n, -1] and len({np.float32(v).tobytes() for v in g["log_weight"][n]}) != 1:
                bad.append(f"prefix {n}: log_weight not equal across the name right after a resampling step")
        if (lw > 0).any() or np.isnan(lw).any() or not np.isfinite(lq).all():
            bad.append(f"prefix {n}: log_weight above 0 / NaN, or logq not finite")
        if not 0 <= int(g["n_resampled"][n]) <= ML - 1:
            bad.append(f"prefix {n}: n_resampled {int(g['n_resampled'][n])}")
        if thr is not None and thr == 0 and int(g["n_resampled"][n]) != 0:
            bad.append(f"prefix {n}: resampled at threshold 0")
        for k in range(W):
            t = int(nt[k])
            if not (plen[n] <= t <= ML and t >= 1 and (rows[k, :plen[n]] == pre[n, :plen[n]]).all() and (rows[k, t:] == 0).all()):
                bad.append(f"prefix {n} particle {k}: prefix / padding")
            elif (rows[k, :max(t - 1, 0)] == cfg.eos).any() or (t < ML and rows[k, t - 1] != cfg.eos):
                bad.append(f"prefix {n} particle {k}: EOS placement")
        if score64 is not None:
            sq, sp = score64[0][n], score64[1][n]
            if not np.isfinite(sq).all():
                bad.append(f"prefix {n}: a row outside the rule")
                continue
            ds = float(np.abs(lq - sq).max())
            if not ds <= ATOL["logq"]:
                bad.append(f"prefix {n}: logq is not the rows' log-probability under the sampler ({ds:.3e})")
            if thr is not None and thr == 0:
                dw = float(np.abs(lw - (sp - sq)).max())
                if not dw <= ATOL["logw"]:
                    bad.append(f"prefix {n}: log_weight is not log p - log q of the row ({dw:.3e})")
    return bad


# planted defects -> where the checks must catch them: "step" (every applicable STEP_CASES entry through
# check_step) or "law" (tests/test_smc_ref.py's law test)
MUTATIONS = {
    "weights_not_equalised": "step",     # the ancestors' own weights kept after a resample
    "resample_on_logw": "law",           # ESS and ancestors from logw instead of u, logm still credited through the mean
    "forced_adds_logm": "step",          # logm added on a forced step
    "finished_reweighted": "step",       # a finished slot re-weighted
    "u_per_slot": "step",                # the resampling uniform drawn per slot instead of per step
    "counter_local_index": "step",       # the Philox counter with the batch-local instead of the global name index
    "counter_without_step": "step",      # ... without the step
    "fanout_counted": "step",            # the fan-out counted as a resample
}


def mutation_applies(mut: str, c: StepCase) -> bool:
    """Whether a step case exercises the branch a mutation breaks."""
    free_live = c.mode == "free" and c.states in ("live", "mix")
    resamples = free_live and c.thr == 1.0 and c.W >= 4 and c.weights == "rand"
    if mut == "weights_not_equalised":
        return resamples
    if mut == "resample_on_logw":
        return resamples and c.mask != "none" and c.states == "live" and not c.single
    if mut == "u_per_slot":
        return resamples and c.W >= 16
    if mut == "forced_adds_logm":
        return c.mode == "forced" and c.states in ("live", "mix", "step0") and c.mask != "none"
    if mut == "finished_reweighted":
        return c.states in ("fin", "mix") and c.mask == "pos" and c.mode == "free" and c.weights == "rand" and c.W >= 2
    if mut == "fanout_counted":
        return c.states == "step0"
    if mut == "counter_without_step":
        return c.mode == "free" and c.states == "live" and c.W >= 4     # (a step-0 case has the step 0 anyway)
    return c.mode == "free" and c.states in ("live", "step0") and c.W >= 4     # the counters: free draws


# ------------------------------------------------------------------------------ the law
LAW_CHARSET = "01"
LAW = dict(charset=LAW_CHARSET, min_len=1)


def law_case():
    """(cfg, fp32 params, rows) of the law tests (tests/test_smc_ref.py on the CPU in float64, tests/test_smc_gpu.py
    on the device): the V = 64, H = 64, ML = 4 model with embedding x 2, fc.weight x 6 and fc.bias + 2.5 on
    LAW_CHARSET and EOS, and the language of the non-empty names over LAW_CHARSET -- 30 rows, enumerable with
    ``score``.  The bias puts a few per cent of the model on the language (Z = 0.033, 0.081 at temperature
    0.7) and leaves a live particle about a third of the mass per step where a finished one keeps all of it,
    so that at W = 4 and threshold 0.5 about 35 % of the systems resample at step 2, in mid-trajectory, and
    about 5 % at the last step; the others carry unequal weights to the end."""
    import itertools
    cfg = GRUConfig(vocab=64, embed=64, hidden=64, layers=1, max_len=4, sos=0, eos=5, seed=4)
    p = init_params(cfg)
    p["embedding"] = p["embedding"] * 2.0
    p["fc.weight"] = p["fc.weight"] * 6.0
    p["fc.bias"] = p["fc.bias"].clone()
    p["fc.bias"][[ord(ch) for ch in LAW_CHARSET] + [cfg.eos]] += 2.5
    rows = []
    for ln in range(1, cfg.max_len + 1):
        for tup in itertools.product([ord(ch) for ch in LAW_CHARSET], repeat=ln):
            r = np.zeros(cfg.max_len + 1, np.uint8)
            r[:ln] = tup
            if ln < cfg.max_len:
                r[ln] = cfg.eos
            rows.append(r)
    return cfg, p, np.stack(rows)


def law_exact(cfg: GRUConfig, params, rows: np.ndarray, temperature=None) -> np.ndarray:
    """float64 p_T(row) of every row of the language under the model (no constraint); their sum is Z."""
    p64 = {k: v.double() for k, v in params.items()}
    return np.exp(cpu_ref.score(p64, cfg, rows, temperature=1.0 if temperature is None else temperature)[1])


# ------------------------------------------------------------------------------ measurement
def step_deviation(c: StepCase, seed: int = 0) -> Dict[str, float]:
    d = step_inputs(c, seed)
    ref, emu = select_ref(d), select_emulate(d)
    out = dict(logm=_dev(emu["logm"], ref["logm"]), decide=0.0, logw=0.0, logq=0.0)
    out["decide"] = _dev(emu["q_ess"], ref["q_ess"]) if d["step"] > 0 else 0.0
    both = np.asarray(ref["resampled"], bool) & np.asarray(emu["resampled"], bool)
    if both.any():
        out["decide"] = max(out["decide"], _dev(emu["q_t"][both], ref["q_t"][both]))
    same = (ref["parent"] == emu["parent"]) & (ref["chr"] == emu["chr"])
    same &= np.repeat(np.asarray(ref["resampled"], bool) == np.asarray(emu["resampled"], bool), c.W)
    sm = same.reshape(c.N, c.W)
    out["decide"] = max(out["decide"], _dev(emu["q_r"][sm], ref["q_r"][sm]))
    out["logw"] = _dev(emu["logw"][same], ref["logw"][same])
    out["logq"] = max(_dev(emu["logq"][same], ref["logq"][same]), _dev(emu["lq"], ref["lq"]))
    return out


def traj_deviation(c: TrajCase) -> Dict[str, float]:
    cfg, p = case_model(c)
    orc = case_oracle(c)
    emu = emulate(p, cfg, c.prefixes, c.W, **case_kwargs(c))
    out = dict(decide=0.0, logm=0.0, logw=0.0, logq=0.0)
    for n in range(len(c.prefixes)):
        if not np.array_equal(emu["rows"][n], orc["rows"][n]) or not np.array_equal(emu["resampled"][n], orc["resampled"][n]):
            assert GUARD == 0 or not orc["settled"][n], f"{c.name}: settled prefix {n} differs in the emulator"
            continue
        out["logw"] = max(out["logw"], _dev(emu["log_weight"][n], orc["log_weight"][n]))
        out["logq"] = max(out["logq"], _dev(emu["logq"][n], orc["logq"][n]))
        for se, so in zip(emu["trace"], orc["trace"]):
            if not (np.array_equal(se["parent"][n], so["parent"][n]) and np.array_equal(se["chr"][n], so["chr"][n])):
                break
            out["logm"] = max(out["logm"], _dev(se["logm"][n], so["logm"][n]))
            out["decide"] = max(out["decide"], _dev(se["q_ess"][n], so["q_ess"][n]), _dev(se["q_t"][n], so["q_t"][n]),
                                _dev(se["q_r"][n], so["q_r"][n]))
    out["unsettled"] = float((~orc["settled"]).sum())
    out["names"] = float(len(c.prefixes))
    return out


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
        for k in out:
            out[k] = max(out[k], dev[k])
    return out


if __name__ == "__main__":
    res = measure_deviations(verbose=True)
    for k in MEASURED_DEV:
        print(f'    "{k}": {res[k]:.3e},')

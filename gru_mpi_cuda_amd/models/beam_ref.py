"""Per-element reference of the beam search (csrc/kernels/beam.hip, Generator::beam; the rule:
docs/DESIGN.md §4d, cpu_ref.beam_search).

* ``step_inputs`` / ``plant_step``: one launch of beam_select_f32 on planted inputs -- logits on exact
  grids (the parts a kernel sums back are exact in fp32, as tests/test_sampling_ctl_gpu.py:
  make_logits), scores on a 2^-7 grid, every beam state, forced / free / mixed steps, exact ties.
* ``select_ref`` / ``select_emulate``: the float64 one-step selection from the given fp32 inputs, and
  the same in float32 with the kernel's order of operations (slabs summed in order, late bias, the
  max-subtracted log-sum-exp, lp = (x - max) - log(sum), candidate = s + lp) and a ``mut`` hook.
* ``oracle`` / ``emulate``: the whole trajectory on a model, float64 / float32.  The oracle also
  returns the clearance of every (name, step): the smallest gap between neighbours among the first
  W + 1 candidates in the total order, exact ties (bitwise-equal candidates: duplicated rows, equal
  logits) not counted.  A name whose smallest clearance is below GUARD is *unsettled*: fp32 may order
  two candidates the other way, so only its invariants are checked, not its bytes.
* ``check_step`` / ``check_result``: what the tests assert; every entry of MUTATIONS must fail them.

The selection is a total order (score descending, then the flat index j = b V + c ascending), so fp32
and fp64 can only differ where two candidate scores are closer than the guard.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from . import cpu_ref
from ..config import GRUConfig
from .params import init_params

Out = Dict[str, object]
DEAD, LIVE, FIN = cpu_ref.BEAM_DEAD, cpu_ref.BEAM_LIVE, cpu_ref.BEAM_FIN

# Deviation of the float32 emulator from float64, the largest over STEP_CASES x seeds 0, 1, 2 (lp, and
# cand of one step) and over TRAJ_CASES (cand along a trajectory, logp of the result), rounded up to
# three digits:
#   lp   : an entry of a row's log-softmax (entries down to -26 on the planted grids)
#   cand : the score s_b + lp[c] of one of the first W + 1 candidates of a (name, step)
#   logp : a returned row's log-probability
# Measured, not chosen: ``python -m gru_mpi_cuda_amd.models.beam_ref`` reprints them.
MEASURED_DEV = {
    "lp": 1.99e-06,
    "cand": 2.21e-05,
    "logp": 2.21e-05,
}
GUARD = 8.0 * MEASURED_DEV["cand"]
ATOL = {"lp": 4.0 * MEASURED_DEV["lp"], "cand": 4.0 * MEASURED_DEV["cand"], "logp": 4.0 * MEASURED_DEV["logp"]}


# ------------------------------------------------------------------------------ one step
class StepCase(NamedTuple):
    V: int
    W: int
    N: int
    splits: int = 1
    bias: bool = False
    mode: str = "free"            # free | forced | mixed (odd names forced)
    states: str = "mix"           # mix | live | fin | step0 (all but beam 0 dead)
    eos: int = 5


def _step_cases() -> List[StepCase]:
    out = []
    modes, states = ("free", "forced", "mixed"), ("mix", "live", "fin", "step0")
    i = 0
    for V in (64, 256, 512):
        for W in (1, 2, 3, 8, 32):
            for N in (1, 3, 9):
                out.append(StepCase(V, W, N, 1 + i % 2, i % 3 == 1, modes[i % 3], states[(i // 3) % 4], (5, 0)[i % 2]))
                i += 1
    return out


STEP_CASES = _step_cases()
SOS = 1


def step_inputs(c: StepCase, seed: int = 0) -> Out:
    """Planted inputs of one beam_select_f32 launch.  Logits rows: permutations of the multiples of 0.05
    (on the 2^-12 grid when more than one part is summed), equal logits planted inside even rows; in
    names with W >= 3 beam 2 is a bitwise copy of beam 0 (row, score and state).  Scores: multiples of
    2^-7 in [-8, 0].  Pad rows up to the 64-row granule hold NaN: the kernel never reads them."""
    V, W, N = c.V, c.W, c.N
    rng = np.random.default_rng(1000 * seed + 7 * V + 131 * W + N + 17 * c.splits)
    R = N * W
    Rp = (R + 63) // 64 * 64
    x = np.stack([(0.05 * rng.permutation(V)).astype(np.float32) for _ in range(R)])
    if c.splits > 1 or c.bias:
        x = (np.round(x.astype(np.float64) * 4096) / 4096).astype(np.float32)
    for i in range(0, R, 2):
        order = np.argsort(-x[i], kind="stable")
        for r in (0, 1, V - 2):
            x[i, order[r + 1]] = x[i, order[r]]
    score = (-rng.integers(0, 1025, R) / 128.0).astype(np.float32)
    if c.states == "live":
        state = np.full(R, LIVE, np.int32)
    elif c.states == "fin":
        state = np.full(R, FIN, np.int32)
    elif c.states == "step0":
        state = np.where(np.arange(R) % W == 0, LIVE, DEAD).astype(np.int32)
    else:
        state = rng.integers(0, 3, R).astype(np.int32)
        state[::W] = np.where(np.arange(N) % 3 == 2, FIN, LIVE)      # beam 0: never dead
    score[state == DEAD] = -np.inf
    if W >= 3:
        for n in range(N):
            x[n * W + 2], score[n * W + 2], state[n * W + 2] = x[n * W], score[n * W], state[n * W]
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
    prefix = rng.integers(0, V, (N, ML)).astype(np.uint8) if V <= 256 else rng.integers(0, 256, (N, ML)).astype(np.uint8)
    prefix[prefix == c.eos] = 7
    return dict(case=c, V=V, W=W, N=N, R=R, Rp=Rp, splits=c.splits, logits=buf, bias=bias, score=score, state=state,
                plen=plen, prefix=prefix, step=step, ML=ML, sos=SOS, eos=c.eos, moved=[])


def _x_of(d: Out, dt, mut: Optional[str] = None) -> np.ndarray:
    R = d["R"]
    x = d["logits"][0, :R].astype(dt)
    for s in range(1, d["splits"]):
        x = x + d["logits"][s, :R].astype(dt)
    if d["bias"] is not None and mut != "late_bias_skipped":
        x = x + d["bias"].astype(dt)
    return x


def log_softmax(x: np.ndarray, f64: bool) -> np.ndarray:
    """Rows' log-softmax: float64, or float32 by the kernel's operations -- exp of the max-subtracted
    values rounded to fp32, their sum (exact, then rounded: the kernel's fixed-order sum is within an ulp
    of it), lp = (x - max) - log(sum), each step rounded."""
    mx = x.max(-1, keepdims=True)
    if f64:
        return (x - mx) - np.log(np.exp(x - mx).sum(-1, keepdims=True))
    e = np.exp((x - mx).astype(np.float64)).astype(np.float32)
    se = e.astype(np.float64).sum(-1, keepdims=True).astype(np.float32)
    return ((x - mx) - np.log(se.astype(np.float64)).astype(np.float32)).astype(np.float32)


def select(lp: np.ndarray, score: np.ndarray, state: np.ndarray, forced: int, eos: int, sos: int,
           mut: Optional[str] = None, allowed: Optional[np.ndarray] = None) -> Out:
    """Steps 3-5 of the rule for one name in the dtype of ``lp``: the W new beams (parent, chr, state,
    score, next_id, sel = the flat index j) and ``gaps``: the neighbour gaps of the first W + 1
    candidates in order.  ``allowed``: bool [V], the name's constraint set at this step (docs/DESIGN.md
    §4e; None: everything), or bool [W, V], a set per beam (an automaton's states, §4g): a live beam offers
    only chars in it, a carry is not masked."""
    W, V = lp.shape
    dt = lp.dtype
    oks = np.ones(V, bool) if allowed is None else np.asarray(allowed, bool)
    cand = np.full((W, V), -np.inf, dt)
    off = np.zeros((W, V), bool)
    for b in range(W):
        ok = oks[b] if oks.ndim == 2 else oks
        st = state[b]
        if st == DEAD and mut == "dead_offered":
            st = LIVE
        if st == FIN and mut == "finished_extended":
            st = LIVE
        if st == LIVE:
            if forced >= 0 and mut != "forced_unrestricted":
                if ok[forced]:
                    add = dt.type(0) if mut == "forced_lp_not_added" else lp[b, forced]
                    cand[b, forced] = score[b] + add
                    off[b, forced] = True
            else:
                cand[b] = np.where(ok, score[b] + lp[b], dt.type(-np.inf))
                off[b] = ok
        elif st == FIN and mut != "carry_dropped":
            cand[b, 0] = score[b]
            off[b, 0] = True
    js = np.flatnonzero(off.reshape(-1))
    sc = cand.reshape(-1)[js]
    tie = -js if mut == "ties_descending_j" else js
    order = js[np.lexsort((tie, -sc))]
    top = order[:W + 1]
    ts = cand.reshape(-1)[top]
    with np.errstate(invalid="ignore"):      # (-inf) - (-inf) of a planted defect's candidates
        gaps = ts[:-1] - ts[1:] if len(top) > 1 else np.zeros(0, dt)
    win = order[:W]
    if mut == "unsorted":
        win = np.sort(win)
    parent, chrs, nst = np.full(W, -1, np.int32), np.full(W, -1, np.int32), np.full(W, DEAD, np.int32)
    nsc, nxt, sel = np.full(W, -np.inf, dt), np.full(W, sos, np.int32), np.full(W, -1, np.int32)
    for k, j in enumerate(win):
        b, c = divmod(int(j), V)
        parent[k], nsc[k], sel[k] = b, cand[b, c], j
        carried = state[b] == FIN and mut != "finished_extended"
        if carried:
            nst[k] = FIN
        else:
            chrs[k] = c
            nst[k] = FIN if c == eos else LIVE
            if c != eos:
                nxt[k] = c
    return dict(parent=parent, chr=chrs, state=nst, score=nsc, next_id=nxt, sel=sel, gaps=gaps)


def _clear(gaps: np.ndarray) -> float:
    g = gaps[gaps != 0]
    g = g[np.isfinite(g)]
    return float(g.min()) if len(g) else float("inf")


def _select_all(d: Out, f64: bool, mut: Optional[str] = None) -> Out:
    V, W, N = d["V"], d["W"], d["N"]
    dt = np.float64 if f64 else np.float32
    lp = log_softmax(_x_of(d, dt, mut), f64).reshape(N, W, V)
    res: Out = {k: [] for k in ("parent", "chr", "state", "score", "next_id", "sel")}
    clear = np.zeros(N)
    for n in range(N):
        forced = -1
        if d["step"] < d["plen"][n]:
            forced = int(d["prefix"][n, d["step"]])
            if forced >= V:
                forced = 0
        s = select(lp[n], d["score"][n * W:(n + 1) * W].astype(dt), d["state"][n * W:(n + 1) * W], forced, d["eos"], d["sos"], mut,
                   None if d.get("allowed") is None else d["allowed"][n])      # "allowed": bool [N][V] or [N][W][V], optional
        for k in res:
            res[k].append(s[k])
        clear[n] = _clear(s["gaps"])
    out: Out = {k: np.concatenate(v) for k, v in res.items()}
    out.update(lp=lp.reshape(N * W, V), clear=clear)
    return out


def select_ref(d: Out) -> Out:
    return _select_all(d, True)


def select_emulate(d: Out, mut: Optional[str] = None) -> Out:
    assert mut is None or mut in MUTATIONS, mut
    return _select_all(d, False, mut)


def plant_step(d: Out) -> Out:
    """The inputs with every non-tie gap among a name's first W + 1 candidates at least GUARD: a name that
    misses it gets the incoming score of its last live beam nudged along the 2^-7 grid until it clears.
    At most one name in eight (one of a launch of fewer than eight) may need that."""
    d = dict(d, score=d["score"].copy(), moved=[])
    W = d["W"]
    for _ in range(16):
        ref = select_ref(d)
        bad = [n for n in range(d["N"]) if ref["clear"][n] < GUARD]
        if not bad:
            break
        for n in bad:
            live = [b for b in range(W) if d["state"][n * W + b] != DEAD and not (W >= 3 and b in (0, 2))]
            assert live, "no beam to nudge"
            d["score"][n * W + live[-1]] -= np.float32(3.0 / 128.0)
            if n not in d["moved"]:
                d["moved"].append(n)
    ref = select_ref(d)
    assert (ref["clear"] >= GUARD).all(), "the planter could not clear the guard"
    assert len(d["moved"]) <= max(d["N"] // 8, 1), f"{len(d['moved'])} of {d['N']} names had to be moved"
    return d


def check_step(ref: Out, got: Out) -> List[str]:
    """The failures of one launch's outputs against the float64 rule (empty: passed)."""
    bad = []
    for k in ("parent", "chr", "state", "next_id", "sel"):
        if k in got and got[k] is not None and not np.array_equal(np.asarray(got[k], np.int64), ref[k].astype(np.int64)):
            bad.append(f"{k}: differs at {np.flatnonzero(np.asarray(got[k], np.int64) != ref[k])[:8].tolist()}")
    gs, rs = np.asarray(got["score"], np.float64), ref["score"]
    if not np.array_equal(np.isneginf(gs), np.isneginf(rs)) or np.isnan(gs).any():
        bad.append("score: the dead slots differ")
    else:
        fin = np.isfinite(rs)
        dev = float(np.abs(gs[fin] - rs[fin]).max()) if fin.any() else 0.0
        if dev > ATOL["cand"]:
            bad.append(f"score: deviation {dev:.3e} > {ATOL['cand']:.3e}")
    if got.get("lp") is not None:
        dev = float(np.abs(np.asarray(got["lp"], np.float64) - ref["lp"]).max())
        if not dev <= ATOL["lp"]:
            bad.append(f"lp: deviation {dev:.3e} > {ATOL['lp']:.3e}")
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
    seed: int = 4
    sharp: float = 8.0


def _alpha(V: int) -> str:
    return "".join(chr(c) for c in range(33, min(V, 127)))


def _mixture(V: int, ML: int, eos: int, n: int) -> tuple:
    """n prefixes: empty, short, of length ML and lengths in between, chars inside the vocabulary, no EOS."""
    ok = [c for c in _alpha(V) if ord(c) != eos]
    out = []
    for i in range(n):
        ln = (0, 1, ML, 2, 0, ML // 2, 1, 3)[i % 8]
        ln = min(ln, ML)
        out.append("".join(ok[(5 * i + 3 * j + i // 8) % len(ok)] for j in range(ln)))
    return tuple(out)


def _long(V: int, ML: int, eos: int, n: int) -> tuple:
    """n prefixes that leave 0 .. 2 free steps."""
    ok = [c for c in _alpha(V) if ord(c) != eos]
    return tuple("".join(ok[(7 * i + 3 * j) % len(ok)] for j in range(ML - i % 3)) for i in range(n))


# W = 32 asks for 33 candidates per step with every neighbour gap above the guard.  A sharper model
# (fc.weight x 64) spreads them; the seeds below are the first from 4 at which at most one prefix in
# eight stays unsettled (tests/test_beam_ref.py asserts that figure, it is a condition of the GPU test).
# At V = 256, ML = 10, W = 32 no seed settles ten free steps, so that case runs long prefixes.
_SEEDS: Dict[str, int] = {"s-L1-ML6-e0-W32": 6, "s-L2-ML6-e0-W32": 5, "s-L2-ML6-e5-W32": 5, "m-batches": 12}


def _traj_cases() -> List[TrajCase]:
    out = []

    def add(name, V, E, H, L, ML, eos, W, prefixes):
        out.append(TrajCase(name, V, E, H, L, ML, eos, W, prefixes, _SEEDS.get(name, 4), 64.0 if W == 32 else 8.0))

    for L in (1, 2):
        for ML in (1, 3, 6):
            for eos in (0, 5):
                for W in (1, 3, 8, 32):
                    add(f"s-L{L}-ML{ML}-e{eos}-W{W}", 64, 64, 64, L, ML, eos, W, _mixture(64, ML, eos, 8))
    for W in (1, 3, 8):
        add(f"m-W{W}", 256, 128, 256, 2, 10, 0, W, _mixture(256, 10, 0, 8))
    add("m-W32", 256, 128, 256, 2, 10, 0, 32, _long(256, 10, 0, 8))
    add("m-granule", 256, 128, 256, 2, 10, 0, 8, _mixture(256, 10, 0, 9))
    add("m-batches", 256, 128, 256, 2, 10, 0, 8, _mixture(256, 10, 0, 20))
    return out


TRAJ_CASES = _traj_cases()
_models: Dict[tuple, tuple] = {}


def case_model(c: TrajCase):
    """(cfg, fp32 params) of a case: init_params with fc.weight scaled by ``sharp`` (as the sharp models of
    tests/test_sampling_ctl_gpu.py: most choices far from a boundary).  Shared, never modified."""
    key = (c.V, c.E, c.H, c.L, c.ML, c.eos, c.seed, c.sharp)
    if key not in _models:
        cfg = GRUConfig(vocab=c.V, embed=c.E, hidden=c.H, layers=c.L, max_len=c.ML, sos=0, eos=c.eos, seed=c.seed)
        p = init_params(cfg)
        p["fc.weight"] = p["fc.weight"] * c.sharp
        _models[key] = (cfg, p)
    return _models[key]


def _run(params, cfg: GRUConfig, pre: np.ndarray, plen: np.ndarray, W: int, f64: bool, mut: Optional[str] = None,
         cons: Optional[cpu_ref.Constraints] = None) -> Out:
    N, ML, V, H = pre.shape[0], cfg.max_len, cfg.vocab, cfg.hidden
    dt = torch.float64 if f64 else torch.float32
    npdt = np.float64 if f64 else np.float32
    p = {k: v.to(dt) for k, v in params.items()}
    rows = np.zeros((N, W, ML + 1), np.uint8)
    score = np.full((N, W), -np.inf, npdt)
    state = np.full((N, W), DEAD, np.int32)
    ntok = np.zeros((N, W), np.int32)
    score[:, 0], state[:, 0] = 0, LIVE
    hs = [torch.zeros(N * W, H, dtype=dt) for _ in range(cfg.layers)]
    cur = torch.full((N * W,), cfg.sos, dtype=torch.int64)
    clear = np.full((N, ML), np.inf)
    tops = []
    aut = cons if isinstance(cons, cpu_ref.Automaton) else None
    if aut is not None:   # §4g: a state per beam, beam 0 in the name's start state
        alines, astate = aut.lines(), np.zeros((N, W), np.int64)
        astate[:, 0] = aut.start
    for l in range(ML):
        pre_h = hs
        inp = p["embedding"][cur]
        new = []
        for k in range(cfg.layers):
            gi = inp @ p[f"weight_ih_l{k}"].T + p[f"bias_ih_l{k}"]
            gh = hs[k] @ p[f"weight_hh_l{k}"].T + p[f"bias_hh_l{k}"]
            hk, _ = cpu_ref._gates(gi, gh, hs[k])
            new.append(hk)
            inp = hk
        logits = (inp @ p["fc.weight"].T + p["fc.bias"]).numpy()
        lp = log_softmax(logits, f64).reshape(N, W, V)
        gather = np.arange(N * W)
        nrows, nscore = np.zeros_like(rows), np.full_like(score, -np.inf)
        nstate, nntok = np.zeros_like(state), np.zeros_like(ntok)
        nxt = np.full(N * W, cfg.sos, np.int64)
        step_top = []
        ok_l = None if cons is None else (alines[astate] if aut is not None else cons.allowed(l))
        nastate = None if aut is None else np.zeros_like(astate)
        for n in range(N):
            s = select(lp[n], score[n], state[n], int(pre[n, l]) if l < plen[n] else -1, cfg.eos, cfg.sos, mut,
                       None if cons is None else ok_l[n])
            clear[n, l] = _clear(s["gaps"])
            step_top.append((s["sel"].copy(), s["score"].copy()))
            for k in range(W):
                b = int(s["parent"][k])
                if b < 0:
                    continue
                gather[n * W + k] = n * W + b
                src = (b + 1) % W if mut == "row_wrong_parent" else b
                nrows[n, k], nntok[n, k] = rows[n, src], ntok[n, src]
                nscore[n, k], nstate[n, k] = s["score"][k], s["state"][k]
                c = int(s["chr"][k])
                if c >= 0:
                    nrows[n, k, l] = c
                    nntok[n, k] = l + 1
                    if aut is not None:   # (a carried or dead beam keeps state 0)
                        nastate[n, k] = aut.nxt[astate[n, b], c]
                nxt[n * W + k] = s["next_id"][k]
        g = torch.from_numpy(gather)
        hs = [h[g] for h in (pre_h if mut == "pre_step_h" else new)]
        rows, score, state, ntok = nrows, nscore, nstate, nntok
        if aut is not None:
            astate = nastate
        cur = torch.from_numpy(nxt)
        tops.append(step_top)
    return dict(rows=rows, logp=score, n_tok=ntok, n_beams=(state != DEAD).sum(1).astype(np.int32), clear=clear, tops=tops)


def oracle(params, cfg: GRUConfig, prefixes, W: int, constraints=None) -> Out:
    """The float64 trajectory: rows, logp, n_tok, n_beams, ``clear`` [N][ML] and ``settled`` [N] (every
    step's clearance at least GUARD).  ``constraints``: as cpu_ref.beam_search's."""
    pre, plen = cpu_ref.beam_inputs(cfg, list(prefixes), W)
    cons = cpu_ref.as_constraints(cfg, pre.shape[0], constraints)
    cpu_ref.check_prefix_allowed(cons, pre, plen)
    out = _run(params, cfg, pre, plen, W, True, cons=cons)
    out["settled"] = out["clear"].min(1) >= GUARD
    return out


def emulate(params, cfg: GRUConfig, prefixes, W: int, mut: Optional[str] = None) -> Out:
    assert mut is None or mut in MUTATIONS, mut
    pre, plen = cpu_ref.beam_inputs(cfg, list(prefixes), W)
    return _run(params, cfg, pre, plen, W, False, mut)


_oracles: Dict[str, Out] = {}


def case_oracle(c: TrajCase) -> Out:
    """A case's float64 trajectory, computed once and shared (never modified)."""
    if c.name not in _oracles:
        cfg, p = case_model(c)
        _oracles[c.name] = oracle(p, cfg, c.prefixes, c.W)
    return _oracles[c.name]


def check_result(cfg: GRUConfig, prefixes, orc: Out, got, score64: Optional[np.ndarray] = None) -> List[str]:
    """The failures of a result (rows, logp, n_tok, n_beams: a BeamResult or a dict) against the oracle:
    bytes and counts of the settled prefixes, logp within ATOL, and for every prefix the invariants
    (distinct rows, logp non-increasing, rows start with the prefix, NUL after the name, dead slots as
    specified).  ``score64``: float64 cpu_ref.score(name_logp) of the returned rows, [N][W]."""
    g = got if isinstance(got, dict) else dict(rows=got.rows, logp=got.logp, n_tok=got.n_tok, n_beams=got.n_beams)
    pre, plen = cpu_ref.encode_prefixes(list(prefixes), cfg)
    N, W = g["logp"].shape
    ML = cfg.max_len
    bad = []
    for n in range(N):
        nb = int(g["n_beams"][n])
        rows, lp, nt = g["rows"][n], np.asarray(g["logp"][n], np.float64), g["n_tok"][n]
        if orc["settled"][n]:
            if not (np.array_equal(rows, orc["rows"][n]) and np.array_equal(nt, orc["n_tok"][n]) and nb == orc["n_beams"][n]):
                bad.append(f"prefix {n}: rows / n_tok / n_beams differ from the oracle's")
            elif nb and float(np.abs(lp[:nb] - orc["logp"][n, :nb]).max()) > ATOL["logp"]:
                bad.append(f"prefix {n}: logp deviates {float(np.abs(lp[:nb] - orc['logp'][n, :nb]).max()):.3e}")
        if not (1 <= nb <= W):
            bad.append(f"prefix {n}: n_beams {nb}")
            continue
        if not (np.isneginf(lp[nb:]).all() and (rows[nb:] == 0).all() and (nt[nb:] == 0).all() and np.isfinite(lp[:nb]).all()):
            bad.append(f"prefix {n}: dead slots not as specified")
        if (np.diff(lp[:nb]) > 0).any():
            bad.append(f"prefix {n}: logp increases")
        if len({bytes(r) for r in rows[:nb]}) != nb:
            bad.append(f"prefix {n}: rows not distinct")
        for k in range(nb):
            t = int(nt[k])
            if not (plen[n] <= t <= ML and (rows[k, :plen[n]] == pre[n, :plen[n]]).all() and (rows[k, t:] == 0).all()):
                bad.append(f"prefix {n} beam {k}: prefix / padding")
            if (rows[k, :max(t - 1, 0)] == cfg.eos).any() or (t < ML and rows[k, t - 1] != cfg.eos):
                bad.append(f"prefix {n} beam {k}: EOS placement")
        if score64 is not None and nb and float(np.abs(lp[:nb] - score64[n, :nb]).max()) > ATOL["logp"]:
            bad.append(f"prefix {n}: logp is not the rows' log-probability ({float(np.abs(lp[:nb] - score64[n, :nb]).max()):.3e})")
    return bad


def score64_of(params, cfg: GRUConfig, got) -> np.ndarray:
    """float64 cpu_ref.score (name_logp) of a result's rows, [N][W]."""
    rows = got["rows"] if isinstance(got, dict) else got.rows
    N, W = rows.shape[:2]
    p64 = {k: v.double() for k, v in params.items()}
    return cpu_ref.score(p64, cfg, rows.reshape(N * W, -1))[1].reshape(N, W)


# planted defects -> where the checks must catch them: a STEP_CASES index or a TRAJ_CASES name
MUTATIONS = {
    "ties_descending_j": ("step", None),
    "carry_dropped": ("step", None),
    "finished_extended": ("step", None),
    "forced_unrestricted": ("step", None),
    "forced_lp_not_added": ("step", None),
    "late_bias_skipped": ("step", None),
    "unsorted": ("step", None),
    "dead_offered": ("step", None),
    "pre_step_h": ("traj", "s-L2-ML6-e5-W8"),
    "row_wrong_parent": ("traj", "s-L2-ML6-e5-W8"),
}


def mutation_applies(mut: str, c: StepCase) -> bool:
    """Whether a step case exercises the branch a mutation breaks."""
    if mut == "late_bias_skipped":
        return c.bias
    if mut in ("forced_unrestricted", "forced_lp_not_added"):
        return c.mode != "free" and c.states != "fin" and not (c.mode == "mixed" and c.N == 1)
    if mut in ("carry_dropped", "finished_extended"):
        return c.states in ("fin", "mix") and c.W >= 2
    if mut == "dead_offered":
        return c.states == "step0" and c.mode == "forced" and c.W >= 2
    if mut == "ties_descending_j":
        return c.W >= 3 and c.states in ("live", "fin")
    if mut == "unsorted":
        return c.W >= 8 and c.mode == "free" and c.states in ("live", "mix")
    return False


# ------------------------------------------------------------------------------ measurement
def step_deviation(c: StepCase, seed: int = 0) -> Dict[str, float]:
    d = step_inputs(c, seed)
    ref, emu = select_ref(d), select_emulate(d)
    fin = np.isfinite(ref["score"])
    same = all(np.array_equal(ref[k], emu[k]) for k in ("parent", "chr", "state", "next_id", "sel"))
    cand = float(np.abs(emu["score"][fin].astype(np.float64) - ref["score"][fin]).max()) if (fin.any() and same) else 0.0
    return dict(lp=float(np.abs(emu["lp"].astype(np.float64) - ref["lp"]).max()), cand=cand)


def traj_deviation(c: TrajCase) -> Dict[str, float]:
    cfg, p = case_model(c)
    orc = case_oracle(c)
    emu = emulate(p, cfg, c.prefixes, c.W)
    cand = logp = 0.0
    for n in range(len(c.prefixes)):
        if not orc["settled"][n]:
            continue
        assert np.array_equal(emu["rows"][n], orc["rows"][n]), f"{c.name}: settled prefix {n} differs in the emulator"
        for l in range(cfg.max_len):
            (js, s64), (je, s32) = orc["tops"][l][n], emu["tops"][l][n]
            assert np.array_equal(js, je), f"{c.name}: settled prefix {n} step {l} selects differently in the emulator"
            ok = np.isfinite(s64)
            if ok.any():
                cand = max(cand, float(np.abs(s32[ok].astype(np.float64) - s64[ok]).max()))
        nb = int(orc["n_beams"][n])
        logp = max(logp, float(np.abs(emu["logp"][n, :nb].astype(np.float64) - orc["logp"][n, :nb]).max()))
    return dict(cand=cand, logp=logp, unsettled=float((~orc["settled"]).sum()), names=float(len(c.prefixes)))


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
        for k in ("cand", "logp"):
            out[k] = max(out[k], dev[k])
    return out


if __name__ == "__main__":
    res = measure_deviations(verbose=True)
    for k in MEASURED_DEV:
        print(f'    "{k}": {res[k]:.3e},')

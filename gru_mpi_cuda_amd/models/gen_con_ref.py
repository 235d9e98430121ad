"""Per-element reference of the persistent generator's CONSTRAINED launch (gen_persist_con.hip; the
rule: docs/DESIGN.md §4e / §4g, sample_ctl_f32's MASK / AUTO instantiations), on top of ``gen_ctl_ref``:
its inputs, its controls and its result keys, so ``gen_ref.check_launch`` / ``synth_got`` / ``ws_decode``
serve unchanged.

* ``tables``: a case's constraint -- a per-position table with its idx rows, or an automaton with its
  start states -- built so that the things that can go wrong are in use (the last line / state, sets
  of exactly one char, sets smaller than top_k, no set that reaches the last chars of the vocabulary,
  prefix bytes outside their sets).
* ``plant``: gen_ctl_ref.plant on the MASKED trajectory: an entry outside the set is -inf after the
  temperature scale, so GUARD_Y, GUARD_MASS and gen_ref.GUARD from every CDF edge are computed inside
  the set, with the same cap on moved names (one in eight).
* ``oracle`` / ``emulate``: the float64 trajectory on given uniforms and the same in float32 with a
  ``mut`` hook that plants one of MUTATIONS.  The rule is applied on every step of every name, dead
  ones included: the sampled id feeds the next char and moves the state whether the name has ended or
  not.

A line (an idx entry, a state) outside [0, rows) is taken as line 0, and the walk continues from
state 0; ``oob`` marks those (step, name) pairs (the launch flags them in its error words).
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from . import gen_ctl_ref as cr
from . import gen_ref as gr

Out = Dict[str, object]
ATOL = cr.ATOL
BEYOND = cr.BEYOND
AUTO_STATES = 3000      # the automaton of the cases: its last state is in use
MASK_LINES = 37         # lines of the per-position table: the last one is in use
TAIL = 8                # no set of a built table holds one of the last TAIL chars: the fallback is never V - 1


class ConCase(NamedTuple):
    name: str
    mode: str                     # "mask" | "auto"
    ctl: cr.CtlCase
    kind: str = "rich"            # "rich"; "ends": every set holds the EOS byte; "free": line 0 / one state, everything allowed


def _ctl(name, H, L, V, N, ML=4, i=0, mix="mix", off=0, probs=True):
    return cr.CtlCase(name, H, L, V, N, ML, *cr._se(i), mix, off, probs)


def _both(name, *a, kind="rich", **k) -> List[ConCase]:
    return [ConCase(f"{m}-{name}", m, _ctl(name, *a, **k), kind) for m in ("mask", "auto")]


CASES_N = [c for i, N in enumerate((1, 8, 9, 16, 17, 33)) for c in _both(f"n-N{N}", 256, 1, 256, N, i=i, off=i)]
CASES_T = [c for i, N in enumerate((1, 17)) for c in _both(f"t-H1024-N{N}", 1024, 2, 256, N, i=i + 1, off=2 * i + 4)]
CASES_V = [c for i, N in enumerate((5, 20)) for c in _both(f"v512-N{N}", 256, 2, 512, N, i=i, off=i + 1)]
CASES_A = [c for i, (H, L) in enumerate(gr.VARIANTS) for c in _both(f"a-H{H}-L{L}", H, L, 256, 3, i=i, off=3 * i)]
CASES_A512 = [c for i, (H, L) in enumerate(cr.V512) for c in _both(f"a512-H{H}-L{L}", H, L, 512, 3, i=i + 1, off=3 * i + 1)]
CASES_G = [c for N in (4, 20) for c in (
    _both(f"g-N{N}-ends-early-exit", 256, 2, 256, N, 5, 0, "ends", probs=False, kind="ends") +
    _both(f"g-N{N}-ends-probs", 256, 2, 256, N, 5, 0, "ends", kind="ends"))]
CASES_F = [c for N in (12, 33) for c in _both(f"f-free-N{N}", 256, 1, 256, N, i=1, off=N, kind="free")]
CON_CASES: List[ConCase] = CASES_N + CASES_T + CASES_V + CASES_A + CASES_A512 + CASES_G + CASES_F


# ------------------------------------------------------------------------------ tables
def pack(bits: np.ndarray) -> np.ndarray:
    """bool [rows][V] -> the table layout of §4e: uint32 [rows][V / 32], bit c % 32 of word c / 32."""
    rows, V = bits.shape
    w = bits.reshape(rows, V // 32, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)
    return np.ascontiguousarray(w.sum(-1).astype(np.uint32))


def unpack(tab: np.ndarray, V: int) -> np.ndarray:
    return ((np.asarray(tab, np.uint32)[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(tab.shape[0], V)


def _random_sets(rng, rows: int, V: int, eos: int, with_eos: bool) -> np.ndarray:
    """Sets of 3, 40, ~V / 2 and V - TAIL chars in turn, none of the last TAIL chars in any."""
    bits = np.zeros((rows, V), dtype=bool)
    for r in range(rows):
        size = (3, 40, V // 2, V - TAIL)[r % 4]
        bits[r, rng.choice(V - TAIL, size, replace=False)] = True
        if with_eos:
            bits[r, eos] = True
    return bits


def tables(c: ConCase) -> Out:
    """The case's constraint: mode, bits bool [rows][V], tab (packed), rows, and idx int32 [N][ML]
    (mask) or nxt uint16 [rows][V] + start int32 [N] (auto); ``single``: the lines / states whose set
    is exactly one char.

    rich, mask: step 1 of every name points at a one-char line, the other steps at random lines, name
    0's last step at the last line.  rich, auto: three layers -- the start states (random sets) lead to
    one-char states on every char, those to random states, those anywhere, the last state among the
    targets; nxt[q][eos] = 0 for every q.  ends: random sets that all hold the EOS byte.  free: one
    line / state with every char, nxt = 0."""
    k = c.ctl
    V, N, ML, eos = k.V, k.N, k.ML, k.eos
    rng = np.random.default_rng(977 + 31 * N + V + 7 * k.off + (c.mode == "auto"))
    if c.kind == "free":
        bits = np.ones((1, V), dtype=bool)
        out = dict(mode=c.mode, bits=bits, tab=pack(bits), rows=1, single=np.zeros(0, np.int64))
        if c.mode == "mask":
            out["idx"] = np.zeros((N, ML), np.int32)
        else:
            out.update(nxt=np.zeros((1, V), np.uint16), start=np.zeros(N, np.int32))
        return out
    rows = MASK_LINES if c.mode == "mask" else AUTO_STATES
    bits = _random_sets(rng, rows, V, eos, c.kind == "ends")
    single = np.zeros(0, np.int64)
    if c.kind == "rich":
        single = np.arange(5, 13) if c.mode == "mask" else np.arange(1000, 1064)
        bits[single] = False
        bits[single, rng.integers(1, V - TAIL, len(single))] = True
    out = dict(mode=c.mode, bits=bits, tab=pack(bits), rows=rows, single=single)
    if c.mode == "mask":
        idx = rng.integers(0, rows, (N, ML)).astype(np.int32)
        if c.kind == "rich":
            idx[:, 1] = single[rng.integers(0, len(single), N)]
        idx[0, ML - 1] = rows - 1
        out["idx"] = idx
    else:
        if c.kind == "rich":
            nxt = rng.integers(2000, rows, (rows, V))                      # from anywhere: the third layer, the last state included
            nxt[:1000] = single[rng.integers(0, len(single), (1000, V))]   # start states -> one-char states
            nxt[1000:2000] = rng.integers(2000, rows, (1000, V))
            nxt[1000:2000, ::7] = rows - 1
            start = rng.integers(1, 1000, N).astype(np.int32)
        else:
            nxt = rng.integers(0, rows, (rows, V))
            start = rng.integers(0, rows, N).astype(np.int32)
            start[0] = rows - 1
        nxt[:, eos] = 0
        out.update(nxt=np.ascontiguousarray(nxt.astype(np.uint16)), start=start)
    return out


# ------------------------------------------------------------------------------ the trajectory
def _strided(allowed: np.ndarray, V: int) -> np.ndarray:
    """The planted defect "a lane holds strided chars": char c = lane PER + e read at the bit of char e 64 + lane."""
    c = np.arange(V)
    per = V // 64
    return allowed[:, (c % per) * 64 + c // per]


def _run(d: Out, ctl: Out, con: Out, rf: Optional[np.ndarray], f64: bool, mut: Optional[str] = None,
         plan: Optional[Out] = None) -> Out:
    """gen_ctl_ref._run with the constrained sampling step: the same result keys, plus ``line`` (the table
    line of each (step, name) after the out-of-range rule), ``oob``, ``allowed`` and, for an automaton,
    ``state_after`` [ML][N]."""
    H, L, V, N, ML, sos, eos = (d[k] for k in ("H", "L", "V", "N", "ML", "sos", "eos"))
    dt = torch.float64 if f64 else torch.float32
    w64 = d["w64"]
    cast = (lambda w: w) if f64 else (lambda w: w.float())
    inv, k, tp, plen, pre = (ctl[x] for x in ("inv_temp", "top_k", "top_p", "plen", "prefix"))
    auto = con["mode"] == "auto"
    bits, rows = con["bits"], con["rows"]
    state = con["start"].astype(np.int64).copy() if auto else None
    planting = rf is None
    rf = np.zeros((N, ML), np.float32) if planting else np.asarray(rf, np.float32)
    h = [torch.zeros(N, H, dtype=dt) for _ in range(L)]
    ids = torch.full((N,), sos, dtype=torch.int64)
    alive = np.ones(N, dtype=bool)
    out = np.zeros((N, ML + 1), np.uint8)
    states = torch.zeros(L, ML, N, H, dtype=dt)
    logits, probs, cdfs, ys, cms = (torch.zeros(ML, N, V, dtype=dt) for _ in range(5))
    keeps = torch.ones(ML, N, V, dtype=torch.bool)
    ids_in, sampled = np.zeros((ML, N), np.int64), np.zeros((ML, N), np.int64)
    alive_after, smp = np.zeros((ML, N), dtype=bool), np.zeros((ML, N), dtype=bool)
    lines, oobs = np.zeros((ML, N), np.int64), np.zeros((ML, N), dtype=bool)
    alloweds = np.zeros((ML, N, V), dtype=bool)
    state_after = np.zeros((ML, N), np.int64)
    P = cast(w64["P"])
    greedy = inv == 0
    for t in range(ML):
        ids_in[t] = ids.numpy()
        x = None
        for l in range(L):
            gh = gr._prod(h[l], w64["Whh"][l], cast(w64["bhh"][l]), f64)
            gi = P[ids] if l == 0 else gr._prod(x, w64["Wih"][l], cast(w64["bih"][l]), f64)
            h[l] = x = gr._gate_math(gi, gh, h[l], f64)
            states[l, t] = x
        lg = gr._prod(x, w64["Wfc"], cast(w64["bfc"]), f64)
        logits[t] = lg
        # ---- the names' lines and sets at this step
        if auto:
            line = np.full(N, state[0]) if mut == "state_of_name_0" else state.copy()
        else:
            line = con["idx"][:, min(t + 1, ML - 1) if mut == "line_of_next_step" else t].astype(np.int64)
        oob = (line < 0) | (line >= rows)
        line = np.where(oob, 0, line)
        if auto:
            state = np.where((state < 0) | (state >= rows), 0, state)
        allowed = bits[line].copy()
        if mut == "bit_index_strided":
            allowed = _strided(allowed, V)
        if mut == "mask_ignored_when_greedy":
            allowed[greedy] = True
        forced = t < plen
        if mut == "mask_on_forced_step":      # a forced char outside its set is not taken: the step samples
            forced = forced & allowed[np.arange(N), pre[:, t]]
        lines[t], oobs[t], alloweds[t] = line, oob, allowed
        al = torch.from_numpy(allowed)
        lgm = torch.where(al, lg, torch.full_like(lg, -np.inf))
        y, cm, p, keep = cr._stats(lgm, inv, k, tp, f64, None)
        keep = keep & al
        top = cr._lowest_argmax(y)
        onehot = forced | greedy
        fid = torch.from_numpy(np.where(forced, pre[:, t], 0).astype(np.int64))
        hot = torch.where(torch.from_numpy(forced), fid, top)
        one = torch.nn.functional.one_hot(hot, V).to(dt)
        oh = torch.from_numpy(onehot).unsqueeze(-1)
        p = torch.where(oh, one, p)
        keep = torch.where(oh, one > 0, keep)
        cs = torch.cumsum(p, 1) if f64 else gr._cumsum_seq(p)
        ys[t], cms[t], keeps[t], cdfs[t], probs[t] = y, cm, keep, cs, p
        csn, pn = cs.numpy(), p.numpy()
        feed = np.zeros(N, np.int64)
        for n in range(N):
            smp[t, n] = not onehot[n]
            if onehot[n]:
                sel = int(hot[n])
                if planting:
                    rf[n, t] = d["rf0"][n, t]                     # ignored by the step
            else:
                if planting:
                    if (n, t) in ctl["beyond"]:
                        rf[n, t] = BEYOND
                    else:
                        force = avoid = None
                        if plan is not None:
                            if plan["eos_at"].get(n) == t:
                                force = eos
                            elif plan.get("no_other_eos"):
                                avoid = eos
                        rf[n, t] = gr._plant(csn[n].astype(np.float64), pn[n].astype(np.float64), d["rf0"][n, t], force, avoid)
                hit = (csn[n] > float(rf[n, t])) & keep[n].numpy()      # only a kept char is a hit
                last = V - 1 if mut == "fallback_last_index" else int(np.flatnonzero(keep[n].numpy())[-1])
                sel = int(hit.argmax()) if hit.any() else last
            if mut == "oob_nothing_allowed" and oob[n] and not forced[n]:
                sel = V - 1                                       # what a row of -inf gives
            feed[n] = sel
            sampled[t, n] = sel
            if alive[n]:
                out[n, t] = sel & 0xFF
                if sel == eos:
                    alive[n] = False
            alive_after[t, n] = alive[n]
        if auto:      # after every pick, a forced one included, alive or not
            step_char = ids_in[t] if mut == "state_by_previous_char" else feed
            new = con["nxt"][state, step_char % V].astype(np.int64)
            if mut == "state_kept_on_forced_step":
                new = np.where(t < plen, state, new)
            state = new
            state_after[t] = state
        ids = torch.from_numpy(feed.copy())
    return dict(rf=rf, ids_in=ids_in, sampled=sampled, alive_after=alive_after, out=out, states=states, logits=logits,
                probs_last=probs[ML - 1], probs=probs, cdf=cdfs, y=ys, cm=cms, keep=keeps, sampled_step=smp,
                id_words=(sampled | (alive_after.astype(np.int64) << 16)).astype(np.uint32),
                line=lines, oob=oobs, allowed=alloweds, state_after=state_after)


def walk(con: Out, sampled: np.ndarray, T: int) -> np.ndarray:
    """The automaton states after the first T chars of ``sampled`` [ML][N]: what allow_state holds after a
    launch that ran T chars."""
    rows = con["rows"]
    state = con["start"].astype(np.int64).copy()
    for t in range(T):
        state = np.where((state < 0) | (state >= rows), 0, state)
        state = con["nxt"][state, sampled[t]].astype(np.int64)
    return state.astype(np.int32)


# ------------------------------------------------------------------------------ the planter
def plant(d: Out, ctl: Out, con: Out, plan: Optional[Out] = None):
    """gen_ctl_ref.plant on the masked trajectory: the same guards (gen_ctl_ref.clearance works on the
    masked y and masses), the same moves, the same cap on moved names."""
    ctl = dict(ctl, top_k=ctl["top_k"].copy(), top_p=ctl["top_p"].copy())
    moved = set()
    V = d["V"]
    for _ in range(8):
        run = _run(d, ctl, con, None, True, plan=plan)
        bad = cr.clearance(ctl, run)
        if not bad:
            break
        for b in bad:
            n, t = b["n"], b["t"]
            moved.add(n)
            if b["what"] == "top_k":
                assert ctl["inv_temp"][n] != 0, "a greedy maximum with a thin gap below it cannot be moved"
                ctl["top_k"][n] += 1 if ctl["top_k"][n] + 1 < V else -1
            else:      # the middle of the widest gap between the cumulative masses next to top_p
                cm = np.concatenate([[0.0], run["cm"][t, n].numpy()])
                j = int(np.searchsorted(cm, float(ctl["top_p"][n])))
                lo, hi = max(j - 3, 0), min(j + 3, len(cm) - 1)
                w = int(np.argmax(np.diff(cm[lo:hi + 1]))) + lo
                ctl["top_p"][n] = np.float32(0.5 * (cm[w] + cm[w + 1]))
    assert not cr.clearance(ctl, run), "the planter could not clear the guards"
    assert len(moved) <= max(d["N"] // 8, 1), f"{len(moved)} of {d['N']} names had to be moved: the case no longer tests its values"
    ctl["moved"] = sorted(moved)
    return ctl, run


def oracle(d: Out, ctl: Out, con: Out, rf: np.ndarray) -> Out:
    return _run(d, ctl, con, rf, True)


def emulate(d: Out, ctl: Out, con: Out, rf: np.ndarray, mut: Optional[str] = None) -> Out:
    assert mut is None or mut in MUTATIONS, mut
    return _run(d, ctl, con, rf, False, mut=mut)


def case_setup(c: ConCase, seed: int = 0):
    """(inputs, controls as planted, constraint, float64 trajectory) of a case."""
    d = cr.case_inputs(c.ctl, seed)
    con = tables(c)
    ctl, orc = plant(d, cr.controls(c.ctl), con, cr.case_plan(c.ctl))
    return d, ctl, con, orc


def with_oob(c: ConCase, con: Out, ctl: Out):
    """The case's constraint with one out-of-range line: (constraint, name, value).  The name is one
    whose step 0 is sampled, and the value is far outside the table."""
    n = int(np.flatnonzero((ctl["plen"] == 0) & (ctl["inv_temp"] != 0))[0])
    bad = dict(con)
    value = con["rows"] + 1234567
    if con["mode"] == "mask":
        bad["idx"] = con["idx"].copy()
        bad["idx"][n, 0] = value
    else:
        bad["start"] = con["start"].copy()
        bad["start"][n] = value
    return bad, n, value


# planted defects of the emulator -> the case whose checks must catch it ("+oob": on with_oob's tables)
MUTATIONS = {
    "mask_ignored_when_greedy": "mask-n-N16",
    "mask_on_forced_step": "mask-n-N17",
    "state_kept_on_forced_step": "auto-n-N17",
    "state_by_previous_char": "auto-n-N9",
    "line_of_next_step": "mask-n-N9",
    "bit_index_strided": "mask-n-N8",
    "state_of_name_0": "auto-n-N33",
    "fallback_last_index": "mask-n-N17",
    "oob_nothing_allowed": "mask-n-N9+oob",
}

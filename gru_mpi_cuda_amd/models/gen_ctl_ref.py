"""Per-element reference of the persistent generator's CONTROLLED launch (gen_persist_ctl.hip; the
rule: docs/DESIGN.md §4b, cpu_ref.sample_controlled), on top of ``gen_ref``: the same inputs, the same
result keys, so ``gen_ref.check_launch`` / ``synth_got`` / ``ws_decode`` serve unchanged.

* ``controls``: the per-name control mixture of a case (MIX: every value the tests name, arranged so
  that a launch of nine or more names takes and skips every branch of the sampler).
* ``plant``: the float64 controlled trajectory.  It builds the uniforms while it runs, as
  ``gen_ref.plant_uniforms`` does but against the FILTERED CDF (forced and greedy steps ignore theirs),
  and it makes sure that the kept set is the same in fp32 as in fp64: at every sampled step of a name
  the gap at the top-k edge (and below a greedy maximum) is at least GUARD_Y and top_p is at least
  GUARD_MASS from every cumulative mass of the sorted post-top-k softmax.  Names are independent, so a
  name that misses a guard gets its top_k stepped by one or its top_p moved to the middle of a gap
  and the trajectory is run again; at most one name in eight may need that (asserted; one name of a
  launch of fewer than eight).
* ``oracle`` / ``emulate``: the float64 trajectory on given uniforms, and the same in float32 with a
  ``mut`` hook that plants one of MUTATIONS.

An exact float64 tie of two scaled logits counts as a tie, not as a thin gap: it only arises from the
duplicated FC row of a ``tie`` case, where the fp32 logits are bitwise equal as well.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from . import cpu_ref
from . import gen_ref as gr

Out = Dict[str, object]

# End-to-end deviation of the float32 emulator from the float64 trajectory, the largest over every case
# of CTL_CASES x seeds 0, 1, 2, rounded up to three digits:
#   y    : a scaled logit x * inv_temp of a sampled step
#   mass : a cumulative mass of the sorted post-top-k softmax of a sampled step
#   probs: the last char's renormalised filtered distribution (entries up to 1, where gen_ref's plain
#          softmax rows hold ~1 / V: its own tolerance, by gen_ref's rule of 4 x the measured figure)
# Measured, not chosen: ``python -m gru_mpi_cuda_amd.models.gen_ctl_ref`` reprints them.
MEASURED_DEV = {
    "y": 4.10e-07,
    "mass": 9.86e-08,
    "probs": 9.86e-08,
}
# 8 x the measured deviation (the rule of gen_ref.GUARD); the mass guard never below the 1e-4 of
# tests/test_sampling_ctl_gpu.py: clear_top_p
GUARD_Y = 8.0 * MEASURED_DEV["y"]
GUARD_MASS = max(1e-4, 8.0 * MEASURED_DEV["mass"])
ATOL = dict(gr.ATOL, probs=4.0 * MEASURED_DEV["probs"])      # for gen_ref.check_launch(atol=...)
BEYOND = np.float32(1.5)      # a uniform beyond every CDF: the fallback to the highest kept index


# ------------------------------------------------------------------------------ cases
class CtlCase(NamedTuple):
    name: str
    H: int
    L: int
    V: int
    N: int
    ML: int
    sos: int = 0
    eos: int = 0
    mix: str = "mix"              # "mix": MIX from name `off`; "neutral"; "ends": see controls()
    off: int = 0
    probs: bool = True
    seed_off: int = 0
    tie: bool = False             # FC rows 5 and 9 are one row with a raised bias: an exact tie at the maximum


def _se(i: int):
    return (7, 3) if i % 2 == 0 else (0, 0)


CASES_A = [CtlCase(f"ca-H{H}-L{L}", H, L, 256, 3, 4, *_se(i), off=3 * i) for i, (H, L) in enumerate(gr.VARIANTS)]
CASES_B = [CtlCase(f"cb-N{N}", 512, 2, 256, N, 4, *_se(i), off=i) for i, N in enumerate((1, 8, 9, 16, 17, 33))]
CASES_C = [CtlCase(f"cc-N{N}", 1024, 2, 256, N, 4, *_se(i + 1), off=2 * i + 4) for i, N in enumerate((1, 8, 9, 17))]
# V = 512: every (H, L) whose plain variant is below the 256-VGPR cap (the support function decides on the device)
V512 = [hl for hl in gr.VARIANTS if hl not in ((512, 4), (1024, 2))]
CASES_E = [CtlCase(f"ce-H{H}-L{L}-N{N}", H, L, 512, N, 4, *_se(i), off=i + j)
           for i, (H, L) in enumerate(V512) for j, N in enumerate((5, 33))]
CASES_G = [c for N in (4, 20) for c in (
    CtlCase(f"cg-N{N}-full-prefix", 256, 2, 256, N, 4, 7, 3, "mix", 3),
    CtlCase(f"cg-N{N}-ends-early-exit", 256, 2, 256, N, 5, 7, 3, "ends", probs=False),
    CtlCase(f"cg-N{N}-ends-probs", 256, 2, 256, N, 5, 7, 3, "ends"))]
CASES_T = [CtlCase("ct-tie-N12", 512, 2, 256, 12, 4, 7, 3, "tie", tie=True),
           CtlCase("ct-tie-N20", 256, 1, 256, 20, 4, 0, 0, "tie", tie=True)]
CASES_N = [CtlCase(f"cn-neutral-N{N}", 1024, 2, 256, N, 4, *_se(i), "neutral") for i, N in enumerate((1, 12, 33))]
CTL_CASES: List[CtlCase] = CASES_A + CASES_B + CASES_C + CASES_E + CASES_G + CASES_T + CASES_N

# (plen: 0, 1 or -1 for ML; T, 0: greedy; top_k, -1: V - 1, -2: V + 7; top_p).  Top-p below 1 goes with a
# top-k of 65 or 2 (or with 1e-6, which keeps the maximum alone): the masses next to top_p are then
# ~1e-2 apart and the 1e-4 guard rarely asks for a move; over all V values they are ~1e-3 apart.
MIX = [(0, 1.0, 0, 1.0), (1, 0.5, 2, 0.9), (0, 0.0, 0, 1.0), (-1, 2.0, 65, 0.5), (0, 2.0, 65, 0.9), (1, 1.0, -1, 1.0),
       (0, 0.5, -2, 1e-6), (0, 1.0, 1, 1.0), (0, 1.0, 65, 0.5), (1, 0.0, 0, 1.0), (0, 0.5, 2, 1.0), (0, 2.0, 0, 1.0)]


TEMPS = (0.5, 1.0, 2.0)


def controls(c: CtlCase) -> Out:
    """The launch's control arrays (inv_temp, top_k, top_p float32 / int32 [N], plen int32 [N], prefix
    uint8 [N][ML]) and ``beyond``: the (name, step) pairs whose uniform lies beyond the CDF.

    mix: name n takes MIX[(n + off) % 12], each further dozen at the next of TEMPS; prefix bytes are seeded, never the EOS byte.  tie: greedy,
    top_k = 1 / 2 and plain names on the tied maximum.  ends: every name has ended after step 1 -- even
    names free (the plan forces their EOS), odd names inside a prefix of full length that holds the EOS
    byte at step n % 4 // 2 (a forced EOS ends a name like a sampled one; the chars after it are still
    fed back)."""
    N, ML, V = c.N, c.ML, c.V
    rng = np.random.default_rng(4242 + 97 * N + V + c.off)
    pre = rng.integers(1, min(V, 256), (N, ML)).astype(np.uint8)
    pre[pre == c.eos] = 11
    inv, k, p, plen = np.ones(N, np.float32), np.zeros(N, np.int32), np.ones(N, np.float32), np.zeros(N, np.int32)
    beyond = set()
    for n in range(N):
        if c.mix == "neutral":
            continue
        if c.mix == "ends":
            if n % 2:
                plen[n] = ML
                pre[n, (n % 4) // 2] = c.eos
            else:
                inv[n] = np.float32(1.0 / (1.0, 2.0)[n % 4 // 2])
            continue
        if c.mix == "tie":
            m = [(0, 0.0, 0, 1.0), (0, 1.0, 1, 1.0), (0, 0.5, 2, 1.0), (1, 0.0, 0, 1.0), (0, 1.0, 0, 1.0)][n % 5]
        else:
            j = n + c.off
            m = MIX[j % len(MIX)]
            if m[1] != 0:      # the next dozen of names: the same cuts at the next temperature (names start
                m = (m[0], TEMPS[(TEMPS.index(m[1]) + j // len(MIX)) % 3], m[2], m[3])   # from one state: no two alike)
        plen[n] = ML if m[0] < 0 else m[0]
        inv[n] = np.float32(0.0 if m[1] == 0 else 1.0 / m[1])
        k[n] = {-1: V - 1, -2: V + 7}.get(m[2], m[2])
        p[n] = np.float32(m[3])
        if plen[n] == 0 and inv[n] != 0 and c.mix == "mix":      # sampled steps whose uniform no CDF reaches
            if n % 4 == 0:
                beyond.add((n, ML - 1))
            if n % 4 == 2:
                beyond.add((n, 0))
    pre[np.arange(ML)[None, :] >= plen[:, None]] = 0
    return dict(inv_temp=inv, top_k=k, top_p=p, plen=plen, prefix=pre, beyond=beyond)


def case_inputs(c: CtlCase, seed: int = 0) -> Out:
    d = gr.persist_inputs(c.H, c.L, c.V, c.N, c.ML, seed + c.seed_off, c.sos, c.eos)
    if c.tie:      # a copy: the cached weights are never modified
        Wfc, bfc = d["Wfc"].clone(), d["bfc"].clone()
        Wfc[9] = Wfc[5]
        bfc[5] = bfc[9] = 3.0
        d.update(Wfc=Wfc, bfc=bfc, w64=dict(d["w64"], Wfc=Wfc.double(), bfc=bfc.double()))
    return d


def case_plan(c: CtlCase) -> Optional[Out]:
    if c.mix == "ends":
        return dict(eos_at={n: (n % 4) // 2 for n in range(0, c.N, 2)}, no_other_eos=True)
    return None


# ------------------------------------------------------------------------------ the sampling step
def _stats(lg: torch.Tensor, inv: np.ndarray, k: np.ndarray, tp: np.ndarray, f64: bool, mut: Optional[str]):
    """Steps 3-7 of the rule on logits [N][V] -> y (scaled logits), cm (cumulative masses of the sorted
    post-top-k softmax), p (the renormalised filtered distribution) and keep.  float64: p and keep are
    cpu_ref's (the oracle's own code); float32: the kernel's order of operations -- y = x * inv_temp
    rounded, exp of the max-subtracted kept values, q = e / sum, the top-p set from q, e / sum again."""
    N, V = lg.shape
    dt = lg.dtype
    inv = inv.copy()
    if mut == "temperature_ignored":
        inv = np.where(inv == 0, inv, np.float32(1.0))
    k = k.copy()
    if mut == "top_k_minus_one":
        k = np.where((k > 0) & (k < V), k - 1, k)
    if mut == "top_p_ignored":
        tp = np.ones_like(tp)
    scale = torch.from_numpy(np.where(inv == 0, np.float32(1.0), inv)).to(dt).unsqueeze(-1)
    y = lg * scale
    kk = torch.from_numpy(k.astype(np.int64))
    kact = (kk > 0) & (kk < V)
    srt = torch.sort(y, -1, descending=True).values
    kth = srt.gather(-1, (kk.clamp(1, V) - 1).unsqueeze(-1))
    keep_k = torch.where(kact.unsqueeze(-1), y >= kth, torch.ones(N, V, dtype=torch.bool))
    mx = y.max(-1, keepdim=True).values
    zero = torch.zeros_like(y)
    if f64:
        e = torch.where(keep_k, torch.exp(y - mx), zero)
        q = e / e.sum(-1, keepdim=True)
    else:
        e = torch.where(keep_k, gr._exp32(y - mx), zero)
        q = e / e.double().sum(-1, keepdim=True).float()
    qs = torch.sort(q, -1, descending=True).values
    cm = torch.cumsum(qs.double(), -1).to(dt)
    if f64:
        p, keep = cpu_ref._filter(lg, inv, k, tp)
    else:
        above = torch.where(q.unsqueeze(-2) > q.unsqueeze(-1), q.unsqueeze(-2).double(), torch.zeros((), dtype=torch.float64))
        above = above.sum(-1).float()                             # mass strictly above each entry
        pt = torch.from_numpy(tp).unsqueeze(-1)
        keep = keep_k & ((pt >= 1) | (above < pt))
        e2 = torch.where(keep, e, zero)
        p = e2 / e2.double().sum(-1, keepdim=True).float()
    return y, cm, p, keep


def _lowest_argmax(y: torch.Tensor) -> torch.Tensor:
    return (y == y.max(-1, keepdim=True).values).to(torch.int64).argmax(-1)


def _run(d: Out, ctl: Out, rf: Optional[np.ndarray], f64: bool, mut: Optional[str] = None, plan: Optional[Out] = None) -> Out:
    """gen_ref._run with the controlled sampling step (the same result keys, plus y / cm / keep and the
    mask ``sampled_step`` of the (step, name) pairs that were neither forced nor greedy)."""
    H, L, V, N, ML, sos, eos = (d[k] for k in ("H", "L", "V", "N", "ML", "sos", "eos"))
    dt = torch.float64 if f64 else torch.float32
    w64 = d["w64"]
    cast = (lambda w: w) if f64 else (lambda w: w.float())
    row = (lambda a: np.roll(a, -1, 0)) if mut == "controls_of_next_row" else (lambda a: a)
    inv, k, tp, plen, pre = (row(ctl[x]) for x in ("inv_temp", "top_k", "top_p", "plen", "prefix"))
    if mut == "prefix_ignored":
        plen = np.zeros_like(plen)
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
        y, cm, p, keep = _stats(lg, inv, k, tp, f64, mut)
        top = _lowest_argmax(y)
        if mut == "greedy_highest_index":
            top = V - 1 - _lowest_argmax(y.flip(-1))
        forced = t < plen
        onehot = forced | greedy
        fid = torch.from_numpy(np.where(forced, pre[:, min(t + 1, ML - 1) if mut == "prefix_indexed_by_t" else t], 0).astype(np.int64))
        hot = torch.where(torch.from_numpy(forced), fid, top)
        one = torch.nn.functional.one_hot(hot, V).to(dt)
        oh = torch.from_numpy(onehot).unsqueeze(-1)
        p = torch.where(oh, one, p)
        keep = torch.where(oh, one > 0, keep)
        cs = torch.cumsum(p, 1) if f64 else gr._cumsum_seq(p)
        ys[t], cms[t], keeps[t], cdfs[t] = y, cm, keep, cs
        probs[t] = torch.softmax(y, -1) if (mut == "probs_unfiltered" and t == ML - 1) else p
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
                hit = csn[n] > float(rf[n, t])
                last = V - 1 if mut == "fallback_last_index" else int(np.flatnonzero(keep[n].numpy())[-1])
                sel = int(hit.argmax()) if hit.any() else last
            feed[n] = sel
            if mut == "forced_not_fed_back" and forced[n]:
                raw = _stats(lg[n:n + 1], inv[n:n + 1], k[n:n + 1], tp[n:n + 1], f64, None)[2][0].numpy()
                feed[n] = int(raw.argmax())                       # what the unforced step would favour
            sampled[t, n] = feed[n]
            if alive[n]:
                out[n, t] = sel & 0xFF
                if sel == eos:
                    alive[n] = False
            alive_after[t, n] = alive[n]
        ids = torch.from_numpy(feed.copy())
    return dict(rf=rf, ids_in=ids_in, sampled=sampled, alive_after=alive_after, out=out, states=states, logits=logits,
                probs_last=probs[ML - 1], probs=probs, cdf=cdfs, y=ys, cm=cms, keep=keeps, sampled_step=smp,
                id_words=(sampled | (alive_after.astype(np.int64) << 16)).astype(np.uint32))


# ------------------------------------------------------------------------------ guards and the planter
def clearance(ctl: Out, run: Out) -> List[Dict[str, object]]:
    """Every (step, name) of a float64 trajectory that misses a guard: the top-k edge (or the gap below a
    greedy maximum) thinner than GUARD_Y, or top_p closer than GUARD_MASS to a cumulative mass."""
    bad = []
    ML, N, V = run["y"].shape
    for t in range(ML):
        for n in range(N):
            if t < ctl["plen"][n]:
                continue
            s = np.sort(run["y"][t, n].numpy())[::-1]
            k = int(ctl["top_k"][n])
            if ctl["inv_temp"][n] == 0:
                k = 1
            if 0 < k < V:
                below = s[s < s[k - 1]]                            # (an exact tie with the k-th value is kept with it)
                above = s[s > s[k]] if s[k] < s[k - 1] else np.empty(0)
                gap = min(s[k - 1] - below[0] if len(below) else np.inf,
                          above[-1] - s[k] if len(above) else np.inf)
                if gap < GUARD_Y:
                    bad.append(dict(t=t, n=n, what="top_k", gap=float(gap)))
            if ctl["inv_temp"][n] != 0 and ctl["top_p"][n] < 1:
                dist = float(np.abs(run["cm"][t, n].numpy() - float(ctl["top_p"][n])).min())
                if dist < GUARD_MASS:
                    bad.append(dict(t=t, n=n, what="top_p", gap=dist))
    return bad


def plant(d: Out, ctl: Out, plan: Optional[Out] = None):
    """The float64 controlled trajectory with planted uniforms.  Returns (controls, trajectory): the
    controls are ``ctl`` except for the names that had to be moved to clear the guards (``moved``)."""
    ctl = dict(ctl, top_k=ctl["top_k"].copy(), top_p=ctl["top_p"].copy())
    moved = set()
    V = d["V"]
    for _ in range(8):
        run = _run(d, ctl, None, True, plan=plan)
        bad = clearance(ctl, run)
        if not bad:
            break
        for b in bad:
            n, t = b["n"], b["t"]
            if n in moved and b["what"] == "top_p":
                pass                                               # moved before: move again below, on this step's masses
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
    assert not clearance(ctl, run), "the planter could not clear the guards"
    # one name in eight; a launch of fewer than eight names may move one
    assert len(moved) <= max(d["N"] // 8, 1), f"{len(moved)} of {d['N']} names had to be moved: the case no longer tests its values"
    ctl["moved"] = sorted(moved)
    return ctl, run


def oracle(d: Out, ctl: Out, rf: np.ndarray) -> Out:
    return _run(d, ctl, rf, True)


def emulate(d: Out, ctl: Out, rf: np.ndarray, mut: Optional[str] = None) -> Out:
    assert mut is None or mut in MUTATIONS, mut
    return _run(d, ctl, rf, False, mut=mut)


# planted defects of the emulator -> the case whose checks must catch it
MUTATIONS = {
    "prefix_ignored": "cb-N9",
    "prefix_indexed_by_t": "cg-N4-full-prefix",
    "forced_not_fed_back": "cb-N17",
    "controls_of_next_row": "cc-N9",
    "top_k_minus_one": "cb-N16",
    "top_p_ignored": "cc-N17",
    "temperature_ignored": "cb-N33",
    "greedy_highest_index": "ct-tie-N12",
    "fallback_last_index": "cb-N17",
    "probs_unfiltered": "cc-N8",
}


# ------------------------------------------------------------------------------ measurement
def case_deviation(c: CtlCase, seed: int = 0) -> Dict[str, float]:
    d = case_inputs(c, seed)
    ctl, orc = plant(d, controls(c), case_plan(c))
    emu = emulate(d, ctl, orc["rf"])
    T = gr.chars_run(orc["alive_after"], c.ML, c.probs)
    hit = torch.from_numpy((np.arange(c.ML)[:, None] < T) & orc["sampled_step"]).unsqueeze(-1)
    return dict(y=float(((emu["y"].double() - orc["y"]).abs() * hit).max()),
                mass=float(((emu["cm"].double() - orc["cm"]).abs() * hit).max()),
                probs=gr.deviation(emu["probs_last"], orc["probs_last"]),
                moved=float(len(ctl["moved"])),
                rows_equal=float(np.array_equal(emu["out"], orc["out"]) and np.array_equal(emu["sampled"], orc["sampled"])
                                 and bool((emu["keep"] == orc["keep"])[:T].all())))


def measure_deviations(seeds=(0, 1, 2), verbose: bool = False) -> Dict[str, float]:
    out = {k: 0.0 for k in MEASURED_DEV}
    for c in CTL_CASES:
        for seed in seeds:
            dev = case_deviation(c, seed)
            assert dev.pop("rows_equal") == 1.0, f"{c.name} seed {seed}: the emulator's rows or kept sets differ from the oracle's"
            if verbose:
                print(c.name, seed, {k: f"{v:.3e}" for k, v in dev.items()}, flush=True)
            for k in out:
                out[k] = max(out[k], dev[k])
    return out


if __name__ == "__main__":
    res = measure_deviations(verbose=True)
    for k in MEASURED_DEV:
        print(f'    "{k}": {res[k]:.3e},')

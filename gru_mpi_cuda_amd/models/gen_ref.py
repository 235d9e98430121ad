"""Per-element reference of the generation path: the persistent generator (gen_persist.hip), the fp32
gates and the batch reset (gen_f32.hip: gru_gates_f32, gen_reset) and the scorer's kernels (score.hip:
score_prep, score_logprob_f32), in the style of ``head_ref.py`` / ``seq_ref.py``.

* ``persist_inputs``: seeded fp32 weights at ``init_params`` scale with every bias scaled up (BIAS_X)
  and a random layer-0 table P, so a dropped or mis-indexed bias moves values far beyond a tolerance.
* ``plant_uniforms``: the float64 trajectory from h = 0 (``oracle`` re-runs it on given uniforms).  It
  builds the uniforms while it runs: each one is at least GUARD away from every edge of the float64
  CDF of its step (moved to the middle of an interval where the seeded draw is not), and a plan can
  force chosen ids (EOS at a chosen step, or never).  Every (name, step) is kept: none is skipped.
* ``emulate``: the same trajectory in float32 on the CPU (the CPU stand-in for "a correct kernel"),
  with a ``mut`` hook that plants one of MUTATIONS.
* ``ws_decode`` / ``ws_encode``: the exchange workspace of a launch (kernels.h, GenPersistArgs::ws):
  both state layouts, the logits and id slots, and the mask of the slots a launch owns.
* ``step_ref``: float64 ONE-step reference from the kernel's own stored inputs: h_l(t) from the decoded
  h_l(t-1) and h_{l-1}(t) (or P[id_t]), logits(t) from the decoded h_{L-1}(t).  Error does not pile up
  over chars or layers, so one tolerance serves every t.
* ``check_launch``: every check of one persistent launch, shared by tests/test_gen_gpu.py (on the
  kernel's buffers) and tests/test_gen_ref.py (on the encoded output of the emulator and of its
  mutations).
* the gates / scorer references (float64 from the given inputs) and their float32 emulators.
"""
from __future__ import annotations

import functools
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

Out = Dict[str, object]

# ------------------------------------------------------------------------------ the kernel's constants
KG = 256          # workgroups = producers
NMAX = 64         # name rows of every slot
XLINE = 32        # floats of a producer's line in the tagged state layout
DIST_N = 16       # more names than this: distributed sampling, name tiles of 16 rows
TAG_X = 8         # up to this many names at H = 1024 the layer states use the tagged layout
EMPTY = 0xFFFFFFFF   # the fill word of an unwritten tagged slot
BIAS_X = 8.0

# ------------------------------------------------------------------------------ tolerances
# |got - ref| <= ATOL per element (RTOL = 0: fp32 values of magnitude <= 1, or logits of a few units).
#   state : h_l(t), one step from the stored inputs
#   logit : logits(t), one step from the stored h_{L-1}(t)
#   probs : the last char's softmax, end to end against the float64 trajectory
#   cdf   : the running sum of a sampled step's softmax, end to end (makes GUARD, not a tolerance)
#   gates : gru_gates_f32's h', from the given pre-activations
#   logp  : score_logprob_f32's tok_logp, from the given logits
#   name_logp : its per-name sum against the float64 sum (up to 64 tokens, sums near -800: an fp32 ulp
#           there is 6e-5); the test also holds it bitwise to the fp32 sum of the kernel's own tok_logp
# Measured, not chosen: ``python -m gru_mpi_cuda_amd.models.gen_ref`` (measure_deviations) runs every
# case of tests/test_gen_gpu.py through ``emulate`` at seeds 0, 1, 2 and takes the largest deviation of
# each family (recorded here rounded up to three digits).
MEASURED_DEV = {
    "state": 1.28e-07,
    "logit": 1.76e-07,
    "probs": 1.50e-09,
    "cdf": 1.09e-06,
    "gates": 3.21e-07,
    "logp": 1.10e-06,
    "name_logp": 2.55e-04,
}
RTOL = {k: 0.0 for k in MEASURED_DEV}
# atol = 4 x the measured deviation (the margin covers the MFMA / 8-wave summation order and the device
# expf / tanhf, which the emulator does not reproduce)
ATOL = {k: 4.0 * v for k, v in MEASURED_DEV.items()}
GUARD = max(1e-5, 8.0 * MEASURED_DEV["cdf"])


# ------------------------------------------------------------------------------ cases of the GPU test
class Case(NamedTuple):
    name: str
    H: int
    L: int
    V: int
    N: int
    ML: int
    sos: int = 0
    eos: int = 0
    plan: Optional[str] = None    # None: seeded uniforms; "ends01": name 0 ends at step 0, name 1 at step 1,
                                  # the rest never; "all_end": every name ended by step 1
    probs: bool = True            # False: probs = nullptr (the launch stops once every name has ended)
    seed_off: int = 0


def _se(i: int):
    return (7, 3) if i % 2 == 0 else (0, 0)


VARIANTS = [(256, 1), (256, 2), (256, 3), (256, 4), (512, 1), (512, 2), (512, 3), (512, 4), (1024, 1), (1024, 2)]
CASES_A = [Case(f"a-H{H}-L{L}", H, L, 256, 3, 3, *_se(i)) for i, (H, L) in enumerate(VARIANTS)]
CASES_B = [Case(f"b-N{N}", 512, 2, 256, N, 4, *_se(i)) for i, N in enumerate((1, 2, 8, 9, 16, 17, 32, 33, 48, 49, 64))]
CASES_C = [Case(f"c-N{N}", 1024, 2, 256, N, 3, *_se(i + 1)) for i, N in enumerate((1, 8, 9, 16, 17, 64))]
CASES_D = [Case("d-512-L3-N33", 512, 3, 256, 33, 3, 7, 3), Case("d-512-L4-N16", 512, 4, 256, 16, 3),
           Case("d-512-L4-N40", 512, 4, 256, 40, 3, 7, 3), Case("d-256-L4-N64", 256, 4, 256, 64, 3)]
CASES_E = [Case("e-256-L1-N1", 256, 1, 512, 1, 3, 7, 3), Case("e-512-L2-N12", 512, 2, 512, 12, 3),
           Case("e-512-L1-N33", 512, 1, 512, 33, 3, 7, 3), Case("e-1024-L2-N5", 1024, 2, 512, 5, 3)]
CASES_F = [Case(f"f-L{L}-N{N}-ML{ML}", 512, L, 256, N, ML, *_se(i + j))
           for j, (L, N) in enumerate(((1, 5), (2, 20))) for i, ML in enumerate((1, 2, 10))]
CASES_G = [c for N in (4, 20) for c in (
    Case(f"g-N{N}-ends01", 256, 2, 256, N, 4, 7, 3, "ends01"),
    Case(f"g-N{N}-all-end-early-exit", 256, 2, 256, N, 5, 7, 3, "all_end", False),
    Case(f"g-N{N}-all-end-probs", 256, 2, 256, N, 5, 7, 3, "all_end", True))]
# one workspace, launches with parity 0, 1, 0, 1: different weights and names each, so that a slot left
# over from an earlier launch never holds the value the current one must write
CASES_H = [Case(f"h-launch{i}-N{N}", 1024, 2, 256, N, 3, *_se(i), seed_off=10 * (i + 1))
           for i, N in enumerate((16, 5, 64, 8))]
PERSIST_CASES: List[Case] = CASES_A + CASES_B + CASES_C + CASES_D + CASES_E + CASES_F + CASES_G + CASES_H


# ------------------------------------------------------------------------------ layout
def set_floats(H: int, L: int, V: int, ML: int) -> int:
    """Floats of one of the two sets of GenPersistArgs::ws."""
    return L * ML * NMAX * H + ML * NMAX * (V + 1)


def tagged_states(H: int, N: int) -> bool:
    return H == 1024 and N <= TAG_X


def rows_written(N: int) -> int:
    """Name rows of a plain slot that a launch may write: N up to 16 names, else N rounded up to 16."""
    return N if N <= DIST_N else (N + 15) // 16 * 16


def refill_floats(H: int, L: int, V: int, ML: int):
    """(state floats from the set's start, logit floats from the logits' start) that a launch fills with
    EMPTY in the OTHER set."""
    return L * ML * KG * XLINE, ML * NMAX * V


def chars_run(alive_after: np.ndarray, ML: int, probs: bool) -> int:
    """Chars whose states and logits a launch computes: ML, or with probs == nullptr the first t >= 1
    before which every name has ended."""
    if not probs:
        for t in range(1, ML):
            if not alive_after[t - 1].any():
                return t
    return ML


def _views(s: np.ndarray, H, L, V, ML):
    nst, nlg = L * ML * NMAX * H, ML * NMAX * V
    return s[:nst], s[nst:nst + nlg].reshape(ML, NMAX, V), s[nst + nlg:].reshape(ML, NMAX)


def ws_decode(ws: np.ndarray, par: int, H: int, L: int, V: int, ML: int, N: int, T: Optional[int] = None) -> Out:
    """Set ``par`` of a workspace (uint32 or float32 words) after a launch of N names that ran T chars
    (default ML).  Returns states [L][ML][N][H] and logits [ML][N][V] (float32), ids [ML][N] (uint32:
    id | alive << 16 of the char sampled after step t; written with more than 16 names, for
    t < min(T, ML - 1)), and ``mask`` over the set's words: the slots this launch owns (may write)."""
    T = ML if T is None else T
    sf = set_floats(H, L, V, ML)
    s = np.ascontiguousarray(ws).view(np.uint32)[par * sf:(par + 1) * sf]
    mask = np.zeros(sf, dtype=bool)
    st, lg, idw = _views(s, H, L, V, ML)
    mst, mlg, mid = _views(mask, H, L, V, ML)
    nw = rows_written(N)
    if tagged_states(H, N):
        U = 4
        n4 = L * ML * KG * XLINE
        v = st[:n4].reshape(L, ML, KG, XLINE)[..., :N * U].reshape(L, ML, KG, N, U)
        states = v.transpose(0, 1, 3, 2, 4).reshape(L, ML, N, H)          # unit = producer * U + u
        mst[:n4].reshape(L, ML, KG, XLINE)[:, :T, :, :N * U] = True
    else:
        states = st.reshape(L, ML, NMAX, H)[:, :, :N]
        mst.reshape(L, ML, NMAX, H)[:, :T, :nw] = True
    mlg[:T, :nw] = True
    if N > DIST_N:
        mid[:min(T, ML - 1), :N] = True
    return dict(states=np.ascontiguousarray(states).view(np.float32), logits=np.ascontiguousarray(lg[:, :N]).view(np.float32),
                ids=np.ascontiguousarray(idw[:, :N]), mask=mask)


def ws_encode(base: np.ndarray, par: int, states, logits, ids, H, L, V, ML, N, T: Optional[int] = None) -> np.ndarray:
    """The inverse: a copy of ``base`` (uint32 words of both sets) with set ``par`` holding what a launch
    of N names over T chars stores (rows n < N only) and the other set refilled as a launch does."""
    T = ML if T is None else T
    sf = set_floats(H, L, V, ML)
    out = np.array(base, dtype=np.uint32, copy=True)
    st, lg, idw = _views(out[par * sf:(par + 1) * sf], H, L, V, ML)
    sb = np.ascontiguousarray(np.asarray(states, dtype=np.float32)).view(np.uint32)
    lb = np.ascontiguousarray(np.asarray(logits, dtype=np.float32)).view(np.uint32)
    if tagged_states(H, N):
        U = 4
        n4 = L * ML * KG * XLINE
        v = sb.reshape(L, ML, N, KG, U).transpose(0, 1, 3, 2, 4).reshape(L, ML, KG, N * U)
        st[:n4].reshape(L, ML, KG, XLINE)[:, :T, :, :N * U] = v[:, :T]
    else:
        st.reshape(L, ML, NMAX, H)[:, :T, :N] = sb[:, :T]
    lg[:T, :N] = lb[:T]
    if N > DIST_N:
        k = min(T, ML - 1)
        idw[:k, :N] = np.asarray(ids, dtype=np.uint32)[:k]
    rs, rl = refill_floats(H, L, V, ML)
    o = out[(1 - par) * sf:(2 - par) * sf]
    o[:rs] = EMPTY
    o[L * ML * NMAX * H:L * ML * NMAX * H + rl] = EMPTY
    return out


# ------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=3)
def _weights(H: int, L: int, V: int, seed: int) -> Out:
    g = torch.Generator(device="cpu").manual_seed(7000 + seed)
    k = H ** -0.5

    def u(*shape, scale=k):
        return ((torch.rand(shape, generator=g) * 2 - 1) * scale).contiguous()

    d: Out = dict(Whh=[u(3 * H, H) for _ in range(L)], Wih=[None] + [u(3 * H, H) for _ in range(1, L)],
                  bhh=[u(3 * H, scale=BIAS_X * k) for _ in range(L)],
                  bih=[None] + [u(3 * H, scale=BIAS_X * k) for _ in range(1, L)],
                  Wfc=u(V, H), bfc=u(V, scale=BIAS_X * k), P=u(V, 3 * H, scale=1.0))
    d["w64"] = {key: ([None if w is None else w.double() for w in val] if isinstance(val, list) else val.double())
                for key, val in d.items()}
    return d


def persist_inputs(H, L, V, N, ML, seed=0, sos=0, eos=0) -> Out:
    """Weights (shared by every N and ML of a shape and seed, never modified) and the seeded uniforms
    rf0 [N][ML] that plant_uniforms starts from."""
    d = dict(_weights(H, L, V, seed))
    g = torch.Generator(device="cpu").manual_seed(9000 + 131 * seed + N + 64 * ML)
    d.update(H=H, L=L, V=V, N=N, ML=ML, sos=sos, eos=eos, rf0=torch.rand(N, ML, generator=g).numpy().astype(np.float32))
    return d


def case_inputs(c: Case, seed: int = 0) -> Out:
    return persist_inputs(c.H, c.L, c.V, c.N, c.ML, seed + c.seed_off, c.sos, c.eos)


def case_plan(c: Case) -> Optional[Out]:
    if c.plan == "ends01":
        return dict(eos_at={0: 0, 1: 1}, no_other_eos=True)
    if c.plan == "all_end":
        return dict(eos_at={n: n % 2 for n in range(c.N)}, no_other_eos=True)
    return None


# ------------------------------------------------------------------------------ the trajectory
def _exp32(x):
    return torch.exp(x.double()).float()


def _prod(x, W64, b, f64: bool, skip: Optional[int] = None):
    """x [N][K] . W [R][K]^T + b.  float32: the 32 (wave, quarter) pieces of K / 32 columns, each summed
    exactly and rounded, added in index order in fp32 -- the same bits on every host.  ``skip``: one
    wave's K-slice (four pieces) left out."""
    if f64 and skip is None:
        y = x @ W64.T
        return y if b is None else y + b
    N, K = x.shape
    kj = K // 32
    part = torch.bmm(x.double().reshape(N, 32, kj).permute(1, 0, 2), W64.reshape(-1, 32, kj).permute(1, 2, 0))
    if f64:
        keep = [s for s in range(32) if s // 4 != skip]
        y = part[keep].sum(0)
        return y if b is None else y + b
    part = part.float()
    acc = torch.zeros(N, W64.shape[0], dtype=torch.float32)
    for s in range(32):
        if skip is not None and s // 4 == skip:
            continue
        acc = acc + part[s]
    return acc if b is None else acc + b


def _gate_math(gi, gh, hp, f64: bool, mut=None, bhn=None):
    """PyTorch's GRU cell: r, z = sigmoid, n = tanh(gi_n + r gh_n), h' = (1 - z) n + z h."""
    H = hp.shape[-1]
    if f64:
        sig = lambda v: 1.0 / (1.0 + torch.exp(-v))
        tanh = torch.tanh
    else:
        sig = lambda v: 1.0 / (1.0 + _exp32(-v))
        tanh = lambda v: torch.tanh(v.double()).float()
    r = sig(gi[..., :H] + gh[..., :H])
    z = sig(gi[..., H:2 * H] + gh[..., H:2 * H])
    ghn = gh[..., 2 * H:]
    if mut == "bhh_n_outside_r":
        n = tanh(gi[..., 2 * H:] + r * (ghn - bhn) + bhn)
    else:
        n = tanh(gi[..., 2 * H:] + r * ghn)
    if mut == "blend_swapped":
        return z * n + (1.0 - z) * hp
    return (1.0 - z) * n + z * hp


def _cumsum_seq(p: torch.Tensor) -> torch.Tensor:
    """Strictly left-to-right running sum in p's dtype (cpu_ref.sample_inverse_cdf's rule)."""
    cs = torch.empty_like(p)
    acc = torch.zeros_like(p[..., 0])
    for i in range(p.shape[-1]):
        acc = acc + p[..., i]
        cs[..., i] = acc
    return cs


def _pick(cdf: np.ndarray, r) -> int:
    hit = cdf > float(r)
    return int(hit.argmax()) if hit.any() else len(cdf) - 1


def _plant(cdf: np.ndarray, p: np.ndarray, r0: np.float32, force: Optional[int], avoid: Optional[int]) -> np.float32:
    """The uniform of one (name, step): r0 where it clears every CDF edge by GUARD (and does not pick
    ``avoid``), else the middle of its interval, else of the widest allowed one; ``force``: the middle of
    that id's interval."""
    def mid(j):
        return np.float32(cdf[j] - 0.5 * p[j])

    if force is not None:
        r = mid(force)
    else:
        r = np.float32(r0)
        j = _pick(cdf, r)
        if j == avoid or np.abs(cdf - float(r)).min() < GUARD:
            if j == avoid or p[j] < 4 * GUARD:
                q = p.copy()
                if avoid is not None:
                    q[avoid] = -1.0
                j = int(q.argmax())
            r = mid(j)
    assert np.abs(cdf - float(r)).min() >= GUARD and 0.0 <= float(r) < 1.0, "no interval wide enough for the guard"
    assert force is None or _pick(cdf, r) == force
    assert avoid is None or _pick(cdf, r) != avoid
    return r


def _run(d: Out, rf: Optional[np.ndarray], f64: bool, mut: Optional[str] = None, plan: Optional[Out] = None) -> Out:
    H, L, V, N, ML, sos, eos = (d[k] for k in ("H", "L", "V", "N", "ML", "sos", "eos"))
    dt = torch.float64 if f64 else torch.float32
    w64 = d["w64"]
    cast = (lambda w: w) if f64 else (lambda w: w.float())
    planting = rf is None
    rf = np.zeros((N, ML), np.float32) if planting else np.asarray(rf, np.float32)
    h = [torch.zeros(N, H, dtype=dt) for _ in range(L)]
    hold = [torch.zeros(N, H, dtype=dt) for _ in range(L)]     # h_l(t-2), for the stale-gh mutation
    ids = torch.full((N,), sos, dtype=torch.int64)
    alive = np.ones(N, dtype=bool)
    out = np.zeros((N, ML + 1), np.uint8)
    states = torch.zeros(L, ML, N, H, dtype=dt)
    logits = torch.zeros(ML, N, V, dtype=dt)
    probs = torch.zeros(ML, N, V, dtype=dt)
    cdfs = torch.zeros(ML, N, V, dtype=dt)
    ids_in = np.zeros((ML, N), np.int64)
    sampled = np.zeros((ML, N), np.int64)
    alive_after = np.zeros((ML, N), dtype=bool)
    P = cast(w64["P"])
    if mut == "P_gate_blocks_permuted":
        P = torch.cat([P[:, H:2 * H], P[:, 2 * H:], P[:, :H]], 1)
    for t in range(ML):
        ids_in[t] = ids.numpy()
        x = None
        for l in range(L):
            hp = h[l]
            src = hold[l] if mut == "stale_gh" else hp
            gh = _prod(src, w64["Whh"][l], cast(w64["bhh"][l]), f64, skip=3 if (mut == "k_slice_missing" and l == 0) else None)
            if l == 0:
                gi = P[ids]
            else:
                xin = x
                if mut == "name_shift_second_tile" and N > 17:
                    xin = x.clone()
                    xin[16:N - 1] = x[17:N]
                gi = _prod(xin, w64["Wih"][l], None if mut == "bih_dropped_upper_layers" else cast(w64["bih"][l]), f64)
            hn = _gate_math(gi, gh, hp, f64, mut, cast(w64["bhh"][l])[2 * H:])
            hold[l], h[l], x = hp, hn, hn
            states[l, t] = hn
        xin = x
        if mut == "name_shift_second_tile" and L == 1 and N > 17:
            xin = x.clone()
            xin[16:N - 1] = x[17:N]
        lg = _prod(xin, w64["Wfc"], None if mut == "bfc_dropped" else cast(w64["bfc"]), f64)
        logits[t] = lg
        mx = lg.max(1, keepdim=True).values
        if f64:
            e = torch.exp(lg - mx)
            p = e / e.sum(1, keepdim=True)
            cs = torch.cumsum(p, 1)
        else:
            e = _exp32(lg - mx)
            p = e / e.double().sum(1, keepdim=True).float()
            cs = _cumsum_seq(p)
        probs[t], cdfs[t] = p, cs
        csn, pn = cs.numpy(), p.numpy()
        for n in range(N):
            if planting:
                force = avoid = None
                if plan is not None:
                    if plan["eos_at"].get(n) == t:
                        force = eos
                    elif plan.get("no_other_eos"):
                        avoid = eos
                rf[n, t] = _plant(csn[n].astype(np.float64), pn[n].astype(np.float64), d["rf0"][n, t], force, avoid)
            sel = _pick(csn[n], rf[n, t])     # (float32 running sums compare exactly after the widening)
            if mut == "sample_index_plus_one":
                sel = min(sel + 1, V - 1)
            sampled[t, n] = sel
            if alive[n] or mut == "out_written_after_eos":
                if not (mut == "eos_byte_not_written" and sel == eos):
                    out[n, t] = sel & 0xFF                     # (a byte: V = 512 keeps the low eight bits, as the kernel)
                if sel == eos:
                    alive[n] = False
            alive_after[t, n] = alive[n]
        nxt = torch.from_numpy(sampled[t].copy())
        if mut == "id_frozen_at_eos":
            nxt = torch.where(torch.from_numpy(alive_after[t]), nxt, torch.full_like(nxt, eos))
        ids = nxt
    last = ML - 2 if (mut == "probs_one_step_early" and ML > 1) else ML - 1
    return dict(rf=rf, ids_in=ids_in, sampled=sampled, alive_after=alive_after, out=out, states=states, logits=logits,
                probs_last=probs[last], probs=probs, cdf=cdfs,
                id_words=(sampled | (alive_after.astype(np.int64) << 16)).astype(np.uint32))


def plant_uniforms(d: Out, plan: Optional[Out] = None) -> Out:
    """The float64 trajectory, building the uniforms (``rf`` of the result) while it runs."""
    return _run(d, None, True, plan=plan)


def oracle(d: Out, rf: np.ndarray) -> Out:
    """The float64 trajectory from h = 0 on given uniforms: per-step ids (the sampled id feeds the next
    step whether or not the name has ended), alive flags, the output rows (which stop at the EOS byte),
    states [L][ML][N][H], logits [ML][N][V] and the last step's probabilities."""
    return _run(d, rf, True)


def emulate(d: Out, rf: np.ndarray, mut: Optional[str] = None) -> Out:
    """The same trajectory in float32: products as _prod, exp / tanh the correctly rounded ones, the
    sampler's `psum > r` on a left-to-right fp32 running sum.  ``mut``: one of MUTATIONS."""
    assert mut is None or mut in MUTATIONS, mut
    return _run(d, rf, False, mut=mut)


# planted defects of the emulator -> the GPU case whose checks must catch it.  (A sampler with `>=` for
# `>` is not among them: the two differ only where a running sum equals the uniform exactly, which the
# guard rules out for every uniform the tests use; an index moved by one stands in for a wrong rule.)
MUTATIONS = {
    "bhh_n_outside_r": "b-N2",
    "blend_swapped": "b-N2",
    "stale_gh": "b-N9",
    "bih_dropped_upper_layers": "a-H256-L2",
    "bfc_dropped": "a-H512-L1",
    "k_slice_missing": "c-N8",
    "name_shift_second_tile": "b-N33",
    "P_gate_blocks_permuted": "a-H1024-L1",
    "probs_one_step_early": "f-L1-N5-ML2",
    "sample_index_plus_one": "b-N17",
    "id_frozen_at_eos": "g-N4-ends01",
    "eos_byte_not_written": "g-N20-ends01",
    "out_written_after_eos": "g-N4-all-end-probs",
}


# ------------------------------------------------------------------------------ one-step reference
def step_ref(d: Out, states: np.ndarray, ids_in: np.ndarray, T: int):
    """float64 h_l(t) and logits(t), t < T, each from the STORED float32 inputs: h_l(t-1) (0 at t = 0),
    h_{l-1}(t) or P[id_t], and h_{L-1}(t).  Returns (states [L][T][N][H], logits [T][N][V])."""
    H, L, V, N = d["H"], d["L"], d["V"], d["N"]
    w = d["w64"]
    S = torch.from_numpy(np.ascontiguousarray(states[:, :T])).double()
    ref = torch.zeros(L, T, N, H, dtype=torch.float64)
    ids = torch.from_numpy(np.asarray(ids_in[:T])).long()
    for l in range(L):
        hp = torch.cat([torch.zeros(1, N, H, dtype=torch.float64), S[l, :T - 1]], 0).reshape(T * N, H)
        gh = hp @ w["Whh"][l].T + w["bhh"][l]
        gi = w["P"][ids.reshape(-1)] if l == 0 else S[l - 1].reshape(T * N, H) @ w["Wih"][l].T + w["bih"][l]
        ref[l] = _gate_math(gi, gh, hp, True).reshape(T, N, H)
    lg = S[L - 1].reshape(T * N, H) @ w["Wfc"].T + w["bfc"]
    return ref, lg.reshape(T, N, V)


def deviation(got, ref) -> float:
    """Largest |got - ref| (inf for a NaN)."""
    g = torch.as_tensor(np.asarray(got)).double() if not torch.is_tensor(got) else got.double()
    r = torch.as_tensor(np.asarray(ref)).double() if not torch.is_tensor(ref) else ref.double()
    if g.numel() == 0:
        return 0.0
    e = (g - r).abs()
    return float("inf") if bool(torch.isnan(e).any()) else float(e.max())


# ------------------------------------------------------------------------------ the launch checker
def check_launch(d: Out, orc: Out, got: Out, probs: bool = True, atol: Optional[Dict[str, float]] = None):
    """Every check of one persistent launch.  ``orc``: the float64 trajectory on the launch's uniforms.
    ``got``: err, sync (uint32 words), out [rows >= N][ML + 1] uint8 that started as out_canary, par,
    ws_before / ws_after (uint32 words of both sets) and, with ``probs``, probs / probs_before
    [rows][V] float32.  Returns (failures, figures): the failed checks as text and the worst deviation
    of each family."""
    H, L, V, N, ML = d["H"], d["L"], d["V"], d["N"], d["ML"]
    atol = ATOL if atol is None else atol
    fails: List[str] = []
    T = chars_run(orc["alive_after"], ML, probs)
    Np = (N + 15) // 16 * 16
    if np.asarray(got["err"]).any():
        fails.append(f"err = {np.asarray(got['err']).tolist()}")
    if np.asarray(got["sync"]).any():
        fails.append(f"{int(np.count_nonzero(got['sync']))} sync words are not zero after the launch")
    out = np.asarray(got["out"], np.uint8)
    if not np.array_equal(out[:N], orc["out"]):
        bad = np.argwhere(out[:N] != orc["out"])[0]
        fails.append(f"out row {bad[0]} byte {bad[1]}: got {out[bad[0], bad[1]]}, oracle {orc['out'][bad[0], bad[1]]}")
    if not (out[N:] == got["out_canary"]).all():
        fails.append("out rows after row N were written")
    par = int(got["par"])
    sf = set_floats(H, L, V, ML)
    before = np.asarray(got["ws_before"]).view(np.uint32)
    after = np.asarray(got["ws_after"]).view(np.uint32)
    dec = ws_decode(after, par, H, L, V, ML, N, T)
    if N > DIST_N:
        k = min(T, ML - 1)
        if not np.array_equal(dec["ids"][:k], orc["id_words"][:k]):
            bad = np.argwhere(dec["ids"][:k] != orc["id_words"][:k])[0]
            fails.append(f"ID[{bad[0]}][{bad[1]}] = {dec['ids'][bad[0], bad[1]]:#x}, oracle {orc['id_words'][bad[0], bad[1]]:#x}")
    rs, rl = step_ref(d, dec["states"], orc["ids_in"], T)
    fig = dict(state=deviation(dec["states"][:, :T], rs), logit=deviation(dec["logits"][:T], rl))
    for fam in ("state", "logit"):
        if not fig[fam] <= atol[fam]:
            g = dec["states"][:, :T] if fam == "state" else dec["logits"][:T]
            r = (rs if fam == "state" else rl).numpy()
            e = np.abs(g.astype(np.float64) - r)
            e = np.where(np.isnan(e), np.inf, e)
            idx = np.unravel_index(int(e.argmax()), e.shape)
            fails.append(f"{fam} {('[l][t][n][h]' if fam == 'state' else '[t][n][v]')} {tuple(int(i) for i in idx)}: got {g[idx]:.9g}, one-step "
                         f"reference {r[idx]:.9g}; {int((e > atol[fam]).sum())} of {e.size} beyond atol {atol[fam]:.3g}")
    if probs:
        pb = np.ascontiguousarray(got["probs"], dtype=np.float32)
        fig["probs"] = deviation(pb[:N], orc["probs_last"])
        if not fig["probs"] <= atol["probs"]:
            fails.append(f"probs: worst |got - oracle| {fig['probs']:.3g} beyond atol {atol['probs']:.3g}")
        if not np.array_equal(pb[Np:].view(np.uint32), np.ascontiguousarray(got["probs_before"], dtype=np.float32)[Np:].view(np.uint32)):
            fails.append("probs rows after Np were written")
    own = dec["mask"]
    s0, s1 = par * sf, (par + 1) * sf
    if not np.array_equal(after[s0:s1][~own], before[s0:s1][~own]):
        i = int(np.flatnonzero((after[s0:s1] != before[s0:s1]) & ~own)[0])
        fails.append(f"set {par}: word {i} outside the launch's slots changed ({before[s0 + i]:#x} -> {after[s0 + i]:#x})")
    # the other set: the refill region is EMPTY, every other word is what it was
    o0 = (1 - par) * sf
    ns, nl = refill_floats(H, L, V, ML)
    refill = np.zeros(sf, dtype=bool)
    refill[:ns] = True
    refill[L * ML * NMAX * H:L * ML * NMAX * H + nl] = True
    oa, ob = after[o0:o0 + sf], before[o0:o0 + sf]
    if not (oa[refill] == EMPTY).all():
        fails.append(f"set {1 - par}: {int((oa[refill] != EMPTY).sum())} words of the refill region are not EMPTY")
    if not np.array_equal(oa[~refill], ob[~refill]):
        fails.append(f"set {1 - par}: words outside the refill region changed")
    return fails, fig


def synth_got(d: Out, run: Out, par: int = 0, probs: bool = True, T: Optional[int] = None) -> Out:
    """The buffers a launch would leave if it computed ``run`` (an emulate / oracle result): what the
    CPU tests feed check_launch in place of the kernel's."""
    H, L, V, N, ML = d["H"], d["L"], d["V"], d["N"], d["ML"]
    T = chars_run(run["alive_after"], ML, probs) if T is None else T
    Np = (N + 15) // 16 * 16
    before = np.full(2 * set_floats(H, L, V, ML), EMPTY, dtype=np.uint32)
    after = ws_encode(before, par, run["states"].float().numpy(), run["logits"].float().numpy(), run["id_words"], H, L, V, ML, N, T)
    out = np.full((N + 2, ML + 1), 0xA5, np.uint8)
    out[:N] = run["out"]
    got = dict(err=np.zeros(4, np.uint32), sync=np.zeros(8, np.uint32), out=out, out_canary=0xA5, par=par,
               ws_before=before, ws_after=after)
    if probs:
        pb = np.full((Np + 2, V), np.nan, np.float32)
        got["probs_before"] = pb.copy()
        pb[:N] = run["probs_last"].float().numpy()
        got["probs"] = pb
    return got


# ------------------------------------------------------------------------------ gates (gru_gates_f32)
GATES_SHAPES = [(1, 40), (3, 200), (5, 256), (64, 1024)]     # (Bp, H); the first two are no multiple of 256 threads
GATES_V = 50


def gates_inputs(Bp: int, H: int, table: bool, gh_splits: int, gi_splits: int, bias: bool, seed: int = 0,
                 bad_ids: bool = False) -> Out:
    """Gh / Gi as split-K slabs [splits][slab] with slab = Bp 3H + 24 and NaN in the gap, hprev, the
    optional biases, and for the table path P [V][3H] and ids."""
    g = torch.Generator(device="cpu").manual_seed(11000 + seed + Bp + H)
    row = Bp * 3 * H
    slab = row + 24

    def slabs(k):
        t = torch.full((k, slab), float("nan"))
        t[:, :row] = torch.rand(k, row, generator=g) * 2 - 1
        return t

    d: Out = dict(Bp=Bp, H=H, V=GATES_V, table=table, gh_splits=gh_splits, gi_splits=gi_splits, slab=slab,
                  Gh=slabs(gh_splits), hprev=torch.rand(Bp, H, generator=g) * 2 - 1,
                  bgh=(torch.rand(3 * H, generator=g) * 2 - 1) if bias else None,
                  bgi=(torch.rand(3 * H, generator=g) * 2 - 1) if bias else None)
    if table:
        d["P"] = torch.rand(GATES_V, 3 * H, generator=g) * 4 - 2
        ids = torch.randint(0, GATES_V, (Bp,), generator=g, dtype=torch.int32)
        if Bp > 1:
            ids[0], ids[-1] = 0, GATES_V - 1
        if bad_ids:
            ids[min(1, Bp - 1)], ids[Bp // 2 + 1 if Bp > 2 else 0] = -1, GATES_V
        d["ids"] = ids
    else:
        d["Gi"] = slabs(gi_splits)
    return d


def _gates_pre(d: Out, dt):
    Bp, H = d["Bp"], d["H"]
    row = Bp * 3 * H

    def total(t, b):
        acc = t[0, :row].to(dt)
        for s in range(1, t.shape[0]):
            acc = acc + t[s, :row].to(dt)                      # slab order
        acc = acc.reshape(Bp, 3 * H)
        return acc if b is None else acc + b.to(dt)

    gh = total(d["Gh"], d["bgh"])
    if d["table"]:
        ids = d["ids"].long()
        ids = torch.where((ids < 0) | (ids >= d["V"]), torch.zeros_like(ids), ids)    # an invalid id reads row 0
        gi = d["P"].to(dt)[ids]                                # the table holds b_ih already: bgi is not added
    else:
        gi = total(d["Gi"], d["bgi"])
    return gi, gh


def gates_ref(d: Out) -> torch.Tensor:
    gi, gh = _gates_pre(d, torch.float64)
    return _gate_math(gi, gh, d["hprev"].double(), True)


def gates_emulate(d: Out) -> torch.Tensor:
    gi, gh = _gates_pre(d, torch.float32)
    return _gate_math(gi, gh, d["hprev"], False)


def bf16_bits(x: torch.Tensor) -> torch.Tensor:
    """Round-to-nearest-even bf16 words (int32 values 0 .. 65535) of fp32 x."""
    return x.float().bfloat16().view(torch.int16).to(torch.int32) & 0xFFFF


def hsplit_of(h: torch.Tensor) -> torch.Tensor:
    """[Bp][3H] bf16 words [hi | hi | lo] of fp32 h: hi = bf16(h), lo = bf16(h - hi)."""
    hi = h.float().bfloat16()
    lo = (h.float() - hi.float()).bfloat16()
    return torch.cat([bf16_bits(hi.float()), bf16_bits(hi.float()), bf16_bits(lo.float())], 1)


# ------------------------------------------------------------------------------ scorer
def score_prep_ref(rows: np.ndarray, N: int, Bp: int, ML: int, V: int, sos: int, eos: int):
    """score_prep, exactly: ids / tgt [ML][Bp], n_tok [Bp], and whether the error bit is set.  A byte >= V
    at a scored position is clamped to 0 (as target and as the next input)."""
    ids = np.full((ML, Bp), sos, np.int32)
    tgt = np.full((ML, Bp), -1, np.int32)
    ntok = np.zeros(Bp, np.int32)
    bad = False
    for b in range(N):
        c = rows[b]
        nt = ML
        for l in range(ML):
            if c[l] == eos:
                nt = l + 1
                break
        prev = sos
        for l in range(nt):
            t = int(c[l])
            if t >= V:
                bad, t = True, 0
            ids[l, b], tgt[l, b] = prev, t
            prev = t
        ntok[b] = nt
    return ids, tgt, ntok, bad


SCORE_V = [64, 192, 256, 512]


def score_inputs(V: int, ML: int, Bp: int, splits: int, bias: bool, seed: int = 0) -> Out:
    """Planted logits [splits][ML Bp V (+ gap)] (row l Bp + b), targets and n_tok for score_logprob.
    Name b: n_tok cycles through 0, 1, ML and others.  Token (l, b) by (l + b) % 6: 0 random logits;
    1 the target has the row maximum; 2 the minimum; 3 exact ties with the target at a lower and a
    higher index; 4 every logit equal; 5 a +12 spike off the target.  All slabs but the first hold
    multiples of 1/8 so the slab sum is exact where the rank rule needs exact ties."""
    g = torch.Generator(device="cpu").manual_seed(13000 + seed + V + ML)
    rows = ML * Bp
    slab = rows * V + 40
    lg = torch.full((splits, slab), float("nan"))
    base = (torch.randint(-64, 64, (rows, V), generator=g).float() / 8.0)
    tgt = torch.randint(0, V, (ML, Bp), generator=g, dtype=torch.int32)
    ntok = torch.tensor([(0, 1, ML, max(ML // 2, 1), ML, min(2, ML))[b % 6] for b in range(Bp)], dtype=torch.int32)
    b_vec = (torch.randint(-16, 16, (V,), generator=g).float() / 8.0) if bias else None
    for l in range(ML):
        for b in range(Bp):
            r, t, k = l * Bp + b, int(tgt[l, b]), (l + b) % 6
            if k == 1:
                base[r, t] = 12.0
            elif k == 2:
                base[r, t] = -12.0
            elif k == 3:
                t = min(max(t, 1), V - 2)
                tgt[l, b] = t
                base[r, t - 1] = base[r, t + 1] = base[r, (t + 7) % V] = base[r, t]
            elif k == 4:
                base[r] = 1.5
            elif k == 5:
                base[r, (t + 3) % V] = 12.0
            if l >= int(ntok[b]):
                tgt[l, b] = -1 if (l + b) % 2 else 0              # masked positions: either value, never read
    # ties must survive the bias: planted on the biased sum
    total = base.clone()
    if bias:
        for l in range(ML):
            for b in range(Bp):
                if (l + b) % 6 in (3, 4):
                    total[l * Bp + b] -= b_vec
    for l in range(ML):
        for b in range(Bp):
            if l >= int(ntok[b]):
                total[l * Bp + b] = float("nan")                  # rows of masked tokens are not read
    parts = [torch.randint(-32, 32, (rows, V), generator=g).float() / 8.0 for _ in range(splits - 1)]
    first = total - sum(parts) if parts else total
    lg[0, :rows * V] = first.reshape(-1)
    for s, p in enumerate(parts):
        lg[s + 1, :rows * V] = p.reshape(-1)
    return dict(V=V, ML=ML, Bp=Bp, splits=splits, slab=slab, logits=lg, bias=b_vec, tgt=tgt, ntok=ntok)


def _score(d: Out, f64: bool):
    V, ML, Bp = d["V"], d["ML"], d["Bp"]
    dt = torch.float64 if f64 else torch.float32
    rows = ML * Bp
    x = d["logits"][0, :rows * V].to(dt)
    for s in range(1, d["splits"]):
        x = x + d["logits"][s, :rows * V].to(dt)
    x = x.reshape(ML, Bp, V)
    if d["bias"] is not None:
        x = x + d["bias"].to(dt)
    ntok = d["ntok"].clamp(0, ML)
    mask = torch.arange(ML)[:, None] < ntok[None, :]
    t = d["tgt"].long().clamp(0, V - 1)
    x = torch.where(mask[..., None], x, torch.zeros_like(x))      # rows of masked tokens are not read (NaN-safe)
    xt = x.gather(-1, t[..., None])
    mx = x.max(-1, keepdim=True).values
    if f64:
        lp = (xt - mx).squeeze(-1) - torch.log(torch.exp(x - mx).sum(-1))
    else:
        se = _exp32(x - mx).double().sum(-1).float()
        lp = (xt - mx).squeeze(-1) - torch.log(se.double()).float()
    j = torch.arange(V).view(1, 1, -1)
    rank = ((x > xt) | ((x == xt) & (j < t[..., None]))).sum(-1)
    lp = torch.where(mask, lp, torch.zeros_like(lp))
    rank = torch.where(mask, rank, torch.full_like(rank, -1))
    name = torch.zeros(Bp, dtype=dt)
    for l in range(ML):
        name = name + lp[l]                                      # step order
    return lp.T.contiguous(), name, rank.T.contiguous().to(torch.int32), ntok.to(torch.int32)


def score_ref(d: Out):
    """float64 (tok_logp [Bp][ML], name_logp [Bp], rank [Bp][ML], n_tok [Bp]) from the given logits."""
    return _score(d, True)


def score_emulate(d: Out):
    return _score(d, False)


SCORE_CASES = [(64, 1, 6, 1, False), (192, 10, 7, 3, True), (256, 10, 6, 1, True), (256, 64, 6, 3, False),
               (512, 10, 7, 1, False), (512, 64, 6, 3, True)]     # (V, ML, Bp, splits, bias)


def gates_cases():
    """(Bp, H, table, gh_splits, gi_splits, bias) of the gates test: every shape on both paths, splits 1
    and 3, biases null and set."""
    return [(Bp, H, table, ghs, gis, bias) for Bp, H in GATES_SHAPES for table in (True, False)
            for ghs, gis, bias in ((1, 1, False), (3, 3, True), (3, 1, False), (1, 3, True))]


# ------------------------------------------------------------------------------ measurement
def case_deviation(c: Case, seed: int = 0, mut: Optional[str] = None) -> Dict[str, float]:
    d = case_inputs(c, seed)
    orc = plant_uniforms(d, case_plan(c))
    emu = emulate(d, orc["rf"], mut)
    T = chars_run(orc["alive_after"], c.ML, c.probs)
    st = emu["states"].numpy()
    rs, rl = step_ref(d, st, orc["ids_in"], T)
    hit = torch.from_numpy(np.arange(c.ML)[:, None, None] < T)
    return dict(state=deviation(st[:, :T], rs),
                logit=deviation(emu["logits"][:T], rl),
                probs=deviation(emu["probs_last"], orc["probs_last"]),
                cdf=float(((emu["cdf"].double() - orc["cdf"]).abs() * hit).max()),
                rows_equal=float(np.array_equal(emu["out"], orc["out"]) and np.array_equal(emu["sampled"], orc["sampled"])))


def measure_deviations(seeds=(0, 1, 2), verbose: bool = False) -> Dict[str, float]:
    """Largest deviation per family over every case of tests/test_gen_gpu.py and ``seeds``."""
    out: Dict[str, float] = {k: 0.0 for k in MEASURED_DEV}
    for c in sorted(PERSIST_CASES, key=lambda c: (c.H, c.L, c.V, c.seed_off)):
        for seed in seeds:
            dev = case_deviation(c, seed)
            assert dev.pop("rows_equal") == 1.0, f"{c.name} seed {seed}: the emulator's rows differ from the oracle's"
            for k, v in dev.items():
                out[k] = max(out[k], v)
            if verbose:
                print(c.name, seed, {k: f"{v:.3e}" for k, v in dev.items()}, flush=True)
    for seed in seeds:
        for a in gates_cases():
            d = gates_inputs(*a, seed=seed)
            out["gates"] = max(out["gates"], deviation(gates_emulate(d), gates_ref(d)))
        for a in SCORE_CASES:
            d = score_inputs(*a, seed=seed)
            e, r = score_emulate(d), score_ref(d)
            out["logp"] = max(out["logp"], deviation(e[0], r[0]))
            out["name_logp"] = max(out["name_logp"], deviation(e[1], r[1]))
            assert torch.equal(e[2], r[2]) and torch.equal(e[3], r[3])
    return out


if __name__ == "__main__":
    res = measure_deviations(verbose=True)
    for k in MEASURED_DEV:
        print(f'    "{k}": {res[k]:.3e},')

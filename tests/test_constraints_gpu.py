"""Constrained names on the device (docs/DESIGN.md §4e): the MASK instantiations of sample_ctl_f32 and
beam_select_f32 against the fp64 rule on planted inputs, and HipGenerator.generate / beam_search with
constraints against the fp64 oracles.  The helpers, tolerances and clearances are those of
tests/test_sampling_ctl_gpu.py and tests/test_beam_gpu.py (masking only replaces terms by exact zeros,
so their bounds hold)."""
import string

import numpy as np
import pytest
import torch

import test_sampling_ctl_gpu as sc
from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import beam_ref as br
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.utils.data import random_floats

gpu = pytest.mark.gpu
DEV = "cuda"
ML, STEP, EOS = sc.ML, sc.STEP, sc.EOS
LETTERS, LOWER = string.ascii_letters, string.ascii_lowercase


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stream():
    return torch.cuda.current_stream().cuda_stream


def pack(sets):
    """bool [M, V] -> uint32 [M, V / 32]: bit c % 32 of word c / 32."""
    M, V = sets.shape
    w = (sets.reshape(M, V // 32, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1)
    return w.astype(np.uint32)


def table_of(per_row):
    """Rows' sets bool [R, V] -> (tab uint32 [M, V / 32] with line 0 all ones and distinct lines, line [R])."""
    V = per_row.shape[1]
    lines = {np.ones(V, bool).tobytes(): 0}
    idx = np.array([lines.setdefault(s.tobytes(), len(lines)) for s in per_row], np.int32)
    return pack(np.stack([np.frombuffer(k, bool) for k in lines])), idx


# ------------------------------------------------------------------------------- sample_ctl_f32
KINDS = ("no_argmax", "below_k", "singleton", "one_lane", "low_top", "free")
CTLS = [(0, 1.0, 1.0), (5, 1.0, 1.0), (2, 0.9, 0.5), (0, 0.5, 2.0), (7, 1.0, 0.0), (0, 1.0, 0.0), (5, 0.5, 1.0)]   # (k, p, T)


def mask_of(kind, x, rng):
    """One row's allowed set.  below_k: 3 chars (every active k of CTLS but 2 is above it); one_lane: the
    V / 64 consecutive chars of one lane; low_top: a random fifth of the lower three quarters of the
    indices, cut off above its most probable char -- the highest allowed index then carries at least
    1 / |A| of the mass, so an fp32 running sum stays far below 1 before it and r = 1.0 falls through
    every earlier index in any precision."""
    V = len(x)
    per = V // 64
    a = np.zeros(V, bool)
    if kind == "no_argmax":
        a[:] = True
        a[int(np.argmax(x))] = False
    elif kind == "below_k":
        a[rng.choice(V, 3, replace=False)] = True
    elif kind == "singleton":
        a[rng.integers(0, V)] = True
    elif kind == "one_lane":
        lane = int(rng.integers(0, 64))
        a[lane * per:(lane + 1) * per] = True
    elif kind == "low_top":
        a[:3 * V // 4] = rng.random(3 * V // 4) < 0.2
        a[rng.integers(0, 3 * V // 4)] = True
        a[int(np.argmax(np.where(a, x, -np.inf))) + 1:] = False
    else:
        a[:] = True
    return a


def clear_top_p(x64, T, k, p, A):
    """sc.clear_top_p inside the allowed sets: an active top-p within 1e-4 of a cumulative mass of the
    sorted post-top-k softmax (fp64) moves to the midpoint of the gap it falls in."""
    p = np.asarray(p, np.float32).copy()
    for i in range(x64.shape[0]):
        if T[i] == 0 or p[i] >= 1:
            continue
        q = cpu_ref.filter_probs(x64[i], float(T[i]), int(k[i]), 1.0, allowed=A[i]).numpy()
        c = np.cumsum(np.sort(q[q > 0])[::-1])
        if np.abs(c - float(p[i])).min() < 1e-4:
            j = int(np.searchsorted(c, float(p[i])))
            lo, hi = (c[j - 1] if j > 0 else 0.0), c[min(j, len(c) - 1)]
            p[i] = np.float32(0.5 * (lo + hi))
        assert np.abs(c - float(p[i])).min() >= 1e-4 and 0 < p[i] <= 1, (i, p[i])
    return p


def launch(ext, x_buf, bias, R, V, slabs, r, ctl, tab=None, idx=None, rows=None, row0=0, alive=None):
    """sc.launch with the constraint keys: tab uint32 [M, V / 32], idx int32 [row0 + R, ML]."""
    lg = t(x_buf)
    rf = np.zeros((R, ML), np.float32)
    rf[:, STEP] = r
    rf = t(rf)
    ids = torch.full((R,), -1, dtype=torch.int32, device=DEV)
    out = torch.full((R, ML + 1), 7, dtype=torch.uint8, device=DEV)
    al = t(np.ones(R, np.int32) if alive is None else alive.astype(np.int32))
    probs = torch.full((R, V), -1.0, device=DEV)
    err = torch.zeros(4, dtype=torch.int32, device=DEV)
    cd = [t(a) for a in ctl]
    d = dict(logits=lg.data_ptr(), splits=slabs, slab=R * V, rf=rf.data_ptr(), ids=ids.data_ptr(), out=out.data_ptr(),
             alive=al.data_ptr(), N=R, V=V, step=STEP, max_len=ML, eos=EOS, probs=probs.data_ptr(),
             inv_temp=cd[0].data_ptr(), top_k=cd[1].data_ptr(), top_p=cd[2].data_ptr(), plen=cd[3].data_ptr(),
             prefix=cd[4].data_ptr(), row0=row0, err=err.data_ptr())
    keep = [lg, rf, cd]
    if bias is not None:
        b = t(bias)
        keep.append(b)
        d["bias"] = b.data_ptr()
    if tab is not None:
        dt, di = t(tab.view(np.int32)), t(idx)
        keep += [dt, di]
        d.update(allow_tab=dt.data_ptr(), allow_idx=di.data_ptr(), allow_rows=tab.shape[0] if rows is None else rows)
    ext.sample_ctl(d, stream())
    torch.cuda.synchronize()
    return ids.cpu().numpy(), out.cpu().numpy(), al.cpu().numpy(), probs.cpu().numpy(), err.cpu().numpy()


def idx_of(line, row0, R, filler):
    """[row0 + R, ML]: the rows' lines at STEP; every other entry (other steps, the rows before row0)
    names ``filler``, a line that would change every result."""
    idx = np.full((row0 + R, ML), filler, np.int32)
    idx[row0:, STEP] = line
    return idx


@gpu
@pytest.mark.parametrize("late_bias", [False, True])
@pytest.mark.parametrize("slabs", [1, 2])
@pytest.mark.parametrize("R", [1, 3, 70])
@pytest.mark.parametrize("V", [64, 256, 512])
def test_sample_ctl_masked_kept_set_probs_and_choice(ext, V, R, slabs, late_bias):
    """Every kind of mask x a mixture of (k, p, T) per row: the kept set exactly the fp64 one, masked
    chars at probability exactly 0, probabilities at the unmasked kernel's fp32 bar, the chosen index
    exact (r = 1.5 rows, and r = 1.0 on the low_top rows: the highest kept index inside the set), forced
    rows, dead rows, row0 > 0."""
    x, buf, bias = sc.make_logits(V, R, slabs, late_bias, seed=2 * V + 7 * R + slabs)
    x64 = torch.from_numpy(x).double()
    rng = np.random.default_rng(V + R)
    cells = [(kd, c) for kd in KINDS for c in CTLS]                      # 42
    for j in range(-(-len(cells) // R)):
        mine = [cells[(j * R + i) % len(cells)] for i in range(R)]
        A = np.stack([mask_of(m[0], x[i], rng) for i, m in enumerate(mine)])
        k = np.array([m[1][0] for m in mine], np.int32)
        T = np.array([m[1][2] for m in mine], np.float64)
        p = clear_top_p(x64, T, k, np.array([m[1][1] for m in mine], np.float32), A)
        ctl = cpu_ref.make_controls(GRUConfig(vocab=V, max_len=ML, eos=EOS), R, T, k, p)
        forced = (np.arange(R) + j) % 9 == 8
        plen = np.where(forced, STEP + 1, np.arange(R) % (STEP + 1)).astype(np.int32)
        pre = ((np.arange(R)[:, None] * 7 + np.arange(ML)[None, :] * 3 + j) % V).astype(np.uint8)
        alive = (np.arange(R) + j) % 4 != 3
        want = cpu_ref.filter_probs(x64, T, k, p, allowed=A).numpy()
        want[forced] = np.eye(V)[pre[forced, STEP]]                      # a forced step reads no mask
        r = rng.random(R, dtype=np.float32)
        r[(np.arange(R) + j) % 3 == 2] = 1.5                             # past every CDF
        r[np.array([m[0] == "low_top" for m in mine]) & ((np.arange(R) + j) % 3 == 1)] = 1.0
        r, sel = sc.clear_uniforms(want, r)
        free = ~forced
        top = V - 1 - A[:, ::-1].argmax(1)
        past = free & (r >= 1) & (T != 0)
        assert A[free, sel[free]].all() and (sel[past] <= top[past]).all()      # the oracle itself stays inside
        row0 = 5 if j % 2 else 0
        tab, line = table_of(A)
        filler = int(line[np.argmax([m[0] == "singleton" for m in mine])]) if tab.shape[0] > 1 else 0
        arrs = sc.pad_ctl((ctl.inv_temp, ctl.top_k, ctl.top_p, plen, pre), row0)
        ids, out, al, probs, err = launch(ext, buf, bias, R, V, slabs, r, arrs, tab, idx_of(line, row0, R, filler),
                                          row0=row0, alive=alive)
        assert err[0] == 0
        assert (probs[free][~A[free]] == 0).all()                        # exactly 0, no tolerance
        assert ((probs > 0) == (want > 0)).all(), (j, np.argwhere((probs > 0) != (want > 0))[:4])
        torch.testing.assert_close(torch.from_numpy(probs).double(), torch.from_numpy(want), atol=2e-7, rtol=1e-5)
        assert (ids == sel).all(), (j, np.argwhere(ids != sel)[:4], [mine[i] for i in np.flatnonzero(ids != sel)[:4]])
        assert (out[:, STEP] == np.where(alive, sel & 255, 7)).all()
        assert (np.delete(out, STEP, 1) == 7).all()
        assert (al == (alive & (sel != EOS))).all()


@gpu
@pytest.mark.parametrize("V,R", [(64, 3), (256, 70), (512, 70)])
def test_sample_ctl_low_top_fallback_is_the_highest_allowed_index(ext, V, R):
    """r = 1.0 with nothing else filtered: the highest allowed index, which lies below V - 1."""
    x, buf, bias = sc.make_logits(V, R, 1, False, seed=V)
    rng = np.random.default_rng(V)
    A = np.stack([mask_of("low_top", x[i], rng) for i in range(R)])
    ctl = cpu_ref.make_controls(GRUConfig(vocab=V, max_len=ML, eos=EOS), R, 1.0, 0, 1.0)
    tab, line = table_of(A)
    arrs = (ctl.inv_temp, ctl.top_k, ctl.top_p, ctl.plen, ctl.prefix)
    ids, _, _, probs, err = launch(ext, buf, bias, R, V, 1, np.ones(R, np.float32), arrs, tab, idx_of(line, 0, R, 0))
    top = V - 1 - A[:, ::-1].argmax(1)
    assert err[0] == 0 and (ids == top).all() and (top < 3 * V // 4).all() and (probs[~A] == 0).all()


@gpu
@pytest.mark.parametrize("late_bias", [False, True])
@pytest.mark.parametrize("slabs", [1, 2])
@pytest.mark.parametrize("V,R", [(64, 3), (256, 1), (256, 70), (512, 70), (128, 3)])
def test_sample_ctl_line_zero_only_is_bitwise_the_unmasked_launch(ext, V, R, slabs, late_bias):
    x, buf, bias = sc.make_logits(V, R, slabs, late_bias, seed=3 * V + R)
    rng = np.random.default_rng(V)
    r = rng.random(R, dtype=np.float32)
    r[::4] = 1.5
    alive = np.arange(R) % 3 != 1
    cells = [CTLS[i % len(CTLS)] for i in range(R)]
    ctl = cpu_ref.make_controls(GRUConfig(vocab=V, max_len=ML, eos=EOS), R, [c[2] for c in cells], [c[0] for c in cells],
                                [c[1] for c in cells])
    plen = (np.arange(R) % 5 == 4).astype(np.int32) * (STEP + 1)
    pre = np.full((R, ML), 9, np.uint8)
    arrs = sc.pad_ctl((ctl.inv_temp, ctl.top_k, ctl.top_p, plen, pre), 5)
    tab = np.full((1, V // 32), 0xFFFFFFFF, np.uint32)
    a = launch(ext, buf, bias, R, V, slabs, r, arrs, tab, np.zeros((5 + R, ML), np.int32), row0=5, alive=alive)
    b = sc.launch(ext, buf, bias, R, V, slabs, r, arrs, row0=5, alive=alive)
    for u, v in zip(a, b):           # ids, out, alive, probs, err
        assert (u.view(np.uint8) == v.view(np.uint8)).all()


@gpu
def test_sample_ctl_flags_an_idx_entry_outside_the_table(ext):
    V, R = 256, 3
    x, buf, bias = sc.make_logits(V, R, 1, False, seed=1)
    rng = np.random.default_rng(0)
    A = np.stack([mask_of("below_k", x[i], rng) for i in range(R)])
    tab, line = table_of(A)
    ctl = cpu_ref.make_controls(GRUConfig(vocab=V, max_len=ML, eos=EOS), R, 1.0, 0, 1.0)
    arrs = (ctl.inv_temp, ctl.top_k, ctl.top_p, ctl.plen, ctl.prefix)
    r = np.full(R, 0.5, np.float32)
    for bad in (tab.shape[0], -1, 1 << 20):
        idx = idx_of(line, 0, R, 0)
        idx[1, STEP] = bad
        ids, _, _, probs, err = launch(ext, buf, bias, R, V, 1, r, arrs, tab, idx)
        assert err[0] == 16 and err[1] == np.int32(bad) and err[2] == 1 and err[3] == 0
        ok = idx.copy()
        ok[1, STEP] = 0                                              # ... and the row takes line 0
        ids0, _, _, probs0, err0 = launch(ext, buf, bias, R, V, 1, r, arrs, tab, ok)
        assert err0[0] == 0 and (ids == ids0).all() and (probs.view(np.uint32) == probs0.view(np.uint32)).all()
        assert (probs[1] > 0).all() and (probs[0] > 0).sum() == 3
    # a table shorter than the lines in use: allow_rows is the bound, not the buffer
    idx = idx_of(line, 0, R, 0)
    _, _, _, _, err = launch(ext, buf, bias, R, V, 1, r, arrs, tab, idx, rows=int(line.max()))
    assert err[0] == 16 and err[1] == line.max()


@gpu
def test_sample_ctl_rejects_half_a_constraint_and_odd_vocabularies(ext):
    V, R = 192, 2                      # V / 64 = 3 chars per lane straddle a word
    x, buf, bias = sc.make_logits(V, R, 1, False, seed=1)
    ctl = cpu_ref.make_controls(GRUConfig(vocab=V, max_len=ML, eos=EOS), R, 1.0, 0, 1.0)
    arrs = (ctl.inv_temp, ctl.top_k, ctl.top_p, ctl.plen, ctl.prefix)
    tab = np.full((1, V // 32), 0xFFFFFFFF, np.uint32)
    with pytest.raises(RuntimeError):
        launch(ext, buf, bias, R, V, 1, np.full(R, 0.5, np.float32), arrs, tab, np.zeros((R, ML), np.int32))
    z = torch.zeros(4096, dtype=torch.int32, device=DEV)
    base = dict(logits=z.data_ptr(), rf=z.data_ptr(), ids=z.data_ptr(), out=z.data_ptr(), alive=z.data_ptr(), N=1, V=64,
                step=0, max_len=4, eos=0, inv_temp=z.data_ptr(), top_k=z.data_ptr(), top_p=z.data_ptr(), plen=z.data_ptr(),
                prefix=z.data_ptr())
    for bad in (dict(allow_tab=z.data_ptr()), dict(allow_idx=z.data_ptr()),
                dict(allow_tab=z.data_ptr(), allow_idx=z.data_ptr(), allow_rows=0)):
        with pytest.raises(RuntimeError):
            ext.sample_ctl(dict(base, **bad), stream())


# ------------------------------------------------------------------------------- beam_select_f32
def select_cases():
    out = []
    i = 0
    for V in (64, 256):
        for W in (1, 4, 17, 32):
            for mode, states in (("free", "mix"), ("mixed", "live"), ("free", "step0"), ("forced", "mix")):
                out.append(br.StepCase(V, W, 3, 1 + i % 2, i % 3 == 1, mode, states, (5, 0)[i % 2]))
                i += 1
    return out


SELECT_CASES = select_cases()


def masked_step(c, seed):
    """br.step_inputs plus one allowed set per name: name 0 two chars (with step0 states: fewer candidates
    than W > 2, dead slots), name 1 a random half, name 2 everything.  Char 0 -- the carries' flat index
    -- is masked in names 0 and 1, and a forced char is inside its name's set."""
    d = br.step_inputs(c, seed)
    rng = np.random.default_rng(seed + 31 * c.V + c.W)
    A = np.zeros((c.N, c.V), bool)
    A[0, rng.choice(np.arange(1, c.V), 2, replace=False)] = True
    A[1, 1:] = rng.random(c.V - 1) < 0.5
    A[2] = True
    for n in range(c.N):
        if d["step"] < d["plen"][n]:
            A[n, int(d["prefix"][n, d["step"]])] = True
    assert not A[0, 0] and not A[1, 0] or c.mode != "free"
    d["allowed"] = A
    return d


def run_select(ext, d, tab=None, idx=None, rows=None):
    """tests/test_beam_gpu.py: run_select, with the constraint keys."""
    R, V, W, N = d["R"], d["V"], d["W"], d["N"]
    lg, scr, st = t(d["logits"]), t(d["score"]), t(d["state"])
    pl, pre = t(d["plen"]), t(d["prefix"])
    out_f = torch.full((R + 3,), float("nan"), device=DEV)
    outs = {k: torch.full((R + 3,), -77, dtype=torch.int32, device=DEV) for k in ("parent", "chr", "state_out", "next_id", "sel")}
    lp = torch.full((R + 3, V), float("nan"), device=DEV)
    err = torch.zeros(4, dtype=torch.int32, device=DEV)
    a = dict(logits=lg.data_ptr(), splits=d["splits"], slab=d["Rp"] * V, score_in=scr.data_ptr(), state_in=st.data_ptr(),
             plen=pl.data_ptr(), prefix=pre.data_ptr(), score_out=out_f.data_ptr(), err=err.data_ptr(), lp=lp.data_ptr(),
             N=N, W=W, V=V, step=d["step"], max_len=d["ML"], sos=d["sos"], eos=d["eos"],
             **{k: v.data_ptr() for k, v in outs.items()})
    keep = [lg, scr, st, pl, pre]
    if d["bias"] is not None:
        b = t(d["bias"])
        keep.append(b)
        a["bias"] = b.data_ptr()
    if tab is not None:
        dt, di = t(tab.view(np.int32)), t(idx)
        keep += [dt, di]
        a.update(allow_tab=dt.data_ptr(), allow_idx=di.data_ptr(), allow_rows=tab.shape[0] if rows is None else rows)
    ext.beam_select(a, stream())
    torch.cuda.synchronize()
    return dict(score=out_f.cpu().numpy(), parent=outs["parent"].cpu().numpy(), chr=outs["chr"].cpu().numpy(),
                state=outs["state_out"].cpu().numpy(), next_id=outs["next_id"].cpu().numpy(), sel=outs["sel"].cpu().numpy(),
                lp=lp.cpu().numpy(), err=err.cpu().numpy())


def step_idx(d, line, filler=0):
    idx = np.full((d["N"], d["ML"]), filler, np.int32)
    idx[:, d["step"]] = line
    return idx


@pytest.mark.parametrize("i", range(len(SELECT_CASES)), ids=lambda i: "-".join(map(str, SELECT_CASES[i])))
def test_masked_select_inputs_clear_the_guard(i):
    """The condition of the GPU test below, on the CPU: the planter clears every name's first W + 1
    candidates (it asserts that at most one name of the launch had to be moved)."""
    d = br.plant_step(masked_step(SELECT_CASES[i], i % 3))
    ref = br.select_ref(d)
    assert (ref["clear"] >= br.GUARD).all()
    A, W, V = d["allowed"], d["W"], d["V"]
    for n in range(d["N"]):
        for k in range(W):
            j = int(ref["sel"][n * W + k])
            if j >= 0 and ref["chr"][n * W + k] >= 0:
                assert A[n, j % V]                                   # every extension lies inside the set
    if SELECT_CASES[i].states == "mix" and W > 1:                    # a carry (flat index b V: char 0) under a mask without char 0
        carried = (ref["chr"] < 0) & (ref["parent"] >= 0)
        assert carried[:2 * W].any() or not (d["state"][:2 * W] == br.FIN).any()


@gpu
@pytest.mark.parametrize("i", range(len(SELECT_CASES)), ids=lambda i: "-".join(map(str, SELECT_CASES[i])))
def test_masked_select_matches_fp64_rule(ext, i):
    c = SELECT_CASES[i]
    d = br.plant_step(masked_step(c, i % 3))
    ref = br.select_ref(d)
    tab, line = table_of(d["allowed"])
    got = run_select(ext, d, tab, step_idx(d, line, filler=int(line[0])))
    R = d["R"]
    own = {k: (v[:R] if k != "err" else v) for k, v in got.items()}
    assert br.check_step(ref, own) == []
    assert (got["err"] == 0).all()
    assert np.isnan(got["score"][R:]).all() and all((got[k][R:] == -77).all() for k in ("parent", "chr", "state", "next_id", "sel"))
    if c.states == "step0" and c.mode == "free" and c.W > 4:
        # name 0: two allowed chars, live beams 0 and 2 (a planted copy of 0): 4 candidates, then dead slots
        assert (own["parent"][:c.W] >= 0).sum() == 4 and (own["state"][4:c.W] == br.DEAD).all()
        assert np.isneginf(own["score"][4:c.W]).all() and (own["sel"][4:c.W] == -1).all()


@gpu
@pytest.mark.parametrize("i", [0, 5, 10, 15, 18, 23, 28, 31], ids=lambda i: "-".join(map(str, SELECT_CASES[i])))
def test_select_line_zero_only_is_bitwise_the_unmasked_launch(ext, i):
    d = br.step_inputs(SELECT_CASES[i], i % 3)
    tab = np.full((1, d["V"] // 32), 0xFFFFFFFF, np.uint32)
    a = run_select(ext, d, tab, np.zeros((d["N"], d["ML"]), np.int32))
    b = run_select(ext, d)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


@gpu
def test_select_flags_an_idx_entry_outside_the_table(ext):
    c = br.StepCase(64, 3, 3, 1, False, "free", "live", 5)
    d = masked_step(c, 1)
    tab, line = table_of(d["allowed"])
    for bad in (tab.shape[0], -3):
        idx = step_idx(d, line)
        idx[1, d["step"]] = bad
        got = run_select(ext, d, tab, idx)
        assert got["err"][0] == 16 and got["err"][1] == np.int32(bad) and got["err"][2] == 1 * c.W and got["err"][3] == 0
        free = d["allowed"].copy()
        free[1] = True                                               # the name takes line 0
        ref = br.select_ref(dict(d, allowed=free))
        assert br.check_step(ref, {k: got[k][:d["R"]] for k in ("score", "parent", "chr", "state", "next_id", "sel", "lp")}) == []
    z = torch.zeros(64, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):                                # half a constraint
        ext.beam_select(dict(logits=z.data_ptr(), score_in=z.data_ptr(), state_in=z.data_ptr(), plen=z.data_ptr(),
                             prefix=z.data_ptr(), score_out=z.data_ptr() + 64, parent=z.data_ptr(), chr=z.data_ptr(),
                             state_out=z.data_ptr() + 64, next_id=z.data_ptr(), N=1, W=2, V=64, step=0, max_len=4, sos=1,
                             eos=0, allow_tab=z.data_ptr()), stream())


# ------------------------------------------------------------------------------- HipGenerator.generate
CFG = sc.CFG          # GRUConfig(vocab=256, embed=128, hidden=256, layers=2, max_len=10)
BAR = sc.BAR
PATS = ["M[aeiou].", "[A-Z][a-z]", None, "[^aeiou]"]
SETS = [LETTERS, LETTERS + "-'", None, LOWER]
MINS, MAXS = [4, 2, None, 3], [7, 9, None, 5]


def mixture(N, shift=0):
    """make_constraints keywords of N names, name n of kind (n + n // 64 + shift) % 4: the kind depends
    on the 64-name batch as well, so a batch that read rows 0.. would follow another name's constraint."""
    kind = [(n + n // 64 + shift) % 4 for n in range(N)]
    return dict(pattern=[PATS[k] for k in kind], charset=[SETS[k] for k in kind], min_len=[MINS[k] for k in kind],
                max_len=[MAXS[k] for k in kind])


def obeys(row, sets, eos=0):
    for l, ch in enumerate(row[:len(sets)]):
        if not sets[l][ch]:
            return False
        if ch == eos:
            return True
    return True


def all_obey(rows, cons):
    a = cons.allowed()
    return all(obeys(rows[n], a[n]) for n in range(len(rows)))


@gpu
def test_generate_small_batch_takes_the_per_char_graph_and_obeys():
    N = 40
    rf = random_floats(N, CFG.max_len, seed=9)
    gen = sc.make_gen()
    assert gen.g.uses_persist_ctl(N)                     # 40 names with controls alone: the persistent launch
    before = gen.generate(rf)
    before_ctl = gen.generate(rf, temperature=0.7, prefix="Jo")
    assert gen.g.ctl_workspace_bytes() == 0 and gen.g.ctl_graphs() == 0
    cons = cpu_ref.make_constraints(CFG, N, **mixture(N))
    got = gen.generate(rf, constraints=cons)
    assert gen.g.read_error() == 0
    assert gen.g.ctl_graphs() == 1 and gen.g.ctl_workspace_bytes() > 0      # ... with a constraint: the per-char graph
    assert all_obey(got, cons)
    want = sc.oracle(("cons40", 0), False, rf, constraints=mixture(N))
    print("40 constrained names identical to the fp64 oracle:", sc.same(got, want))
    # the dict form, and controls on top
    assert (gen.generate(rf, constraints=mixture(N)) == got).all()
    mix = gen.generate(rf, temperature=0.8, top_k=3, prefix="M", constraints=dict(pattern="M[aeiou]", charset=LETTERS, max_len=6))
    assert all_obey(mix, cpu_ref.make_constraints(CFG, N, pattern="M[aeiou]", charset=LETTERS, max_len=6))
    assert gen.g.ctl_graphs() == 2                       # (a table of another line count: a recording of its own)
    # an unconstrained call after a constrained one: the bytes it gave before, on the path it took before
    assert gen.g.uses_persist(N) and (gen.generate(rf) == before).all()
    assert (gen.generate(rf, temperature=0.7, prefix="Jo") == before_ctl).all() and gen.g.ctl_graphs() == 2
    assert gen.g.read_error() == 0


@gpu
def test_generate_1000_constrained_names_match_fp64_oracle():
    """The fp32 cpu_ref against the fp64 cpu_ref gives 1000 of 1000 identical names for this mixture at
    seed 9, with and without the controls, so the bar is reachable by fp32 arithmetic."""
    N = 1000
    rf = random_floats(N, CFG.max_len, seed=9)
    kw = mixture(N)
    cons = cpu_ref.make_constraints(CFG, N, **kw)
    gen = sc.make_gen()
    got = gen.generate(rf, constraints=cons)
    assert gen.g.read_error() == 0 and all_obey(got, cons)                 # 100 %, no tolerance
    s = sc.same(got, sc.oracle(("cons1000", 0), False, rf, constraints=kw))
    print("constrained names identical to the fp64 oracle:", s)
    assert s >= BAR
    ctl = dict(temperature=0.8, top_k=20, top_p=0.9)
    got = gen.generate(rf, constraints=cons, **ctl)
    assert all_obey(got, cons)
    s = sc.same(got, sc.oracle(("cons1000", 1), False, rf, constraints=kw, **ctl))
    print("constrained names with top-k / top-p / temperature identical to the fp64 oracle:", s)
    assert s >= BAR


@gpu
def test_generate_batches_read_their_own_constraints():
    """max_batch = 64, 150 names: three batches, the constraint kinds shifted at every batch boundary."""
    N = 150
    rf = random_floats(N, CFG.max_len, seed=13)
    cons = cpu_ref.make_constraints(CFG, N, **mixture(N))
    gen = sc.make_gen(max_batch=64)
    got = gen.generate(rf, constraints=cons)
    assert gen.g.read_error() == 0 and all_obey(got, cons)
    assert gen.g.ctl_graphs() == 2                                        # 64 and 22 names
    wrong = cpu_ref.make_constraints(CFG, N, **mixture(N, shift=1))
    assert not all_obey(got, wrong)
    want = sc.oracle(("cons150", 0), False, rf, constraints=mixture(N))
    # (150 names cannot express the 0.995 bar: they are held to it with the 1000-name test above)
    print("150 batched constrained names identical to the fp64 oracle:", sc.same(got, want))


@gpu
def test_generate_constraints_are_read_from_memory_not_captured():
    """Two constraints with the same number of table lines replay one graph; the outputs follow each."""
    N = 300
    rf = random_floats(N, CFG.max_len, seed=9)
    a_kw = dict(pattern="[A-M][aeiou]", charset=LETTERS, min_len=3, max_len=6)
    b_kw = dict(pattern="[N-Z][^aeiou]", charset=LOWER, min_len=4, max_len=5)
    a_c, b_c = cpu_ref.make_constraints(CFG, N, **a_kw), cpu_ref.make_constraints(CFG, N, **b_kw)
    assert a_c.rows == b_c.rows
    gen = sc.make_gen()
    a = gen.generate(rf, constraints=a_c)
    b = gen.generate(rf, constraints=b_c)
    a2 = gen.generate(rf, constraints=a_c)
    assert gen.g.read_error() == 0 and gen.g.ctl_graphs() == 1
    assert (a == a2).all() and not (a == b).all(1).any()
    assert all_obey(a, a_c) and all_obey(b, b_c) and not all_obey(a, b_c) and not all_obey(b, a_c)
    for nm, rows, kw in (("a", a, a_kw), ("b", b, b_kw)):
        print(f"constraint {nm}: names identical to the fp64 oracle:", sc.same(rows, sc.oracle(("mem", nm), False, rf, constraints=kw)))


@gpu
def test_generate_bf16x3_works_and_bf16_raises():
    N = 1000
    rf = random_floats(N, CFG.max_len, seed=9)
    kw = mixture(N)
    cons = cpu_ref.make_constraints(CFG, N, **kw)
    gen = sc.make_gen("bf16x3")
    got = gen.generate(rf, constraints=cons)
    assert gen.g.read_error() == 0 and all_obey(got, cons)
    s = sc.same(got, sc.oracle(("cons1000", 0), False, rf, constraints=kw))
    print("bf16x3 constrained names identical to the fp64 oracle:", s)
    assert s >= BAR
    fast = sc.make_gen("bf16")
    with pytest.raises(ValueError):
        fast.generate(rf[:16 * CFG.max_len], constraints=dict(charset=LETTERS))
    with pytest.raises(RuntimeError):
        z = torch.zeros(4096, dtype=torch.int32, device=DEV)
        fast.g.generate_ctl(z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(),
                            z.data_ptr(), stream(), z.data_ptr(), z.data_ptr(), 1)


@gpu
def test_generate_bad_constraints_raise_before_any_launch():
    rf = random_floats(16, CFG.max_len, seed=9)
    gen = sc.make_gen()
    for kw in (dict(constraints=dict(min_len=5, max_len=3)), dict(constraints=dict(pattern="[a")),
               dict(prefix="Mx", constraints=dict(pattern="M[aeiou]")),
               dict(constraints=cpu_ref.make_constraints(CFG, 15))):
        with pytest.raises(ValueError):
            gen.generate(rf, **kw)
    assert gen.g.ctl_workspace_bytes() == 0 and gen.g.ctl_graphs() == 0


# ------------------------------------------------------------------------------- HipGenerator.beam_search
BEAM_MODEL = next(x for x in br.TRAJ_CASES if x.name == "m-W8")       # V 256, E 128, H 256, L 2, ML 10, eos 0
BEAM_CASES = {
    "six-letter-Mar": (["Mar"], 4, dict(charset=LETTERS, min_len=6, max_len=6)),
    "one-W8": ([""], 8, dict(pattern="[A-Z][aeiou]", charset=LETTERS, min_len=4, max_len=7)),
    "len4-W4": (["", "a", "bc", "Zed", "q"], 4, dict(charset=LETTERS, min_len=4, max_len=4)),
    "mixed-W8": (["", "M", "Jo", "", "Ka"], 8,
                 dict(pattern=["[A-Z][a-z]", "M[aeiou]", None, "[^A-Z].", "Ka."], charset=[LETTERS, LOWER + "M", LETTERS, None, LOWER + "K"],
                      min_len=[3, 3, None, 2, 3], max_len=[7, 5, None, 4, 5])),
    "fewer-than-W": (["", "Ma"], 8, dict(pattern="M[ae][xy]", min_len=3, max_len=3)),
}
_orc = {}


def beam_oracle(name):
    if name not in _orc:
        cfg, p = br.case_model(BEAM_MODEL)
        pre, W, kw = BEAM_CASES[name]
        _orc[name] = br.oracle(p, cfg, pre, W, constraints=kw)
    return _orc[name]


@pytest.mark.parametrize("name", list(BEAM_CASES))
def test_beam_cases_are_settled_in_the_fp64_oracle(name):
    """A condition, not a measurement (as tests/test_beam_ref.py): the GPU test compares bytes on settled
    prefixes only, and at most one prefix in eight may be unsettled -- of 1 or 5 prefixes, none."""
    orc = beam_oracle(name)
    assert int((~orc["settled"]).sum()) * 8 <= len(BEAM_CASES[name][0]), orc["clear"].min(1)


@gpu
@pytest.mark.parametrize("name", list(BEAM_CASES))
def test_beam_search_with_constraints_matches_fp64_oracle(name):
    cfg, p = br.case_model(BEAM_MODEL)
    pre, W, kw = BEAM_CASES[name]
    from test_beam_gpu import gen_of
    g = gen_of(BEAM_MODEL)
    cons = cpu_ref.make_constraints(cfg, len(pre), **kw)
    got = g.beam_search(pre, width=W, constraints=cons)
    orc = beam_oracle(name)
    s64 = br.score64_of(p, cfg, got)
    assert br.check_result(cfg, pre, orc, got, s64) == []              # rows, order, n_beams; logp vs fp64 score
    A = cons.allowed()
    for n in range(len(pre)):
        nb = int(got.n_beams[n])
        assert all(obeys(got.rows[n, k], A[n]) for k in range(nb)), n   # every returned row obeys
    sc32 = g.score(got.rows.reshape(-1, cfg.max_len + 1)).name_logp.reshape(len(pre), W)
    live = np.isfinite(got.logp)
    assert np.abs(got.logp[live].astype(np.float64) - sc32[live]).max() <= br.ATOL["logp"]      # what score() returns
    if name in ("six-letter-Mar", "len4-W4"):                          # min_len == max_len: exact-length names
        want = 6 if name == "six-letter-Mar" else 4
        names = got.names()
        assert all(len(nm) == want for row in names for nm in row) and all(len(row) == W for row in names)
    if name == "fewer-than-W":
        assert got.n_beams.tolist() == [4, 2]
        assert sorted(got.names()[0]) == ["Max", "May", "Mex", "Mey"] and sorted(got.names()[1]) == ["Max", "May"]
        assert np.isneginf(got.logp[0, 4:]).all() and (got.rows[0, 4:] == 0).all() and (got.n_tok[0, 4:] == 0).all()
    assert (g.beam_search(pre, width=W, constraints=kw).rows == got.rows).all()      # the dict form


@gpu
def test_beam_constrained_graphs_are_separate_and_read_memory():
    cfg, p = br.case_model(BEAM_MODEL)
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    g = HipGenerator(cfg, p)
    pre = ["", "M"]
    plain = g.beam_search(pre, width=4)
    assert g.g.beam_graphs() == 1
    a_kw, b_kw = dict(charset=LOWER + "M", min_len=3, max_len=3), dict(charset=string.ascii_uppercase, min_len=2, max_len=2)
    a = g.beam_search(pre, width=4, constraints=a_kw)
    b = g.beam_search(pre, width=4, constraints=b_kw)
    assert g.g.beam_graphs() == 2                                       # one more recording served both (three table lines each)
    assert all(len(nm) == 3 and nm[-1] in LOWER + "M" for row in a.names() for nm in row)
    assert all(len(nm) == 2 and nm.isupper() for row in b.names() for nm in row)
    assert all(nm.startswith("M") for nm in a.names()[1] + b.names()[1])
    again = g.beam_search(pre, width=4)
    assert g.g.beam_graphs() == 2 and g.g.read_error() == 0
    assert np.array_equal(again.rows, plain.rows) and np.array_equal(again.logp.view(np.uint32), plain.logp.view(np.uint32))
    free = g.beam_search(pre, width=4, constraints=cpu_ref.make_constraints(cfg, 2))      # line 0 only
    assert np.array_equal(free.rows, plain.rows) and np.array_equal(free.logp.view(np.uint32), plain.logp.view(np.uint32))
    with pytest.raises(ValueError):
        g.beam_search(["Mx"], width=2, constraints=dict(pattern="M[aeiou]"))

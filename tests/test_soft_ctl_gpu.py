"""Soft sampling preferences on the device (docs/DESIGN.md §4h): the SOFT instantiations of sample_ctl_f32 and
score_ctl_logprob_f32 against the fp64 rule on planted inputs, and HipGenerator.generate / score with
logit_bias / presence_penalty / frequency_penalty against the fp64 oracles.

The planted logits are tests/test_sampling_ctl_gpu.py's, always on its 2^-12 grid (two slabs, or a late
bias), and every soft value is a multiple of 0.25: x + bias, frequency * n, + presence and the difference
are then exact in fp32, so the device's v is the fp64 v bit for bit and that file's tolerances and
clearances hold unchanged on filter_probs(v64)."""
import numpy as np
import pytest
import torch

import test_automaton_gpu as ta
import test_constraints_gpu as cg
import test_sampling_ctl_gpu as sc
import test_score_ctl_gpu as tsg
import test_soft_ctl as ts
from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.utils.data import random_floats

pytestmark = pytest.mark.gpu
DEV = "cuda"
ML, EOS = sc.ML, sc.EOS
STEP = 4                                   # four emitted bytes before the sampled one: room for a char three times
CFG, BAR = sc.CFG, sc.BAR
t, stream = cg.t, cg.stream
KINDS = ("no_argmax", "below_k", "free")


# ------------------------------------------------------------------------------- sample_ctl_f32, SOFT
def launch(ext, buf, bias, R, V, slabs, r, ctl, step, emitted, soft=None, tab=None, idx=None, auto=None, row0=0,
           alive=None, soft_rows=None):
    """One sampler launch at ``step`` of a [R][ML] job whose rows hold ``emitted`` [R, step] already.  soft:
    (tab [S, V], idx, pres, freq) with row0 + R rows; tab / idx: cg.launch's constraint keys; auto: (tab, nxt,
    state [row0 + R]).  Returns ids, out, alive, probs, err (and the state buffer) as numpy."""
    lg = t(buf)
    rf = np.zeros((R, ML), np.float32)
    rf[:, step] = r
    rf = t(rf)
    ids = torch.full((R,), -1, dtype=torch.int32, device=DEV)
    o = np.full((R, ML + 1), 7, np.uint8)
    o[:, :step] = emitted
    out = t(o)
    al = t(np.ones(R, np.int32) if alive is None else alive.astype(np.int32))
    probs = torch.full((R, V), -1.0, device=DEV)
    err = torch.zeros(4, dtype=torch.int32, device=DEV)
    cd = [t(a) for a in ctl]
    d = dict(logits=lg.data_ptr(), splits=slabs, slab=R * V, rf=rf.data_ptr(), ids=ids.data_ptr(), out=out.data_ptr(),
             alive=al.data_ptr(), N=R, V=V, step=step, max_len=ML, eos=EOS, probs=probs.data_ptr(),
             inv_temp=cd[0].data_ptr(), top_k=cd[1].data_ptr(), top_p=cd[2].data_ptr(), plen=cd[3].data_ptr(),
             prefix=cd[4].data_ptr(), row0=row0, err=err.data_ptr())
    keep = [lg, rf, cd]
    if bias is not None:
        b = t(bias)
        keep.append(b)
        d["bias"] = b.data_ptr()
    if soft is not None:
        sd = [t(np.ascontiguousarray(a)) for a in (soft[0].astype(np.float32), soft[1].astype(np.int32),
                                                   soft[2].astype(np.float32), soft[3].astype(np.float32))]
        keep.append(sd)
        d.update(soft_tab=sd[0].data_ptr(), soft_idx=sd[1].data_ptr(), soft_pres=sd[2].data_ptr(), soft_freq=sd[3].data_ptr(),
                 soft_rows=soft[0].shape[0] if soft_rows is None else soft_rows)
    sb = None
    if auto is not None:
        atab, nxt, state = auto
        assert state.shape == (row0 + R,)
        sb = t(np.concatenate([[ta.CANARY], state, [ta.CANARY]]).astype(np.int32))
        dt, dn = t(atab.view(np.int32)), t(nxt.view(np.int16))
        keep += [dt, dn]
        d.update(allow_tab=dt.data_ptr(), allow_next=dn.data_ptr(), allow_state=sb.data_ptr() + 4, allow_rows=atab.shape[0])
    elif tab is not None:
        dt, di = t(tab.view(np.int32)), t(idx)
        keep += [dt, di]
        d.update(allow_tab=dt.data_ptr(), allow_idx=di.data_ptr(), allow_rows=tab.shape[0])
    ext.sample_ctl(d, stream())
    torch.cuda.synchronize()
    res = (ids.cpu().numpy(), out.cpu().numpy(), al.cpu().numpy(), probs.cpu().numpy(), err.cpu().numpy())
    return res if sb is None else res + (sb.cpu().numpy(),)


def idx_of(line, row0, R, step, filler):
    idx = np.full((row0 + R, ML), filler, np.int32)
    idx[row0:, step] = line
    return idx


def plant_soft(V, R, x, step, rng):
    """Bias lines, per-row line / penalties (multiples of 0.25; V = 512: bias only) and the rows' emitted
    bytes: row i % 3 == 0 holds its most probable char three times and the second once, i % 3 == 1 four
    distinct probable chars, i % 3 == 2 random bytes (for V = 64 mostly no char at all)."""
    tab = np.zeros((4, V), np.float32)
    tab[1:] = 0.25 * rng.integers(-8, 9, (3, V))
    sidx = rng.integers(0, 4, R).astype(np.int32)
    if V <= 256:
        pres = (0.25 * rng.integers(-1, 6, R)).astype(np.float32)
        freq = (0.25 * rng.integers(-1, 6, R)).astype(np.float32)
        pres[::5], freq[1::5] = 0.0, 0.0                                    # one of the two alone
    else:
        pres, freq = np.zeros(R, np.float32), np.zeros(R, np.float32)
    em = rng.integers(0, 256, (R, step)).astype(np.uint8)
    order = np.argsort(-x, -1, kind="stable")
    for i in range(R):
        if step >= 4 and i % 3 == 0:
            em[i, :4] = np.array([order[i, 0], order[i, 1], order[i, 0], order[i, 0]]) & 255
        elif step >= 4 and i % 3 == 1:
            em[i, :4] = order[i, :4] & 255
    return tab, sidx, pres, freq, em


def v64_of(x, tab, sidx, pres, freq, em):
    """The rule in fp64, written out: v = (x + bias) - (freq * n (+ pres if n > 0))."""
    R, V = x.shape
    n = np.zeros((R, V))
    for i in range(R):
        for c in em[i]:
            if c < V:
                n[i, c] += 1
    pen = freq.astype(np.float64)[:, None] * n + np.where(n > 0, pres.astype(np.float64)[:, None], 0.0)
    return x.astype(np.float64) + tab[sidx].astype(np.float64) - pen, n


def pad_soft(sidx, pres, freq, row0):
    """The rows before row0 hold values that would change every result."""
    return (np.concatenate([np.full(row0, 3, np.int32), sidx]), np.concatenate([np.full(row0, 5.0, np.float32), pres]),
            np.concatenate([np.full(row0, 5.0, np.float32), freq]))


def plant_launch(V, R, x, x64cfg, j, rng, masked=True):
    """Launch j's inputs: per-row (mask kind, (k, p, T)) cells, forced and dead rows, soft values, emitted
    bytes and the fp64 expectation."""
    step = 0 if j % 4 == 3 else STEP                                        # step 0: a row with no byte yet
    cells = [(kd, c) for kd in KINDS for c in cg.CTLS]                      # 21
    mine = [cells[(j * R + i) % len(cells)] for i in range(R)]
    tab, sidx, pres, freq, em = plant_soft(V, R, x, step, rng)
    v64, n = v64_of(x, tab, sidx, pres, freq, em)
    v32 = v64.astype(np.float32)
    assert (v32.astype(np.float64) == v64).all()                            # exact in fp32: the grid holds
    soft = cpu_ref.Soft(tab, sidx, pres, freq)
    twin = cpu_ref.soft_adjust(torch.from_numpy(x), soft, em).numpy()
    assert (twin.view(np.uint32) == v32.view(np.uint32)).all()              # the fp32 twin forms the same bits
    A = np.stack([cg.mask_of(m[0] if masked else "free", v32[i], rng) for i, m in enumerate(mine)])
    k = np.array([m[1][0] for m in mine], np.int32)
    T = np.array([m[1][2] for m in mine], np.float64)
    vt = torch.from_numpy(v64)
    p = cg.clear_top_p(vt, T, k, np.array([m[1][1] for m in mine], np.float32), A)
    ctl = cpu_ref.make_controls(x64cfg, R, T, k, p)
    forced = (np.arange(R) + j) % 9 == 8
    plen = np.where(forced, step + 1, np.arange(R) % (step + 1)).astype(np.int32)
    pre = ((np.arange(R)[:, None] * 7 + np.arange(ML)[None, :] * 3 + j) % V).astype(np.uint8)
    alive = (np.arange(R) + j) % 4 != 3
    want = cpu_ref.filter_probs(vt, T, k, p, allowed=A).numpy()
    # cpu_ref's own soft path gives the same fp64 distribution
    again = cpu_ref.filter_probs(torch.from_numpy(x).double(), T, k, p, allowed=A, soft=soft, emitted=em).numpy()
    assert (again == want).all()
    want[forced] = np.eye(V)[pre[forced, step]]                             # a forced step reads none of it
    r = rng.random(R, dtype=np.float32)
    r[(np.arange(R) + j) % 3 == 2] = 1.5
    r, sel = sc.clear_uniforms(want, r)
    return dict(step=step, mine=mine, tab=tab, sidx=sidx, pres=pres, freq=freq, em=em, A=A, T=T, ctl=ctl, forced=forced,
                plen=plen, pre=pre, alive=alive, want=want, r=r, sel=sel, n=n, v32=v32)


def check_launch(c, got, V):
    ids, out, al, probs, err = got[:5]
    step, want, sel, alive, free = c["step"], c["want"], c["sel"], c["alive"], ~c["forced"]
    assert err[0] == 0
    assert (probs[free][~c["A"][free]] == 0).all()
    assert ((probs > 0) == (want > 0)).all(), np.argwhere((probs > 0) != (want > 0))[:4]          # the kept set
    torch.testing.assert_close(torch.from_numpy(probs).double(), torch.from_numpy(want), atol=2e-7, rtol=1e-5)
    assert (ids == sel).all(), (np.argwhere(ids != sel)[:4], [c["mine"][i] for i in np.flatnonzero(ids != sel)[:4]])
    assert (out[:, :step] == c["em"]).all()                                 # the bytes before the step: untouched
    assert (out[:, step] == np.where(alive, sel & 255, 7)).all() and (out[:, step + 1:] == 7).all()
    assert (al == (alive & (sel != EOS))).all()


@pytest.mark.parametrize("slabs", [1, 2])
@pytest.mark.parametrize("R", [1, 3, 70])
@pytest.mark.parametrize("V", [64, 256, 512])
def test_soft_sampler_kept_set_probs_and_choice(ext, V, R, slabs):
    """Bias lines and penalties per row x masks (no_argmax -- of the adjusted values --, below_k, free) x cg.CTLS
    mixtures, forced and dead rows, row0 in {0, 5}, at step 4 with planted bytes and at step 0 with none: the
    kept set exactly the fp64 one of filter_probs(x64 + b64 - pen64), probabilities and the chosen index as in
    tests/test_sampling_ctl_gpu.py, and the soft terms did move the kept sets."""
    x, buf, bias = sc.make_logits(V, R, slabs, slabs == 1, seed=4 * V + 7 * R + slabs)
    cfg = GRUConfig(vocab=V, max_len=ML, eos=EOS)
    rng = np.random.default_rng(V + R + slabs)
    moved = counted = 0
    for j in range(max(4, -(-21 // R))):
        c = plant_launch(V, R, x, cfg, j, rng)
        row0 = 5 if j % 2 else 0
        tab, line = cg.table_of(c["A"])
        arrs = sc.pad_ctl((c["ctl"].inv_temp, c["ctl"].top_k, c["ctl"].top_p, c["plen"], c["pre"]), row0)
        soft = (c["tab"],) + pad_soft(c["sidx"], c["pres"], c["freq"], row0)
        got = launch(ext, buf, bias, R, V, slabs, c["r"], arrs, c["step"], c["em"], soft, tab,
                     idx_of(line, row0, R, c["step"], 0), row0=row0, alive=c["alive"])
        check_launch(c, got, V)
        plain = cpu_ref.filter_probs(torch.from_numpy(x).double(), c["T"], c["ctl"].top_k, c["ctl"].top_p, allowed=c["A"]).numpy()
        free = ~c["forced"]
        moved += int(((plain > 0) != (c["want"] > 0))[free].any(1).sum())
        counted += int((c["n"].max(1) >= 3).sum()) if V <= 256 else 0
    assert moved > 0 or R == 1
    assert V > 256 or R == 1 or counted > 0                                  # a char three times was among the rows


@pytest.mark.parametrize("V,R", [(256, 70), (512, 70), (256, 3)])
def test_soft_sampler_with_an_automaton_row_state(ext, V, R):
    """The SOFT AUTO instantiation: the line comes from the state buffer, which advances by nxt[state][chosen]
    on every row; the distribution is the soft one inside the state's set."""
    x, buf, bias = sc.make_logits(V, R, 2, False, seed=5 * V + R)
    cfg = GRUConfig(vocab=V, max_len=ML, eos=EOS)
    rng = np.random.default_rng(V + R)
    for j in range(3):
        c = plant_launch(V, R, x, cfg, j, rng)
        row0 = 5 if j % 2 else 0
        atab, nxt, line = ta.big_table(V, c["A"], seed=j + V)
        state = np.concatenate([np.full(row0, 77, np.int32), line])
        arrs = sc.pad_ctl((c["ctl"].inv_temp, c["ctl"].top_k, c["ctl"].top_p, c["plen"], c["pre"]), row0)
        soft = (c["tab"],) + pad_soft(c["sidx"], c["pres"], c["freq"], row0)
        got = launch(ext, buf, bias, R, V, 2, c["r"], arrs, c["step"], c["em"], soft, auto=(atab, nxt, state), row0=row0,
                     alive=c["alive"])
        check_launch(c, got, V)
        sb = got[5]
        assert sb[0] == ta.CANARY and sb[-1] == ta.CANARY and (sb[1:1 + row0] == 77).all()
        assert (sb[1 + row0:-1] == nxt[line, c["sel"]].astype(np.int32)).all()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("V,R", [(64, 3), (256, 1), (256, 70), (512, 70), (128, 3)])
def test_neutral_soft_launch_is_bitwise_the_plain_controlled_launch(ext, V, R, masked):
    """All-zero bias, both penalties 0 (and 0 penalties over a non-zero count) through the SOFT instantiation:
    the ids / out / alive / probs / err bytes of the launch without soft pointers."""
    x, buf, bias = sc.make_logits(V, R, 2, True, seed=3 * V + R)
    rng = np.random.default_rng(V)
    r = rng.random(R, dtype=np.float32)
    r[::4] = 1.5
    alive = np.arange(R) % 3 != 1
    cells = [cg.CTLS[i % len(cg.CTLS)] for i in range(R)]
    ctl = cpu_ref.make_controls(GRUConfig(vocab=V, max_len=ML, eos=EOS), R, [c[2] for c in cells], [c[0] for c in cells],
                                [c[1] for c in cells])
    plen = (np.arange(R) % 5 == 4).astype(np.int32) * (STEP + 1)
    arrs = sc.pad_ctl((ctl.inv_temp, ctl.top_k, ctl.top_p, plen, np.full((R, ML), 9, np.uint8)), 5)
    em = rng.integers(0, V, (R, STEP)).astype(np.uint8)
    em[:, 1] = em[:, 0]
    tab = idx = None
    if masked:
        A = np.stack([cg.mask_of(cg.KINDS[i % len(cg.KINDS)], x[i], rng) for i in range(R)])
        tab, line = cg.table_of(A)
        idx = idx_of(line, 5, R, STEP, 0)
    zero = (np.zeros((1, V), np.float32), np.zeros(5 + R, np.int32), np.zeros(5 + R, np.float32), np.zeros(5 + R, np.float32))
    a = launch(ext, buf, bias, R, V, 2, r, arrs, STEP, em, zero, tab, idx, row0=5, alive=alive)
    b = launch(ext, buf, bias, R, V, 2, r, arrs, STEP, em, None, tab, idx, row0=5, alive=alive)
    for u, v in zip(a, b):
        assert (u.view(np.uint8) == v.view(np.uint8)).all()
    # a line of zeros that is not line 0, and a bias that only the rows before row0 name
    two = (np.stack([np.full(V, 2.0, np.float32), np.zeros(V, np.float32)]), np.concatenate([np.zeros(5, np.int32), np.ones(R, np.int32)]),
           zero[2], zero[3])
    c = launch(ext, buf, bias, R, V, 2, r, arrs, STEP, em, two, tab, idx, row0=5, alive=alive)
    for u, v in zip(c, b):
        assert (u.view(np.uint8) == v.view(np.uint8)).all()


def test_soft_sampler_flags_an_index_outside_the_table_and_refuses_half_a_set(ext):
    V, R = 256, 3
    x, buf, bias = sc.make_logits(V, R, 2, False, seed=1)
    ctl = cpu_ref.make_controls(GRUConfig(vocab=V, max_len=ML, eos=EOS), R, 1.0, 0, 1.0)
    arrs = (ctl.inv_temp, ctl.top_k, ctl.top_p, ctl.plen, ctl.prefix)
    r = np.full(R, 0.5, np.float32)
    em = np.zeros((R, STEP), np.uint8)
    tab = np.zeros((2, V), np.float32)
    tab[1, :8] = 4.0
    pres, freq = np.full(R, 0.5, np.float32), np.full(R, 0.25, np.float32)
    for bad in (2, -1, 1 << 20):
        sidx = np.array([1, bad, 1], np.int32)
        ids, _, _, probs, err = launch(ext, buf, bias, R, V, 2, r, arrs, STEP, em, (tab, sidx, pres, freq))
        assert err[0] == 16 and err[1] == np.int32(bad) and err[2] == 1 and err[3] == 0
        ok = np.array([1, 0, 1], np.int32)                                   # ... and the row takes line 0
        ids0, _, _, probs0, err0 = launch(ext, buf, bias, R, V, 2, r, arrs, STEP, em, (tab, ok, pres, freq))
        assert err0[0] == 0 and (ids == ids0).all() and (probs.view(np.uint32) == probs0.view(np.uint32)).all()
    # soft_rows is the bound, not the buffer
    err = launch(ext, buf, bias, R, V, 2, r, arrs, STEP, em, (tab, np.array([1, 1, 0], np.int32), pres, freq), soft_rows=1)[4]
    assert err[0] == 16 and err[1] == 1
    z = torch.zeros(4096, dtype=torch.int32, device=DEV)
    p = z.data_ptr()
    base = dict(logits=p, rf=p, ids=p, out=p, alive=p, N=1, V=64, step=0, max_len=ML, eos=EOS, inv_temp=p, top_k=p, top_p=p,
                plen=p, prefix=p)
    full = dict(soft_tab=p, soft_idx=p, soft_pres=p, soft_freq=p, soft_rows=1)
    for bad in (dict(full, soft_tab=0), dict(full, soft_idx=0), dict(full, soft_pres=0), dict(full, soft_freq=0),
                dict(full, soft_rows=0)):
        with pytest.raises(RuntimeError):
            ext.sample_ctl(dict(base, **bad), stream())
    sbase = dict(logits=p, tgt=p, ntok=p, tok_logp=p, rank=p, name_logp=p, ntok_out=p, Bp=64, V=64, ML=4, inv_temp=p, top_k=p,
                 top_p=p, plen=p, prefix=p, n_kept=p)
    for bad in (dict(full, soft_tab=0), dict(full, soft_idx=0), dict(full, soft_pres=0), dict(full, soft_freq=0),
                dict(full, soft_rows=0)):
        with pytest.raises(RuntimeError):
            ext.score_ctl_logprob(dict(sbase, **bad), stream())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------- score_ctl_logprob_f32, SOFT
SML = tsg.ML


def score_launch(ext, buf, bias, Bp, V, slabs, tgt, ntok, ctl, soft=None, tab=None, idx=None, row0=0):
    """tsg.launch with the soft keys.  Returns tok, rank, name, ntok_out, n_kept, err as numpy."""
    lg = t(buf)
    tg, nt = t(tgt.astype(np.int32)), t(ntok.astype(np.int32))
    tok = torch.full((Bp, SML), 7.0, device=DEV)
    rank = torch.full((Bp, SML), -7, dtype=torch.int32, device=DEV)
    name = torch.full((Bp,), 7.0, device=DEV)
    nto = torch.full((Bp,), -7, dtype=torch.int32, device=DEV)
    nk = torch.full((Bp, SML), -7, dtype=torch.int32, device=DEV)
    err = torch.zeros(4, dtype=torch.int32, device=DEV)
    cd = [t(a) for a in ctl]
    d = dict(logits=lg.data_ptr(), splits=slabs, slab=SML * Bp * V, tgt=tg.data_ptr(), ntok=nt.data_ptr(),
             tok_logp=tok.data_ptr(), rank=rank.data_ptr(), name_logp=name.data_ptr(), ntok_out=nto.data_ptr(),
             Bp=Bp, V=V, ML=SML, inv_temp=cd[0].data_ptr(), top_k=cd[1].data_ptr(), top_p=cd[2].data_ptr(),
             plen=cd[3].data_ptr(), prefix=cd[4].data_ptr(), row0=row0, err=err.data_ptr(), n_kept=nk.data_ptr())
    keep = [lg, tg, nt, cd]
    if bias is not None:
        b = t(bias)
        keep.append(b)
        d["bias"] = b.data_ptr()
    if soft is not None:
        sd = [t(np.ascontiguousarray(a)) for a in (soft[0].astype(np.float32), soft[1].astype(np.int32),
                                                   soft[2].astype(np.float32), soft[3].astype(np.float32))]
        keep.append(sd)
        d.update(soft_tab=sd[0].data_ptr(), soft_idx=sd[1].data_ptr(), soft_pres=sd[2].data_ptr(), soft_freq=sd[3].data_ptr(),
                 soft_rows=soft[0].shape[0])
    if tab is not None:
        dt, di = t(tab.view(np.int32)), t(idx)
        keep += [dt, di]
        d.update(allow_tab=dt.data_ptr(), allow_idx=di.data_ptr(), allow_rows=tab.shape[0])
    ext.score_ctl_logprob(d, stream())
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in (tok, rank, name, nto, nk, err))


def repeat_targets(tgt, ntok, N):
    """Every third name repeats its first target at steps 1 and 2 (three times by step 3), the next one at
    step 1 only; the masked positions stay -1."""
    tgt = tgt.copy()
    for b in range(N):
        if b % 3 == 0:
            tgt[1, b] = tgt[2, b] = tgt[0, b]
        elif b % 3 == 1:
            tgt[1, b] = tgt[0, b]
    return np.where(np.arange(SML)[:, None] < ntok[None, :], tgt, -1)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("slabs", [1, 2])
@pytest.mark.parametrize("N", [1, 3, 70])
@pytest.mark.parametrize("V", [64, 256, 512])
def test_soft_scorer_matches_fp64_rule(ext, V, N, slabs, masked):
    """tests/test_score_ctl_gpu.py's planted rows, mixtures and bounds with a bias line and penalties per name:
    tok_logp inside its bound, n_kept and the -inf pattern exact on the adjusted values, rank the plain
    scorer's (the model's, on the raw logits)."""
    x, buf, bias, Bp, tgt, ntok = tsg.planted(V, N, slabs, True, seed=6 * V + 7 * N + slabs)
    ntok = ntok.copy()
    ntok[:N:3] = SML                                                         # the repeating names run to the end
    tgt = repeat_targets(np.maximum(tgt, 0), ntok, N)
    rng = np.random.default_rng(V + N + slabs)
    tab = np.zeros((4, V), np.float32)
    tab[1:] = 0.25 * rng.integers(-8, 9, (3, V))
    sidx = rng.integers(0, 4, N).astype(np.int32)
    small = V <= 256
    pres = (0.25 * rng.integers(-1, 6, N)).astype(np.float32) if small else np.zeros(N, np.float32)
    freq = (0.25 * rng.integers(-1, 6, N)).astype(np.float32) if small else np.zeros(N, np.float32)
    v = np.zeros((SML, N, V))
    for l in range(SML):
        em = np.where(tgt[:l, :N].T >= 0, tgt[:l, :N].T, V + 1)              # the row's bytes before l
        v[l], _ = v64_of(x[l, :N], tab, sidx, pres, freq, em)
    assert (v.astype(np.float32).astype(np.float64) == v).all()
    v64 = torch.from_numpy(v)
    plain_rank = tsg.launch(ext, buf, bias, Bp, V, slabs, tgt, ntok)[1]
    worst, differs = 0.0, 0
    for j in range(0, -(-len(sc.combos(V)) // N), 4 if N == 1 else 1):
        A = None
        tabm = idx = None
        row0 = 5 if j % 2 else 0
        if masked:
            A = np.stack([np.stack([cg.mask_of(KINDS[(b + l + j) % len(KINDS)], v[l, b].astype(np.float32), rng) for b in range(N)])
                          for l in range(SML)])
            tabm, line = cg.table_of(A.reshape(SML * N, V))
            idx = np.full((row0 + N, SML), int(line.max()), np.int32)
            idx[row0:] = line.reshape(SML, N).T
        T, ctl, plen = tsg.controls_of(V, N, j, v64, A)
        pre = np.where(np.arange(SML)[None, :] % 2 == 0, np.maximum(tgt[:, :N].T, 0), 9).astype(np.uint8)
        arrs = tsg.pad_ctl((ctl.inv_temp, ctl.top_k, ctl.top_p, plen, pre), row0)
        soft = (tab,) + pad_soft(sidx, pres, freq, row0)
        got = score_launch(ext, buf, bias, Bp, V, slabs, tgt, ntok, arrs, soft, tabm, idx, row0=row0)
        rtok, rnk, _, bound = tsg.reference(v, tgt, ntok, N, T, ctl.top_k, ctl.top_p, plen, pre, A)
        rrank = tsg.reference(x, tgt, ntok, N, T, ctl.top_k, ctl.top_p, plen, pre, A)
        assert (got[1] == plain_rank).all()
        worst = max(worst, tsg.check(got, (rtok, rnk, rrank[2], bound), N, ntok, T, plen))
        differs += int((rnk != rrank[1]).sum())
    assert differs > 0 or N == 1                                             # the soft terms did move kept sets
    print(f"soft score V {V} N {N} slabs {slabs} masked {masked}: max d/bound {worst:.3f}")


def test_neutral_soft_scorer_is_bitwise_the_controlled_scorer(ext):
    V, N = 256, 70
    x, buf, bias, Bp, tgt, ntok = tsg.planted(V, N, 2, True, seed=77)
    T, ctl, plen = tsg.controls_of(V, N, 1, torch.from_numpy(x[:, :N]).double())
    pre = np.full((N, SML), 9, np.uint8)
    arrs = tsg.pad_ctl((ctl.inv_temp, ctl.top_k, ctl.top_p, plen, pre), 5)
    zero = (np.zeros((1, V), np.float32), np.zeros(5 + N, np.int32), np.zeros(5 + N, np.float32), np.zeros(5 + N, np.float32))
    a = score_launch(ext, buf, bias, Bp, V, 2, tgt, ntok, arrs, zero, row0=5)
    b = score_launch(ext, buf, bias, Bp, V, 2, tgt, ntok, arrs, None, row0=5)
    for u, w in zip(a, b):
        assert (u.view(np.uint8) == w.view(np.uint8)).all()


# ------------------------------------------------------------------------------- generator level
_oracle = {}


def oracle(case, N):
    key = (case, N)
    if key not in _oracle:
        rf = random_floats(N, CFG.max_len, seed=ts.SEEDS[case])
        _oracle[key] = (rf, cpu_ref.generate(ts.f64(sc.model()), CFG, rf, **ts.soft_cases(N)[case]))
    return _oracle[key]


@pytest.mark.parametrize("N", [8, 70])
@pytest.mark.parametrize("case", list(ts.SEEDS))
def test_generator_soft_names_match_fp64_oracle(case, N):
    """max_batch = 64: at N = 70 the last six names are a batch of their own and must read their own line and
    penalties (the per_name case gives every name other values).  Soft batches take the per-char graph at every
    size, in recordings of their own."""
    rf, want = oracle(case, N)
    kw = ts.soft_cases(N)[case]
    gen = sc.make_gen(max_batch=64)
    got = gen.generate(rf, **kw)
    assert gen.g.read_error() == 0
    s = sc.same(got, want)
    print(f"{case} N {N}: names identical to the fp64 oracle: {s}")
    assert s >= BAR
    assert gen.g.soft_graphs() == (2 if N == 70 else 1) and gen.g.ctl_graphs() == 0 and gen.g.automaton_graphs() == 0
    hard = {k: v for k, v in kw.items() if k not in ("logit_bias", "presence_penalty", "frequency_penalty")}
    assert not (gen.generate(rf, **hard) == got).all() if hard else not (gen.generate(rf) == got).all()


def test_generator_soft_batches_never_take_the_persistent_launches():
    N = 8
    kw = dict(ts.soft_cases(N)["pattern"])
    rf, want = oracle("pattern", N)
    gen = sc.make_gen(persist_constraints=64)
    assert gen.g.uses_persist_ctl(N) and gen.g.uses_persist_con(N, False)
    got = gen.generate(rf, **kw)
    assert sc.same(got, want) >= BAR and gen.g.persist_con_launches() == 0 and gen.g.soft_graphs() == 1
    hard = gen.generate(rf, constraints=kw["constraints"])                   # the same call without soft controls does
    assert gen.g.persist_con_launches() == 1 and gen.g.soft_graphs() == 1 and not (hard == got).all()


@pytest.mark.parametrize("case", ["alone", "sampled", "regex", "per_name"])
def test_generator_score_with_soft_controls_matches_fp64_oracle(case):
    """The oracle's own rows (possible by construction) and the same rows shifted by one name (mostly not)
    under the case's keywords, 70 rows in batches of 64.  tests/test_score_ctl_gpu.py's per-token bound on the
    names whose kept sets agree at every step; those are at least BAR of the names."""
    N = 70
    kw = ts.soft_cases(N)[case]
    rows = np.concatenate([oracle(case, N)[1][:40], np.roll(oracle(case, N)[1], 1, 0)[:30]])
    tok, name, n_tok, rank, nk = cpu_ref.score(ts.f64(sc.model()), CFG, rows, **kw)
    gen = sc.make_gen(max_batch=64)
    res = gen.score(rows, **kw)
    assert gen.g.read_error() == 0 and gen.g.soft_graphs() == 1 and gen.g.score_graphs() == 0
    assert np.array_equal(res.n_tok, n_tok) and np.array_equal(res.rank, gen.score(rows).rank)
    assert not np.isnan(res.tok_logp).any()
    agree = (res.n_kept == nk).all(1) & (np.isneginf(res.tok_logp) == np.isneginf(tok)).all(1)
    print(f"{case}: kept sets agree on {agree.mean():.4f} of the names; impossible {res.impossible}")
    assert agree.mean() >= BAR
    T = float(kw.get("temperature", 1.0))
    mask = np.arange(CFG.max_len)[None, :] < n_tok[:, None]
    fin = mask & np.isfinite(tok) & agree[:, None]
    bound = np.where(fin, tsg.bound_of(np.where(fin, tok, 0.0), T), 0.0)
    d = np.where(fin, np.abs(res.tok_logp.astype(np.float64) - np.where(fin, tok, 0.0)), 0.0)
    print(f"{case}: tok_logp max |d| {d.max():.3e}, max d/bound {np.max(d[fin] / bound[fin]):.3f}")
    assert (d <= bound).all()
    whole = agree & np.isfinite(name)
    assert np.isfinite(name[:40]).all() and whole.sum() >= 40
    assert (np.abs(res.name_logp.astype(np.float64)[whole] - name[whole]) <= bound.sum(1)[whole]).all()
    assert (np.isneginf(res.name_logp[agree]) == np.isneginf(name[agree])).all()


def test_soft_values_are_read_from_memory_and_plain_calls_stay_as_they_were():
    """Changing only a bias value replays the recording; a plain controlled call and a plain scoring call
    before and after soft calls give a fresh generator's bytes, with its recording counts and workspace
    sizes."""
    N = 70
    rf = random_floats(N, CFG.max_len, seed=9)
    fresh = sc.make_gen(max_batch=64)
    ctl = dict(top_k=20, top_p=0.9, temperature=0.8)
    want = fresh.generate(rf, **ctl)
    want_score = fresh.score(want, **ctl)
    sizes = (fresh.g.score_workspace_bytes(), fresh.g.ctl_graphs(), fresh.g.score_graphs())
    assert fresh.g.soft_graphs() == 0 and fresh.g.ctl_workspace_bytes() == 0   # (70 names: two persistent launches)
    graph = sc.make_gen(max_batch=64)                                        # ... and the same call on the per-char graph
    graph.g.set_persist_ctl_max(0)
    graph.generate(rf, **ctl)
    arena = graph.g.ctl_workspace_bytes()
    assert arena > 0 and graph.g.ctl_graphs() == 2

    gen = sc.make_gen(max_batch=64)
    before = gen.generate(rf, **ctl)
    a = gen.generate(rf, logit_bias={"e": 1.0}, presence_penalty=0.5, **ctl)
    g1 = gen.g.soft_graphs()
    b = gen.generate(rf, logit_bias={"e": 3.0}, presence_penalty=0.5, **ctl)
    b2 = gen.generate(rf, logit_bias={"e": 3.0}, presence_penalty=0.5, **ctl)
    assert gen.g.soft_graphs() == g1 == 2                                    # batches of 64 and 6 names
    assert (b == b2).all() and not (a == b).all() and not (a == before).all()
    oracle_b = cpu_ref.generate(ts.f64(sc.model()), CFG, rf, logit_bias={"e": 3.0}, presence_penalty=0.5, **ctl)
    assert sc.same(b, oracle_b) >= BAR
    sa = gen.score(b, logit_bias={"e": 1.0}, **ctl)
    sb = gen.score(b, logit_bias={"e": 3.0}, **ctl)
    assert gen.g.soft_graphs() == g1 + 1 and not np.array_equal(sa.name_logp, sb.name_logp)
    after = gen.generate(rf, **ctl)
    after_score = gen.score(want, **ctl)
    assert (before == want).all() and (after == want).all()
    for u, v in ((after_score.tok_logp, want_score.tok_logp), (after_score.name_logp, want_score.name_logp)):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
    assert np.array_equal(after_score.n_kept, want_score.n_kept)
    assert sizes == (gen.g.score_workspace_bytes(), gen.g.ctl_graphs(), gen.g.score_graphs())
    # the soft calls took the per-char graph: its control arena, as a call without soft controls commits it --
    # the soft buffers are in no arena
    assert gen.g.ctl_workspace_bytes() == arena
    # neutral soft values on the soft path: the plain controlled bytes
    assert (gen.generate(rf, logit_bias={}, presence_penalty=0.0, frequency_penalty=0.0, **ctl) == want).all()
    assert gen.g.read_error() == 0


def test_bf16_raises_and_bad_soft_values_raise_before_anything_is_launched():
    rf = random_floats(16, CFG.max_len, seed=9)
    fast = sc.make_gen("bf16")
    for kw in (dict(logit_bias={"a": 1.0}), dict(presence_penalty=0.5), dict(frequency_penalty=0.0)):
        with pytest.raises(ValueError):
            fast.generate(rf, **kw)
    gen = sc.make_gen()
    for bad in (dict(logit_bias={"a": float("nan")}), dict(presence_penalty=2e4), dict(frequency_penalty=[0.5] * 15),
                dict(logit_bias=[{"a": 1.0}] * 15), dict(logit_bias=np.zeros(255))):
        with pytest.raises(ValueError):
            gen.generate(rf, **bad)
        with pytest.raises(ValueError):
            gen.score(np.zeros((16, CFG.max_len + 1), np.uint8), **bad)
    assert gen.g.ctl_workspace_bytes() == 0 and gen.g.score_workspace_bytes() == 0 and gen.g.soft_graphs() == 0
    z = torch.zeros(4096, dtype=torch.int32, device=DEV)
    p = z.data_ptr()
    with pytest.raises(RuntimeError):                                        # half a soft set
        gen.g.generate_ctl(p, 1, p, p, p, p, p, p, stream(), soft_tab=p, soft_idx=p, soft_rows=1)
    with pytest.raises(RuntimeError):
        gen.g.generate_ctl(p, 1, p, p, p, p, p, p, stream(), soft_tab=p, soft_idx=p, soft_rows=257, soft_pres=p, soft_freq=p)
    assert gen.g.read_error() == 0

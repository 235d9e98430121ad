"""Scoring under the sampler on the device (docs/DESIGN.md §4f): score_ctl_logprob_f32 against the fp64
rule on planted logits, and HipGenerator.score with generate's keywords against the fp64 oracle
cpu_ref.score.

Bounds.  Membership (the -inf pattern) and n_kept are exact.  A kept target's tok_logp is within
max(1, 1/T) * (1e-5 + 2e-7 * exp(-tok_logp_ref)) of fp64: tests/test_score_gpu.py's per-token bound, scaled
because an error in a logit is multiplied by 1/T in y.  A name's log-prob is within the sum of its
tokens' bounds.  The planted logits keep every edge (top-k gap 0.05 or an exact tie, top-p clearance
1e-4) far from fp32 rounding; on the model's own logits the comparison runs on the names that
tests/test_score_ctl.py calls settled."""
import numpy as np
import pytest
import torch

import test_constraints_gpu as cg
import test_sampling_ctl_gpu as sc
import test_score_ctl as tsc
from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.utils.data import random_floats

pytestmark = pytest.mark.gpu
DEV = "cuda"
ML, EOS = 4, 5
CFG = sc.CFG
t, stream = cg.t, cg.stream


# ------------------------------------------------------------------------------- score_ctl_logprob_f32
def launch(ext, buf, bias, Bp, V, slabs, tgt, ntok, ctl=None, tab=None, idx=None, rows=None, row0=0, ml=ML):
    """One scoring launch over [ml][Bp] logits rows.  ctl: (inv_temp, top_k, top_p, plen, prefix) arrays of
    row0 + names rows, None: score_logprob.  Returns tok, rank, name, ntok_out, n_kept, err as numpy; the
    outputs start as sentinels, so an unwritten word shows."""
    lg = t(buf)
    tg, nt = t(tgt.astype(np.int32)), t(ntok.astype(np.int32))
    tok = torch.full((Bp, ml), 7.0, device=DEV)
    rank = torch.full((Bp, ml), -7, dtype=torch.int32, device=DEV)
    name = torch.full((Bp,), 7.0, device=DEV)
    nto = torch.full((Bp,), -7, dtype=torch.int32, device=DEV)
    nk = torch.full((Bp, ml), -7, dtype=torch.int32, device=DEV)
    err = torch.zeros(4, dtype=torch.int32, device=DEV)
    d = dict(logits=lg.data_ptr(), splits=slabs, slab=ml * Bp * V, tgt=tg.data_ptr(), ntok=nt.data_ptr(),
             tok_logp=tok.data_ptr(), rank=rank.data_ptr(), name_logp=name.data_ptr(), ntok_out=nto.data_ptr(),
             Bp=Bp, V=V, ML=ml)
    keep = [lg, tg, nt]
    if bias is not None:
        b = t(bias)
        keep.append(b)
        d["bias"] = b.data_ptr()
    if ctl is None:
        ext.score_logprob(d, stream())
    else:
        cd = [t(a) for a in ctl]
        keep += cd
        d.update(inv_temp=cd[0].data_ptr(), top_k=cd[1].data_ptr(), top_p=cd[2].data_ptr(), plen=cd[3].data_ptr(),
                 prefix=cd[4].data_ptr(), row0=row0, err=err.data_ptr(), n_kept=nk.data_ptr())
        if tab is not None:
            dt, di = t(tab.view(np.int32)), t(idx)
            keep += [dt, di]
            d.update(allow_tab=dt.data_ptr(), allow_idx=di.data_ptr(), allow_rows=tab.shape[0] if rows is None else rows)
        ext.score_ctl_logprob(d, stream())
    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in (tok, rank, name, nto, nk, err))


def pad_ctl(ctl, row0):
    """Controls of rows row0.. ; the rows before hold values that would change every result."""
    inv, k, p, plen, pre = ctl
    return (np.concatenate([np.full(row0, 0.0, np.float32), inv]), np.concatenate([np.full(row0, 1, np.int32), k]),
            np.concatenate([np.full(row0, 0.01, np.float32), p]), np.concatenate([np.full(row0, ML, np.int32), plen]),
            np.concatenate([np.full((row0, ML), 9, np.uint8), pre]))


def planted(V, N, slabs, late_bias, seed):
    """Logits [ML Bp][V] (row l Bp + b), targets [ML][Bp] and n_tok [Bp] = (3 b + 4) % (ML + 1) for b < N (every
    count 0 .. ML; a single name has ML), 0 for the pad rows.  Targets: by rank in the row -- the arg-max, the ranks around the planted ties and the k edges
    (0, 1, 2, 62 .. 66), the last two and random ones."""
    Bp = -(-N // 64) * 64
    x, buf, bias = sc.make_logits(V, ML * Bp, slabs, late_bias, seed)
    rng = np.random.default_rng(seed + 1)
    order = np.argsort(-x, -1, kind="stable")
    pick = np.array([0, 1, 2, 62, 63, 64, 65, 66, V - 2, V - 1])
    r = np.where(rng.random(ML * Bp) < 0.6, pick[rng.integers(0, len(pick), ML * Bp)], rng.integers(0, V, ML * Bp)) % V
    tgt = order[np.arange(ML * Bp), r].reshape(ML, Bp)
    ntok = np.where(np.arange(Bp) < N, (3 * np.arange(Bp) + 4) % (ML + 1), 0)      # 4, 2, 0, 3, 1, ...
    tgt = np.where(np.arange(ML)[:, None] < ntok[None, :], tgt, -1)
    return x.reshape(ML, Bp, V), buf, bias, Bp, tgt, ntok


def settle_top_p(x64, T, k, p, A=None):
    """One top_p per name that clears the 1e-4 edge at every one of its ML rows: the sampler tests'
    clear_top_p, step after step, until no step moves it."""
    for _ in range(12):
        before = p.copy()
        for l in range(ML):
            p = sc.clear_top_p(x64[l], T, k, p) if A is None else cg.clear_top_p(x64[l], T, k, p, A[l])
        if (p == before).all():
            return p
    raise AssertionError("no top_p clears every step")


def reference(x, tgt, ntok, N, T, k, p, plen, pre, A=None):
    """fp64 rule on the planted logits: tok [N, ML] (-inf outside the kept set), n_kept, rank, bound."""
    V = x.shape[-1]
    tok = np.zeros((N, ML))
    nk = np.full((N, ML), -1, np.int32)
    rank = np.full((N, ML), -1, np.int32)
    for l in range(ML):
        xl = x[l, :N]
        pr = cpu_ref.filter_probs(torch.from_numpy(xl).double(), T, k, p, allowed=None if A is None else A[l]).numpy()
        for b in range(N):
            if l >= ntok[b]:
                continue
            tg = int(tgt[l, b])
            rank[b, l] = int((xl[b] > xl[b, tg]).sum() + ((xl[b] == xl[b, tg]) & (np.arange(V) < tg)).sum())
            if l < plen[b]:
                tok[b, l], nk[b, l] = (0.0 if tg == int(pre[b, l]) else -np.inf), 1
            else:
                tok[b, l] = np.log(pr[b, tg]) if pr[b, tg] > 0 else -np.inf
                nk[b, l] = int((pr[b] > 0).sum())
    with np.errstate(over="ignore"):
        bound = np.maximum(1.0, 1.0 / np.where(T == 0, 1.0, T))[:, None] * (1e-5 + 2e-7 * np.exp(-tok))
    return tok, nk, rank, bound


def check(got, ref, N, ntok, T, plen):
    """The module's bounds; returns the largest d / bound over the kept, unforced, non-greedy targets."""
    tok, rank, name, nto, nk, err = got
    rtok, rnk, rrank, bound = ref
    assert err[0] == 0
    assert not np.isnan(tok).any() and not np.isnan(name).any()
    assert (np.isneginf(tok[:N]) == np.isneginf(rtok)).all(), np.argwhere(np.isneginf(tok[:N]) != np.isneginf(rtok))[:4]
    assert (nk[:N] == rnk).all(), np.argwhere(nk[:N] != rnk)[:4]
    assert (rank[:N] == rrank).all()
    mask = np.arange(ML)[None, :] < ntok[:N, None]
    exact = mask & ((T == 0)[:, None] | (np.arange(ML)[None, :] < plen[:, None]))
    assert (tok[:N][exact] == rtok[exact]).all()                         # forced and greedy steps: exactly 0 or -inf
    fin = mask & np.isfinite(rtok)
    d = np.abs(tok[:N].astype(np.float64)[fin] - rtok[fin])
    worst = float((d / bound[fin]).max()) if fin.any() else 0.0
    assert (d <= bound[fin]).all(), worst
    # masked positions and pad rows: 0 / -1 / -1, a sum of 0 and no token
    full = np.arange(ML)[None, :] < ntok[:, None]
    assert (tok[~full] == 0).all() and (rank[~full] == -1).all() and (nk[~full] == -1).all()
    assert (nto == ntok).all() and (name[N:] == 0).all()
    for b in range(N):                                                   # the step-order fp32 sum, bitwise
        s = np.float32(0)
        for l in range(ntok[b]):
            s = np.float32(s + tok[b, l])
        assert s == name[b] or (np.isneginf(s) and np.isneginf(name[b])), (b, s, name[b])
    return worst


def controls_of(V, N, j, x64, A=None):
    """Name b of launch j takes combo j N + b of sc.combos(V); every fifth name is forced for 1 or 2 steps,
    with a prefix that agrees with the target at even steps only."""
    cs = sc.combos(V)
    mine = [cs[(j * N + b) % len(cs)] for b in range(N)]
    k = np.array([c[0] for c in mine], np.int32)
    T = np.array([c[2] for c in mine], np.float64)
    p = settle_top_p(x64, T, k, np.array([c[1] for c in mine], np.float32), A)
    ctl = cpu_ref.make_controls(GRUConfig(vocab=V, max_len=ML, eos=EOS), N, T, k, p)
    plen = np.where((np.arange(N) + j) % 5 == 4, 1 + (np.arange(N) // 5) % 2, 0).astype(np.int32)
    return T, ctl, plen


@pytest.mark.parametrize("slabs,late_bias", [(1, False), (2, True)])
@pytest.mark.parametrize("N", [1, 3, 70])
@pytest.mark.parametrize("V", [64, 256, 512])
def test_score_ctl_matches_fp64_rule(ext, V, N, slabs, late_bias):
    """Every k in {1, 2, 63, 64, 65, V-1, V, V+7} x p in {1e-6, .5, .9, 1} x T in {0, .5, 1, 2} as per-name
    mixtures, n_tok 0 .. 4, forced steps that hit and miss, the control row offset, pad rows."""
    x, buf, bias, Bp, tgt, ntok = planted(V, N, slabs, late_bias, seed=V + 7 * N + slabs)
    x64 = torch.from_numpy(x[:, :N]).double()
    worst = 0.0
    for j in range(-(-len(sc.combos(V)) // N)):
        T, ctl, plen = controls_of(V, N, j, x64)
        pre = np.where(np.arange(ML)[None, :] % 2 == 0, np.maximum(tgt[:, :N].T, 0), 9).astype(np.uint8)
        row0 = 5 if j % 2 else 0
        arrs = pad_ctl((ctl.inv_temp, ctl.top_k, ctl.top_p, plen, pre), row0)
        got = launch(ext, buf, bias, Bp, V, slabs, tgt, ntok, arrs, row0=row0)
        ref = reference(x, tgt, ntok, N, T, ctl.top_k, ctl.top_p, plen, pre)
        worst = max(worst, check(got, ref, N, ntok, T, plen))
    print(f"V {V} N {N} slabs {slabs}: max d/bound {worst:.3f}")


@pytest.mark.parametrize("slabs,late_bias", [(1, False), (2, True)])
@pytest.mark.parametrize("N", [1, 3, 70])
@pytest.mark.parametrize("V", [64, 256, 512])
def test_score_ctl_masked_matches_fp64_rule(ext, V, N, slabs, late_bias):
    """Every kind of mask of the sampler's tests, one per (name, step), under the mixtures above: a target
    outside its set is -inf, n_kept counts inside the set only."""
    x, buf, bias, Bp, tgt, ntok = planted(V, N, slabs, late_bias, seed=2 * V + 7 * N + slabs)
    x64 = torch.from_numpy(x[:, :N]).double()
    rng = np.random.default_rng(V + N)
    worst, outside = 0.0, 0
    for j in range(0, -(-len(sc.combos(V)) // N), 2 if N == 1 else 1):
        A = np.stack([np.stack([cg.mask_of(cg.KINDS[(b + l + j) % len(cg.KINDS)], x[l, b], rng) for b in range(N)])
                      for l in range(ML)])                               # [ML, N, V]
        T, ctl, plen = controls_of(V, N, j, x64, A)
        pre = np.where(np.arange(ML)[None, :] % 2 == 0, np.maximum(tgt[:, :N].T, 0), 9).astype(np.uint8)
        tab, line = cg.table_of(A.reshape(ML * N, V))
        row0 = 5 if j % 2 else 0
        idx = np.full((row0 + N, ML), int(line.max()), np.int32)         # the rows before row0: a line that would change the result
        idx[row0:] = line.reshape(ML, N).T
        arrs = pad_ctl((ctl.inv_temp, ctl.top_k, ctl.top_p, plen, pre), row0)
        got = launch(ext, buf, bias, Bp, V, slabs, tgt, ntok, arrs, tab, idx, row0=row0)
        ref = reference(x, tgt, ntok, N, T, ctl.top_k, ctl.top_p, plen, pre, A)
        worst = max(worst, check(got, ref, N, ntok, T, plen))
        outside += int(np.isneginf(ref[0]).sum())
    assert outside > 0
    print(f"masked V {V} N {N} slabs {slabs}: max d/bound {worst:.3f}")


@pytest.mark.parametrize("slabs,late_bias", [(1, False), (2, True)])
@pytest.mark.parametrize("V,N", [(64, 3), (256, 1), (256, 70), (512, 70), (128, 3), (448, 3)])
def test_score_ctl_neutral_is_bitwise_score_logprob(ext, V, N, slabs, late_bias):
    x, buf, bias, Bp, tgt, ntok = planted(V, N, slabs, late_bias, seed=3 * V + N)
    ctl = cpu_ref.make_controls(GRUConfig(vocab=V, max_len=ML, eos=EOS), N, 1.0, 0, 1.0)
    a = launch(ext, buf, bias, Bp, V, slabs, tgt, ntok, (ctl.inv_temp, ctl.top_k, ctl.top_p, ctl.plen, ctl.prefix))
    b = launch(ext, buf, bias, Bp, V, slabs, tgt, ntok)
    for u, v in zip(a[:4], b[:4]):                                       # tok_logp, rank, name_logp, ntok_out
        assert (u.view(np.uint8) == v.view(np.uint8)).all()
    full = np.arange(ML)[None, :] < ntok[:, None]
    assert (a[4][full] == V).all() and (a[4][~full] == -1).all() and a[5][0] == 0


@pytest.mark.parametrize("V,N", [(64, 3), (256, 70), (512, 70), (128, 3)])
def test_score_ctl_line_zero_only_is_bitwise_the_unmasked_launch(ext, V, N):
    x, buf, bias, Bp, tgt, ntok = planted(V, N, 2, True, seed=5 * V + N)
    cells = [cg.CTLS[i % len(cg.CTLS)] for i in range(N)]
    ctl = cpu_ref.make_controls(GRUConfig(vocab=V, max_len=ML, eos=EOS), N, [c[2] for c in cells], [c[0] for c in cells],
                                [c[1] for c in cells])
    plen = (np.arange(N) % 5 == 4).astype(np.int32)
    arrs = pad_ctl((ctl.inv_temp, ctl.top_k, ctl.top_p, plen, np.full((N, ML), 9, np.uint8)), 5)
    tab = np.full((1, V // 32), 0xFFFFFFFF, np.uint32)
    a = launch(ext, buf, bias, Bp, V, 2, tgt, ntok, arrs, tab, np.zeros((5 + N, ML), np.int32), row0=5)
    b = launch(ext, buf, bias, Bp, V, 2, tgt, ntok, arrs, row0=5)
    for u, v in zip(a, b):
        assert (u.view(np.uint8) == v.view(np.uint8)).all()
    assert (a[4] > 1).any() and (N < 70 or np.isneginf(a[0]).any())      # (the cuts were active)


def test_score_ctl_flags_an_idx_entry_outside_the_table(ext):
    V, N = 256, 3
    x, buf, bias, Bp, tgt, ntok = planted(V, N, 1, False, seed=1)
    ntok[:N] = ML
    tgt[:, :N] = np.argsort(-x[:, :N], -1)[..., 100]                     # rank 100: outside every 3-char set
    rng = np.random.default_rng(0)
    A = np.stack([cg.mask_of("below_k", x[1, b], rng) for b in range(N)])
    tab, line = cg.table_of(A)
    ctl = cpu_ref.make_controls(GRUConfig(vocab=V, max_len=ML, eos=EOS), N, 1.0, 0, 1.0)
    arrs = (ctl.inv_temp, ctl.top_k, ctl.top_p, ctl.plen, ctl.prefix)
    for bad in (tab.shape[0], -1, 1 << 20):
        idx = np.zeros((N, ML), np.int32)
        idx[:, 1] = line
        idx[1, 1] = bad
        tok, _, _, _, nk, err = launch(ext, buf, bias, Bp, V, 1, tgt, ntok, arrs, tab, idx)
        assert err[0] == 16 and err[1] == np.int32(bad) and err[2] == 1 and err[3] == 0
        ok = idx.copy()
        ok[1, 1] = 0                                                     # ... and the name takes line 0
        tok0, _, _, _, nk0, err0 = launch(ext, buf, bias, Bp, V, 1, tgt, ntok, arrs, tab, ok)
        assert err0[0] == 0 and (tok.view(np.uint32) == tok0.view(np.uint32)).all() and (nk == nk0).all()
        assert nk[1, 1] == V and np.isfinite(tok[1, 1]) and nk[0, 1] == 3 and np.isneginf(tok[0, 1])
    idx = np.zeros((N, ML), np.int32)
    idx[:, 1] = line
    err = launch(ext, buf, bias, Bp, V, 1, tgt, ntok, arrs, tab, idx, rows=int(line.max()))[5]
    assert err[0] == 16 and err[1] == line.max()                         # allow_rows is the bound, not the buffer


def test_score_ctl_launcher_refuses_bad_arguments(ext):
    z = torch.zeros(1 << 16, dtype=torch.int32, device=DEV)
    p = z.data_ptr()
    base = dict(logits=p, tgt=p, ntok=p, tok_logp=p, rank=p, name_logp=p, ntok_out=p, Bp=64, V=64, ML=4,
                inv_temp=p, top_k=p, top_p=p, plen=p, prefix=p, n_kept=p)
    for bad in (dict(allow_tab=p), dict(allow_idx=p), dict(allow_tab=p, allow_idx=p, allow_rows=0),
                dict(V=192, allow_tab=p, allow_idx=p, allow_rows=1), dict(ML=65), dict(V=576), dict(V=96),
                dict(n_kept=0), dict(top_k=0)):
        with pytest.raises(RuntimeError):
            ext.score_ctl_logprob(dict(base, **bad), stream())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------- generator level
def bound_of(tok64, T):
    with np.errstate(over="ignore"):
        return max(1.0, 1.0 / T) * (1e-5 + 2e-7 * np.exp(-tok64))


def check_settled(res, name, rows, kw, T, what):
    """The device against the fp64 oracle on the settled names; at most one name in eight unsettled."""
    tok, nm, n_tok, rank, nk = tsc.oracle_score(name, rows, **kw)
    ok = tsc.settled_names(rows, kw["temperature"], kw.get("top_k", 0), kw.get("top_p", 1.0), kw.get("constraints"))
    print(f"{what}: {int((~ok).sum())} of {len(ok)} names unsettled")
    assert int((~ok).sum()) * 8 <= len(ok)
    assert np.array_equal(res.n_tok, n_tok) and not np.isnan(res.tok_logp).any() and not np.isnan(res.name_logp).any()
    mask = np.arange(CFG.max_len)[None, :] < n_tok[:, None]
    assert (res.tok_logp[~mask] == 0).all() and (res.rank[~mask] == -1).all() and (res.n_kept[~mask] == -1).all()
    assert (np.isneginf(res.tok_logp[ok]) == np.isneginf(tok[ok])).all()
    assert (res.n_kept[ok] == nk[ok]).all()
    fin = mask & np.isfinite(tok) & ok[:, None]
    bound = np.where(fin, bound_of(np.where(fin, tok, 0.0), T), 0.0)
    d = np.where(fin, np.abs(res.tok_logp.astype(np.float64) - np.where(fin, tok, 0.0)), 0.0)
    print(f"{what}: tok_logp max |d| {d.max():.3e}, max d/bound {np.max(d[fin] / bound[fin]):.3f}")
    assert (d <= bound).all()
    whole = ok & np.isfinite(nm)
    assert (np.abs(res.name_logp.astype(np.float64)[whole] - nm[whole]) <= bound.sum(1)[whole]).all()
    assert (np.isneginf(res.name_logp[ok]) == np.isneginf(nm[ok])).all()
    assert res.impossible >= int(np.isneginf(nm[ok]).sum())


@pytest.mark.parametrize("name", ["ctl", "ctl+capital"])
def test_score_with_controls_matches_fp64_oracle(name):
    """300 rows of the fp64 sampler in batches of 64: every batch reads its own slice of the controls and
    of the constraint lines."""
    kw = tsc.SETTINGS[name]
    rows = tsc.oracle_rows(name, 300, 9, **kw)
    gen = sc.make_gen(sharp=True, max_batch=64)
    per_name = dict(kw, temperature=np.full(300, kw["temperature"]), top_k=np.full(300, kw["top_k"]))
    if "constraints" in kw:
        per_name["constraints"] = cpu_ref.make_constraints(CFG, 300, **kw["constraints"])
    res = gen.score(rows, **per_name)
    assert gen.g.read_error() == 0 and gen.g.score_graphs() == 1         # 64 and 44 names pad to the same 64 rows
    check_settled(res, name, rows, kw, kw["temperature"], name)


@pytest.mark.parametrize("name", ["ctl+capital", "mixture+ctl"])
def test_closed_loop_generated_names_score_finite(name):
    """The device sampler's own names under the device scorer.  The generation logits come from per-step
    products and the scoring logits from one batched product, so a char at the very edge of a kept set
    may flip: the project's fp32 bar.  Every name obeys its sets, no tolerance."""
    N = 1000
    kw = dict(tsc.SETTINGS[name])
    if name == "mixture+ctl":
        kw["constraints"] = cg.mixture(N)
    cons = cpu_ref.make_constraints(CFG, N, **kw["constraints"])
    # the mixture's kinds shift at every 64-name boundary: in batches of 64 a batch that read rows 0 ..
    # of the controls would hold its names to another name's sets
    gen = sc.make_gen(sharp=True, **(dict(max_batch=64) if name == "mixture+ctl" else {}))
    rows = gen.generate(random_floats(N, CFG.max_len, seed=9), **kw)
    res = gen.score(rows, **kw)
    assert gen.g.read_error() == 0 and cg.all_obey(rows, cons)
    share = float(np.isfinite(res.name_logp).mean())
    print(f"{name}: {share:.4f} of {N} generated names score finite; impossible {res.impossible}")
    assert share >= sc.BAR and not np.isnan(res.name_logp).any()
    assert res.impossible == N - int(np.isfinite(res.name_logp).sum())
    assert (res.n_kept[res.n_kept >= 0] >= 1).all() and res.n_kept.max() <= kw["top_k"] + 2


@pytest.mark.parametrize("cons", [None, dict(charset="".join(chr(c) for c in range(8, 40)))])
def test_device_probabilities_sum_to_one_under_controls(cons):
    """The 4033 distinct valid rows of the vocab-64, max_len-2 model.  The total is 1 for any
    self-consistent kept sets, so an fp32 / fp64 edge flip does not move it."""
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    from test_score import all_rows_ml2
    rows = all_rows_ml2(0)
    cfg = GRUConfig(vocab=64, embed=64, hidden=64, layers=2, max_len=2, sos=0, eos=0, seed=6)
    gen = HipGenerator(cfg, init_params(cfg), max_batch=1024)
    res = gen.score(rows, temperature=0.7, top_k=20, top_p=0.9, constraints=cons)
    total = np.exp(res.name_logp.astype(np.float64)).sum()
    print(f"sum exp(name_logp) - 1 = {total - 1:.3e}, impossible {res.impossible}")
    assert abs(total - 1.0) <= 1e-4 and 0 < res.impossible < 4033
    assert gen.g.read_error() == 0


def test_one_recording_serves_every_value_and_plain_score_is_untouched():
    rows = tsc.oracle_rows("ctl+capital", 300, 9, **tsc.SETTINGS["ctl+capital"])
    gen = sc.make_gen(sharp=True)
    plain = gen.score(rows)
    w0, g0 = gen.g.score_workspace_bytes(), gen.g.score_graphs()
    assert plain.n_kept is None and plain.impossible == 0 and g0 == 1
    # two control settings on one recording
    a_kw, b_kw = dict(tsc.CTL), dict(temperature=1.25, top_k=5, top_p=0.8)
    a = gen.score(rows, **a_kw)
    assert gen.g.score_workspace_bytes() > w0 and gen.g.score_graphs() == g0 + 1
    w1 = gen.g.score_workspace_bytes()
    b = gen.score(rows, **b_kw)
    a2 = gen.score(rows, **a_kw)
    assert gen.g.score_graphs() == g0 + 1 and gen.g.score_workspace_bytes() == w1
    check_settled(a, "rec-a", rows, a_kw, 0.8, "controls a")
    check_settled(b, "rec-b", rows, b_kw, 1.25, "controls b")
    assert np.array_equal(a.tok_logp.view(np.uint32), a2.tok_logp.view(np.uint32)) and np.array_equal(a.n_kept, a2.n_kept)
    assert not np.array_equal(a.n_kept, b.n_kept)
    # two constraints with equally many table lines on one recording
    c_kw = dict(temperature=0.8, constraints=dict(pattern="[A-M][aeiou]", charset=cg.LETTERS, min_len=3, max_len=6))
    d_kw = dict(temperature=0.8, constraints=dict(pattern="[N-Z][^aeiou]", charset=cg.LOWER, min_len=4, max_len=5))
    assert cpu_ref.make_constraints(CFG, 1, **c_kw["constraints"]).rows == cpu_ref.make_constraints(CFG, 1, **d_kw["constraints"]).rows
    c = gen.score(rows, **c_kw)
    d = gen.score(rows, **d_kw)
    assert gen.g.score_graphs() == g0 + 2
    check_settled(c, "rec-c", rows, c_kw, 0.8, "constraint c")
    check_settled(d, "rec-d", rows, d_kw, 0.8, "constraint d")
    assert not np.array_equal(np.isneginf(c.name_logp), np.isneginf(d.name_logp))
    # the plain call: the graph and the bytes it had
    again = gen.score(rows)
    assert gen.g.score_graphs() == g0 + 2 and again.n_kept is None
    for u, v in ((again.tok_logp, plain.tok_logp), (again.name_logp, plain.name_logp)):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
    assert np.array_equal(again.rank, plain.rank) and np.array_equal(again.n_tok, plain.n_tok)
    assert np.array_equal(a.rank, plain.rank)                            # the model's rank, whatever the controls
    # neutral controls and a line-0-only table: the plain tok_logp, on the new path
    n = gen.score(rows, temperature=1.0, top_k=0, top_p=1.0, prefix="", constraints={})
    assert np.array_equal(n.tok_logp.view(np.uint32), plain.tok_logp.view(np.uint32))
    assert np.array_equal(n.name_logp.view(np.uint32), plain.name_logp.view(np.uint32))
    assert (n.n_kept[n.n_kept >= 0] == CFG.vocab).all()
    assert gen.g.read_error() == 0


def test_bf16_generator_scores_with_controls_and_bad_values_raise_first():
    kw = tsc.SETTINGS["ctl+capital"]
    rows = tsc.oracle_rows("ctl+capital", 300, 9, **kw)[:70]
    g16 = sc.make_gen("bf16", sharp=True)
    got = g16.score(rows, **kw)                                          # exact fp32 whatever the generator samples with
    check_settled(got, "bf16-70", rows, kw, kw["temperature"], "bf16 generator")
    assert g16.g.read_error() == 0
    gen = sc.make_gen(sharp=True)
    for bad in (dict(temperature=-1.0), dict(top_k=-1), dict(top_p=0.0), dict(prefix="x" * 11), dict(top_k=[1, 2]),
                dict(constraints=dict(min_len=5, max_len=3)), dict(prefix="Mx", constraints=dict(pattern="M[aeiou]")),
                dict(constraints=cpu_ref.make_constraints(CFG, 69))):
        with pytest.raises(ValueError):
            gen.score(rows, **bad)
    assert gen.g.score_workspace_bytes() == 0 and gen.g.score_graphs() == 0
    z = torch.zeros(4096, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):                                    # half a control set
        gen.g.score(z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), stream(), z.data_ptr())
    assert gen.g.read_error() == 0

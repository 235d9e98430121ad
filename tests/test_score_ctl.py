"""Scoring under the sampler on the CPU (docs/DESIGN.md §4f): cpu_ref.score with generate's keywords.
fp64 parameters throughout unless a test says otherwise; tests/test_score_ctl_gpu.py shares the helpers
and the cached oracles below."""
import string

import numpy as np
import pytest
import torch

import test_constraints_gpu as cg
import test_sampling_ctl_gpu as sc
from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.engine.generator import ScoreResult, encode_names
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.utils.data import random_floats
from test_score import all_rows_ml2

pytestmark = []          # (the helper modules are GPU suites; this one runs everywhere)
LETTERS = string.ascii_letters
CFG = sc.CFG             # GRUConfig(vocab=256, embed=128, hidden=256, layers=2, max_len=10, sos=0, eos=0)
CTL = dict(temperature=0.8, top_k=40, top_p=0.95)
CAPITAL = dict(pattern="[A-Z]", charset=LETTERS, min_len=4, max_len=7)     # a capital, then letters, 4 to 7 chars
K_GAP, P_GAP = 3.3e-6, 1e-4     # 8 x the 4.1e-7 of DESIGN §4b; the top-p clearance of the sampler's tests
_cache = {}


def p64(sharp=True):
    return {k: v.double() for k, v in sc.model(sharp).items()}


def logits64(cfg, p, rows):
    _, n_tok, x, tgt = cpu_ref.score_inputs(cfg, rows)
    return cpu_ref.forward(p, cfg, torch.from_numpy(x)), n_tok, tgt


def oracle_rows(name, N, seed, **kw):
    """fp64 cpu_ref.generate of the sharp model, once per name."""
    return sc.oracle(("score_ctl", name), True, random_floats(N, CFG.max_len, seed=seed), **kw)


def oracle_score(name, rows, **kw):
    """fp64 cpu_ref.score of the sharp model, once per name: (tok, name, n_tok, rank, n_kept)."""
    if ("s", name) not in _cache:
        _cache[("s", name)] = cpu_ref.score(p64(), CFG, rows, **kw)
    return _cache[("s", name)]


def settled_names(rows, temperature, top_k, top_p, constraints=None):
    """bool [N]: every scored, unforced step of the name clears both edges in fp64 -- the gap in y between
    the k-th and the (k + 1)-th largest allowed value is >= K_GAP (top-k active: more than k allowed), and
    no cumulative mass of the sorted post-top-k softmax lies within P_GAP of top_p."""
    lg, n_tok, _ = logits64(CFG, p64(), rows)
    N = rows.shape[0]
    cons = cpu_ref.as_constraints(CFG, N, constraints)
    ok = np.ones(N, bool)
    for l in range(CFG.max_len):
        A = np.ones((N, CFG.vocab), bool) if cons is None else cons.allowed(l)
        y = np.where(A, lg[:, l].numpy() * (1.0 / temperature), -np.inf)
        ys = -np.sort(-y, -1)
        live = l < n_tok
        if 0 < top_k < CFG.vocab:
            active = A.sum(1) > top_k
            with np.errstate(invalid="ignore"):                 # (-inf - -inf where fewer than k are allowed: not active)
                gap = ys[:, top_k - 1] - ys[:, top_k]
            ok &= ~(live & active & (gap < K_GAP))
        if top_p < 1:
            q = cpu_ref.filter_probs(lg[:, l], temperature, top_k, 1.0, allowed=A).numpy()
            c = np.cumsum(-np.sort(-q, -1), -1)
            c = np.where(-np.sort(-q, -1) > 0, c, 2.0)          # only the masses of kept chars are edges
            ok &= ~(live & (np.abs(c - top_p).min(1) < P_GAP))
    return ok


# ---------------------------------------------------------------------------------- the rule
def small_model(eos=0):
    cfg = GRUConfig(vocab=64, embed=64, hidden=64, layers=2, max_len=2, sos=0, eos=eos)
    return cfg, {k: v.double() for k, v in init_params(cfg, seed=6).items()}


def test_all_none_is_todays_call_bitwise():
    cfg, p = small_model()
    rows = all_rows_ml2(0)[::37]
    a = cpu_ref.score(p, cfg, rows)
    b = cpu_ref.score(p, cfg, rows, None, None, None, None, None)
    assert len(a) == len(b) == 4
    for u, v in zip(a, b):
        assert u.dtype == v.dtype and np.array_equal(u.view(np.uint8), v.view(np.uint8))


@pytest.mark.parametrize("kw", [dict(temperature=1.0), dict(top_k=0), dict(top_p=1.0), dict(prefix=""),
                                dict(temperature=1.0, top_k=0, top_p=1.0, prefix="", constraints={})])
def test_neutral_values_take_the_new_path_and_give_the_plain_tok_logp(kw):
    cfg, p = small_model()
    rows = all_rows_ml2(0)[::37]
    tok, name, n_tok, rank = cpu_ref.score(p, cfg, rows)
    got = cpu_ref.score(p, cfg, rows, **kw)
    assert len(got) == 5
    assert np.array_equal(got[0], tok) and np.array_equal(got[1], name)
    assert np.array_equal(got[2], n_tok) and np.array_equal(got[3], rank)
    mask = np.arange(cfg.max_len)[None, :] < n_tok[:, None]
    assert got[4].dtype == np.int32 and (got[4][mask] == cfg.vocab).all() and (got[4][~mask] == -1).all()
    if "constraints" in kw:                       # a line-0-only table
        assert cpu_ref.as_constraints(cfg, len(rows), {}).rows == 1


@pytest.mark.parametrize("eos", [0, 63])
@pytest.mark.parametrize("cons", [None, dict(charset="".join(chr(c) for c in range(8, 40)))])
def test_probabilities_sum_to_one_under_controls(eos, cons):
    """Every distinct valid row: the masses of the rows the sampler cannot emit are exactly 0, the rest is
    a product of distributions over kept sets."""
    cfg, p = small_model(eos)
    rows = all_rows_ml2(eos)
    assert rows.shape[0] == 4033
    tok, name, n_tok, rank, nk = cpu_ref.score(p, cfg, rows, temperature=0.7, top_k=20, top_p=0.9, constraints=cons)
    assert not np.isnan(tok).any() and not np.isnan(name).any()
    assert abs(np.exp(name).sum() - 1.0) <= 1e-12
    res = ScoreResult(tok, rank, name, n_tok, nk)
    assert 0 < res.impossible < 4033 and res.impossible == int(np.isneginf(name).sum())
    assert nk.max() <= 20 and nk[nk >= 0].min() >= 1
    if cons is not None:                          # nothing outside the charset has any mass
        inside = np.isin(rows[:, 0], list(range(8, 40)) + [eos])
        assert np.isneginf(name[~inside]).all()


SETTINGS = {
    "ctl": dict(CTL),
    "ctl+capital": dict(CTL, constraints=CAPITAL),
    "mixture": dict(constraints=cg.mixture(300)),
    "mixture+ctl": dict(temperature=0.8, top_k=20, top_p=0.9, constraints=cg.mixture(300)),
    "prefix+greedy": dict(temperature=[0.0, 1.3] * 150, prefix=["Ma", ""] * 150, top_k=5),
}


@pytest.mark.parametrize("name", list(SETTINGS))
def test_generated_rows_score_finite_under_their_own_settings(name):
    """300 names of the fp64 sampler: each one is a row the sampler can emit, its n_kept is the oracle's
    kept-set size and every tok_logp is the log of the probability the sampler drew with."""
    kw = SETTINGS[name]
    rows = oracle_rows(name, 300, 9, **kw)
    tok, nm, n_tok, rank, nk = oracle_score(name, rows, **kw)
    assert np.isfinite(nm).all() and np.isfinite(tok).all() and not np.isnan(tok).any()
    plain = cpu_ref.score(p64(), CFG, rows)
    assert np.array_equal(n_tok, plain[2]) and np.array_equal(rank, plain[3])        # read from the row / the raw logits
    lg, _, tgt = logits64(CFG, p64(), rows)
    N = rows.shape[0]
    cons = cpu_ref.as_constraints(CFG, N, kw.get("constraints"))
    ctl = cpu_ref.make_controls(CFG, N, kw.get("temperature"), kw.get("top_k"), kw.get("top_p"), kw.get("prefix"))
    T =np.asarray(kw["temperature"], np.float64) * np.ones(N) if "temperature" in kw else np.ones(N)
    for l in range(CFG.max_len):
        live = l < n_tok
        forced = ctl.plen > l
        pr = cpu_ref.filter_probs(lg[:, l], T, ctl.top_k, ctl.top_p, allowed=None if cons is None else cons.allowed(l)).numpy()
        t = np.maximum(tgt[:, l], 0)
        free = live & ~forced
        np.testing.assert_allclose(tok[free, l], np.log(pr[free, t[free]]), rtol=0, atol=1e-12)
        assert ((pr > 0).sum(1)[free] == nk[free, l]).all()
        assert (tok[live & forced, l] == 0).all() and (nk[live & forced, l] == 1).all()
        assert (nk[live & (T == 0), l] == 1).all()
        assert (tok[~live, l] == 0).all() and (nk[~live, l] == -1).all() and (rank[~live, l] == -1).all()


def test_impossible_rows_are_minus_infinity_at_the_offending_step():
    cfg = CFG
    p = p64()
    names = ["Maria", "Ma7ia", "Bo", "Jonas", "Mario"]
    rows = encode_names(names, cfg)
    kw = dict(prefix=["Ma", "Ma", "", "Ma", ""], constraints=dict(charset=LETTERS, min_len=3))
    tok, nm, n_tok, rank, nk = cpu_ref.score(p, cfg, rows, **kw)
    assert np.isfinite(nm[[0, 4]]).all()
    assert np.isneginf(tok[1]).tolist() == [False, False, True] + [False] * 7      # '7' is outside the charset
    assert np.isneginf(tok[2]).tolist() == [False, False, True] + [False] * 7      # EOS at step 2 < min_len
    assert np.isneginf(tok[3]).tolist() == [True, True] + [False] * 8              # "Jo" is not the prefix "Ma"
    assert (tok[3, :2] == -np.inf).all() and (nk[3, :2] == 1).all() and (tok[0, :2] == 0).all()
    assert np.isneginf(nm[[1, 2, 3]]).all() and not np.isnan(nm).any() and not np.isnan(tok).any()
    res = ScoreResult(tok, rank, nm, n_tok, nk)
    assert res.impossible == 3 and res.nll_per_char == np.inf and res.perplexity == np.inf
    plain = ScoreResult(*[cpu_ref.score(p, cfg, rows)[i] for i in (0, 3, 1, 2)])
    assert res.top1 == plain.top1 and plain.impossible == 0 and plain.n_kept is None
    # greedy: the arg-max chain is the one possible row
    chain = cpu_ref.generate(p, cfg, random_floats(1, cfg.max_len, seed=1), temperature=0.0)
    other = chain.copy()
    nt = int(cpu_ref.score_inputs(cfg, chain)[1][0])
    j = max(nt - 2, 0)                     # another char there: the steps before it still follow the chain
    other[0, j] = 66 if chain[0, j] != 66 else 67
    tok, nm, n_tok, rank, nk = cpu_ref.score(p, cfg, np.concatenate([chain, other]), temperature=0.0)
    assert nm[0] == 0 and (tok[0] == 0).all() and (rank[0, :nt] == 0).all()
    assert np.isneginf(nm[1]) and (tok[1, :j] == 0).all() and np.isneginf(tok[1, j]) and rank[1, j] > 0
    assert (nk[0, :nt] == 1).all() and (nk[1, :j + 1] == 1).all() and not np.isnan(tok).any()


def test_bad_values_raise_before_any_work(monkeypatch):
    cfg, p = small_model()
    rows = all_rows_ml2(0)[:5]
    monkeypatch.setattr(cpu_ref, "forward", lambda *a, **k: (_ for _ in ()).throw(AssertionError("work was done")))
    for kw in (dict(temperature=-1.0), dict(top_k=-2), dict(top_p=0.0), dict(top_p=1.5), dict(temperature=[1.0, 2.0]),
               dict(prefix="abc"), dict(constraints=dict(min_len=2, max_len=1)), dict(constraints="x"),
               dict(constraints=cpu_ref.make_constraints(cfg, 4)),
               dict(prefix="\x05", constraints=dict(charset="\x06\x07"))):
        with pytest.raises(ValueError):
            cpu_ref.score(p, cfg, rows, **kw)


# ------------------------------------------------------------- the GPU suite's oracle, on the CPU
@pytest.mark.parametrize("name", ["ctl", "ctl+capital"])
def test_oracle_rows_are_settled(name):
    """A condition, not a measurement: tests/test_score_ctl_gpu.py compares the device with the fp64 oracle
    on settled names only, and at most one name in eight may be unsettled."""
    kw = SETTINGS[name]
    rows = oracle_rows(name, 300, 9, **kw)
    ok = settled_names(rows, kw["temperature"], kw["top_k"], kw["top_p"], kw.get("constraints"))
    print(f"{name}: {int((~ok).sum())} of {len(ok)} names unsettled")
    assert int((~ok).sum()) * 8 <= len(ok)

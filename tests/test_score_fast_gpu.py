"""HipGenerator.score(rows, fast=True) -- the bf16 fast scorer (Generator::score_fast, docs/DESIGN.md §4a) --
against the fp64 oracle cpu_ref.score on random-init weights rounded to bf16.

Yardstick, from the oracle alone: D = max over the scored tokens of |cpu_ref.score(round_operands=True) -
cpu_ref.score(exact)|, both in fp64.  The device rounds fp32-accumulated states to bf16 where the twin rounds
fp64 ones: single roundings can flip, the effect has the same size, hence 2 D, plus the fp32 softmax bound of
tests/test_score_gpu.py.  Ranks are compared wherever the fp64 target logit is more than 2 D away from every
other logit; the positions left out may be at most 10 % of the scored ones.

Measured on the CPU (D, share of the scored tokens left out of the rank comparison; then how far the two
planted bugs of DESIGN §4a exceed the token bound, as max and median of |d| / bound):
  case (1, 64, 128, 33, 4096), V 64, ML 6, eos 0  : D = 3.70e-4, 2.5 %; wrong target 4937 / 1755; no b_hh 41 / 8.5
  case (2, 64, 256, 130, 64), V 256, ML 10, eos 0 : D = 1.63e-4, 3.4 %; wrong target 12759 / 1953; no b_hh 97 / 14.8
  case (2, 64, 128, 70, 4096), V 64, ML 5, eos 63 : D = 2.83e-4, 1.8 %; wrong target 6507 / 1461; no b_hh 70 / 16.0"""
import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.models.seq_ref import bf16_round

pytestmark = pytest.mark.gpu

CASES = [   # L, E, H, V, ML, eos, N, max_batch
    (1, 64, 128, 64, 6, 0, 33, 4096),
    (2, 64, 256, 256, 10, 0, 130, 64),      # three chunks
    (2, 64, 128, 64, 5, 63, 70, 4096),      # eos != 0; 70 names pad to 128 rows
]


def make_case(L, E, H, V, ML, eos, N, max_batch):
    """cfg, bf16-rounded params, rows with n_tok over 1 .. ML (and rows without an EOS), and the oracle's
    figures: exact (tok, name, n_tok, rank), D, and the mask of scored positions whose rank is compared."""
    cfg = GRUConfig(vocab=V, embed=E, hidden=H, layers=L, max_len=ML, sos=0, eos=eos, seed=6)
    params = init_params(cfg)
    # unit-normal head biases, as a trained model's char frequencies: the init's logits lie within +-0.3, and
    # their own gaps then leave 18 - 54 % of the positions out of the rank comparison whatever the seed
    params["fc.bias"] = torch.randn(V, generator=torch.Generator().manual_seed(6))
    params = {k: bf16_round(v) for k, v in params.items()}
    rng = np.random.default_rng(1)
    rows = rng.integers(0, V, size=(N, ML + 1), dtype=np.uint8)
    rows[:, ML] = 0
    for b in range(N):
        if b % (ML + 1) < ML:
            rows[b, b % (ML + 1)] = eos
    p64 = {k: v.double() for k, v in params.items()}
    exact = cpu_ref.score(p64, cfg, rows)
    twin = cpu_ref.score(p64, cfg, rows, round_operands=True)
    mask = np.arange(ML)[None, :] < exact[2][:, None]
    D = float(np.abs(twin[0] - exact[0])[mask].max())
    _, _, x, tgt = cpu_ref.score_inputs(cfg, rows)
    logits = cpu_ref.forward(p64, cfg, torch.from_numpy(x)).numpy()
    tc = np.maximum(tgt, 0)[..., None]
    gap = np.abs(logits - np.take_along_axis(logits, tc, -1))
    np.put_along_axis(gap, tc, np.inf, -1)
    clear = mask & (gap.min(-1) > 2 * D)
    return cfg, params, rows, exact, D, mask, clear


@pytest.mark.parametrize("case", CASES)
def test_score_fast_matches_fp64(case):
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    cfg, params, rows, (tok, name, n_tok, rank), D, mask, clear = make_case(*case)
    share = 1.0 - clear.sum() / mask.sum()
    assert share <= 0.10, share
    gen = HipGenerator(cfg, params, max_batch=case[-1], precision="bf16")
    res = gen.score(rows, fast=True)
    assert gen.g.read_error() == 0 and not gen.g.score_last_persist()
    assert np.array_equal(res.n_tok, n_tok)
    d = np.abs(res.tok_logp.astype(np.float64) - tok)
    bound = np.where(mask, 2 * D + 1e-5 + 2e-7 * np.exp(-tok), 0.0)
    print(f"D {D:.3e}, rank share left out {share:.4f}, max |d| {d.max():.3e}, max d/bound {np.max(d[mask] / bound[mask]):.3f}")
    assert np.all(d <= bound)
    assert np.all(res.tok_logp[~mask] == 0) and np.all(res.rank[~mask] == -1)
    assert np.array_equal(res.rank[clear], rank[clear])
    again = gen.score(rows, fast=True)     # a replay of the recordings: the same bytes
    assert again.tok_logp.tobytes() == res.tok_logp.tobytes() and np.array_equal(again.rank, res.rank)


@pytest.mark.parametrize("precision,kw", [
    ("fp32", {}), ("bf16x3", {}),
    ("bf16", dict(temperature=0.8)), ("bf16", dict(constraints=dict(pattern="[a-z]"))),
    ("bf16", dict(logit_bias={"a": 1.0})),
])
def test_score_fast_refusals(precision, kw):
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    cfg = GRUConfig(vocab=256, embed=64, hidden=64, layers=1, max_len=4, sos=0, eos=0, seed=6)
    gen = HipGenerator(cfg, init_params(cfg), max_batch=64, precision=precision)
    rows = np.zeros((3, cfg.max_len + 1), np.uint8)
    rows[:, 0] = 97
    graphs, ws = gen.g.score_graphs(), gen.g.score_workspace_bytes()
    with pytest.raises(ValueError):
        gen.score(rows, fast=True, **kw)
    assert gen.g.score_graphs() == graphs and gen.g.score_workspace_bytes() == ws

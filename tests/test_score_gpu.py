"""Teacher-forced scoring on the device (Generator::score, csrc/kernels/score.hip) against the fp64
oracle cpu_ref.score.

Bounds.  Per token |d tok_logp| <= 1e-5 + 2e-7 * exp(-tok_logp_ref): the project's fp32-vs-fp64 bound
on the generator's probabilities (test_generator_fp32_probs_match_fp64: rtol 1e-5, atol 2e-7) carried
over to the logarithm (d log p = dp / p).  A name's log-prob must be within the sum of its tokens'
bounds.  Ranks are compared wherever the fp64 target logit is at least 1e-6 away from every other
logit; closer positions may be at most 1 % of the scored ones."""
import json

import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models.params import init_params

pytestmark = pytest.mark.gpu


def _p64(params):
    return {k: v.double() for k, v in params.items()}


def make_rows(cfg, n, seed=1):
    """Random rows (np.random.default_rng(seed)) with an EOS forced into most of them so that n_tok
    covers 1 .. ML."""
    rng = np.random.default_rng(seed)
    ML = cfg.max_len
    rows = rng.integers(0, cfg.vocab, size=(n, ML + 1), dtype=np.uint8)
    rows[:, ML] = 0
    for b in range(n):
        k = b % (ML + 1)              # k < ML: EOS at k; k == ML: rows as drawn
        if k < ML:
            rows[b, k] = cfg.eos
    return rows


def check_against_oracle(res, cfg, p64, rows):
    """Device result vs the fp64 oracle under the module's bounds."""
    tok, name, n_tok, rank = cpu_ref.score(p64, cfg, rows)
    assert np.array_equal(res.n_tok, n_tok)
    mask = np.arange(cfg.max_len)[None, :] < n_tok[:, None]
    bound = np.where(mask, 1e-5 + 2e-7 * np.exp(-tok), 0.0)
    d = np.abs(res.tok_logp.astype(np.float64) - tok)
    print(f"tok_logp: max |d| {d.max():.3e}, max d/bound {np.max(d[mask] / bound[mask]):.3f}")
    assert np.all(d <= bound), (d.max(), np.max(d[mask] / bound[mask]))
    assert np.all(res.tok_logp[~mask] == 0) and np.all(res.rank[~mask] == -1)
    dn = np.abs(res.name_logp.astype(np.float64) - name)
    assert np.all(dn <= bound.sum(1)), dn.max()
    # ranks where the fp64 target logit is clear of every other logit
    _, _, x, tgt = cpu_ref.score_inputs(cfg, rows)
    logits = cpu_ref.forward(p64, cfg, torch.from_numpy(x)).numpy()
    xt = np.take_along_axis(logits, np.maximum(tgt, 0)[..., None], -1)
    gap = np.abs(logits - xt)
    np.put_along_axis(gap, np.maximum(tgt, 0)[..., None], np.inf, -1)
    clear = mask & (gap.min(-1) >= 1e-6)
    close = int(mask.sum() - clear.sum())
    print(f"rank: {close} of {int(mask.sum())} positions within 1e-6 of another logit")
    assert close <= 0.01 * mask.sum()
    assert np.array_equal(res.rank[clear], rank[clear])
    return tok, name, n_tok, rank


@pytest.mark.parametrize("L,E,H,V,ML,eos,N,max_batch", [
    (1, 64, 64, 64, 3, 0, 1, 64),            # the smallest legal tile, a single name
    (2, 128, 256, 256, 4, 255, 70, 4096),    # Bp crosses 64 -> 128, with pad rows
    (2, 128, 256, 256, 4, 0, 150, 64),       # three chunks, the last one partial
    (1, 72, 100, 64, 3, 63, 33, 64),         # E / H off the 64-grid through pad_config
])
def test_score_matches_fp64(L, E, H, V, ML, eos, N, max_batch):
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    cfg = GRUConfig(vocab=V, embed=E, hidden=H, layers=L, max_len=ML, sos=0, eos=eos, seed=6)
    params = init_params(cfg)
    rows = make_rows(cfg, N)
    gen = HipGenerator(cfg, params, max_batch=max_batch)
    assert gen.g.score_workspace_bytes() == 0          # nothing allocated before the first score()
    res = gen.score(rows)
    assert gen.g.score_workspace_bytes() > 0
    _, _, n_tok, _ = check_against_oracle(res, cfg, _p64(params), rows)
    if N > ML:
        assert sorted(set(n_tok.tolist())) == list(range(1, ML + 1))
    assert gen.g.read_error() == 0
    # flat rows are the same rows
    again = gen.score(rows.reshape(-1))
    assert np.array_equal(again.tok_logp, res.tok_logp) and np.array_equal(again.rank, res.rank)


@pytest.mark.parametrize("eos", [0, 63])
def test_device_probabilities_sum_to_one(eos):
    """All 4033 distinct valid rows of a vocab-64, max_len-2 model: 63 non-EOS first chars x 64 second
    chars, plus the one row that starts with EOS.  Under the per-token bound a two-token name's
    probability is off by at most 2e-5 + 2e-7 (1/p1 + 1/p2) relative; weighted by p1 p2 and summed over
    the rows that is 2e-5 + 2e-7 (63 + 64 (1 - p_eos)) < 4.6e-5 on the total, within the 1e-4 asked."""
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    rows = [[eos, 0, 0]] + [[a, b, 0] for a in range(64) if a != eos for b in range(64)]
    rows = np.array(rows, dtype=np.uint8)
    assert rows.shape[0] == 4033
    cfg = GRUConfig(vocab=64, embed=64, hidden=64, layers=2, max_len=2, sos=0, eos=eos, seed=6)
    params = init_params(cfg)
    gen = HipGenerator(cfg, params, max_batch=1024)
    res = gen.score(rows)
    total = np.exp(res.name_logp.astype(np.float64)).sum()
    print(f"sum exp(name_logp) - 1 = {total - 1:.3e}")
    assert abs(total - 1.0) <= 1e-4
    assert gen.g.read_error() == 0


def test_closed_loop_generated_rows():
    from gru_mpi_cuda_amd.engine.generator import HipGenerator, decode_names
    from gru_mpi_cuda_amd.utils.data import random_floats
    cfg = GRUConfig(vocab=256, embed=128, hidden=256, layers=2, max_len=10, sos=0, eos=0, seed=6)
    params = init_params(cfg)
    N = 65
    gen = HipGenerator(cfg, params, precision="fp32")
    rows = gen.generate(random_floats(N, cfg.max_len, seed=3))
    res = gen.score(rows)
    check_against_oracle(res, cfg, _p64(params), rows)
    lens = [len(nm) for nm in decode_names(rows, N, cfg.max_len)]
    assert res.n_tok.tolist() == [min(n + 1, cfg.max_len) for n in lens]
    assert gen.g.read_error() == 0


def test_reproducible_and_state_free():
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    from gru_mpi_cuda_amd.utils.data import random_floats
    cfg = GRUConfig(vocab=256, embed=128, hidden=256, layers=2, max_len=4, sos=0, eos=255, seed=6)
    params = init_params(cfg)
    rows = make_rows(cfg, 70)
    gen = HipGenerator(cfg, params, precision="fp32")
    a = gen.score(rows)
    b = gen.score(rows)                                  # graph replay
    gen.generate(random_floats(70, cfg.max_len, seed=2))
    c = gen.score(rows)
    for o in (b, c):
        assert np.array_equal(o.tok_logp, a.tok_logp) and np.array_equal(o.rank, a.rank)
        assert np.array_equal(o.name_logp, a.name_logp) and np.array_equal(o.n_tok, a.n_tok)
    gen.g.set_use_graph(False)                           # the same launches, issued directly
    d = gen.score(rows)
    assert np.array_equal(d.tok_logp, a.tok_logp) and np.array_equal(d.name_logp, a.name_logp)
    # a bf16 generator scores in exact fp32 too
    g16 = HipGenerator(cfg, params, precision="bf16")
    e = g16.score(rows)
    check_against_oracle(e, cfg, _p64(params), rows)
    check_against_oracle(a, cfg, _p64(params), rows)
    assert gen.g.read_error() == 0 and g16.g.read_error() == 0


def test_load_state_refreshes_every_table():
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    cfg = GRUConfig(vocab=256, embed=128, hidden=256, layers=2, max_len=4, sos=0, eos=0, seed=6)
    rows = make_rows(cfg, 40)
    other = init_params(cfg, seed=11)
    for precision in ("fp32", "bf16"):
        gen = HipGenerator(cfg, init_params(cfg), precision=precision)
        before = gen.score(rows)
        gen.load_state(other)
        got = gen.score(rows)
        fresh = HipGenerator(cfg, other, precision=precision).score(rows)
        assert not np.array_equal(before.tok_logp, got.tok_logp)
        assert np.array_equal(got.tok_logp, fresh.tok_logp) and np.array_equal(got.rank, fresh.rank)
        assert np.array_equal(got.name_logp, fresh.name_logp)
        assert gen.g.read_error() == 0


def test_guards():
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    cfg = GRUConfig(vocab=64, embed=64, hidden=64, layers=1, max_len=3, sos=0, eos=0, seed=6)
    gen = HipGenerator(cfg, init_params(cfg), max_batch=64)
    with pytest.raises(ValueError):
        gen.score(np.array([[1, 64, 0, 0]], dtype=np.uint8))
    assert gen.g.score_workspace_bytes() == 0            # raised before anything was launched
    ok = gen.score(np.array([[1, 0, 200, 0]], dtype=np.uint8))   # a byte >= vocab after the EOS is ignored
    assert ok.n_tok.tolist() == [2] and ok.rank[0, 2] == -1
    empty = gen.score(np.zeros((0, 4), dtype=np.uint8))
    assert empty.tok_logp.shape == (0, 3) and empty.rank.shape == (0, 3)
    assert empty.name_logp.shape == (0,) and empty.n_tok.shape == (0,) and empty.tokens == 0
    assert gen.g.read_error() == 0


def test_train_eval_hook(tmp_path):
    from gru_mpi_cuda_amd import cli
    from gru_mpi_cuda_amd.engine.generator import HipGenerator, encode_names
    from gru_mpi_cuda_amd.parallel import dist as gdist
    from gru_mpi_cuda_amd.utils import ckpt
    gdist.shutdown()                   # a context an earlier test left behind must not pick the device
    held = ["Anna", "Boris", "Clara", "Dmitri", "Elena", "Fyodor", "Galina"]
    data = tmp_path / "heldout.txt"
    data.write_text("\n".join(held) + "\n")
    met, m = str(tmp_path / "m.jsonl"), str(tmp_path / "model.bin")
    assert cli.main(["train", "--preset", "cpu_tiny", "--batch", "32", "--steps", "4", "--eval-data", str(data),
                     "--eval-every", "2", "--metrics", met, "--ckpt", m, "--lr", "0.01"]) == 0
    recs = [json.loads(l) for l in open(met)]
    assert [r["step"] for r in recs] == [2, 4] and all("eval_nll" in r for r in recs)
    cfg, params = ckpt.load(m)
    want = HipGenerator(cfg, params).score(encode_names(held, cfg))
    assert recs[-1]["eval_nll"] == pytest.approx(want.nll_per_char, abs=1e-6)
    assert recs[-1]["eval_names"] == 7 and recs[-1]["eval_top1"] == pytest.approx(want.top1)

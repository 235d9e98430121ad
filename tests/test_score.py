"""Teacher-forced scoring on the CPU: the oracle (cpu_ref.score), the row encoding, `cli score --cpu`
and `cli train --eval-data`."""
import json

import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd import cli
from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.engine.generator import ScoreResult, decode_names, encode_names
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.utils import ckpt


def _p64(cfg, seed=6):
    return {k: v.double() for k, v in init_params(cfg, seed=seed).items()}


def _rows(cfg, n, seed=1):
    """Random rows over the vocabulary with an EOS forced so that n_tok covers 1 .. ML."""
    rng = np.random.default_rng(seed)
    ML = cfg.max_len
    rows = rng.integers(0, cfg.vocab, size=(n, ML + 1), dtype=np.uint8)
    rows[:, ML] = 0
    for b in range(n):
        k = b % (ML + 1)              # k < ML: EOS at k; k == ML: no EOS at all
        non_eos = (cfg.eos + 1) % cfg.vocab
        rows[b, :ML][rows[b, :ML] == cfg.eos] = non_eos
        if k < ML:
            rows[b, k] = cfg.eos
    return rows


@pytest.mark.parametrize("eos", [0, 255])
def test_score_matches_hand_gather(eos):
    cfg = GRUConfig(vocab=256, embed=16, hidden=24, layers=2, max_len=5, sos=1, eos=eos)
    p = _p64(cfg)
    ML = cfg.max_len
    rows = _rows(cfg, 13)
    tok, name, n_tok, rank = cpu_ref.score(p, cfg, rows)
    assert tok.dtype == np.float64 and n_tok.dtype == np.int32 and rank.dtype == np.int32
    assert sorted(set(n_tok.tolist())) == list(range(1, ML + 1))
    assert n_tok[0] == 1 and rows[0, 0] == eos            # the first byte is EOS
    assert n_tok[ML] == ML and eos not in rows[ML, :ML]   # no EOS: cut off at ML
    for b in range(rows.shape[0]):
        nt = int(n_tok[b])
        c = rows[b].astype(np.int64)
        hit = np.flatnonzero(c[:ML] == eos)
        assert nt == (hit[0] + 1 if hit.size else ML)
        # by hand: inputs SOS, c0, c1, ... for this row alone, exactly nt steps
        x = torch.tensor([[cfg.sos] + c[:nt - 1].tolist()])
        logits = cpu_ref.forward(p, cfg, x)[0]
        lp = torch.log_softmax(logits, -1)
        want = np.array([lp[l, c[l]].item() for l in range(nt)])
        np.testing.assert_allclose(tok[b, :nt], want, rtol=0, atol=1e-13)
        assert np.all(tok[b, nt:] == 0) and np.all(rank[b, nt:] == -1)
        assert name[b] == pytest.approx(want.sum(), abs=1e-12)
        for l in range(nt):
            row = logits[l].numpy()
            t = c[l]
            r = int((row > row[t]).sum() + ((row == row[t]) & (np.arange(cfg.vocab) < t)).sum())
            assert rank[b, l] == r
    # fp32 params -> fp32 results, close to the oracle
    tok32, name32, n32, rank32 = cpu_ref.score({k: v.float() for k, v in p.items()}, cfg, rows)
    assert tok32.dtype == np.float32 and np.array_equal(n32, n_tok)
    np.testing.assert_allclose(tok32, tok, atol=1e-5)


def test_rank_ties_break_by_index():
    """All-zero weights: every logit equal, so the rank is the target's own index."""
    cfg = GRUConfig(vocab=64, embed=8, hidden=8, layers=1, max_len=3, sos=0, eos=63)
    p = {k: torch.zeros_like(v).double() for k, v in init_params(cfg).items()}
    rows = np.array([[5, 17, 63, 0], [63, 9, 9, 0]], dtype=np.uint8)
    tok, name, n_tok, rank = cpu_ref.score(p, cfg, rows)
    assert n_tok.tolist() == [3, 1]
    assert rank.tolist() == [[5, 17, 63], [63, -1, -1]]
    np.testing.assert_allclose(tok[0], -np.log(64.0), atol=1e-14)
    assert name[1] == pytest.approx(-np.log(64.0))


def all_rows_ml2(eos):
    """Every distinct valid row of a vocab-64, max_len-2 model: 63 non-EOS first chars x 64 second
    chars, plus the one row that starts with EOS."""
    rows = [[eos, 0, 0]]
    for a in range(64):
        if a == eos:
            continue
        for b in range(64):
            rows.append([a, b, 0])
    return np.array(rows, dtype=np.uint8)


@pytest.mark.parametrize("eos", [0, 63])
def test_probabilities_sum_to_one(eos):
    cfg = GRUConfig(vocab=64, embed=64, hidden=64, layers=2, max_len=2, sos=0, eos=eos)
    rows = all_rows_ml2(eos)
    assert rows.shape[0] == 4033 and len({bytes(r) for r in rows}) == 4033
    tok, name, n_tok, rank = cpu_ref.score(_p64(cfg), cfg, rows)
    assert n_tok[0] == 1
    assert abs(np.exp(name).sum() - 1.0) <= 1e-12


def test_score_is_generate_probability():
    """exp(name_logp) of a generated row is the product of the sampled chars' softmax probabilities:
    the row's empirical frequency over many uniforms approaches it."""
    cfg = GRUConfig(vocab=64, embed=8, hidden=8, layers=1, max_len=2, sos=0, eos=0)
    p = _p64(cfg)
    n = 4000
    out = cpu_ref.generate(p, cfg, np.random.default_rng(0).random(n * 2, dtype=np.float32))
    vals, counts = np.unique(out, axis=0, return_counts=True)
    k = counts.argmax()
    _, name, _, _ = cpu_ref.score(p, cfg, vals[k:k + 1])
    pr = float(np.exp(name[0]))
    assert abs(counts[k] / n - pr) < 5 * np.sqrt(pr * (1 - pr) / n) + 1e-3


def test_encode_decode_round_trip_and_errors():
    cfg = GRUConfig(vocab=256, max_len=5, eos=0)
    names = ["", "a", "Anna", "Boris", b"\xe9t\xe9".decode("latin-1")]
    rows = encode_names(names, cfg)
    assert rows.shape == (5, 6) and rows.dtype == np.uint8
    assert decode_names(rows, len(names), cfg.max_len) == names
    _, n_tok, _, _ = cpu_ref.score_inputs(cfg, rows)
    assert n_tok.tolist() == [1, 2, 5, 5, 4]          # "Boris": exactly ML chars, no EOS
    assert rows[3].tolist() == list(b"Boris") + [0]
    assert np.array_equal(encode_names([b"Anna"], cfg), rows[2:3])
    cfg2 = cfg.replace(eos=10)
    rows2 = encode_names(["ab"], cfg2)
    assert rows2[0].tolist() == [97, 98, 10, 0, 0, 0]
    assert decode_names(rows2, 1, 5) == ["ab\n"]
    with pytest.raises(ValueError):
        encode_names(["toolong"], cfg)
    with pytest.raises(ValueError):
        encode_names(["abc"], GRUConfig(vocab=64, max_len=5, eos=0))   # 'a' = 97 >= 64
    with pytest.raises(ValueError):
        encode_names(["a\nb"], cfg2)                   # holds the EOS byte
    with pytest.raises(ValueError):
        cpu_ref.score_inputs(GRUConfig(vocab=64, max_len=3, eos=0), np.array([[1, 64, 0, 0]], dtype=np.uint8))
    # ... but a byte >= vocab after the EOS is ignored, and flat rows are accepted
    _, nt, x, tgt = cpu_ref.score_inputs(GRUConfig(vocab=64, max_len=3, eos=0, sos=2),
                                         np.array([1, 0, 200, 0], dtype=np.uint8))
    assert nt.tolist() == [2] and x.tolist() == [[2, 1, 2]] and tgt.tolist() == [[1, 0, -1]]


def test_score_result_summaries():
    tok = np.array([[-1.0, -2.0, 0.0], [-3.0, 0.0, 0.0]], dtype=np.float32)
    rank = np.array([[0, 4, -1], [0, -1, -1]], dtype=np.int32)
    r = ScoreResult(tok, rank, tok.sum(1), np.array([2, 1], dtype=np.int32))
    assert r.tokens == 3 and r.nll_per_char == pytest.approx(2.0)
    assert r.perplexity == pytest.approx(np.exp(2.0)) and r.top1 == pytest.approx(2 / 3)


def _parse(text):
    out = []
    for ln in text.splitlines():
        name, lp, nt = ln.split("\t")
        out.append((name, float(lp), int(nt)))
    return out


def test_cli_score_cpu(tmp_path, capsys):
    cfg = GRUConfig(vocab=256, embed=16, hidden=24, layers=2, max_len=6, sos=0, eos=0)
    params = init_params(cfg, seed=3)
    m = str(tmp_path / "model.bin")
    ckpt.save(m, cfg, params)
    names = ["Anna", "Boris", "", "Dmitri", "El"]
    f = tmp_path / "names.txt"
    f.write_text("\n".join(names) + "\n")
    out = str(tmp_path / "scores.tsv")
    capsys.readouterr()
    assert cli.main(["score", "--ckpt", m, "--names", str(f), "--out", out, "--cpu"]) == 0
    summary = json.loads(capsys.readouterr().err.strip().splitlines()[-1])
    rows = encode_names(names, cfg)
    tok, name, n_tok, rank = cpu_ref.score(params, cfg, rows)
    want = ScoreResult(tok, rank, name, n_tok)
    got = _parse(open(out).read())
    assert [g[0] for g in got] == names
    assert [g[2] for g in got] == n_tok.tolist() == [5, 6, 1, 6, 3]
    np.testing.assert_allclose([g[1] for g in got], name, atol=1e-6)
    assert summary["names"] == 5 and summary["tokens"] == int(n_tok.sum())
    assert summary["nll_per_char"] == pytest.approx(want.nll_per_char, abs=1e-9)
    assert summary["perplexity"] == pytest.approx(want.perplexity, rel=1e-9)
    assert summary["top1"] == pytest.approx(want.top1) and summary["seconds"] >= 0

    # --raw of generated rows == --names of their decoded names (rows whose chars survive a text file)
    gen = cpu_ref.generate(params, cfg, np.random.default_rng(5).random(40 * cfg.max_len, dtype=np.float32))
    keep = [r for r in gen if not np.isin(r[:cfg.max_len], (10, 13)).any()]
    assert len(keep) >= 20
    gen = np.stack(keep)
    raw = tmp_path / "gen.bin"
    gen.tofile(str(raw))
    dec = decode_names(gen, gen.shape[0], cfg.max_len)
    nf = tmp_path / "gen.txt"
    nf.write_bytes(b"\n".join(d.encode("latin-1") for d in dec) + b"\n")
    o1, o2 = str(tmp_path / "a.tsv"), str(tmp_path / "b.tsv")
    assert cli.main(["score", "--ckpt", m, "--raw", str(raw), "--out", o1, "--cpu"]) == 0
    assert cli.main(["score", "--ckpt", m, "--names", str(nf), "--out", o2, "--cpu"]) == 0
    assert open(o1).read() == open(o2).read()
    assert len(_parse(open(o1).read())) == gen.shape[0]


@pytest.fixture
def fresh_ctx():
    """`train --cpu` picks its device when the process context is created: drop one left by an earlier test."""
    from gru_mpi_cuda_amd.parallel import dist as gdist
    gdist.shutdown()


def test_cli_train_eval(tmp_path, fresh_ctx):
    data = tmp_path / "heldout.txt"
    held = ["Anna", "Boris", "Clara", "Dmitri", "Elena", "Fyodor", "Galina"]
    data.write_text("\n".join(held) + "\n")
    met, m = str(tmp_path / "m.jsonl"), str(tmp_path / "model.bin")
    assert cli.main(["train", "--cpu", "--preset", "cpu_tiny", "--steps", "4", "--eval-data", str(data),
                     "--eval-every", "2", "--metrics", met, "--ckpt", m, "--lr", "0.01"]) == 0
    recs = [json.loads(l) for l in open(met)]
    assert [r["step"] for r in recs] == [2, 4]
    assert all("eval_nll" in r and r["eval_names"] == 7 for r in recs)
    assert all(r["eval_ppl"] == pytest.approx(np.exp(r["eval_nll"])) and 0 <= r["eval_top1"] <= 1 for r in recs)
    assert recs[0]["eval_nll"] != recs[1]["eval_nll"]
    cfg, params = ckpt.load(m)
    tok, name, n_tok, rank = cpu_ref.score(params, cfg, encode_names(held, cfg))
    want = ScoreResult(tok, rank, name, n_tok)
    assert recs[-1]["eval_nll"] == pytest.approx(want.nll_per_char, abs=1e-6)
    assert recs[-1]["eval_top1"] == pytest.approx(want.top1)


def test_cli_train_without_eval_is_unchanged(tmp_path, fresh_ctx):
    met = str(tmp_path / "m.jsonl")
    assert cli.main(["train", "--cpu", "--preset", "cpu_tiny", "--steps", "4", "--log-every", "2",
                     "--metrics", met]) == 0
    recs = [json.loads(l) for l in open(met)]
    assert [r["step"] for r in recs] == [2, 4] and not any("eval_nll" in r for r in recs)

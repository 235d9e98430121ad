"""`cli score` under the sampler (docs/DESIGN.md §4f): generate's flags on the CPU path."""
import json
import string

import numpy as np
import pytest

from gru_mpi_cuda_amd import cli
from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.engine.generator import ScoreResult, encode_names
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.utils import ckpt

LETTERS = string.ascii_letters
NAMES = ["Anna", "Boris", "Ma", "Mar7a", "Maria", "Dmitri"]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("score_ctl_cli")
    cfg = GRUConfig(vocab=256, embed=16, hidden=24, layers=2, max_len=6, sos=0, eos=0)
    params = init_params(cfg, seed=3)
    m = str(d / "model.bin")
    ckpt.save(m, cfg, params)
    f = d / "names.txt"
    f.write_text("\n".join(NAMES) + "\n")
    return cfg, params, m, str(f), d


def run(capsys, args):
    capsys.readouterr()
    assert cli.main(args) == 0
    return json.loads(capsys.readouterr().err.strip().splitlines()[-1])


def parse(path):
    return [ln.split("\t") for ln in open(path).read().splitlines()]


def test_cli_score_with_controls_and_constraints(model, capsys):
    cfg, params, m, f, d = model
    out = str(d / "a.tsv")
    summary = run(capsys, ["score", "--ckpt", m, "--names", f, "--out", out, "--cpu", "--temperature", "0.8", "--top-k", "200",
                           "--top-p", "0.999", "--charset", LETTERS, "--min-len", "3", "--max-name-len", "5"])
    rows = encode_names(NAMES, cfg)
    kw = dict(temperature=0.8, top_k=200, top_p=0.999, constraints=dict(charset=LETTERS, min_len=3, max_len=5))
    tok, name, n_tok, rank, nk = cpu_ref.score(params, cfg, rows, **kw)
    want = ScoreResult(tok, rank, name, n_tok, nk)
    got = parse(out)
    assert [g[0] for g in got] == NAMES and [int(g[2]) for g in got] == n_tok.tolist()
    # "Ma" ends before min_len, "Mar7a" holds a char outside the charset, "Dmitri" is longer than 5
    assert [g[1] for g in got if g[1] == "-inf"] == ["-inf"] * 3 and [g[0] for g in got if g[1] == "-inf"] == ["Ma", "Mar7a", "Dmitri"]
    fin = np.isfinite(name)
    np.testing.assert_allclose([float(g[1]) for g in got if g[1] != "-inf"], name[fin], atol=1e-6)
    assert summary["impossible"] == 3 == want.impossible and summary["names"] == 6
    assert summary["nll_per_char"] == float("inf") and summary["perplexity"] == float("inf")
    assert summary["top1"] == pytest.approx(want.top1) and summary["tokens"] == int(n_tok.sum())


def test_cli_score_prefix_flags_and_plain_summary(model, capsys):
    cfg, params, m, f, d = model
    rows = encode_names(NAMES, cfg)
    out = str(d / "b.tsv")
    summary = run(capsys, ["score", "--ckpt", m, "--names", f, "--out", out, "--cpu", "--prefix", "Ma"])
    name = cpu_ref.score(params, cfg, rows, prefix="Ma")[1]
    assert [g[1] == "-inf" for g in parse(out)] == np.isneginf(name).tolist() == [True, True, False, False, False, True]
    assert summary["impossible"] == 3
    pf = d / "prefixes.txt"
    pf.write_text("A\nBo\n")                                            # cycled over the names
    summary = run(capsys, ["score", "--ckpt", m, "--names", f, "--out", out, "--cpu", "--prefix-file", str(pf), "--pattern", "[A-Z]"])
    name = cpu_ref.score(params, cfg, rows, prefix=["A", "Bo"] * 3, constraints=dict(pattern="[A-Z]"))[1]
    assert [g[1] == "-inf" for g in parse(out)] == np.isneginf(name).tolist() == [False, False, True, True, True, True]
    np.testing.assert_allclose([float(g[1]) for g in parse(out)[:2]], name[:2], atol=1e-6)
    # no flag: the call as it was, and nothing is impossible
    summary = run(capsys, ["score", "--ckpt", m, "--names", f, "--out", out, "--cpu"])
    plain = cpu_ref.score(params, cfg, rows)[1]
    np.testing.assert_allclose([float(g[1]) for g in parse(out)], plain, atol=1e-6)
    assert summary["impossible"] == 0 and np.isfinite(summary["nll_per_char"])
    with pytest.raises(SystemExit):
        cli.main(["score", "--ckpt", m, "--names", f, "--cpu", "--prefix", "M", "--prefix-file", str(pf)])
    with pytest.raises(ValueError):
        cli.main(["score", "--ckpt", m, "--names", f, "--cpu", "--top-p", "0"])

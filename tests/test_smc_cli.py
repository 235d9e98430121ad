"""`cli conditional --cpu` prints the CPU rule's weighted particles of a saved checkpoint and a JSON summary."""
import json

import numpy as np
import pytest

from gru_mpi_cuda_amd import cli
from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.utils import ckpt


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    cfg = GRUConfig(vocab=128, embed=16, hidden=24, layers=2, max_len=5, sos=0, eos=10, seed=2)
    params = init_params(cfg)
    params["fc.weight"] = params["fc.weight"] * 4
    m = str(tmp_path_factory.mktemp("smc") / "model.bin")
    ckpt.save(m, cfg, params)
    return (m,) + tuple(ckpt.load(m))


def rule(cfg, params, prefixes, width, **kw):
    return cpu_ref.sample_conditional({k: v.float() for k, v in params.items()}, cfg, prefixes, width, **kw)


def test_conditional_cpu_prints_particles_and_a_summary(model, tmp_path, capsys):
    m, cfg, params = model
    assert cli.main(["conditional", "--cpu", "--ckpt", m, "--width", "4", "--runs", "3", "--prefix", "M", "--seed", "3",
                     "--charset", "Mabc"]) == 0
    cap = capsys.readouterr()
    res = rule(cfg, params, ["M"], 4, runs=3, seed=3, constraints=dict(charset="Mabc"))
    lines = cap.out.splitlines()
    assert len(lines) == 12
    w = res.weights()
    for k, ln in enumerate(lines):
        pre, i, name, weight = ln.split("\t")
        assert pre == "M" and int(i) == k and name == cli._escape(res.names()[0][k]) and name.startswith("M")
        assert set(name) <= set("Mabc") and weight == f"{float(w[0, k]):.6f}"
    assert abs(sum(float(ln.split("\t")[3]) for ln in lines) - 1) < 1e-4
    summ = [json.loads(ln) for ln in cap.err.splitlines() if ln.startswith("{")]
    assert len(summ) == 1 and set(summ[0]) == {"prefix", "log_z", "probability", "z_stderr", "ess", "resamples"}
    s = summ[0]
    assert s["prefix"] == "M" and s["log_z"] == float(res.log_z[0]) and s["probability"] == float(np.exp(res.log_z[0]))
    assert 0 < s["probability"] < 1 and s["z_stderr"] == float(res.z_stderr[0]) and 1 <= s["ess"] <= 12
    assert s["resamples"] == [int(v) for v in res.n_resampled[0]] and len(s["resamples"]) == 3


def test_conditional_prefix_file_out_and_one_run(model, tmp_path, capsys):
    m, cfg, params = model
    pf = tmp_path / "prefixes.txt"
    pf.write_text("a\n\n")
    out = str(tmp_path / "particles.tsv")
    assert cli.main(["conditional", "--cpu", "--ckpt", m, "--width", "3", "--prefix-file", str(pf), "--out", out,
                     "--temperature", "0.7", "--charset", "abc", "--min-len", "2", "--ess-threshold", "1"]) == 0
    cap = capsys.readouterr()
    assert cap.out == ""
    got = open(out).read().splitlines()
    res = rule(cfg, params, ["a", ""], 3, temperature=0.7, constraints=dict(charset="abc", min_len=2), ess_threshold=1.0)
    assert [ln.split("\t")[2] for ln in got] == [cli._escape(nm) for names in res.names() for nm in names] and len(got) == 6
    assert all(set(ln.split("\t")[2]) <= set("abc") and len(ln.split("\t")[2]) >= 2 for ln in got)
    summ = [json.loads(ln) for ln in cap.err.splitlines() if ln.startswith("{")]
    assert [s["prefix"] for s in summ] == ["a", ""] and all(s["z_stderr"] is None for s in summ)      # one run: no spread


def test_conditional_draw_resamples_the_pool(model, capsys):
    m, cfg, params = model
    args = ["conditional", "--cpu", "--ckpt", m, "--width", "8", "--runs", "2", "--charset", "abc", "--seed", "5"]
    assert cli.main(args + ["--draw", "7"]) == 0
    lines = capsys.readouterr().out.splitlines()
    res = rule(cfg, params, [""], 8, runs=2, seed=5, constraints=dict(charset="abc"))
    assert [ln.split("\t")[2] for ln in lines] == [cli._escape(nm) for nm in res.draw(7, 5)[0]] and len(lines) == 7
    assert all(ln.split("\t")[:2] == ["", str(k)] and ln.split("\t")[3] == f"{1 / 7:.6f}" for k, ln in enumerate(lines))
    assert set(ln.split("\t")[2] for ln in lines) <= set(cli._escape(nm) for nm in res.names()[0])
    assert cli.main(args + ["--draw", "7"]) == 0
    assert capsys.readouterr().out.splitlines() == lines      # deterministic in the seed


@pytest.mark.parametrize("extra", [["--top-k", "5"], ["--top-p", "0.9"], ["--logit-bias", "a=1"], ["--presence-penalty", "0.5"],
                                   ["--frequency-penalty", "0.5"], ["--temperature", "0"], ["--width", "33"],
                                   ["--runs", "0"], ["--ess-threshold", "2"], ["--draw", "0"]])
def test_conditional_rejects_what_the_rule_does_not_carry(model, extra, capsys):
    m, cfg, params = model
    with pytest.raises(SystemExit) as e:
        cli.main(["conditional", "--cpu", "--ckpt", m, "--charset", "abc"] + extra)
    assert e.value.code not in (0, None)
    assert capsys.readouterr().out == ""

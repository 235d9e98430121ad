"""`cli generate` / `cli score` with the soft-preference flags (docs/DESIGN.md §4h) on the CPU path."""
import json

import numpy as np
import pytest

from gru_mpi_cuda_amd import cli
from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.engine.generator import encode_names
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.utils import ckpt
from gru_mpi_cuda_amd.utils.data import random_floats

NAMES = ["Anna", "Boris", "Ma", "Maria", "Aaanna", "xqz"]
FLAGS = ["--logit-bias", "xqz=-2.5", "--logit-bias", "ae=0.5", "--logit-bias", "a=b=1.25", "--eos-bias", "-0.75",
         "--presence-penalty", "0.5", "--frequency-penalty", "1.5"]
# "a=b=1.25": the last '=' splits, so the chars are 'a', '=' and 'b'; values for the same char add up
KW = dict(logit_bias={"xqz": -2.5, "e": 0.5, "a": 1.75, "=b": 1.25, 0: -0.75}, presence_penalty=0.5, frequency_penalty=1.5)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("soft_ctl_cli")
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


def test_cli_generate_soft_flags_reach_cpu_ref(model, capsys):
    cfg, params, m, f, d = model
    N = 24
    rf = random_floats(N, cfg.max_len, seed=5)
    raw = str(d / "a.raw")
    run(capsys, ["generate", "--ckpt", m, "-n", str(N), "--seed", "5", "--cpu", "--raw-out", raw, "--out", str(d / "a.txt")] + FLAGS)
    got = np.fromfile(raw, dtype=np.uint8).reshape(N, cfg.max_len + 1)
    want = cpu_ref.generate(params, cfg, rf, **KW)
    assert (got == want).all() and not (want == cpu_ref.generate(params, cfg, rf)).all()
    # combined with a control and a constraint; one flag alone takes the controlled path too
    run(capsys, ["generate", "--ckpt", m, "-n", str(N), "--seed", "5", "--cpu", "--raw-out", raw, "--out", str(d / "a.txt"),
                 "--top-k", "40", "--charset", "abcdexyz=", "--frequency-penalty", "2"])
    got = np.fromfile(raw, dtype=np.uint8).reshape(N, cfg.max_len + 1)
    assert (got == cpu_ref.generate(params, cfg, rf, top_k=40, constraints=dict(charset="abcdexyz="), frequency_penalty=2.0)).all()
    run(capsys, ["generate", "--ckpt", m, "-n", str(N), "--seed", "5", "--cpu", "--raw-out", raw, "--out", str(d / "a.txt"),
                 "--eos-bias", "4"])
    got = np.fromfile(raw, dtype=np.uint8).reshape(N, cfg.max_len + 1)
    assert (got == cpu_ref.generate(params, cfg, rf, logit_bias={cfg.eos: 4.0})).all()


def test_cli_generate_exclude_emitted_passes_the_soft_flags_through(model, capsys):
    cfg, params, m, f, d = model
    N = 12
    raw = str(d / "e.raw")
    run(capsys, ["generate", "--ckpt", m, "-n", str(N), "--seed", "5", "--cpu", "--raw-out", raw, "--out", str(d / "e.txt"),
                 "--exclude-emitted", "--emit-batch", "12", "--logit-bias", "q=10000", "--eos-bias", "-10000"])
    got = np.fromfile(raw, dtype=np.uint8).reshape(N, cfg.max_len + 1)
    # the first batch is the API's call with an empty exclusion list; +1e4 on q leaves one name: the batch's
    # duplicates are dropped and the exclusion of "qqqqqq" lets the later batches draw other names
    first = cpu_ref.generate(params, cfg, random_floats(N, cfg.max_len, seed=5), constraints=dict(exclude=[]),
                             logit_bias={"q": 1e4, cfg.eos: -1e4})
    assert (first[:, :cfg.max_len] == ord("q")).all() and (got[0] == first[0]).all()
    assert len({bytes(r) for r in got}) == N


def test_cli_score_soft_flags_reach_cpu_ref(model, capsys):
    cfg, params, m, f, d = model
    out = str(d / "s.tsv")
    summary = run(capsys, ["score", "--ckpt", m, "--names", f, "--out", out, "--cpu", "--temperature", "0.8"] + FLAGS)
    rows = encode_names(NAMES, cfg)
    name = cpu_ref.score(params, cfg, rows, temperature=0.8, **KW)[1]
    got = [ln.split("\t") for ln in open(out).read().splitlines()]
    assert [g[0] for g in got] == NAMES
    np.testing.assert_allclose([float(g[1]) for g in got], name, atol=1e-6)
    assert summary["impossible"] == 0
    plain = cpu_ref.score(params, cfg, rows, temperature=0.8)[1]
    assert np.abs(name - plain).min() > 1e-3                               # every name's number moved
    run(capsys, ["score", "--ckpt", m, "--names", f, "--out", out, "--cpu", "--presence-penalty", "1"])
    got = [ln.split("\t") for ln in open(out).read().splitlines()]
    np.testing.assert_allclose([float(g[1]) for g in got], cpu_ref.score(params, cfg, rows, presence_penalty=1.0)[1], atol=1e-6)


@pytest.mark.parametrize("bad", ["abc", "=1", "abc=", "abc=x", "Ā=1"])
def test_cli_bad_logit_bias_is_an_argument_error(model, capsys, bad):
    cfg, params, m, f, d = model
    for cmd in (["generate", "--ckpt", m, "-n", "2", "--cpu"], ["score", "--ckpt", m, "--names", f, "--cpu"]):
        with pytest.raises(SystemExit) as e:
            cli.main(cmd + ["--logit-bias", bad])
        assert e.value.code == 2 and "--logit-bias" in capsys.readouterr().err


def test_cli_bad_soft_values_raise_value_error(model):
    cfg, params, m, f, d = model
    with pytest.raises(ValueError):
        cli.main(["score", "--ckpt", m, "--names", f, "--cpu", "--presence-penalty", "20000"])
    with pytest.raises(ValueError):
        cli.main(["generate", "--ckpt", m, "-n", "2", "--cpu", "--logit-bias", "a=nan"])

"""`cli distinct --cpu` prints the CPU rule's draws of a saved checkpoint."""
import pytest

from gru_mpi_cuda_amd import cli
from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.utils import ckpt


def expected_lines(cfg, params, prefixes, width, **kw):
    res = cpu_ref.sample_distinct({k: v.float() for k, v in params.items()}, cfg, prefixes, width, **kw)
    out = []
    for pre, names, lqs in zip(prefixes, res.names(), res.logq):
        assert 1 <= len(names) <= width and len(set(names)) == len(names)
        for k, nm in enumerate(names):
            out.append(f"{pre}\t{k}\t{cli._escape(nm)}\t{float(lqs[k]):.6f}")      # unprintable chars as \\xNN
    return out


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    cfg = GRUConfig(vocab=128, embed=16, hidden=24, layers=2, max_len=5, sos=0, eos=10, seed=2)
    params = init_params(cfg)
    params["fc.weight"] = params["fc.weight"] * 8
    m = str(tmp_path_factory.mktemp("sbs") / "model.bin")
    ckpt.save(m, cfg, params)
    return (m,) + tuple(ckpt.load(m))


def test_distinct_cpu_prints_the_rules_lines(model, tmp_path, capsys):
    m, cfg, params = model
    assert cli.main(["distinct", "--cpu", "--ckpt", m, "--width", "5", "--prefix", "Ma", "--seed", "3"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines == expected_lines(cfg, params, ["Ma"], 5, seed=3) and len(lines) == 5
    for k, ln in enumerate(lines):
        pre, draw, name, logq = ln.split("\t")
        assert pre == "Ma" and int(draw) == k and name.startswith("Ma") and float(logq) <= 0
    pf = tmp_path / "prefixes.txt"
    pf.write_text("Jo\n\nMaria\n")
    out = str(tmp_path / "draws.tsv")
    assert cli.main(["distinct", "--cpu", "--ckpt", m, "--width", "3", "--prefix-file", str(pf), "--out", out,
                     "--temperature", "0.7", "--charset", "JoMariaxyz", "--min-len", "2"]) == 0
    got = open(out).read().splitlines()
    assert got == expected_lines(cfg, params, ["Jo", "", "Maria"], 3, temperature=0.7,
                                 constraints=dict(charset="JoMariaxyz", min_len=2))
    assert [ln for ln in got if ln.startswith("Maria\t")] == [got[-1]]      # a full-length prefix: one row
    assert all(set(ln.split("\t")[2]) <= set("JoMariaxyz") and len(ln.split("\t")[2]) >= 2 for ln in got)


def test_distinct_is_deterministic_in_the_seed(model, capsys):
    m, cfg, params = model
    outs = []
    for seed in ("1", "1", "2"):
        assert cli.main(["distinct", "--cpu", "--ckpt", m, "--width", "4", "--seed", seed]) == 0
        outs.append(capsys.readouterr().out)
    assert outs[0] == outs[1] and outs[0] != outs[2]
    assert cli.main(["distinct", "--cpu", "--ckpt", m, "--width", "4"]) == 0      # the default seed is 0
    assert capsys.readouterr().out.splitlines() == expected_lines(cfg, params, [""], 4, seed=0)


def test_distinct_misuse(model, capsys):
    m, cfg, params = model
    for flag in ("--top-k", "--top-p", "--presence-penalty", "--logit-bias"):      # not in the parser: argparse exits
        with pytest.raises(SystemExit):
            cli.main(["distinct", "--cpu", "--ckpt", m, flag, "5"])
        capsys.readouterr()
    p32 = {k: v.float() for k, v in params.items()}
    for kw, word in ((dict(top_k=5), "top_k"), (dict(top_p=0.9), "top_p"), (dict(presence_penalty=1.0), "presence_penalty"),
                     (dict(frequency_penalty=1.0), "frequency_penalty"), (dict(logit_bias={"a": 1.0}), "logit_bias")):
        with pytest.raises(ValueError, match=f"does not take {word}"):
            cpu_ref.sample_distinct(p32, cfg, "Ma", 4, **kw)
    with pytest.raises(ValueError, match="temperature must be finite and > 0"):
        cli.main(["distinct", "--cpu", "--ckpt", m, "--temperature", "0"])
    with pytest.raises(ValueError, match="width must be an integer"):
        cli.main(["distinct", "--cpu", "--ckpt", m, "--width", "33"])
    with pytest.raises(ValueError, match="not allowed by the constraint"):
        cli.main(["distinct", "--cpu", "--ckpt", m, "--prefix", "Ma", "--charset", "xyz"])
    with pytest.raises(SystemExit):
        cli.main(["distinct", "--cpu", "--ckpt", m, "--prefix", "Ma", "--prefix-file", "x"])

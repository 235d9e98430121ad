"""`cli generate / beam / score --cpu` with --regex, --exclude-file and --exclude-emitted (docs/DESIGN.md §4g)."""
import itertools
import json
import re
import string

import numpy as np
import pytest

from gru_mpi_cuda_amd import cli
from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.engine.generator import encode_names
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.utils import ckpt
from gru_mpi_cuda_amd.utils.data import random_floats

CFG = GRUConfig(vocab=128, embed=16, hidden=24, layers=2, max_len=8, sos=0, eos=0, seed=2)
RX = "Ma[rl][a-z]{2,4}"


def saved(tmp_path):
    params = init_params(CFG)
    params["fc.weight"] = params["fc.weight"] * 8
    m = str(tmp_path / "model.bin")
    ckpt.save(m, CFG, params)
    return m, ckpt.load(m)


def names_of(rows, cfg):
    return [bytes(r[:cfg.max_len]).split(bytes([cfg.eos]))[0].decode("latin-1") for r in rows]


def test_generate_cpu_with_regex_and_exclude_file(tmp_path, capsys):
    m, (cfg, params) = saved(tmp_path)
    p32 = {k: v.float() for k, v in params.items()}
    N = 12
    assert cli.main(["generate", "--cpu", "--ckpt", m, "-n", str(N), "--seed", "3", "--regex", RX]) == 0
    cap = capsys.readouterr()
    names = cap.out.splitlines()
    assert len(names) == N and all(re.fullmatch(RX, nm) for nm in names), names
    assert json.loads(cap.err.strip().splitlines()[-1])["names"] == N
    rf = random_floats(N, cfg.max_len, seed=3)
    assert names == names_of(cpu_ref.generate(p32, cfg, rf, constraints=dict(regex=RX)), cfg)
    # the same call with its own output excluded: none of those names again, still in the language
    ex = tmp_path / "seen.txt"
    ex.write_text("\n".join(names) + "\n")
    assert cli.main(["generate", "--cpu", "--ckpt", m, "-n", str(N), "--seed", "3", "--regex", RX, "--exclude-file", str(ex),
                     "--top-k", "5"]) == 0
    novel = capsys.readouterr().out.splitlines()
    assert len(novel) == N and not set(novel) & set(names) and all(re.fullmatch(RX, nm) for nm in novel)
    assert novel == names_of(cpu_ref.generate(p32, cfg, rf, top_k=5, constraints=dict(regex=RX, exclude=names)), cfg)
    # a suffix with a prefix, a charset and a length bound
    assert cli.main(["generate", "--cpu", "--ckpt", m, "-n", "6", "--regex", ".*son", "--charset", string.ascii_lowercase + "J",
                     "--prefix", "J", "--max-name-len", "6"]) == 0
    got = capsys.readouterr().out.splitlines()
    assert len(got) == 6 and all(re.fullmatch("J[a-zJ]*son", nm) and len(nm) <= 6 for nm in got), got
    # --pattern and --regex exclude each other; a bad regex is a ValueError before any work
    with pytest.raises(SystemExit):
        cli.main(["generate", "--cpu", "--ckpt", m, "-n", "2", "--regex", RX, "--pattern", "M"])
    with pytest.raises(ValueError):
        cli.main(["generate", "--cpu", "--ckpt", m, "-n", "2", "--regex", "(a"])


def test_generate_cpu_exclude_emitted_gives_distinct_names(tmp_path, capsys):
    m, (cfg, params) = saved(tmp_path)
    flags = ["--charset", "abc", "--min-len", "1", "--max-name-len", "3"]              # a language of 39 names
    assert cli.main(["generate", "--cpu", "--ckpt", m, "-n", "30", "--seed", "3", *flags]) == 0
    assert len(set(capsys.readouterr().out.splitlines())) < 30                         # a sharp model repeats itself
    assert cli.main(["generate", "--cpu", "--ckpt", m, "-n", "30", "--seed", "3", *flags, "--exclude-emitted",
                     "--emit-batch", "10"]) == 0
    names = capsys.readouterr().out.splitlines()
    assert len(names) == 30 and len(set(names)) == 30 and all(re.fullmatch("[abc]{1,3}", nm) for nm in names), names
    # with an exclusion file on top; and more names than the language holds ends with a message
    ex = tmp_path / "seen.txt"
    ex.write_text("a\nb\nabc\n")
    assert cli.main(["generate", "--cpu", "--ckpt", m, "-n", "36", *flags, "--exclude-emitted", "--emit-batch", "12",
                     "--exclude-file", str(ex)]) == 0
    names = capsys.readouterr().out.splitlines()
    lang = {"".join(w) for L in (1, 2, 3) for w in itertools.product("abc", repeat=L)} - {"a", "b", "abc"}
    assert len(names) == 36 and set(names) == lang                     # every name of the language, once
    with pytest.raises(SystemExit, match="36 of 40"):
        cli.main(["generate", "--cpu", "--ckpt", m, "-n", "40", *flags, "--exclude-emitted", "--emit-batch", "12",
                  "--exclude-file", str(ex)])


def test_beam_and_score_cpu_with_regex(tmp_path, capsys):
    m, (cfg, params) = saved(tmp_path)
    p32 = {k: v.float() for k, v in params.items()}
    ex = tmp_path / "seen.txt"
    assert cli.main(["beam", "--cpu", "--ckpt", m, "--width", "5", "--regex", RX]) == 0
    lines = capsys.readouterr().out.splitlines()
    res = cpu_ref.beam_search(p32, cfg, [""], 5, constraints=dict(regex=RX))
    assert len(lines) == 5
    for k, (ln, nm) in enumerate(zip(lines, res.names()[0])):
        pre, rank, name, logp = ln.split("\t")
        assert pre == "" and int(rank) == k and name == nm and re.fullmatch(RX, name)
        assert logp == f"{float(res.logp[0, k]):.6f}"
    # the best name excluded: the rest move up
    best = lines[0].split("\t")[2]
    ex.write_text(best + "\n")
    assert cli.main(["beam", "--cpu", "--ckpt", m, "--width", "4", "--regex", RX, "--exclude-file", str(ex)]) == 0
    again = [ln.split("\t")[2] for ln in capsys.readouterr().out.splitlines()]
    assert again == [ln.split("\t")[2] for ln in lines[1:5]]
    # score: the beams under the regex they came from are finite and sum below 1; the excluded one is -inf
    nf = tmp_path / "names.txt"
    nf.write_text("\n".join([ln.split("\t")[2] for ln in lines] + ["Mbxyz", "Mar"]) + "\n")
    assert cli.main(["score", "--cpu", "--ckpt", m, "--names", str(nf), "--regex", RX, "--exclude-file", str(ex)]) == 0
    cap = capsys.readouterr()
    lp = [float(ln.split("\t")[1]) for ln in cap.out.splitlines()]
    assert lp[0] == -np.inf and np.isfinite(lp[1:5]).all() and lp[5] == -np.inf and lp[6] == -np.inf
    assert np.exp(lp[1:5]).sum() < 1 and json.loads(cap.err.strip().splitlines()[-1])["impossible"] == 3
    want = cpu_ref.score(p32, cfg, encode_names([ln.split("\t")[2] for ln in lines], cfg),
                         constraints=dict(regex=RX, exclude=[best]))
    assert [f"{float(v):.6f}" for v in want[1][1:5]] == [f"{v:.6f}" for v in lp[1:5]]

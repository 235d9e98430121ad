"""`cli generate --cpu` and `cli beam --cpu` with --pattern / --charset / --min-len / --max-name-len
(docs/DESIGN.md §4e)."""
import json
import string

import numpy as np

from gru_mpi_cuda_amd import cli
from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.utils import ckpt
from gru_mpi_cuda_amd.utils.data import random_floats

CFG = GRUConfig(vocab=128, embed=16, hidden=24, layers=2, max_len=8, sos=0, eos=0, seed=2)
FLAGS = ["--pattern", "M[aeiou].", "--charset", string.ascii_lowercase, "--min-len", "4", "--max-name-len", "6"]
KW = dict(pattern="M[aeiou].", charset=string.ascii_lowercase, min_len=4, max_len=6)


def saved(tmp_path):
    params = init_params(CFG)
    params["fc.weight"] = params["fc.weight"] * 8
    m = str(tmp_path / "model.bin")
    ckpt.save(m, CFG, params)
    return m, ckpt.load(m)


def obeys_flags(nm):
    return (4 <= len(nm) <= 6 and nm[0] == "M" and nm[1] in "aeiou" and
            all(c in string.ascii_lowercase for c in nm[2:]))


def test_generate_cpu_with_constraint_flags(tmp_path, capsys):
    m, (cfg, params) = saved(tmp_path)
    N = 12
    assert cli.main(["generate", "--cpu", "--ckpt", m, "-n", str(N), "--seed", "3", *FLAGS]) == 0
    cap = capsys.readouterr()
    names = cap.out.splitlines()
    assert len(names) == N and all(obeys_flags(nm) for nm in names), names
    assert json.loads(cap.err.strip().splitlines()[-1])["names"] == N
    want = cpu_ref.generate({k: v.float() for k, v in params.items()}, cfg, random_floats(N, cfg.max_len, seed=3),
                            constraints=KW)
    assert names == [bytes(r).split(bytes([cfg.eos]))[0].decode("latin-1") for r in want]
    # with a prefix and a sampling control, to a file
    out = str(tmp_path / "names.txt")
    assert cli.main(["generate", "--cpu", "--ckpt", m, "-n", "5", "--prefix", "Ma", "--top-k", "3", "--out", out, *FLAGS]) == 0
    got = open(out).read().splitlines()
    assert len(got) == 5 and all(obeys_flags(nm) and nm.startswith("Ma") for nm in got)
    # unconstrained output is what it was
    assert cli.main(["generate", "--cpu", "--ckpt", m, "-n", "4", "--seed", "3"]) == 0
    plain = cpu_ref.generate({k: v.float() for k, v in params.items()}, cfg, random_floats(4, cfg.max_len, seed=3))
    esc = lambda s: "".join(c if c.isprintable() else f"\\x{ord(c):02x}" for c in s)
    assert capsys.readouterr().out.splitlines() == [esc(bytes(r).split(b"\0")[0].decode("latin-1")) for r in plain]


def test_beam_cpu_with_constraint_flags(tmp_path, capsys):
    m, (cfg, params) = saved(tmp_path)
    assert cli.main(["beam", "--cpu", "--ckpt", m, "--width", "5", *FLAGS]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 5
    res = cpu_ref.beam_search({k: v.float() for k, v in params.items()}, cfg, [""], 5, constraints=KW)
    for k, (ln, nm) in enumerate(zip(lines, res.names()[0])):
        pre, rank, name, logp = ln.split("\t")
        assert pre == "" and int(rank) == k and name == nm and obeys_flags(name)
        assert logp == f"{float(res.logp[0, k]):.6f}"
    assert np.all(np.diff([float(ln.split("\t")[3]) for ln in lines]) <= 0)
    # exact-length names from prefixes, to a file; a constraint that leaves fewer names than the width
    pf = tmp_path / "prefixes.txt"
    pf.write_text("Ma\nMe\n")
    out = str(tmp_path / "beams.tsv")
    assert cli.main(["beam", "--cpu", "--ckpt", m, "--width", "3", "--prefix-file", str(pf), "--out", out,
                     "--pattern", "M[ae][xy]", "--min-len", "3", "--max-name-len", "3"]) == 0
    got = [ln.split("\t") for ln in open(out).read().splitlines()]
    assert [g[0] for g in got] == ["Ma", "Ma", "Me", "Me"]          # two names each: dead slots left out
    assert sorted(g[2] for g in got) == ["Max", "May", "Mex", "Mey"]

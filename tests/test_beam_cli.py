"""`cli beam --cpu` prints the CPU rule's beams of a saved checkpoint."""
from gru_mpi_cuda_amd import cli
from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.utils import ckpt


def expected_lines(cfg, params, prefixes, width):
    res = cpu_ref.beam_search({k: v.float() for k, v in params.items()}, cfg, prefixes, width)
    out = []
    for pre, names, lps in zip(prefixes, res.names(), res.logp):
        assert 1 <= len(names) <= width
        for k, nm in enumerate(names):
            out.append(f"{pre}\t{k}\t{nm}\t{float(lps[k]):.6f}")
    return out


def test_beam_cpu_prints_the_oracles_lines(tmp_path, capsys):
    cfg = GRUConfig(vocab=128, embed=16, hidden=24, layers=2, max_len=5, sos=0, eos=10, seed=2)
    params = init_params(cfg)
    params["fc.weight"] = params["fc.weight"] * 8
    m = str(tmp_path / "model.bin")
    ckpt.save(m, cfg, params)
    cfg2, loaded = ckpt.load(m)
    assert cli.main(["beam", "--cpu", "--ckpt", m, "--width", "5", "--prefix", "Ma"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines == expected_lines(cfg2, loaded, ["Ma"], 5) and len(lines) == 5
    assert all(ln.split("\t")[2].startswith("Ma") for ln in lines)
    pf = tmp_path / "prefixes.txt"
    pf.write_text("Jo\n\nMaria\n")
    out = str(tmp_path / "beams.tsv")
    assert cli.main(["beam", "--cpu", "--ckpt", m, "--width", "3", "--prefix-file", str(pf), "--out", out]) == 0
    got = open(out).read().splitlines()
    assert got == expected_lines(cfg2, loaded, ["Jo", "", "Maria"], 3)
    assert [ln for ln in got if ln.startswith("Maria\t")] == [got[-1]]      # a full-length prefix: one beam

"""`cli beam` / `cli distinct` accept --persist-constraints; with --cpu it has no effect on the output."""
import pytest

from gru_mpi_cuda_amd import cli
from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.utils import ckpt


@pytest.mark.parametrize("cmd,flag", [
    (["beam", "--width", "4", "--prefix", "Ma", "--min-len", "4", "--charset", "Mabcdefgh"], ["--persist-constraints"]),
    (["distinct", "--width", "4", "--prefix", "Ma", "--regex", "Ma(b|c|d)+", "--seed", "3"],
     ["--persist-constraints", "32"]),
])
def test_persist_constraints_parses_and_leaves_the_cpu_output_alone(tmp_path, capsys, cmd, flag):
    cfg = GRUConfig(vocab=256, embed=16, hidden=24, layers=1, max_len=6, sos=0, eos=10, seed=2)
    m = str(tmp_path / "model.bin")
    ckpt.save(m, cfg, init_params(cfg))
    base = [cmd[0], "--cpu", "--ckpt", m] + cmd[1:]
    assert cli.main(base) == 0
    plain = capsys.readouterr().out
    assert cli.main(base + flag) == 0
    assert capsys.readouterr().out == plain and len(plain.splitlines()) == 4

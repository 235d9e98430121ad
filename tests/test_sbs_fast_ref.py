"""The fast bf16 distinct names' reference module (models/sbs_fast_ref.py) and CPU twin
(cpu_ref.sample_distinct(round_operands=True)): the condition the GPU test relies on, the switch itself, and
`cli distinct --fast --cpu`."""
import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models import sbs_fast_ref as sf
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.models.seq_ref import bf16_round

KEYS = ("rows", "logq", "gumbel", "n_tok", "n_found")


@pytest.mark.parametrize("case", sf.CASES, ids=lambda c: c.name)
def test_at_most_half_of_the_prefixes_are_unsettled(case):
    t = sf.twin(case)
    cfg, p = sf.case_model(case)
    res = cpu_ref.sample_distinct({k: v.double() for k, v in p.items()}, cfg, list(case.prefixes), case.W,
                                  round_operands=True, **sf.case_kwargs(case))
    assert np.array_equal(res.rows, t["rows"]) and np.array_equal(res.n_found, t["n_found"])   # one rule, two entries
    unsettled = int((~t["settled"]).sum())
    print(f"{case.name}: D {t['D']:.3e}, largest scale {t['scale'].max():.3g}, unsettled {unsettled} of {len(case.prefixes)}")
    assert len(case.prefixes) >= 8 and 1e-4 < t["D"] < 5e-2
    assert 2 * unsettled <= len(case.prefixes)


def test_round_operands_on_bf16_exact_inputs_changes_nothing():
    """One step, matrices bf16-exact and the GRU's input side zero: h after the step is exactly 0, so every
    operand the switch rounds is bf16-exact already and the draw equals the default bit for bit; with the plain
    init the rounding shows.  cpu_ref.score takes the switch beside temperature and prefix."""
    cfg = GRUConfig(vocab=64, embed=16, hidden=32, layers=2, max_len=1, sos=0, eos=0, seed=3)
    p = {k: bf16_round(v).double() for k, v in init_params(cfg).items()}
    z = {k: (torch.zeros_like(v) if k.startswith(("weight_ih", "bias_ih", "bias_hh")) else v) for k, v in p.items()}
    kw = dict(seed=5, start=2 ** 33, temperature=0.8)
    a, b = cpu_ref.sample_distinct(z, cfg, ["", "0"], 5, **kw), cpu_ref.sample_distinct(z, cfg, ["", "0"], 5, round_operands=True, **kw)
    assert all(np.array_equal(getattr(a, k), getattr(b, k)) for k in KEYS)
    a, b = cpu_ref.sample_distinct(p, cfg, [""], 5, **kw), cpu_ref.sample_distinct(p, cfg, [""], 5, round_operands=True, **kw)
    assert 0 < np.abs(a.logq - b.logq).max() < 1e-2
    c = cpu_ref.sample_distinct(p, cfg, [""], 5, round_operands=False, **kw)
    assert all(np.array_equal(getattr(a, k), getattr(c, k)) for k in KEYS)
    sc = cpu_ref.score(p, cfg, b.rows[0], temperature=0.8, prefix=[""] * 5, round_operands=True)[1]
    assert np.abs(sc - b.logq[0]).max() < 1e-12       # logq is the rows' log-probability under the rounded model


def test_cli_distinct_fast_cpu(tmp_path):
    from gru_mpi_cuda_amd import cli
    from gru_mpi_cuda_amd.utils import ckpt
    cfg = GRUConfig(vocab=64, embed=16, hidden=32, layers=1, max_len=4, sos=0, eos=0, seed=2)
    path = str(tmp_path / "m.bin")
    ckpt.save(path, cfg, init_params(cfg))
    outs = []
    for extra in ([], ["--fast"]):
        out = str(tmp_path / f"d{len(extra)}.tsv")
        assert cli.main(["distinct", "--ckpt", path, "--width", "3", "--prefix", "0", "--cpu", "--seed", "1", "--out", out] + extra) == 0
        outs.append(open(out).read())
    assert len(outs[1].splitlines()) == 3 and outs[0] != outs[1]      # the rounded operands show in logq
    with pytest.raises(SystemExit):
        cli.main(["distinct", "--ckpt", path, "--cpu", "--fast", "--charset", "0123"])

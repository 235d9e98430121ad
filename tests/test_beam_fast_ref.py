"""The fast bf16 beam search's reference module (models/beam_fast_ref.py) and CPU twin
(cpu_ref.beam_search(round_operands=True)): the condition the GPU test relies on, and the switch itself."""
import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import beam_fast_ref as bf
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.models.seq_ref import bf16_round


@pytest.mark.parametrize("case", bf.CASES, ids=lambda c: c.name)
def test_at_most_half_of_the_prefixes_are_unsettled(case):
    t = bf.twin(case)
    cfg, p = bf.case_model(case)
    res = cpu_ref.beam_search({k: v.double() for k, v in p.items()}, cfg, list(case.prefixes), case.W, round_operands=True)
    assert np.array_equal(res.rows, t["rows"]) and np.array_equal(res.n_beams, t["n_beams"])   # one rule, two loops
    unsettled = int((~t["settled"]).sum())
    print(f"{case.name}: D {t['D']:.3e}, unsettled {unsettled} of {len(case.prefixes)}")
    assert len(case.prefixes) >= 8 and 1e-4 < t["D"] < 5e-2
    if case.compare:
        assert 2 * unsettled <= len(case.prefixes)


def test_round_operands_on_bf16_exact_inputs_changes_nothing():
    """One step, matrices bf16-exact and the GRU's input side zero: h after the step is exactly 0, so every
    operand the switch rounds is bf16-exact already and the search equals the default bit for bit; with the
    plain init the rounding shows."""
    cfg = GRUConfig(vocab=64, embed=16, hidden=32, layers=2, max_len=1, sos=0, eos=0, seed=3)
    p = {k: bf16_round(v).double() for k, v in init_params(cfg).items()}
    z = {k: (torch.zeros_like(v) if k.startswith(("weight_ih", "bias_ih", "bias_hh")) else v) for k, v in p.items()}
    a, b = cpu_ref.beam_search(z, cfg, ["", "0"], 5), cpu_ref.beam_search(z, cfg, ["", "0"], 5, round_operands=True)
    assert all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("rows", "logp", "n_tok", "n_beams"))
    a, b = cpu_ref.beam_search(p, cfg, [""], 5), cpu_ref.beam_search(p, cfg, [""], 5, round_operands=True)
    assert 0 < np.abs(a.logp - b.logp).max() < 1e-2
    c = cpu_ref.beam_search(p, cfg, [""], 5, round_operands=False)
    assert np.array_equal(a.logp, c.logp) and np.array_equal(a.rows, c.rows)

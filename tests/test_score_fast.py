"""cpu_ref.score(round_operands=True), the CPU twin of the bf16 fast scorer: its operand rounding is that of
seq_ref.fwd_ref(exact=False), and without the switch nothing changes."""
import numpy as np
import torch

from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import cpu_ref, seq_ref
from gru_mpi_cuda_amd.models.params import init_params


def test_round_operands_is_the_step_kernels_rounding():
    cfg = GRUConfig(vocab=64, embed=32, hidden=48, layers=1, max_len=5, sos=0, eos=0, seed=3)
    p = {k: v.double() for k, v in init_params(cfg).items()}
    B, T, rnd = 7, cfg.max_len, seq_ref.bf16_round
    x = torch.from_numpy(np.random.default_rng(0).integers(0, cfg.vocab, size=(B, T)))
    P = rnd(p["embedding"]) @ rnd(p["weight_ih_l0"]).T + p["bias_ih_l0"]
    HS = seq_ref.fwd_ref(rnd(p["weight_hh_l0"]), p["bias_hh_l0"], T, B, P=P, ids=x.T.contiguous())["HS"]
    want = rnd(HS[1:]).transpose(0, 1) @ rnd(p["fc.weight"]).T + p["fc.bias"]
    got = cpu_ref.forward(p, cfg, x, round_operands=True)
    assert torch.allclose(got, want, rtol=0, atol=1e-12)
    exact = cpu_ref.forward(p, cfg, x)
    assert 1e-6 < (got - exact).abs().max() < 1e-2      # the rounding is there, and it is bf16-sized
    rows = np.zeros((B, T + 1), np.uint8)
    rows[:, :T] = x.numpy()
    a, b = cpu_ref.score(p, cfg, rows), cpu_ref.score(p, cfg, rows, round_operands=False)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    fast = cpu_ref.score(p, cfg, rows, round_operands=True)
    assert np.array_equal(fast[2], a[2]) and 0 < np.abs(fast[0] - a[0]).max() < 1e-2

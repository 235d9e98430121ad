"""GemmVariants.small_ring inside the training step: the P table (prologue launch), dW_ih0 / dEmb and the
held dW_fc K-slices (the grouped launch after the backward, StepLdsVariants.dwfc_group) run through the
ring body by default and through the burst body at small_ring = 0.

The ring keeps every accumulator's MFMA order and every slab, so the loss of each step, every gradient
and the parameters after Adam steps must be bitwise equal between the two: a difference is a bug (a slot
read before its block landed or overwritten while it was read), not rounding.

One-layer H = 512, E = 512, V = 256 at 2048 tokens (B = 64, T = 32 and B = 128, T = 16): dW_fc is two
1024-deep K-slices, 16 k-blocks each through the ring, beside the 4-block dW_ih0 / dEmb jobs.  H = 256 takes
other routes and must not move either.
"""
import pytest
import torch

from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.utils.data import NameStream

pytestmark = pytest.mark.gpu


def _cfg(B, T, H=512, E=512):
    return GRUConfig(vocab=256, embed=E, hidden=H, layers=1, batch=B, seq=T, seed=41, keep_grads=True)


def _both(run, cfg):
    """run(trainer) -> result under small_ring = 0 and under the default, on the same seeded parameters."""
    from gru_mpi_cuda_amd.engine.trainer import HipTrainer
    from gru_mpi_cuda_amd.ops import load_ext
    C = load_ext()
    saved = C.gemm_variants()
    assert saved["small_ring"] in (3, 4) and C.step_lds_variants()["dwfc_group"] == 1
    params = init_params(cfg)
    out = []
    try:
        for v in (0, saved["small_ring"]):
            C.set_gemm_variants(dict(small_ring=v))
            tr = HipTrainer(cfg, params=params)
            out.append(run(tr))
            torch.cuda.synchronize()
            assert tr.t.read_error() == 0
    finally:
        C.set_gemm_variants(saved)
    return out


def _steps(batches):
    def run(tr):
        losses, g = [], None
        for i, (x, y) in enumerate(batches):
            tr.step(x, y)
            losses.append(tr.loss())
            if i == 0:
                g = {k: t.clone() for k, t in tr.grad_dict().items()}
        torch.cuda.synchronize()
        return g, losses, tr.params.clone(), tr.t.plan()
    return run


def _assert_same(a, b):
    (g0, l0, p0, plan0), (g1, l1, p1, plan1) = a, b
    print(f"SMALLRING losses {l0} / {l1}")
    assert plan0 == plan1, (plan0, plan1)
    assert l0 == l1, (l0, l1)
    assert all(x == x for x in l0)
    assert g0.keys() == g1.keys() and len(g0) > 0
    for k in g0:
        assert torch.equal(g0[k], g1[k]), f"grad {k}: {int((g0[k] != g1[k]).sum())} of {g0[k].numel()} elements differ"
    assert torch.equal(p0, p1), f"params: {int((p0 != p1).sum())} elements differ"


@pytest.mark.parametrize("B,T", [(64, 32), (128, 16)])
def test_small_ring_steps_bitwise(B, T):
    cfg = _cfg(B, T)
    ds = NameStream(B, T, seed=42)
    batches = [ds.next() for _ in range(3)]
    a, b = _both(_steps(batches), cfg)
    assert "bwd0=persistent" in a[3], a[3]
    _assert_same(a, b)


def test_small_ring_multi_step_graph():
    """tr.steps([...]) with three batches (one graph) against three single steps, under both bodies."""
    B, T = 64, 32
    cfg = _cfg(B, T)
    ds = NameStream(B, T, seed=43)
    batches = [ds.next() for _ in range(3)]

    def run(tr):
        from gru_mpi_cuda_amd.engine.trainer import HipTrainer
        tr.steps(batches)
        torch.cuda.synchronize()
        one = HipTrainer(cfg, params=init_params(cfg))
        for x, y in batches:
            one.step(x, y)
        torch.cuda.synchronize()
        assert one.t.plan() == tr.t.plan()
        assert one.t.read_error() == 0
        assert torch.equal(one.params, tr.params), "multi-step graph differs from three single steps"
        assert one.loss() == tr.loss()
        return tr.params.clone(), tr.loss()

    (p0, s0), (p1, s1) = _both(run, cfg)
    assert torch.equal(p0, p1), f"{int((p0 != p1).sum())} elements differ"
    assert s0 == s1, (s0, s1)


def test_small_ring_h256_step():
    """One step at H = 256, E = 64 (other kernels for the recurrences and the head): nothing else moved."""
    B, T = 64, 8
    cfg = _cfg(B, T, H=256, E=64)
    ds = NameStream(B, T, seed=44)
    a, b = _both(_steps([ds.next()]), cfg)
    _assert_same(a, b)

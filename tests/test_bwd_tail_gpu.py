"""StepLdsVariants.bwd_tail: the sum of the persistent backward's dP row-block partials (-> the bf16
dP / dP^T GEMM operands), the sum of the loss partials and the step-counter bump run as the tail of the
backward launch itself (gru_bwd_seq_tail) against the same three jobs in the reduce_multi launch after it
(bwd_tail = 0).

Both sum the same slabs in the same order (slab 0, += 1, 2, ..; the loss through one shared device
function), so the loss of every step, every gradient and the weights after Adam steps must be bitwise
equal: any difference is a bug (a slab read before it was complete, a stale line, a wrong share of the
rows), not rounding.  Only the single-GPU one-graph step() takes the tail, and only where the reduce launch
would hold nothing else; the plan string says which path a trainer took (" dP=bwd-tail").

The trainer pads the batch to a multiple of 64 rows, so it never runs fewer than two 32-row blocks:
B = 32 and B = 40 run 2 row blocks (128-row shares), B = 96 runs 4 (128 rows), B = 160 runs 6, which does
not divide V = 256 into whole shares -- that one and the clipped step must keep the reduce launch.
"""
import pytest
import torch

from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.utils.data import NameStream

pytestmark = pytest.mark.gpu

TAIL_TAG = "dP=bwd-tail"


def _cfg(B, T, **kw):
    return GRUConfig(vocab=256, embed=512, hidden=512, layers=1, batch=B, seq=T, seed=31, keep_grads=True, **kw)


def _both(run, cfg, nrb, tail):
    """run(trainer) -> result, once per variant (bwd_tail = 0, 1) on the same seeded parameters.
    nrb: the 32-row blocks the padded batch makes; tail: whether bwd_tail = 1 takes the tail here."""
    from gru_mpi_cuda_amd.engine.trainer import HipTrainer
    from gru_mpi_cuda_amd.ops import load_ext
    C = load_ext()
    saved = C.step_lds_variants()
    params = init_params(cfg)
    out = []
    try:
        for v in (0, 1):
            C.set_step_lds_variants(dict(bwd_tail=v))
            tr = HipTrainer(cfg, params=params)
            assert tr.t.padded_batch() // 32 == nrb
            plan = tr.t.plan()
            assert "bwd0=persistent+dWhh+dP" in plan, plan
            assert (TAIL_TAG in plan) == (v == 1 and tail), plan
            out.append(run(tr))
            torch.cuda.synchronize()
            plan = tr.t.plan()   # now what the recorded step did
            assert (TAIL_TAG in plan) == (v == 1 and tail), plan
            assert tr.t.read_error() == 0
    finally:
        C.set_step_lds_variants(saved)
    return out


def _three_steps(batches):
    def run(tr):
        losses, g = [], None
        for i, (x, y) in enumerate(batches):
            tr.step(x, y)
            losses.append(tr.loss())
            if i == 0:
                g = {k: t.clone() for k, t in tr.grad_dict().items()}
        torch.cuda.synchronize()
        return g, losses, tr.params.clone()
    return run


def _assert_same(a, b):
    (g0, l0, p0), (g1, l1, p1) = a, b
    print(f"BWDTAIL losses {l0} / {l1}")
    assert l0 == l1, (l0, l1)
    assert g0.keys() == g1.keys() and len(g0) > 0
    for k in g0:
        assert torch.equal(g0[k], g1[k]), f"grad {k}: {int((g0[k] != g1[k]).sum())} of {g0[k].numel()} elements differ"
    assert torch.equal(p0, p1), f"params after three steps: {int((p0 != p1).sum())} elements differ"


@pytest.mark.parametrize("B,T,xcd,clip,nrb,tail", [
    (32, 2, "1", 0.0, 2, True),     # the smallest batch: padded to two row blocks, 128-row shares
    (64, 3, "1", 0.0, 2, True),     # two row blocks, 128-row shares
    (128, 3, "1", 0.0, 4, True),    # four row blocks
    (256, 2, "1", 0.0, 8, True),    # the headline grid: 8 row blocks on 8 XCDs
    (256, 2, "0", 0.0, 8, True),    # placement independence
    (256, 1, "1", 0.0, 8, True),    # the loop's s > 0 branch never runs
    (40, 3, "1", 0.0, 2, True),     # padded to 64 rows with ignore-labelled rows
    (96, 3, "1", 0.0, 4, True),     # padded to 128 rows: four row blocks, a quarter of them ignore-labelled
    (160, 3, "1", 0.0, 6, False),   # 6 row blocks do not divide V: the tag must be absent, results still equal
    (64, 3, "1", 1.0, 2, False),    # clipping: the reduce launch has other jobs: tag absent, results equal
])
def test_bwd_tail_bitwise(B, T, xcd, clip, nrb, tail, monkeypatch):
    monkeypatch.setenv("GK_XCD_LOCAL", xcd)
    cfg = _cfg(B, T, clip_norm=clip)
    ds = NameStream(B, T, seed=32)
    batches = [ds.next() for _ in range(3)]
    a, b = _both(_three_steps(batches), cfg, nrb, tail)
    _assert_same(a, b)


def test_bwd_tail_multi_step_graph():
    """tr.steps([...]) with three batches (one graph) against three single steps, tail on and off: the
    flags are zeroed again between the steps of one graph, and the tail's epoch is T + 1 in each."""
    B, T = 64, 3
    cfg = _cfg(B, T)
    ds = NameStream(B, T, seed=33)
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

    (p0, s0), (p1, s1) = _both(run, cfg, 2, True)
    assert torch.equal(p0, p1), f"{int((p0 != p1).sum())} elements differ"
    assert s0 == s1, (s0, s1)

"""StepLdsVariants.fb_one: the persistent forward (with the FC head as its tail) and the persistent backward
(with the dP / loss / step-counter tail) of the one-layer H = 512, V = 256 single-GPU step as ONE launch
(gru_fb_one) against the two launches (fb_one = 0).

The merged kernel runs the same step loops and tails (one source text), so the loss of every step, every
gradient and the weights after Adam steps must be bitwise equal: any difference is a bug (a stale line, a
hand-over passed early, a wiped flag line, the two exchange rings on one region), not rounding.  Only the
step that takes both tails, with T >= 2, takes the merged launch; the plan string says which path a trainer
took (" fb=one-launch"), predicted at construction and then reporting the last recorded step.

The trainer pads the batch to a multiple of 64 rows: B = 32 and B = 40 run 2 row blocks, B = 96 runs 4,
B = 160 runs 6 (no whole shares of V = 256: no backward tail, so no merged launch).
"""
import pytest
import torch

from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.utils.data import NameStream

pytestmark = pytest.mark.gpu

ONE_TAG = "fb=one-launch"


def _cfg(B, T, **kw):
    return GRUConfig(vocab=256, embed=512, hidden=512, layers=1, batch=B, seq=T, seed=41, keep_grads=True, **kw)


def _both(run, cfg, one, extra=None):
    """run(trainer) -> result, once per variant (fb_one = 0, 1) on the same seeded parameters.
    one: whether fb_one = 1 takes the merged launch here; extra: other variant fields held for both runs."""
    from gru_mpi_cuda_amd.engine.trainer import HipTrainer
    from gru_mpi_cuda_amd.ops import load_ext
    C = load_ext()
    saved = C.step_lds_variants()
    params = init_params(cfg)
    out = []
    try:
        for v in (0, 1):
            C.set_step_lds_variants(dict(extra or {}, fb_one=v))
            tr = HipTrainer(cfg, params=params)
            plan = tr.t.plan()
            assert "bwd0=persistent+dWhh+dP" in plan, plan
            assert (ONE_TAG in plan) == (v == 1 and one), plan
            out.append(run(tr))
            torch.cuda.synchronize()
            plan = tr.t.plan()   # now what the recorded step did
            assert (ONE_TAG in plan) == (v == 1 and one), plan
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
    print(f"FBONE losses {l0} / {l1}")
    assert l0 == l1, (l0, l1)
    assert g0.keys() == g1.keys() and len(g0) > 0
    for k in g0:
        assert torch.equal(g0[k], g1[k]), f"grad {k}: {int((g0[k] != g1[k]).sum())} of {g0[k].numel()} elements differ"
    assert torch.equal(p0, p1), f"params after three steps: {int((p0 != p1).sum())} elements differ"


def _run_case(monkeypatch, B, T, xcd, one, clip=0.0, extra=None):
    monkeypatch.setenv("GK_XCD_LOCAL", xcd)
    cfg = _cfg(B, T, clip_norm=clip)
    ds = NameStream(B, T, seed=42)
    batches = [ds.next() for _ in range(3)]
    a, b = _both(_three_steps(batches), cfg, one, extra)
    _assert_same(a, b)


@pytest.mark.parametrize("B,T,xcd", [
    (32, 2, "1"),     # the smallest batch (two row blocks) and the smallest T the merged launch takes
    (64, 3, "1"),
    (128, 3, "1"),    # four row blocks
    (256, 2, "1"),    # the headline grid: 8 row blocks on 8 XCDs
    (256, 2, "0"),    # every row block on the release / acquire hand-over and the write-through exchange
    (256, 6, "1"),    # T above both ring depths (4 and 2): both rings wrap inside one launch
    (40, 3, "1"),     # padded to 64 rows with ignore-labelled rows
    (96, 3, "1"),     # padded to 128 rows, a quarter of them ignore-labelled
])
def test_fb_one_bitwise(B, T, xcd, monkeypatch):
    _run_case(monkeypatch, B, T, xcd, True)


@pytest.mark.parametrize("B,T,clip,extra", [
    (256, 1, 0.0, None),                 # T = 1: two launches
    (160, 3, 0.0, None),                 # 6 row blocks: no backward tail
    (64, 3, 1.0, None),                  # clipping: no backward tail
    (64, 3, 0.0, {"fc_tail": 0}),        # the FC head on its own launch
    (64, 3, 0.0, {"bwd_tail": 0}),       # the reduce launch kept
])
def test_fb_one_fallbacks(B, T, clip, extra, monkeypatch):
    """Where the step is not eligible the tag is absent and fb_one = 1 records what fb_one = 0 records."""
    _run_case(monkeypatch, B, T, "1", False, clip, extra)


def test_fb_one_multi_step_graph():
    """tr.steps([...]) with four batches (one graph: both parities of the flag sets, twice) against four
    single steps, merged launch on and off; then a fifth single step on the trainer that ran the graph.
    Every step feeds the next through Adam, so equal parameters after the last step mean every step was
    equal; the single steps' losses are compared one by one as well."""
    B, T = 64, 3
    cfg = _cfg(B, T)
    ds = NameStream(B, T, seed=43)
    batches = [ds.next() for _ in range(5)]

    def run(tr):
        from gru_mpi_cuda_amd.engine.trainer import HipTrainer
        tr.steps(batches[:4])
        torch.cuda.synchronize()
        one = HipTrainer(cfg, params=init_params(cfg))
        losses = []
        for x, y in batches[:4]:
            one.step(x, y)
            losses.append(one.loss())
        torch.cuda.synchronize()
        assert one.t.plan() == tr.t.plan()
        assert one.t.read_error() == 0
        assert torch.equal(one.params, tr.params), "four-step graph differs from four single steps"
        assert one.loss() == tr.loss()
        for t2 in (tr, one):
            t2.step(*batches[4])
        torch.cuda.synchronize()
        assert torch.equal(one.params, tr.params), "fifth step differs after the four-step graph"
        assert one.loss() == tr.loss()
        losses.append(tr.loss())
        return tr.params.clone(), losses

    (p0, l0), (p1, l1) = _both(run, cfg, True)
    print(f"FBONE graph losses {l0} / {l1}")
    assert l0 == l1, (l0, l1)
    assert torch.equal(p0, p1), f"{int((p0 != p1).sum())} elements differ"


def test_fb_one_matches_fp64_oracle():
    """One merged-launch step at (64, 3) against the fp64 manual-BPTT oracle, with the tolerances of
    tests/test_engine_gpu.py::test_trainer_grads_match_cpu (loss 1 % relative, each gradient 4 % in norm)."""
    from gru_mpi_cuda_amd.engine.trainer import HipTrainer
    from gru_mpi_cuda_amd.ops import load_ext
    assert load_ext().step_lds_variants()["fb_one"] == 1
    cfg = _cfg(64, 3)
    params = init_params(cfg)
    x, y = NameStream(64, 3, seed=44).next()
    tr = HipTrainer(cfg, params=params)
    tr.step(x, y)
    torch.cuda.synchronize()
    assert ONE_TAG in tr.t.plan(), tr.t.plan()
    assert tr.t.read_error() == 0
    g = tr.grad_dict()
    p64 = {k: v.double() for k, v in params.items()}
    ref_loss, ref_g = cpu_ref.manual_backward(p64, cfg, torch.from_numpy(x), torch.from_numpy(y))
    print(f"FBONE oracle loss {tr.loss()} / {float(ref_loss)}")
    assert abs(tr.loss() - float(ref_loss)) < 1e-2 * float(ref_loss)
    for k in ref_g:
        a, b = g[k].double().cpu(), ref_g[k].double().cpu()
        e = float((a - b).norm() / b.norm().clamp_min(1e-12))
        print(f"FBONE oracle {k}: rel err {e:.5f}")
        assert e < 0.04, f"{k}: rel err {e:.4f}"

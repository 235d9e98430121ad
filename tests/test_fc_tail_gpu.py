"""StepLdsVariants.fc_tail: the fused V = 256 FC head run as the tail of the persistent forward launch
(gru_fwd_seq_tail: after its last timestep every forward workgroup runs the fc_xent blocks of its own
row block) against the same head in its own launch after the forward (fc_tail = 0).

Both run ONE device function (csrc/kernels/fc_block.h, fc_xent_v256_block) over the same token blocks,
so the loss, every gradient and the weights after Adam steps must be bitwise equal: any difference is
a bug (a block read before its rows were complete, a stale line, a wrong block index), not rounding.
fwd_fc = 0 and fc_flash = 0 in both runs; the plan string says which path a trainer took.

The last test launches the stand-alone fc_xent (the wrapper around that function) on the cases of
tests/test_head_gpu.py::test_fc_xent_v256 against an fp32 torch reference, within that test's
tolerances (gru_mpi_cuda_amd.models.head_ref).
"""
import functools

import pytest
import torch

from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import head_ref as hr
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.utils.data import NameStream

pytestmark = pytest.mark.gpu

TAIL_TAG = "head=fwd-tail"


def _cfg(B, T, **kw):
    return GRUConfig(vocab=256, embed=512, hidden=512, layers=1, batch=B, seq=T, seed=21, **kw)


def _both(run, cfg):
    """run(trainer) -> result, once per variant (fc_tail = 0, 1) on the same seeded parameters."""
    from gru_mpi_cuda_amd.engine.trainer import HipTrainer
    from gru_mpi_cuda_amd.ops import load_ext
    C = load_ext()
    saved = C.step_lds_variants()
    params = init_params(cfg)
    out = []
    try:
        for v in (0, 1):
            C.set_step_lds_variants(dict(fc_tail=v, fwd_fc=0, fc_flash=0))
            tr = HipTrainer(cfg, params=params)
            plan = tr.t.plan()
            assert (TAIL_TAG in plan) == (v == 1), plan
            assert "fwd=persistent+fc" not in plan, plan
            out.append(run(tr))
            torch.cuda.synchronize()
            assert tr.t.read_error() == 0
    finally:
        C.set_step_lds_variants(saved)
    return out


def _fb_then_steps(batches):
    def run(tr):
        tr.forward_backward(*batches[0])
        g = {k: t.clone() for k, t in tr.grad_dict().items()}
        loss = tr.loss()
        for x, y in batches:
            tr.step(x, y)
        torch.cuda.synchronize()
        return g, loss, tr.params.clone(), tr.loss()
    return run


def _assert_same(a, b):
    (g0, l0, p0, s0), (g1, l1, p1, s1) = a, b
    assert l0 == l1, (l0, l1)
    assert g0.keys() == g1.keys()
    for k in g0:
        assert torch.equal(g0[k], g1[k]), f"grad {k}: {int((g0[k] != g1[k]).sum())} of {g0[k].numel()} elements differ"
    assert torch.equal(p0, p1), f"params after three steps: {int((p0 != p1).sum())} elements differ"
    assert s0 == s1, (s0, s1)


@pytest.mark.parametrize("B,T,xcd", [
    (32, 32, "1"),    # one row block, one item per workgroup
    (32, 5, "1"),     # workgroups with no item
    (64, 40, "1"),    # workgroups with two items
    (96, 8, "1"),     # 3 row blocks that cannot be XCD-local: write-through HSb and sc1 X loads
    (256, 8, "0"),    # the write-through path forced at the headline's grid
    (40, 8, "1"),     # padded to 64 rows: ignore-labelled rows, inv_count
])
def test_fc_tail_bitwise(B, T, xcd, monkeypatch):
    monkeypatch.setenv("GK_XCD_LOCAL", xcd)
    cfg = _cfg(B, T)
    ds = NameStream(B, T, seed=22)
    batches = [ds.next() for _ in range(3)]
    a, b = _both(_fb_then_steps(batches), cfg)
    _assert_same(a, b)


def test_fc_tail_carry_hidden():
    """h0: the carried state feeds the first step; two consecutive batches before the comparison."""
    B, T = 64, 8
    cfg = _cfg(B, T, carry_hidden=True)
    ds = NameStream(B, T, seed=23)
    batches = [ds.next() for _ in range(3)]

    def run(tr):
        tr.forward_backward(*batches[0])
        tr.forward_backward(*batches[1])   # starts from the state the first batch left
        g = {k: t.clone() for k, t in tr.grad_dict().items()}
        loss = tr.loss()
        for x, y in batches:
            tr.step(x, y)
        torch.cuda.synchronize()
        return g, loss, tr.params.clone(), tr.loss()

    a, b = _both(run, cfg)
    _assert_same(a, b)


def test_fc_tail_multi_step_graph():
    """tr.steps([...]) with three batches (one graph) against three single steps, tail on and off."""
    B, T = 64, 8
    cfg = _cfg(B, T)
    ds = NameStream(B, T, seed=24)
    batches = [ds.next() for _ in range(3)]

    def run(tr):
        from gru_mpi_cuda_amd.engine.trainer import HipTrainer
        tr.steps(batches)
        torch.cuda.synchronize()
        one = HipTrainer(cfg, params=init_params(cfg))
        assert one.t.plan() == tr.t.plan()
        for x, y in batches:
            one.step(x, y)
        torch.cuda.synchronize()
        assert one.t.read_error() == 0
        assert torch.equal(one.params, tr.params), "multi-step graph differs from three single steps"
        assert one.loss() == tr.loss()
        return tr.params.clone(), tr.loss()

    (p0, s0), (p1, s1) = _both(run, cfg)
    assert torch.equal(p0, p1), f"{int((p0 != p1).sum())} elements differ"
    assert s0 == s1, (s0, s1)


# ------------------------------------------------------------------ the stand-alone wrapper
DEV, BF = "cuda", torch.bfloat16
M = hr.M_ROWS
LDT, COLT = M + 16, 8
SENTINEL = 12352.0     # exact in bf16


@functools.lru_cache(maxsize=None)
def _head_case(kind, H):
    """(inputs, fp32 torch reference) on the CPU; shared and never modified."""
    d = hr.inputs(kind, 256, H, seed=0)
    f = torch.float32
    X, W, b, y, inv = d["X"].to(f), d["W"].to(f), d["b"].to(f), d["labels"].long(), float(d["inv"])
    lg = X @ W.T + b
    valid = y >= 0
    yc = y.clamp_min(0)
    m = lg.max(1, keepdim=True).values
    e = torch.exp(lg - m)
    s = e.sum(1, keepdim=True)
    nll = torch.where(valid, (torch.log(s) + m).squeeze(1) - lg.gather(1, yc[:, None]).squeeze(1), torch.zeros(M)) * inv
    dl = (e / s - torch.nn.functional.one_hot(yc, 256).to(f)) * valid[:, None].to(f) * inv
    return d, dict(dl=dl, loss_part=nll.reshape(M // 32, 32).sum(1), dy=dl @ W)


def _launch(ext, d, H, dh):
    from gru_mpi_cuda_amd.ops import ft_layout
    X, W = d["X"].to(DEV, BF).contiguous(), d["W"].to(DEV, BF).contiguous()
    b, y, inv = d["b"].to(DEV), d["labels"].to(DEV), d["inv"].reshape(1).to(DEV)
    WT = W.T.contiguous()
    Wf, WTf = ft_layout(W), ft_layout(WT)
    o = dict(dlT=torch.full((256, LDT), SENTINEL, device=DEV, dtype=BF),
             lp=torch.full((M // 32,), float("nan"), device=DEV))
    a = dict(X=X.data_ptr(), W=W.data_ptr(), b=b.data_ptr(), labels=y.data_ptr(), inv_count=inv.data_ptr(),
             dlT=o["dlT"].data_ptr(), loss_part=o["lp"].data_ptr(), M=M, H=H, V=256, ldT=LDT, colT=COLT,
             Wf=Wf.data_ptr(), WTf=WTf.data_ptr())
    if dh:
        o["dy"] = torch.full((M, H), float("nan"), device=DEV)
        a.update(dy=o["dy"].data_ptr(), WT=WT.data_ptr())
    else:
        o["dl"] = torch.full((M, 256), float("nan"), device=DEV, dtype=BF)
        a["dl"] = o["dl"].data_ptr()
    ext.fc_xent(a, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


def _close(got, ref, family, what, inv):
    print(f"FCTAIL {family:6s} err/tol {hr.err_over_tol(got, ref, family, inv):9.3e}  {what}")
    m = hr.mismatch(got, ref, family, inv)
    assert m is None, f"{what}: {m}"


@pytest.mark.parametrize("kind", ["planted", "random"])
@pytest.mark.parametrize("dh", [True, False])
@pytest.mark.parametrize("H", hr.V256_H)
def test_fc_xent_wrapper_matches_fp32_reference(ext, H, dh, kind):
    """fc_xent_v256_kernel<H, DH> as a wrapper of fc_xent_v256_block: dl^T (and dl), the loss partials
    and dy against fp32 torch, in the families and tolerances of test_head_gpu.py::test_fc_xent_v256."""
    saved = ext.step_lds_variants()
    try:
        ext.set_step_lds_variants(dict(fc_flash=0))
        d, ref = _head_case(kind, H)
        o, o2 = _launch(ext, d, H, dh), _launch(ext, d, H, dh)
    finally:
        ext.set_step_lds_variants(saved)
    what = f"fc_xent wrapper H={H} DH={int(dh)} {kind}"
    inv, lab = float(d["inv"]), d["labels"]
    for k in o:
        assert torch.equal(o[k].view(torch.int16 if o[k].dtype == BF else torch.int32),
                           o2[k].view(torch.int16 if o2[k].dtype == BF else torch.int32)), f"{what}: {k} not repeatable"
    fill = torch.full((256, LDT), SENTINEL, dtype=BF)
    assert torch.equal(o["dlT"][:, :COLT], fill[:, :COLT]) and torch.equal(o["dlT"][:, COLT + M:], fill[:, COLT + M:]), \
        f"{what}: dl^T written outside its window"
    dlT = hr.dlt_decode(o["dlT"], M, COLT)
    _close(dlT, ref["dl"], "dl", what + " dlT", inv)
    if "dl" in o:
        assert torch.equal(dlT.contiguous(), o["dl"]), f"{what}: dl^T differs from dl"
    ign = lab < 0
    assert not bool(dlT[ign].float().abs().any()), f"{what}: dl of an ignored row is not exactly 0"
    _close(o["lp"], ref["loss_part"], "loss", what + " loss_part", inv)
    if "dy" in o:
        assert not bool(torch.isnan(o["dy"]).any()), f"{what}: dy not fully written"
        assert bool((o["dy"][ign] == 0).all()), f"{what}: dy of an ignored row is not exactly 0"
        c0 = d["dy_from"]
        _close(o["dy"][:, c0:], ref["dy"][:, c0:], "dy", what + " dy end to end", inv)
        print(f"FCTAIL dy_gemm err/tol {hr.gemm_err_over_bound(o['dy'], dlT.float(), d['W'], 256):9.3e}  {what}")
        m = hr.gemm_mismatch(o["dy"], dlT.float(), d["W"], 256)
        assert m is None, f"{what} dy = dl . W: {m}"

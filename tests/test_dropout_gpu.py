"""Training dropout on the non-recurrent connections, on the device (csrc/kernels/dropout.hip, the trainer's
dropout plan; docs/DESIGN.md §3.5): the two mask kernels bit for bit against numpy built from
cpu_ref.dropout_mask, the step's gradients against the fp64 oracle under the same masks, the masks following
the device step counter through graph replay, multi-step graphs and resume, and dropout = 0 changing nothing."""
import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.config import GRUConfig, preset
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models.params import init_params
from gru_mpi_cuda_amd.utils.data import NameStream, make_padded_batch, synthetic_names

pytestmark = pytest.mark.gpu

SENT16 = 0x7B7B   # sentinel bit patterns no masked value below can take (a bf16 of 3.3e36, an fp32 NaN)
SENT32 = 0x7FC12345


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


def _bits16(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _mask_tbh(cfg, layer, step, b0, Bp, T):
    """cpu_ref.dropout_mask for the device's rows b0 .. b0 + Bp, time-major [T, Bp, H]."""
    return np.ascontiguousarray(cpu_ref.dropout_mask(cfg, layer, step, b0 + np.arange(Bp), T).transpose(1, 0, 2))


# (B, T, H): 96 tokens = an edge tile in the token dimension | three unit tiles | a batch padded 40 -> 64
@pytest.mark.parametrize("B,T,H", [(32, 3, 64), (64, 2, 192), (40, 2, 128)])
@pytest.mark.parametrize("step", [0, 7])
@pytest.mark.parametrize("p", [0.5, 0.1])
@pytest.mark.parametrize("layer", [0, 1])
def test_mask_kernels_bitwise(B, T, H, step, p, layer):
    from gru_mpi_cuda_amd.ops._ext import dropout_bwd_seq, dropout_fwd_seq
    dev = torch.device("cuda")
    Bp = (B + 63) // 64 * 64 if B % 32 else B
    b0 = 0 if layer == 0 else 3 * Bp      # layer 1's cases also move the rank offset
    seed = 1234 if step == 0 else (5 << 32) | 77
    cfg = GRUConfig(vocab=64, embed=64, hidden=H, batch=Bp, seq=T, dropout=p, seed=seed)
    gen = torch.Generator().manual_seed(100 * T + H + step)
    m = _mask_tbh(cfg, layer, step, b0, Bp, T)
    s = cpu_ref.dropout_scale(p)
    stepw = torch.tensor([step, -1], dtype=torch.int32, device=dev)
    # ---- forward: hsb (slot 0 = h0) -> xd and xdT, each inside a sentinel-filled buffer
    hsb = torch.randn(T + 1, Bp, H, generator=gen).to(torch.bfloat16)
    hsb[1, 0, :4] = torch.tensor([0.0, -0.0, 1.0, -1.0])
    ldT = (T + 1) * Bp + 8                                    # a pitch wider than the written columns
    xd_all = torch.full((T + 1, Bp, H), SENT16, dtype=torch.int16, device=dev).view(torch.bfloat16)
    xdT_all = torch.full((H + 2, ldT), SENT16, dtype=torch.int16, device=dev).view(torch.bfloat16)
    hd = hsb.to(dev)
    dropout_fwd_seq(hd, xd_all[:T], xdT_all[1:H + 1], stepw, seed=seed, p=p, layer=layer, b0=b0)
    torch.cuda.synchronize()
    hf = (_bits16(hsb[1:]).astype(np.uint32) << 16).view(np.float32)
    prod = torch.from_numpy(hf * s).to(torch.bfloat16)        # one fp32 multiply, one rounding to bf16 (RNE)
    want = np.where(m, _bits16(prod), np.uint16(0))
    got = _bits16(xd_all)
    np.testing.assert_array_equal(got[:T], want)
    assert (got[T] == SENT16).all()                           # the rows behind the sequence
    gotT = _bits16(xdT_all)
    np.testing.assert_array_equal(gotT[1:H + 1, Bp:(T + 1) * Bp], want.reshape(T * Bp, H).T)
    assert (gotT[0] == SENT16).all() and (gotT[H + 1] == SENT16).all()
    assert (gotT[:, :Bp] == SENT16).all()                     # the h0 columns
    assert (gotT[:, (T + 1) * Bp:] == SENT16).all()           # the pitch's padding
    torch.testing.assert_close(hd.cpu().view(torch.int16), hsb.view(torch.int16), atol=0, rtol=0)   # the input is untouched
    # ---- backward: fp32 dy in place
    dy = torch.randn(T, Bp, H, generator=gen)
    dy[0, 0, :2] = torch.tensor([0.0, -0.0])
    dy_all = torch.full((T + 1, Bp, H), SENT32, dtype=torch.int32, device=dev).view(torch.float32)
    dy_all[:T] = dy.to(dev)
    dropout_bwd_seq(dy_all[:T], stepw, seed=seed, p=p, layer=layer, b0=b0)
    torch.cuda.synchronize()
    wantd = np.where(m, (dy.numpy() * s).view(np.uint32), np.uint32(0))
    gotd = dy_all.view(torch.int32).cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(gotd[:T], wantd)
    assert (gotd[T] == SENT32).all()
    assert stepw.cpu().tolist() == [step, -1]


def test_mask_kernels_refuse_bad_arguments():
    from gru_mpi_cuda_amd.ops._ext import dropout_bwd_seq, dropout_fwd_seq
    dev = torch.device("cuda")
    stepw = torch.zeros(1, dtype=torch.int32, device=dev)
    h = torch.zeros(3, 32, 64, dtype=torch.bfloat16, device=dev)
    xd = torch.zeros(2, 32, 64, dtype=torch.bfloat16, device=dev)
    with pytest.raises(ValueError):      # a transposed buffer narrower than (T + 1) Bp
        dropout_fwd_seq(h, xd, torch.zeros(64, 64, dtype=torch.bfloat16, device=dev), stepw, seed=1, p=0.5)
    with pytest.raises(RuntimeError):    # Bp % 4 != 0
        dropout_bwd_seq(torch.zeros(2, 6, 64, device=dev), stepw, seed=1, p=0.5)
    with pytest.raises(RuntimeError):    # the layer field of the counter is 8 bits
        dropout_bwd_seq(torch.zeros(2, 8, 64, device=dev), stepw, seed=1, p=0.5, layer=256)


GRAD_CASES = [
    # (layers, H, E, B, GK_PERSIST)
    (1, 128, 128, 64, "1"),
    (1, 512, 512, 64, "1"),      # the persistent forward and backward with the head unfused
    (2, 256, 128, 64, "1"),      # no wavefront forward
    (1, 128, 128, 40, "1"),      # padded batch with ignore labels
    (2, 256, 128, 64, "0"),      # the per-step kernels
]


@pytest.mark.parametrize("layers,H,E,B,persist", GRAD_CASES)
def test_trainer_grads_match_oracle_under_dropout(monkeypatch, layers, H, E, B, persist):
    """HipTrainer.forward_backward against cpu_ref.manual_backward in fp64 with step 0's masks, at
    tests/test_engine_gpu.py's bounds (loss 1e-2 relative, every tensor's relative error below 0.04)."""
    from gru_mpi_cuda_amd.engine.trainer import HipTrainer
    monkeypatch.setenv("GK_PERSIST", persist)
    cfg = GRUConfig(vocab=256, embed=E, hidden=H, layers=layers, batch=B, seq=8, seed=7, dropout=0.3)
    params = init_params(cfg)
    if B == 40:
        x, y = make_padded_batch(synthetic_names(B, seed=3, max_len=10), cfg.seq)
    else:
        x, y = NameStream(B, cfg.seq, seed=3).next()
    tr = HipTrainer(cfg, params=params)
    plan = tr.t.plan()
    assert "dropout=0.3" in plan, plan
    assert "head=fwd-tail" not in plan and "fb=one-launch" not in plan and "+wave" not in plan and "+fc" not in plan, plan
    if persist == "1" and H >= 256:
        assert "fwd=persistent" in plan and "bwd0=persistent" in plan, plan
    if persist == "0":
        assert "persistent" not in plan, plan
    tr.forward_backward(x, y)
    loss = tr.loss()
    g = tr.grad_dict()
    p64 = {k: v.double() for k, v in params.items()}
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    ref_loss, ref_g = cpu_ref.manual_backward(p64, cfg, xt, yt, dropout_step=0)
    print(f"{plan}: loss {loss:.6f} vs {float(ref_loss):.6f}")
    for k in ref_g:
        print(f"  {k}: rel {rel(g[k], ref_g[k]):.5f}")
    assert abs(loss - float(ref_loss)) < 1e-2 * float(ref_loss)
    for k in ref_g:
        e = rel(g[k], ref_g[k])
        assert e < 0.04, f"{k}: rel err {e:.4f} ({plan})"
    # the bound tells masks apart: the undropped oracle lies outside it (at least twice the bound)
    _, plain_g = cpu_ref.manual_backward(p64, cfg, xt, yt)
    assert rel(g["fc.weight"], plain_g["fc.weight"]) > 2 * 0.04


def test_trainer_grads_split_head_large_h_under_dropout():
    """The large-H plan under dropout: the head as logits GEMM + softmax-xent + the dl . W_fc GEMM (the masked
    copy is the logits GEMM's A operand, the backward mask runs behind the dy GEMM, big_dy off) in front of the
    persistent large-H backward; tests/test_engine_gpu.py's large-H shape and bounds."""
    from gru_mpi_cuda_amd.engine.trainer import HipTrainer
    cfg = GRUConfig(vocab=256, embed=128, hidden=2048, layers=1, batch=512, seq=4, seed=6, dropout=0.3)
    params = init_params(cfg)
    x, y = NameStream(cfg.batch, cfg.seq, seed=9).next()
    tr = HipTrainer(cfg, params=params)
    plan = tr.t.plan()
    assert "bwd0=persistent-big" in plan and "+dy" not in plan and "dropout=0.3" in plan, plan
    tr.forward_backward(x, y)
    assert tr.t.read_error() == 0
    g = tr.grad_dict()
    p64 = {k: v.double() for k, v in params.items()}
    ref_loss, ref_g = cpu_ref.manual_backward(p64, cfg, torch.from_numpy(x), torch.from_numpy(y), dropout_step=0)
    print(f"{plan}: loss {tr.loss():.6f} vs {float(ref_loss):.6f}")
    for k in ref_g:
        print(f"  {k}: rel {rel(g[k], ref_g[k]):.5f}")
    assert abs(tr.loss() - float(ref_loss)) < 1e-2 * float(ref_loss)
    for k in ref_g:
        e = rel(g[k], ref_g[k])
        assert e < 0.04, f"{k}: rel err {e:.4f} ({plan})"


def _sgd_cfg(**kw):
    base = dict(vocab=256, embed=128, hidden=256, layers=1, batch=64, seq=8, lr=5e-2, seed=2, optimizer="sgd",
                keep_grads=True, dropout=0.3)
    base.update(kw)
    return GRUConfig(**base)


@pytest.mark.parametrize("layers", [1, 2])
def test_masks_follow_the_device_step_counter(layers):
    """Two step() calls, then steps() with a group of 4, against CpuTrainer stepping the same batches (its own
    counter picks the masks).  The issue words this check as "the comparison test_trainer_lr_schedule_matches_cpu
    makes, at its tolerances"; that test makes no CpuTrainer comparison (its 2e-3 / 1e-3 are for ratios of two
    device quantities, in which the bf16 operand error cancels), so this test departs from that wording and
    takes the suite's device-against-CPU bounds instead.  Under SGD the two runs' weights stay together (an update is -lr g, and g agrees
    to the bf16 operands' error), so every step's device gradient is compared with the CPU step's at the
    suite's device-against-CPU bounds (tests/test_engine_gpu.py: loss 1e-2 relative, tensors 0.04) -- a mask
    drawn for another step lies outside these bounds, asserted below.  The group of 4 equals 4 single step() calls on
    a second trainer bit for bit: the masks follow the counter through graph replay."""
    from gru_mpi_cuda_amd.engine.trainer import CpuTrainer, HipTrainer
    cfg = _sgd_cfg(layers=layers)
    params = init_params(cfg)
    ds = NameStream(cfg.batch, cfg.seq, seed=5)
    batches = [ds.next() for _ in range(6)]
    a = HipTrainer(cfg, params={k: v.clone() for k, v in params.items()})
    b = HipTrainer(cfg, params={k: v.clone() for k, v in params.items()})
    c = CpuTrainer(cfg, params={k: v.clone() for k, v in params.items()})

    def check(it):
        g, rg = a.grad_dict(), c.grad_dict()
        print(f"step {it}: loss {a.loss():.6f} vs {c.loss():.6f}")
        assert abs(a.loss() - c.loss()) < 1e-2 * c.loss(), it
        for k in rg:
            e = rel(g[k], rg[k])
            assert e < 0.04, f"step {it} {k}: rel err {e:.4f}"
        return g

    for it in range(2):
        c.step(*batches[it])
        a.step(*batches[it])
        check(it)
    assert a.t.get_step() == 2
    for x, y in batches[2:]:
        c.step(x, y)
    a.steps(batches[2:])
    assert a.t.graph_steps() == 4 and a.t.get_step() == 6
    g = check(5)
    # the same batch under step 4's masks is another gradient altogether
    p_now = {k: v.double() for k, v in c.params.items()}
    _, wrong = cpu_ref.manual_backward(p_now, cfg, torch.from_numpy(batches[5][0]), torch.from_numpy(batches[5][1]),
                                       dropout_step=4)
    assert rel(g["fc.weight"], wrong["fc.weight"]) > 2 * 0.04
    for x, y in batches:
        b.step(x, y)
    torch.testing.assert_close(a.params, b.params, atol=0, rtol=0)
    assert a.loss() == b.loss() and b.t.get_step() == 6


def test_resume_is_bitwise():
    from gru_mpi_cuda_amd.engine.trainer import HipTrainer
    cfg = GRUConfig(vocab=256, embed=256, hidden=512, layers=1, batch=64, seq=8, seed=3, dropout=0.3)
    ds = NameStream(cfg.batch, cfg.seq, seed=4)
    batches = [ds.next() for _ in range(3)]
    params = init_params(cfg)
    whole = HipTrainer(cfg, params={k: v.clone() for k, v in params.items()})
    for x, y in batches:
        whole.step(x, y)
    first = HipTrainer(cfg, params={k: v.clone() for k, v in params.items()})
    for x, y in batches[:2]:
        first.step(x, y)
    sd, (m, v), step = first.state_dict(), first.opt_state(), first.t.get_step()
    assert step == 2
    second = HipTrainer(cfg, params=sd)
    second.load_opt_state(m, v)
    second.t.set_step(step)
    second.step(*batches[2])
    torch.testing.assert_close(second.params, whole.params, atol=0, rtol=0)
    assert second.loss() == whole.loss()
    # a resumed trainer left at step 0 draws step 0's masks: the loss of the third batch differs
    third = HipTrainer(cfg, params=sd)
    third.load_opt_state(m, v)
    third.step(*batches[2])
    assert third.loss() != whole.loss()


def test_nothing_changes_at_zero():
    from gru_mpi_cuda_amd.engine.trainer import HipTrainer
    base = preset("h512", batch=64, seq=8)
    zero = GRUConfig(**{**{f: getattr(base, f) for f in base.__dataclass_fields__ if f != "dropout"}, "dropout": 0.0})
    ds = NameStream(base.batch, base.seq, seed=4)
    batches = [ds.next() for _ in range(3)]
    a = HipTrainer(base, params=init_params(base))
    b = HipTrainer(zero, params=init_params(zero))
    c = HipTrainer(base.replace(dropout=0.2), params=init_params(base))
    for x, y in batches:
        a.step(x, y)
        b.step(x, y)
    pa, pb = a.t.plan(), b.t.plan()
    assert pa == pb and "dropout" not in pb, (pa, pb)
    assert "head=fwd-tail" in pb and "fb=one-launch" in pb, pb     # the fused launches are still taken at 0
    assert a.t.workspace_bytes() == b.t.workspace_bytes()
    torch.testing.assert_close(a.params, b.params, atol=0, rtol=0)
    assert a.loss() == b.loss()
    # the masked copies are the dropout trainer's only extra workspace (per layer Xd [tok][H] + XdT [tok + Bp][H], bf16)
    tok, Bp, H = base.seq * 64, 64, 512
    extra = c.t.workspace_bytes() - a.t.workspace_bytes()
    assert 2 * H * (2 * tok + Bp) <= extra <= 2 * H * (2 * tok + Bp) + 1024, extra
    pc = c.t.plan()
    assert pc.endswith(" dropout=0.2") and "fwd=persistent" in pc and "dP=bwd-tail" in pc, pc


def test_refusals():
    from gru_mpi_cuda_amd.engine.trainer import HipTrainer
    kw = dict(vocab=256, embed=128, hidden=128, layers=1, batch=64, seq=8)
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            GRUConfig(dropout=bad, **kw)
        cfg = GRUConfig(**kw)
        cfg.dropout = bad                     # past the config's own check: the engine refuses it too
        with pytest.raises((ValueError, RuntimeError), match="dropout"):
            HipTrainer(cfg, params=init_params(GRUConfig(**kw)))
    with pytest.raises((ValueError, RuntimeError), match="overlap"):
        HipTrainer(GRUConfig(dropout=0.2, overlap=True, **kw))

"""score_head_bf16 alone (csrc/kernels/score_fast.hip), exact by construction.

h holds values from {-1, -1/2, 0, 1/2, 1}, W_fc and b_fc multiples of 1/8 of magnitude <= 1: every product is
a multiple of 1/16 and every partial sum stays below 2^9, so a logit is exact in fp32 in any summation order
and only the softmax arithmetic separates the kernel from fp64 -- the project's fp32 scoring bound
1e-5 + 2e-7 exp(-ref) (tests/test_score_gpu.py) applies to tok_logp, and ranks must be equal everywhere.  The
last quarter of W_fc's rows repeats the first, so about half the targets are tied with another column, in
both directions of the tie rule."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("ML", [1, 10])
@pytest.mark.parametrize("names", [1, 65])      # a padded block; a second block whose names all end early
@pytest.mark.parametrize("V", [64, 256, 512])
@pytest.mark.parametrize("H", [64, 192])        # one k-tile; an odd number that wraps the two-slot ring
def test_score_head_exact_operands(ext, H, V, names, ML):
    rng = np.random.default_rng(H + V + names + ML)
    Bp = (names + 63) // 64 * 64
    h = torch.from_numpy(rng.integers(-2, 3, size=(ML, Bp, H)) / 2.0)
    W = torch.from_numpy(rng.integers(-8, 9, size=(V, H)) / 8.0)
    b = torch.from_numpy(rng.integers(-8, 9, size=V) / 8.0)
    W[3 * V // 4:], b[3 * V // 4:] = W[:V // 4], b[:V // 4]
    ntok = np.zeros(Bp, np.int32)
    ntok[:names] = 1 + np.arange(names) % ML    # 1 .. ML; name 64 ends before its block's late steps
    mask = np.arange(ML)[None, :] < ntok[:, None]                      # [Bp][ML]
    tgt = rng.integers(0, V, size=(ML, Bp))
    tgt[0, 0] = 3 * V // 4 + 1                                          # the single-token cases hold a tie too
    tgt = np.where(mask.T, tgt, -1).astype(np.int32)

    logits = h @ W.T + b                                                # fp64, exact
    tc = torch.from_numpy(np.maximum(tgt, 0)).long().unsqueeze(-1)
    xt = logits.gather(-1, tc)
    j = torch.arange(V).view(1, 1, -1)
    ref_rank = ((logits > xt) | ((logits == xt) & (j < tc))).sum(-1).numpy().T
    ref_rank = np.where(mask, ref_rank, -1)
    ref_tok = np.where(mask, torch.log_softmax(logits, -1).gather(-1, tc).squeeze(-1).numpy().T, 0.0)
    tied = ((logits == xt).sum(-1).numpy().T > 1) & mask
    assert tied.any()

    dev = [h.to(torch.bfloat16).to(DEV), W.to(torch.bfloat16).to(DEV), b.float().to(DEV),
           torch.from_numpy(tgt).to(DEV), torch.from_numpy(ntok).to(DEV)]
    err = torch.zeros(4, dtype=torch.int32, device=DEV)

    def launch():
        out = [torch.full((Bp, ML), np.nan, device=DEV), torch.full((Bp, ML), -9, dtype=torch.int32, device=DEV),
               torch.full((Bp,), np.nan, device=DEV), torch.full((Bp,), -9, dtype=torch.int32, device=DEV)]
        ext.score_head(dict(h=dev[0].data_ptr(), Wfc=dev[1].data_ptr(), bfc=dev[2].data_ptr(), tgt=dev[3].data_ptr(),
                            ntok=dev[4].data_ptr(), tok_logp=out[0].data_ptr(), rank=out[1].data_ptr(),
                            name_logp=out[2].data_ptr(), ntok_out=out[3].data_ptr(), err=err.data_ptr(),
                            Bp=Bp, H=H, V=V, ML=ML), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in out]

    tok, rank, name, nout = launch()
    assert int(err[0]) == 0 and np.array_equal(nout, ntok)
    assert np.array_equal(rank, ref_rank)
    d = np.abs(tok.astype(np.float64) - ref_tok)
    bound = np.where(mask, 1e-5 + 2e-7 * np.exp(-ref_tok), 0.0)
    print(f"tok_logp: max |d| {d.max():.3e}, max d/bound {np.max(d[mask] / bound[mask]):.3f}, tied {int(tied.sum())}")
    assert np.all(d <= bound)
    seq = np.zeros(Bp, np.float32)
    for l in range(ML):
        seq = seq + tok[:, l]
    assert np.array_equal(name.view(np.int32), seq.view(np.int32))
    for first, second in zip((tok, rank, name, nout), launch()):
        assert first.tobytes() == second.tobytes()

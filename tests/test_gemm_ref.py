"""CPU tests of models/gemm_ref.py: the exact reference and its guard, the property the GPU tests rest
on (fp32 accumulation of grid operands does not depend on the order), the planted mutations, the
canaries, and the guard over every case of tests/test_gemm_gpu.py for seeds 0-2."""
import numpy as np
import pytest
import torch

import test_gemm_gpu as G
from gru_mpi_cuda_amd.models import gemm_ref as R


@pytest.mark.parametrize("M,N,K,splits", [(64, 64, 32, 1), (128, 192, 384, 3), (64, 128, 4096, 2)])
def test_product_ref_equals_fp64_matmul(M, N, K, splits):
    op = R.grid_operands(M, N, K, 0, kdepth=K // splits, bias=True, c0=True)
    ref = R.product_ref(op, splits=splits, accumulate=True)
    kper = K // splits
    for s in range(splits):
        want = op.A[:, s * kper:(s + 1) * kper] @ op.B[:, s * kper:(s + 1) * kper].T + op.C0
        if splits == 1:
            want = want + op.bias
        assert torch.equal(ref.C[s].double(), want)
        assert torch.equal(ref.rowsum[s].double(), op.A[:, s * kper:(s + 1) * kper].sum(1))
    f32 = R.product_ref(op, splits=splits, bias_in="slab0")
    assert torch.equal(f32.C.double().sum(0), op.A @ op.B.T + op.bias)


def test_operands_are_what_they_claim():
    op = R.grid_operands(128, 64, 256, 1, bias=True, c0=True)
    p, q = op.bits
    assert (p, q) == (8, 7) and R.operand_bits(64) == (8, 8) and R.operand_bits(8192) == (5, 5)
    ia, ib = op.A / torch.exp2(op.ea.double())[:, None], op.B / torch.exp2(op.eb.double())[:, None]
    assert torch.equal(ia, ia.round()) and torch.equal(ib, ib.round())
    assert ia.abs().max() == 2 ** p - 1 and ib.abs().max() == 2 ** q - 1          # every bit used
    assert ia.abs().min() >= 1 and (ia != ia.flip(0)).any() and not torch.equal(op.A, op.A.T[:128, :256].T.flip(1))
    assert op.ea.min() >= -3 and op.eb.max() <= 3 and len(op.ea.unique()) > 1
    assert torch.equal(op.A.bfloat16().double(), op.A) and torch.equal(op.B.bfloat16().double(), op.B)
    blocks = op.A.view(128, 4, 64)
    assert not torch.equal(blocks[:, 0], blocks[:, 1])                             # differs per k-block
    assert torch.isfinite(op.A).all() and (op.A.abs() >= 2.0 ** -3).all()          # no zeros, no subnormals


def test_a32_rounding_cases():
    op = R.grid_operands(128, 64, 256, 2, a32=True)
    x = (op.A32.double() / torch.exp2(op.ea.double())[:, None]).abs()
    r = (op.A / torch.exp2(op.ea.double())[:, None]).abs()
    assert torch.equal(r, r.round()) and r.min() >= 128 and r.max() == 256        # on the grid; next binade reached
    frac = x - x.floor()
    assert (frac != 0).any()                                                       # more than 8 significant bits
    tie = frac == 0.5
    assert (tie & (r > x)).any() and (tie & (r < x)).any()                         # ties both ways
    assert torch.equal(r[tie] % 2, torch.zeros_like(r[tie]))                       # .. to even
    assert not torch.equal(R.bf16_trunc(op.A32).double(), op.A)                    # truncation differs


def test_guard_fires():
    op = R.grid_operands(64, 64, 4096, 0, kdepth=32)         # 8 + 8 bits sized for 32 products, summed over 4096
    with pytest.raises(R.GridError, match="2\\^24"):
        R.product_ref(op)
    R.product_ref(op, splits=128)
    wide = R.grid_operands(64, 64, 64, 0)
    wide.A[3, 5] += 2.0 ** -9                                 # off the grid
    with pytest.raises(R.GridError, match="off its grid"):
        R.product_ref(wide)
    big = R.grid_operands(64, 64, 64, 0, c0=True)
    big.C0 *= 16                                              # |C0| up to 2^25 lsbs
    with pytest.raises(R.GridError):
        R.product_ref(big, accumulate=True)
    with pytest.raises(R.GridError):
        R.operand_bits(1 << 22)


def _seeds():
    return (0, 1, 2)


@pytest.mark.parametrize("i", range(len(G.ALL_CASES)), ids=lambda i: G.cid(G.ALL_CASES[i]))
def test_guard_holds_for_gpu_case(i):
    c = G.ALL_CASES[i]
    for seed in _seeds():
        op, B2, ref = G.host(c, seed)
        assert torch.isfinite(ref.C).all()
        p, q = op.bits
        if not c["onehot"]:
            assert p + q == min(16, 23 - R.ceil_log2(c["K"] // c["splits"]))      # as many bits as fit
        if c["onehot"] in ("uniform", "names", "tile", "holes"):
            assert ref.C.abs().max() > 0
        if c["onehot"] == "invalid":
            assert not ref.C.any() and (op.ids == -1).any() and (op.ids == c["M"]).any()
        if c["onehot"] == "holes":                                                # some wave idle, the others busy
            waves = (op.ids.view(-1, c["kt"]).long() // 64)
            present = torch.stack([(waves == w).any(1) for w in range(4)], 1)
            assert (present.sum(1) == 3).all() and len({tuple(r.tolist()) for r in present}) >= min(4, len(present))


@pytest.mark.parametrize("M,N,K,splits", G.F32)
def test_guard_holds_for_f32_case(M, N, K, splits):
    for seed in _seeds():
        op, ref = G.f32_host(M, N, K, splits, seed)
        assert max(op.bits) > 8 and torch.equal(op.A.float().double(), op.A)


def test_case_tables_cover_what_they_claim():
    k1 = {c["K"] // c["splits"] for c in G.ALGO1 if not c["onehot"]}
    assert {32, 64, 96, 128, 160} <= k1
    wgs = [(c["M"] // 64) * (c["N"] // 64) * c["splits"] for c in G.ALGO1]
    assert all(w > 8 and w % 8 for w in wgs) and {9, 18} <= set(wgs)
    assert {c["K"] // c["splits"] for c in G.ALGO2} == {128, 192, 320}
    assert {(c["raster"], c["M"] < c["N"]) for c in G.ALGO2 if c["M"] != c["N"]} == {(0, True), (0, False), (1, True), (1, False)}
    assert {c["K"] // c["splits"] // 64 for c in G.ALGO3 if not c["a32"]} == {2, 3, 4, 8, 16, 32}
    assert {c["a32"] for c in G.ALGO3} == {0, 1, 2}
    assert len(G.OH_CASES) == 3 * 7 * 5
    for geo in G.OH_GEO:
        for n in G.OH_NKT:
            mine = [c for c in G.OH_CASES if c["tag"] == f"g{geo}" and c["K"] // c["splits"] == n * G.OH_GEO[geo][1]]
            assert {c["splits"] for c in mine} == {1, 2} and len({c["N"] for c in mine}) == 2
    for c in G.ALL_CASES:      # lda, ldb > K always (Job); ldc > N wherever the kernel allows it
        dense = c["tag"].startswith("g") or (c["algo"] == 5 and c["splits"] > 1) or c["ldc_pad"] > 0
        assert dense or c in (G.ALGO1[8], G.ALGO2[7], G.ALGO3[6], G.LIBRARY[1], G.AUTO[3]) or c in G.BIAS_SPLIT


def _acc32(terms, order):
    """Sequential fp32 accumulation of fp32 products in the given order ('pairwise': a tree)."""
    t = terms.astype(np.float32)
    if order == "pairwise":
        while t.shape[-1] > 1:
            if t.shape[-1] % 2:
                t = np.concatenate([t, np.zeros_like(t[..., :1])], -1)
            t = (t[..., 0::2] + t[..., 1::2]).astype(np.float32)
        return t[..., 0]
    idx = range(t.shape[-1]) if order == "forward" else range(t.shape[-1] - 1, -1, -1)
    acc = np.zeros(t.shape[:-1], np.float32)
    for k in idx:
        acc = (acc + t[..., k]).astype(np.float32)
    return acc


@pytest.mark.parametrize("K", [64, 320, 2048])
def test_fp32_accumulation_is_order_free_on_the_grid(K):
    """The property the GPU test rests on: forward, reversed and pairwise fp32 sums of the products are
    bit-identical and equal the exact result.  Random N(0, 1) operands of the same shape are not."""
    op = R.grid_operands(32, 48, K, 0)
    ref = R.product_ref(op).C[0].numpy()
    a32, b32 = op.A.numpy().astype(np.float32), op.B.numpy().astype(np.float32)
    terms = a32[:, None, :] * b32[None, :, :]
    assert np.array_equal(terms.astype(np.float64), op.A.numpy()[:, None, :] * op.B.numpy()[None, :, :])
    got = [_acc32(terms, o) for o in ("forward", "reversed", "pairwise")]
    for g in got:
        assert g.dtype == np.float32 and np.array_equal(g.view(np.int32), ref.view(np.int32))
    rng = np.random.default_rng(0)
    x = rng.standard_normal((32, K)).astype(np.float32)[:, None, :] * rng.standard_normal((48, K)).astype(np.float32)[None]
    assert not np.array_equal(_acc32(x, "forward"), _acc32(x, "reversed"))


def _mutation_case(m):
    if m in ("a32_trans_ignored", "a32_truncated"):
        op = R.grid_operands(128, 64, 128, 0, a32=True)
        return op, dict(a32_trans_storage=op.A32.T.contiguous())
    if m == "id_M_matches_last":
        return R.grid_operands(256, 64, 256, 0, kdepth=128, onehot="invalid"), dict(splits=2)
    return R.grid_operands(128, 128, 384, 0, kdepth=128, bias=True), dict(splits=3)


@pytest.mark.parametrize("m", R.MUTATIONS)
def test_every_planted_mutation_is_caught(m):
    op, kw = _mutation_case(m)
    ref, bad = R.product_ref(op, **kw), R.product_ref(op, mutate=m, **kw)
    R.compare(ref.C, ref.C.clone())
    R.compare(ref.rowsum, ref.rowsum.clone(), "rowsum")
    with pytest.raises(AssertionError) as e:
        R.compare(bad.C, ref.C)
        R.compare(bad.rowsum, ref.rowsum, "rowsum")
    msg = str(e.value)
    assert "first at slab" in msg and "per 64x64 tile" in msg
    if m == "transpose_subtile":                    # the message points at the tile
        assert "slab 0 (row 16, col 3" in msg and "{'(0,0)':" in msg
    if m == "padding_as_data":
        assert "non-finite: 128" in msg and "(row 64," in msg


def test_compare_semantics():
    a = torch.tensor([[0.0, 1.0], [2.0, 3.0]])
    R.compare(a, a.clone())
    R.compare(torch.tensor([[-0.0]]), torch.tensor([[0.0]]))                      # 0 == -0
    for v in (float("nan"), float("inf")):
        b = a.clone()
        b[1, 0] = v
        with pytest.raises(AssertionError, match="non-finite: 1"):
            R.compare(b, b.clone())                                                # even against itself
    b = a.clone()
    b[0, 1] = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
    with pytest.raises(AssertionError, match="1 of 4 elements differ"):
        R.compare(b, a)


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.bfloat16])
def test_padding_and_canaries(dtype):
    t = torch.arange(24, dtype=torch.float32).view(2, 3, 4)
    p = R.padded(t, 7, guard_rows=2)
    assert p.buf.shape == (10, 7) and torch.equal(p.view(), t) and torch.isnan(p.buf).sum() == 70 - 24
    assert p.ptr() == p.buf.data_ptr() + 2 * 7 * 4
    c = R.canary(2, 3, 4, 6, guard_rows=1, slab_rows=5, dtype=dtype)
    assert c.buf.shape == (12, 6)
    R.check_canary(c)
    c.view().fill_(1)                                   # the payload may change
    R.check_canary(c)
    for r, col in ((0, 0), (1, 4), (4, 0), (6, 5), (11, 3)):   # guard before, padding column, slab gap, guard after
        d = R.canary(2, 3, 4, 6, guard_rows=1, slab_rows=5, dtype=dtype)
        d.buf[r, col] = 1
        with pytest.raises(AssertionError, match="stray"):
            R.check_canary(d)
    if dtype == torch.float32:
        assert c.buf[0, 0].view(torch.int32).item() == R.PATTERN and torch.isfinite(c.buf[0, 0])

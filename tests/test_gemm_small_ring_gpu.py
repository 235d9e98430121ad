"""GemmVariants.small_ring: gemm_small's K-slice as one stream of 64-deep k-blocks through an LDS-DMA
ring of 3 or 4 slots (gemm_small_ring_body) against the burst body (small_ring = 0), in the three
launches that take it: gemm_small, gemm_small_group and gemm_small_with_prep.

(a) Exactness on the dyadic grid of models/gemm_ref.py, through the case / host / Job helpers of
    tests/test_gemm_gpu.py: every element of every slab and every row sum EQUALS the float64 reference,
    the NaN padding behind lda / ldb > K is never read, and the guard rows and padding columns of the
    outputs keep their canary bitwise.  Tolerance zero, as there.
(b) Order.  Grid operands cannot see a changed k order (every partial sum is exact), so the same shapes
    run on random bf16 operands, where fp32 rounding depends on the order of the MFMAs and of the row-sum
    additions: slabs and row sums must be torch.equal under small_ring = 0, 3 and 4.

Depths are every supported k-block count, so a ring runs below (2, 3 blocks), at (3, 4) and past its wrap
(8 .. 32); one 64 x 64 tile, and 128 x 192 (both wave rows and columns, six tiles, twelve when split).
"""
import functools

import pytest
import torch

from gru_mpi_cuda_amd.models import gemm_ref as R
from test_gemm_gpu import DEV, Job, Prep, S, case, cid, host, variants

pytestmark = pytest.mark.gpu

RINGS = (3, 4)
DEPTHS = (2, 3, 4, 8, 16, 24, 32)          # 64-deep blocks per K-slice
SHAPES = ((64, 64), (128, 192))


def _cases():
    out = []
    for M, N in SHAPES:
        for nkb in DEPTHS:
            for sp in (1, 2):
                for rowsum in (True, False):
                    for acc in (True, False):
                        # bias is fused only when unsplit; with (rowsum != acc) every <BIAS, ROWSUM>
                        # instantiation of the ring kernel is reached with and without `accumulate`
                        out.append(case(M, N, 64 * nkb * sp, sp, 3, bias=sp == 1 and rowsum != acc, acc=acc, rowsum=rowsum))
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def _host(key, seed):
    return host(dict(key), seed)


def _job(c, seed=0):
    return Job(c, seed, a32_from=_host(tuple(sorted(c.items())), seed))


def _randomise(j, seed):
    """Replace the payload of A and B by random bf16 values (the NaN padding stays) and an accumulated C by
    random fp32 ones; the same values for the same (case, seed)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    c = j.c
    A, B = j.keep[0], j.keep[1]
    A.view().copy_(torch.randn(c["M"], c["K"], generator=g).bfloat16()[None])
    B.view().copy_(torch.randn(c["N"], c["K"], generator=g).bfloat16()[None])
    if c["acc"]:
        j.C.view().copy_(torch.randn(c["M"], c["N"], generator=g)[None].expand(c["splits"], -1, -1))


def _outputs(j):
    return j.C.view().clone(), (j.rs.view().clone() if j.rs is not None else None)


def _assert_equal_outputs(a, b, what):
    assert torch.equal(a[0], b[0]), f"{what}: {int((a[0] != b[0]).sum())} C elements differ"
    assert (a[1] is None) == (b[1] is None)
    if a[1] is not None:
        assert torch.equal(a[1], b[1]), f"{what}: {int((a[1] != b[1]).sum())} row sums differ"


# ------------------------------------------------------------------ gemm_small
@pytest.mark.parametrize("c", CASES, ids=cid)
def test_ring_exact(ext, c):
    for ring in RINGS:
        with variants(ext, small_ring=ring):
            j = _job(c)
            assert ext.gemm_small_kblocks(j.d) == c["K"] // c["splits"] // 64
            ext.gemm_nt(j.d, S())
            torch.cuda.synchronize()
        j.check(f"ring {ring} {cid(c)}")


@pytest.mark.parametrize("c", CASES, ids=cid)
def test_ring_order(ext, c):
    outs = {}
    for ring in (0,) + RINGS:
        with variants(ext, small_ring=ring):
            j = _job(c)
            _randomise(j, 17)
            ext.gemm_nt(j.d, S())
            torch.cuda.synchronize()
        assert bool(torch.isfinite(j.C.view()).all()), f"ring {ring}: padding was read"
        R.check_canary(j.C, f"ring {ring} {cid(c)}: C")
        if j.rs is not None:
            R.check_canary(j.rs, f"ring {ring} {cid(c)}: rowsumA")
        outs[ring] = _outputs(j)
    for ring in RINGS:
        _assert_equal_outputs(outs[0], outs[ring], f"ring {ring} against the burst body, {cid(c)}")


def test_ring_switch(ext):
    """The field is reported, defaults to a ring, and takes 0, 3 and 4 only."""
    assert ext.gemm_variants()["small_ring"] in RINGS
    with variants(ext, small_ring=0):
        assert ext.gemm_variants()["small_ring"] == 0
        for bad in (1, 2, 5, -1):
            with pytest.raises(RuntimeError, match="small_ring"):
                ext.set_gemm_variants(dict(small_ring=bad))
        assert ext.gemm_variants()["small_ring"] == 0


# ------------------------------------------------------------------ gemm_small_group
# the headline's group scaled down: a split-K job with 1024-deep slices (16 blocks) and row sums, and two
# 256-deep jobs, one of them split; every tile count a multiple of 8 (the per-XCD deal) / not (the flat one)
GROUPS = {
    "per_xcd": ([case(128, 256, 2048, 2, 3), case(256, 128, 256, 1, 3, rowsum=False),
                 case(128, 128, 512, 2, 3, rowsum=False)], 1),
    "flat": ([case(64, 192, 2048, 2, 3), case(192, 64, 256, 1, 3, rowsum=False),
              case(128, 64, 512, 2, 3, rowsum=False)], 0),
}


@pytest.mark.parametrize("name", list(GROUPS))
def test_ring_group(ext, name):
    cases, per_xcd = GROUPS[name]
    tiles = [(c["M"] // 64) * (c["N"] // 64) * c["splits"] for c in cases]
    assert int(all(t % 8 == 0 for t in tiles)) == per_xcd          # the deal the group is there for
    outs = {}
    for ring in (0,) + RINGS:
        with variants(ext, small_ring=ring):
            jobs = [_job(c, seed=i) for i, c in enumerate(cases)]
            assert ext.gemm_small_group_depth([j.d for j in jobs]) == 4
            assert [ext.gemm_small_kblocks(j.d) for j in jobs] == [16, 4, 4]
            ext.gemm_group("small", [j.d for j in jobs], S())
            torch.cuda.synchronize()
            for i, j in enumerate(jobs):
                j.check(f"ring {ring} group {name} job {i}")
            rnd = [_job(c, seed=i) for i, c in enumerate(cases)]
            for i, j in enumerate(rnd):
                _randomise(j, 23 + i)
            ext.gemm_group("small", [j.d for j in rnd], S())
            torch.cuda.synchronize()
        for i, j in enumerate(rnd):
            R.check_canary(j.C, f"ring {ring} group {name} job {i}: C")
        outs[ring] = [_outputs(j) for j in rnd]
    for ring in RINGS:
        for i in range(len(cases)):
            _assert_equal_outputs(outs[0][i], outs[ring][i], f"ring {ring} against the burst body, group {name} job {i}")


# ------------------------------------------------------------------ gemm_small_with_prep
PREP_TABLE = case(64, 192, 512, 1, 0, bias=True, rowsum=False)


def test_ring_prep(ext):
    """The P table beside the batch preparation: exact, bitwise equal across small_ring on random operands,
    and ids / labels / inv_count equal to the prep_batch reference under every value."""
    tables = {}
    for ring in (0,) + RINGS:
        with variants(ext, small_ring=ring):
            j, p = _job(PREP_TABLE), Prep(8, 64)
            assert ext.gemm_small_kblocks(j.d) == 8
            ext.gemm_with_prep(j.d, p.d, S())
            torch.cuda.synchronize()
            j.check(f"ring {ring} prep table")
            p.check(f"ring {ring} prep")
            j, p = _job(PREP_TABLE), Prep(65, 256)
            _randomise(j, 29)
            ext.gemm_with_prep(j.d, p.d, S())
            torch.cuda.synchronize()
        p.check(f"ring {ring} prep (random table)")
        R.check_canary(j.C, f"ring {ring} prep table: C")
        tables[ring] = _outputs(j)
    for ring in RINGS:
        _assert_equal_outputs(tables[0], tables[ring], f"ring {ring} against the burst body, prep table")

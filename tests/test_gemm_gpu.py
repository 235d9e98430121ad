"""Exact per-element tests of the product kernels and their companions (gemm.hip, gemm_lds.hip,
gemm_small.hip, gemm256.hip, onehot.hip, gemm_f32_nt / split_bf16x3 of gen_f32.hip, the casts, sums
and the batch preparation of misc.hip) against models/gemm_ref.py.

Operands sit on a dyadic grid, so every fp32 partial sum is exact and the kernel's result must EQUAL
the float64 reference in every element of every split-K slab, whatever its summation order, pipeline
or tile shape (gemm_ref.py; tests/test_gemm_ref.py proves the property and the guard on the CPU).  The
tolerance is zero and derived.  Every case also checks the row sums per slab, reads operands through
lda > K and ldb > K with NaN padding, writes C through ldc > N where the kernel allows it, and compares
the padding columns and guard rows of every output bitwise with the canary they were filled with.

No case is skipped: where a kernel has a predicate, the test asserts that it accepts the case.
The case tables at module level are imported by tests/test_gemm_ref.py, which runs `host()` of every
case for seeds 0-2 (the exactness guard) on the CPU.
"""
import itertools
import struct

import pytest
import torch

from gru_mpi_cuda_amd.models import gemm_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


def S():
    return torch.cuda.current_stream().cuda_stream


def case(M, N, K, splits=1, algo=0, bias=False, acc=False, rowsum=True, ldc_pad=32, a32=0, raster=0, onehot=None,
         b2_row=0, exps=True, kt=64, tag=""):
    """One product.  K is the whole depth (K / splits per slab).  a32: 1 = fp32 A [M][lda], 2 = fp32 A
    stored transposed [K][lda].  onehot: an id distribution of gemm_ref.onehot_ids (A synthesised from
    ids; no row sums, no bias).  b2_row: B rows >= b2_row come from a second buffer."""
    if onehot:
        rowsum = False
    return dict(M=M, N=N, K=K, splits=splits, algo=algo, bias=bias, acc=acc, rowsum=rowsum, ldc_pad=ldc_pad, a32=a32,
                raster=raster, onehot=onehot, b2_row=b2_row, exps=exps, kt=kt, tag=tag)


def cid(c):
    flags = "".join(f for f, on in (("b", c["bias"]), ("a", c["acc"]), ("r", c["rowsum"]), ("T", c["a32"] == 2),
                                    ("F", c["a32"] == 1), ("c", c["raster"]), ("2", c["b2_row"])) if on)
    return (f"a{c['algo']}-{c['M']}x{c['N']}x{c['K']}s{c['splits']}" + (f"-{flags}" if flags else "") +
            (f"-{c['onehot']}" if c["onehot"] else "") + (f"-{c['tag']}" if c["tag"] else ""))


def host(c, seed=0):
    """CPU side of a case: grid operands and the exact reference (raises GridError if not exact)."""
    kper = c["K"] // c["splits"]
    op = R.grid_operands(c["M"], c["N"], c["K"], seed, kdepth=kper, bias=c["bias"], c0=c["acc"], a32=bool(c["a32"]),
                         onehot=c["onehot"], exps=c["exps"], onehot_kt=c["kt"])
    B2 = -op.B.flip(1) if c["b2_row"] else None      # same per-row grid, other values
    ref = R.product_ref(op, splits=c["splits"], B2=B2, b2_row=c["b2_row"], accumulate=c["acc"])
    return op, B2, ref


def bf16_exact(t):
    b = t.to(torch.bfloat16)
    assert torch.equal(b.double(), t.double()), "operand is not a bf16 value"
    return b


class Job:
    """Device buffers and the argument dict of one case, and the checks after the launch."""

    def __init__(self, c, seed=0, a32_from=None):
        self.c = c
        M, N, K, sp = c["M"], c["N"], c["K"], c["splits"]
        self.op, B2, self.ref = a32_from if a32_from is not None else host(c, seed)
        op = self.op
        d = dict(M=M, N=N, K=K, splits=sp, algo=c["algo"], accumulate=int(c["acc"]), raster=c["raster"])
        self.keep = []
        if c["onehot"]:
            ids = op.ids.to(DEV)
            self.keep.append(ids)
            d["onehot_ids"] = ids.data_ptr()
        elif c["a32"] == 1:
            A = R.padded(op.A32, K + 8).to(DEV)
            d.update(A32=A.ptr(), lda=A.ld)
        elif c["a32"] == 2:
            A = R.padded(op.A32.T.contiguous(), M + 8).to(DEV)
            d.update(A32=A.ptr(), lda=A.ld, a32_trans=1)
        else:
            A = R.padded(bf16_exact(op.A), K + 40).to(DEV)
            d.update(A=A.ptr(), lda=A.ld)
        if not c["onehot"]:
            self.keep.append(A)
        Bh = bf16_exact(op.B)
        if c["b2_row"]:
            B1, B2h = Bh.clone(), bf16_exact(B2)
            B1[c["b2_row"]:] = float("nan")          # rows the kernel must take from B2
            B2h[:c["b2_row"]] = float("nan")         # rows it must take from B
            Bp, B2p = R.padded(B1, K + 72).to(DEV), R.padded(B2h, K + 72).to(DEV)
            d.update(B2=B2p.ptr(), b2_row=c["b2_row"])
            self.keep.append(B2p)
        else:
            Bp = R.padded(Bh, K + 72).to(DEV)
        self.keep.append(Bp)
        d.update(B=Bp.ptr(), ldb=Bp.ld)
        Cp = R.canary(sp, M, N, N + c["ldc_pad"])
        if c["acc"]:
            Cp.view().copy_(op.C0.float()[None].expand(sp, M, N))
        self.C = Cp.to(DEV)
        d.update(C=self.C.ptr(), ldc=self.C.ld)
        if c["bias"]:
            bias = op.bias.float().to(DEV)
            self.keep.append(bias)
            d["bias"] = bias.data_ptr()
        self.rs = None
        if c["rowsum"]:
            self.rs = R.canary(1, sp, M, M).to(DEV)
            d["rowsumA"] = self.rs.ptr()
        self.d = d

    def check(self, what=""):
        what = what or cid(self.c)
        R.compare(self.C.view(), self.ref.C, f"{what}: C")
        R.check_canary(self.C, f"{what}: C")
        if self.rs is not None:
            R.compare(self.rs.view()[0], self.ref.rowsum, f"{what}: rowsumA")
            R.check_canary(self.rs, f"{what}: rowsumA")


class variants:
    """GemmVariants set for a block and restored after it."""

    def __init__(self, ext, **kw):
        self.ext, self.kw = ext, kw

    def __enter__(self):
        self.saved = self.ext.gemm_variants()
        self.ext.set_gemm_variants(self.kw)

    def __exit__(self, *exc):
        self.ext.set_gemm_variants(self.saved)


def run_nt(ext, c, seed=0):
    j = Job(c, seed)
    ext.gemm_nt(j.d, S())
    torch.cuda.synchronize()
    j.check()
    return j


# ------------------------------------------------------------------ algo 1: gemm_nt_kernel
# 9 or 18 workgroups (more than 8, no multiple of 8: the XCD remap's remainder); K-slices of 32 .. 160
# reach KB = 1, 2, 4 and odd k-step counts of the two-batch pipeline
ALGO1 = [
    case(192, 192, 32, 1, 1, bias=True),
    case(128, 192, 192, 3, 1),
    case(192, 192, 96, 1, 1, acc=True),
    case(64, 192, 384, 3, 1, acc=True),
    case(192, 64, 480, 3, 1),
    case(192, 192, 160, 1, 1, bias=True, acc=True),
    case(192, 192, 128, 1, 1, bias=True),
    case(128, 192, 288, 3, 1, rowsum=False),
    case(192, 192, 64, 1, 1, rowsum=False, ldc_pad=0),
] + [case(192, 192, 32 * n * s, s, 1, onehot=dist)          # the one-hot path with 1-4 k-steps
     for (n, s, dist) in ((1, 1, "uniform"), (2, 3, "names"), (3, 1, "invalid"), (4, 3, "uniform"), (3, 3, "tile"))]

# ------------------------------------------------------------------ algo 2: gemm_lds
# k-tile counts 2, 3, 5 (even / odd ends of the double buffer); raster with ntm < ntn and ntm > ntn
ALGO2 = [
    case(128, 256, 128, 1, 2, bias=True),
    case(256, 128, 576, 3, 2, acc=True),
    case(384, 128, 320, 1, 2, raster=1, acc=True),
    case(128, 384, 192, 1, 2, raster=1, bias=True),
    case(256, 256, 384, 3, 2),
    case(128, 256, 960, 3, 2, raster=1),
    case(384, 256, 192, 1, 2, bias=True, acc=True, rowsum=False),
    case(256, 128, 128, 1, 2, ldc_pad=0),
]
ALGO2_ONEHOT = [
    case(256, 256, 128, 1, 2, onehot="uniform"),
    case(256, 256, 576, 3, 2, onehot="names", b2_row=128),
    case(256, 384, 320, 1, 2, onehot="invalid", b2_row=128),
    case(128, 256, 384, 2, 2, onehot="uniform", raster=1),
    case(256, 256, 192, 1, 2, onehot="holes", b2_row=128, raster=1),
]
LDS_GROUP = [case(128, 256, 128, 1, 2), case(256, 128, 576, 3, 2, acc=True)]

# ------------------------------------------------------------------ algo 3: gemm_small
# K-slices of 2, 3, 4, 8, 16 and 32 64-deep blocks: one burst, or 2 / 4 chunks of 8 blocks
ALGO3 = [
    case(64, 128, 128, 1, 3, bias=True),
    case(128, 64, 384, 2, 3, acc=True),
    case(192, 64, 256, 1, 3, acc=True, bias=True),
    case(64, 192, 1024, 2, 3),
    case(128, 128, 1024, 1, 3, bias=True),
    case(64, 64, 4096, 2, 3),
    case(128, 64, 192, 1, 3, rowsum=False, ldc_pad=0),
    case(128, 64, 128, 1, 3, a32=1),
    case(64, 128, 512, 2, 3, a32=1, acc=True),
    case(128, 64, 128, 1, 3, a32=2),
    case(64, 64, 384, 2, 3, a32=2),
    case(192, 128, 256, 1, 3, a32=2, bias=True),
]
# gemm_small_group: [jobs], per_xcd expected
# the fc_held_ mirror: a first job with row sums and four chunks (K-slices of 4 x the group's depth) and
# two short jobs without; every tile count a multiple of 8 (per-XCD deal) / not (flat deal)
SMALL_GROUPS = {
    "three_per_xcd": ([case(128, 256, 2048, 2, 3), case(256, 128, 256, 1, 3, rowsum=False),
                       case(128, 128, 512, 2, 3, rowsum=False)], 1),
    "three_flat": ([case(64, 192, 1024, 1, 3), case(192, 64, 256, 1, 3, rowsum=False),
                    case(128, 128, 768, 3, 3, rowsum=False)], 0),
    "two_flat_depth2": ([case(192, 64, 128, 1, 3, acc=True), case(64, 64, 768, 3, 3)], 0),
    "four_per_xcd_bias": ([case(128, 256, 192, 1, 3, bias=True), case(256, 128, 192, 1, 3, bias=True, rowsum=False),
                           case(512, 64, 192, 1, 3, bias=True), case(64, 512, 192, 1, 3, bias=True, acc=True)], 1),
}
# record_emb_tail's pair at V = 256, E = 64, H = 256: dW_ih0 = dP^T . Emb (A32 read transposed) and
# dEmb = dP . W_ih0 in H3 / V = 3 slabs, BOTH from the one fp32 dP [V][3H]
EMB_V, EMB_E, EMB_H3 = 256, 64, 768
EMB_TAIL = [case(EMB_H3, EMB_E, EMB_V, 1, 3, a32=2, exps=False, tag="dWih0"),
            case(EMB_V, EMB_E, EMB_H3, 3, 3, a32=1, exps=False, tag="dEmb")]

# ------------------------------------------------------------------ gemm_with_prep
# (case, the route gemm_with_prep takes): the one-shot kernel, the same past 256 tiles at 8 blocks
# (4-block chunks), the LDS kernel (a 5-block K-slice the one-shot kernel has no form for), and the
# two-launch fallback (neither kernel takes N = 192 with 5 blocks)
PREP = [
    (case(256, 192, 128, 1, 0, bias=True, rowsum=False), "small"),
    (case(256, 4160, 512, 1, 0, bias=True, rowsum=False), "small4"),
    (case(128, 256, 320, 1, 0, bias=True, rowsum=False), "lds"),
    (case(64, 192, 320, 1, 0, bias=True, rowsum=False), "two"),
]
# (T, Bp): T * Bp below, at and above the 64 x 256 items one pass of the capped grid covers
PREP_SHAPES = [(8, 64), (64, 256), (65, 256), (3, 32)]

# ------------------------------------------------------------------ algo 5: gemm256
GEMM256 = [
    case(256, 256, 64, 1, 5, bias=True, acc=True, rowsum=False),
    case(256, 512, 192, 1, 5),
    case(768, 256, 576, 3, 5, ldc_pad=0),
    case(1280, 512, 128, 1, 5, bias=True, rowsum=False),
    case(512, 256, 320, 1, 5, acc=True, rowsum=False),
]
GEMM256_192 = case(576, 256, 128, 1, 5)       # 192-row tiles only: the phased 16x16x32 kernel
GEMM256_VARIANTS = [dict(mfma=m, phased=p, sched=0, groupm=g) for m, p, g in itertools.product((16, 32), (0, 1), (1, 4))]

# ------------------------------------------------------------------ onehot_dp
OH_GEO = {1: (128, 64), 2: (64, 128), 3: (32, 256)}      # GemmVariants.onehot -> (NC columns, KT tokens)
OH_NKT = (1, 2, 3, 4, 5, 7, 9)
OH_DISTS = ("uniform", "names", "tile", "invalid", "holes")


def oh_case(geo, nkt, dist):
    """N in {NC, 3 NC} (B2 from row NC) and splits in {1, 2}, alternating over the (nkt, dist) table so
    that every k-tile count meets both of each."""
    NC, KT = OH_GEO[geo]
    i = OH_NKT.index(nkt) + OH_DISTS.index(dist)
    wide, sp = i % 2 == 1, 1 + (i // 2) % 2
    return case(256, 3 * NC if wide else NC, nkt * KT * sp, sp, 2, onehot=dist, b2_row=NC if wide else 0, ldc_pad=0,
                kt=KT, tag=f"g{geo}")


OH_CASES = [oh_case(g, n, d) for g in OH_GEO for n in OH_NKT for d in OH_DISTS]

# ------------------------------------------------------------------ gemm_f32 (fp32 MFMA, gen_f32.hip)
# (M, N, K, splits): the 64 x 64 kernel with K-slices of 16 and 48, and the 128 x 128 kernel at its
# smallest reachable shape (256 tiles)
F32 = [(64, 128, 16, 1), (128, 64, 48, 1), (64, 64, 48, 3), (128, 128, 144, 3), (2048, 2048, 16, 1)]


def f32_host(M, N, K, splits, seed=0):
    op = R.grid_operands(M, N, K, seed, kdepth=K // splits, bias=True, max_bits=12)
    return op, R.product_ref(op, splits=splits, bias_in="slab0")


# ------------------------------------------------------------------ library path / auto dispatch / bias
LIBRARY = [case(128, 256, 512, 1, 4), case(256, 128, 1024, 1, 4, acc=True, ldc_pad=0)]
# algo 0, by reading gemm_nt: one-shot / LDS (5 blocks) / gemm256 (256 tiles) / streaming one-hot /
# register kernel (a 96-deep K-slice) / one-hot LDS (M != 256)
AUTO = [case(64, 128, 128, 1, 0, bias=True), case(128, 128, 320, 1, 0, bias=True), case(4096, 4096, 256, 1, 0, rowsum=False),
        case(256, 128, 128, 1, 0, onehot="uniform", ldc_pad=0), case(64, 64, 96, 1, 0, bias=True),
        case(128, 128, 256, 1, 0, onehot="uniform")]
BIAS_SPLIT = [case(256, 256, 384, 3, algo, bias=True, ldc_pad=0) for algo in (1, 2, 3, 5)]

ALL_CASES = (ALGO1 + ALGO2 + ALGO2_ONEHOT + LDS_GROUP + ALGO3 + [c for g, _ in SMALL_GROUPS.values() for c in g] +
             EMB_TAIL + [c for c, _ in PREP] + GEMM256 + [GEMM256_192] + OH_CASES + LIBRARY + AUTO + BIAS_SPLIT)


# ================================================================== tests
@pytest.mark.parametrize("c", ALGO1, ids=cid)
def test_algo1(ext, c):
    run_nt(ext, c)


@pytest.mark.parametrize("c", ALGO2, ids=cid)
def test_algo2(ext, c):
    j = Job(c)
    assert ext.gemm_lds_ok(j.d)
    ext.gemm_nt(j.d, S())
    torch.cuda.synchronize()
    j.check()


@pytest.mark.parametrize("c", ALGO2_ONEHOT, ids=cid)
def test_algo2_onehot(ext, c):
    with variants(ext, onehot=0):
        j = Job(c)
        assert ext.gemm_lds_ok(j.d)
        ext.gemm_nt(j.d, S())
        torch.cuda.synchronize()
    j.check()


def test_lds_group(ext):
    jobs = [Job(c, seed=i) for i, c in enumerate(LDS_GROUP)]
    assert all(ext.gemm_lds_ok(j.d) for j in jobs)
    ext.gemm_group("lds", [j.d for j in jobs], S())
    torch.cuda.synchronize()
    for i, j in enumerate(jobs):
        j.check(f"lds group job {i}")


@pytest.mark.parametrize("c", ALGO3, ids=cid)
def test_algo3(ext, c):
    j = Job(c)
    assert ext.gemm_small_kblocks(j.d) == c["K"] // c["splits"] // 64
    ext.gemm_nt(j.d, S())
    torch.cuda.synchronize()
    j.check()


def test_a32_needs_algo3(ext):
    j = Job(ALGO3[7])
    for algo in (0, 1, 2, 5):
        with pytest.raises(RuntimeError, match="A32"):
            ext.gemm_nt(dict(j.d, algo=algo), S())


@pytest.mark.parametrize("name", list(SMALL_GROUPS))
def test_small_group(ext, name):
    cases, per_xcd = SMALL_GROUPS[name]
    jobs = [Job(c, seed=i) for i, c in enumerate(cases)]
    depth = ext.gemm_small_group_depth([j.d for j in jobs])
    assert depth in (2, 3, 4, 8)
    tiles = [(c["M"] // 64) * (c["N"] // 64) * c["splits"] for c in cases]
    assert int(all(t % 8 == 0 for t in tiles)) == per_xcd          # the deal the case is there for
    if name.startswith("three"):                                   # first job: row sums, four chunks
        assert cases[0]["rowsum"] and ext.gemm_small_kblocks(jobs[0].d) == 4 * depth
    ext.gemm_group("small", [j.d for j in jobs], S())
    torch.cuda.synchronize()
    for i, j in enumerate(jobs):
        j.check(f"small group {name} job {i}")


def test_small_group_emb_tail(ext):
    """record_emb_tail's grouped pair: one fp32 dP [V][3H] staged transposed by dW_ih0 and plain, in three
    K-slices, by dEmb."""
    cw, ce = EMB_TAIL
    opw, _, refw = host(cw)                       # A = dP^T [3H][V]; the storage of its A32 is dP itself
    dP32 = opw.A32.T.contiguous()                 # [V][3H]
    ope = R.grid_operands(EMB_V, EMB_E, EMB_H3, 1, kdepth=EMB_V, exps=False)
    ope.A32, ope.A = dP32, dP32.bfloat16().double()
    refe = R.product_ref(ope, splits=3)
    jw, je = Job(cw, a32_from=(opw, None, refw)), Job(ce, a32_from=(ope, None, refe))
    dP = R.padded(dP32, EMB_H3 + 8).to(DEV)
    jw.d.update(A32=dP.ptr(), lda=dP.ld)
    je.d.update(A32=dP.ptr(), lda=dP.ld)
    assert ext.gemm_small_kblocks(jw.d) == ext.gemm_small_kblocks(je.d) == 4
    assert ext.gemm_small_group_depth([jw.d, je.d]) == 4
    ext.gemm_group("small", [jw.d, je.d], S())
    torch.cuda.synchronize()
    jw.check("emb tail dW_ih0")
    je.check("emb tail dEmb")


# ------------------------------------------------------------------ batch preparation
class Prep:
    """A staging slot of Bmax > Bp rows holding B < Bp real ones, and canaried outputs."""

    def __init__(self, T, Bp, seed=0):
        g = torch.Generator(device="cpu").manual_seed(seed + 31 * T + Bp)
        self.T, self.Bp, self.Bmax, self.B = T, Bp, Bp + 5, Bp - 3
        x = torch.randint(1, 256, (self.Bmax, T), generator=g, dtype=torch.int32)
        y = torch.randint(0, 256, (self.Bmax, T), generator=g, dtype=torch.int32)
        self.inv = 1.0 / (self.B * T - 7)
        hdr = torch.zeros(16, dtype=torch.int32)
        hdr[0] = self.B
        hdr[1] = struct.unpack("i", struct.pack("f", self.inv))[0]
        self.slot = torch.cat([hdr, x.flatten(), y.flatten()]).to(DEV)
        real = (torch.arange(Bp) < self.B)[None, :]
        self.ids_ref = torch.where(real, x[:Bp].T, torch.zeros((), dtype=torch.int32))
        self.lab_ref = torch.where(real, y[:Bp].T, torch.full((), -1, dtype=torch.int32))
        self.ids = R.canary(1, T, Bp, Bp, dtype=torch.int32).to(DEV)
        self.lab = R.canary(1, T, Bp, Bp, dtype=torch.int32).to(DEV)
        self.ic = R.canary(1, 1, 1, 4).to(DEV)
        self.d = dict(Bmax=self.Bmax, T=T, Bp=Bp, ids=self.ids.ptr(), labels=self.lab.ptr(), inv_count=self.ic.ptr())
        self.d["in"] = self.slot.data_ptr()

    def check(self, what):
        assert torch.equal(self.ids.view()[0].cpu(), self.ids_ref), f"{what}: ids"
        assert torch.equal(self.lab.view()[0].cpu(), self.lab_ref), f"{what}: labels"
        assert self.ic.view().cpu().item() == struct.unpack("f", struct.pack("f", self.inv))[0], f"{what}: inv_count"
        for p, n in ((self.ids, "ids"), (self.lab, "labels"), (self.ic, "inv_count")):
            R.check_canary(p, f"{what}: {n}")


@pytest.mark.parametrize("T,Bp", PREP_SHAPES)
def test_prep_batch(ext, T, Bp):
    p = Prep(T, Bp)
    ext.prep_batch(p.d, S())
    torch.cuda.synchronize()
    p.check(f"prep_batch T={T} Bp={Bp}")


def test_prep_batch_rejects_short_slot(ext):
    """Bp > Bmax would read past the staging slot (kernels.h prep_batch): the bindings refuse it."""
    p = Prep(8, 64)
    with pytest.raises(RuntimeError, match="Bmax"):
        ext.prep_batch(dict(p.d, Bmax=p.Bp - 1), S())
    j = Job(PREP[0][0])
    with pytest.raises(RuntimeError, match="Bmax"):
        ext.gemm_with_prep(j.d, dict(p.d, Bmax=p.Bp - 1), S())


@pytest.mark.parametrize("c,route", PREP, ids=[r for _, r in PREP])
def test_gemm_with_prep(ext, c, route):
    j = Job(c)
    tiles = (c["M"] // 64) * (c["N"] // 64)
    small = ext.gemm_small_kblocks(j.d) and (c["M"] % 128 or c["N"] % 128 or (c["M"] // 128) * (c["N"] // 128) < 256)
    got = ("small4" if ext.gemm_small_kblocks(j.d) == 8 and tiles > 256 else "small") if small else (
        "lds" if ext.gemm_lds_ok(j.d) else "two")
    assert got == route                                           # the route the case is there for
    p = Prep(*PREP_SHAPES[PREP.index((c, route)) % len(PREP_SHAPES)])
    ext.gemm_with_prep(j.d, p.d, S())
    torch.cuda.synchronize()
    j.check(f"gemm_with_prep {route}")
    p.check(f"gemm_with_prep {route}")
    if route.startswith("small"):       # "the same k order, so the same table" (gemm_small_with_prep)
        plain = Job(dict(c, algo=3))
        ext.gemm_nt(plain.d, S())
        torch.cuda.synchronize()
        assert torch.equal(plain.C.view(), j.C.view())


# ------------------------------------------------------------------ gemm256
@pytest.mark.parametrize("v", GEMM256_VARIANTS, ids=lambda v: f"m{v['mfma']}p{v['phased']}g{v['groupm']}")
def test_gemm256(ext, v):
    rows = set()
    with variants(ext, **v):
        for c in GEMM256:
            j = Job(c)
            assert ext.gemm256_ok(j.d), cid(c)
            rows.add(ext.gemm256_tile_rows(j.d))
            ext.gemm_nt(j.d, S())
            torch.cuda.synchronize()
            j.check()
        j = Job(GEMM256_192)
        if v["mfma"] == 16 and v["phased"] == 1:
            assert ext.gemm256_ok(j.d) and ext.gemm256_tile_rows(j.d) == 192
            rows.add(192)
            ext.gemm_nt(j.d, S())
            torch.cuda.synchronize()
            j.check()
        else:                            # 256-row tiles only: M = 576 has no fit, and gemm_nt says so
            assert not ext.gemm256_ok(j.d) and ext.gemm256_tile_rows(j.d) == 0
            with pytest.raises(RuntimeError):
                ext.gemm_nt(j.d, S())
    assert rows == ({256, 192} if v["mfma"] == 16 and v["phased"] == 1 else {256})


def test_gemm256_tile_rows_both(ext):
    """Under the phased 16x16x32 form the case list reaches 256- and 192-row tiles (768 x 256 in three
    K-slices fills more of a round with 192-row tiles)."""
    with variants(ext, mfma=16, phased=1, sched=0, groupm=4):
        rows = {cid(c): ext.gemm256_tile_rows(Job(c).d) for c in GEMM256 + [GEMM256_192]}
    assert set(rows.values()) == {256, 192}, rows
    assert rows[cid(GEMM256[2])] == 192 and rows[cid(GEMM256[3])] == 256


def test_gemm256_split_needs_dense_c(ext):
    """gemm256 writes split-K slabs only to a dense C: the predicate says so and gemm_nt refuses ldc > N."""
    c = dict(GEMM256[2], ldc_pad=32)
    j = Job(c)
    assert not ext.gemm256_ok(j.d)
    with pytest.raises(RuntimeError):
        ext.gemm_nt(j.d, S())
    torch.cuda.synchronize()
    assert bool((j.C.buf.cpu().view(torch.int32) == R.PATTERN).all()), "a refused launch wrote to C"


# ------------------------------------------------------------------ onehot_dp
@pytest.mark.parametrize("c", OH_CASES, ids=cid)
def test_onehot_dp(ext, c):
    geo = int(c["tag"][1:])
    with variants(ext, onehot=geo):
        j = Job(c)
        assert ext.onehot_dp_ok(j.d)
        ext.gemm_nt(j.d, S())
        torch.cuda.synchronize()
    j.check()
    with variants(ext, onehot=0):        # the one-hot gemm_lds kernel, wherever it takes the shape: bitwise
        l = Job(c)
        if ext.gemm_lds_ok(l.d):
            ext.gemm_nt(l.d, S())
            torch.cuda.synchronize()
            l.check("one-hot gemm_lds")
            assert torch.equal(l.C.view(), j.C.view())


@pytest.mark.parametrize("geo", list(OH_GEO))
def test_onehot_dp_needs_dense_c(ext, geo):
    """ldc > N: the predicate refuses, and gemm_nt does not take the streaming kernel -- N = 64 fits no
    other one-hot kernel of algo 2, so the call throws; with N = 128 the one-hot gemm_lds kernel runs."""
    NC, KT = OH_GEO[geo]
    with variants(ext, onehot=geo):
        j = Job(case(256, 64, 2 * KT, 1, 2, onehot="uniform", ldc_pad=32, kt=KT))
        assert ext.onehot_dp_ok(dict(j.d, ldc=64)) == (64 % NC == 0)
        assert not ext.onehot_dp_ok(j.d)
        with pytest.raises(RuntimeError):
            ext.gemm_nt(j.d, S())
        j = Job(case(256, 128, 2 * KT, 1, 2, onehot="uniform", ldc_pad=32, kt=KT))
        assert not ext.onehot_dp_ok(j.d) and ext.gemm_lds_ok(j.d)
        ext.gemm_nt(j.d, S())
        torch.cuda.synchronize()
        j.check()


def test_onehot_dp_splits(ext):
    for geo, (NC, KT) in OH_GEO.items():
        with variants(ext, onehot=geo):
            for N, K in ((3 * NC, 8 * KT), (NC, 3 * KT), (6144, 65536)):
                sp = 1
                while sp * 2 * (N // NC) <= 384 and K % (sp * 2 * KT) == 0:
                    sp *= 2
                assert ext.onehot_dp_splits(dict(M=256, N=N, K=K)) == sp


# ------------------------------------------------------------------ gemm_f32
@pytest.mark.parametrize("M,N,K,splits", F32)
def test_gemm_f32(ext, M, N, K, splits):
    op, ref = f32_host(M, N, K, splits)
    A, B = R.padded(op.A.float(), K + 4).to(DEV), R.padded(op.B.float(), K + 12).to(DEV)
    assert torch.equal(A.view()[0].double().cpu(), op.A)
    C = R.canary(splits, M, N, N + 8, slab_rows=M + 3).to(DEV)      # slab > M * ldc
    bias = op.bias.float().to(DEV)
    ext.gemm_f32(dict(A=A.ptr(), lda=A.ld, B=B.ptr(), ldb=B.ld, C=C.ptr(), ldc=C.ld, bias=bias.data_ptr(), M=M, N=N, K=K,
                      splits=splits, slab=(M + 3) * C.ld), S())
    torch.cuda.synchronize()
    R.compare(C.view(), ref.C, "gemm_f32: C")
    R.check_canary(C, "gemm_f32: C")


# ------------------------------------------------------------------ library path, auto dispatch, bias
@pytest.mark.parametrize("c", LIBRARY, ids=cid)
def test_library(ext, c):
    run_nt(ext, c)


@pytest.mark.parametrize("K", [8, 264, 8192, 8200])
def test_rowsum_bf16(ext, K):
    """The 4-deep loop (K / 8 > 768 chunks), its remainder, and fewer chunks than threads."""
    M = 5
    op = R.grid_operands(M, 64, K, K)
    A = R.padded(bf16_exact(op.A), K + 8).to(DEV)
    out = R.canary(1, 1, M, M).to(DEV)
    ext.rowsum_bf16(A.ptr(), A.ld, M, K, out.ptr(), S())
    torch.cuda.synchronize()
    R.compare(out.view()[0], R.product_ref(op).rowsum, "rowsum_bf16")
    R.check_canary(out, "rowsum_bf16")


@pytest.mark.parametrize("c", AUTO, ids=cid)
def test_auto_dispatch(ext, c):
    run_nt(ext, c)


def test_bias_ignored_when_split(ext):
    """One contract (kernels.h GemmArgs::bias, "non-split only"): with splits > 1 gemm_nt ignores the bias
    on every kernel -- a bias per slab would count `splits` times in the caller's slab sum.  The
    reference (gemm_ref.product_ref bias_in="unsplit") adds none."""
    outs = []
    for c in BIAS_SPLIT:
        j = run_nt(ext, c)
        assert "bias" in j.d and j.op.bias.abs().min() > 0
        outs.append(j.C.view().clone())
    for o in outs[1:]:
        assert torch.equal(o, outs[0])


# ------------------------------------------------------------------ companions
@pytest.mark.parametrize("Rr,Cc", [(1, 64), (3, 70), (256, 1536)])
def test_colsum(ext, Rr, Cc):
    g = torch.Generator(device="cpu").manual_seed(Rr + Cc)
    x = torch.randint(-(1 << 14), 1 << 14, (Rr, Cc), generator=g).double() * torch.exp2(
        torch.randint(-3, 4, (Cc,), generator=g).double())[None, :]
    src = x.float().to(DEV)
    out = R.canary(1, 1, Cc, Cc).to(DEV)
    ext.colsum(src.data_ptr(), Rr, Cc, out.ptr(), S())
    torch.cuda.synchronize()
    R.compare(out.view()[0, 0], x.sum(0).float(), "colsum")          # |sum| < 256 * 2^14 lsbs: exact
    R.check_canary(out, "colsum")


def rounding_values(n, seed):
    """fp32 values for the bf16 conversions: random ones, exact ties both ways, +-0, the largest bf16
    and the values around it that still round to a finite bf16."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-20, 20, (n,), generator=g).float())
    special = torch.tensor([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x00000000,
                            0x80000000, 0x7F7F0000, 0x7F7F7FFF, 0x7F7E8000, 0x7F7E8001, 0xFF7F7FFF, 0x3FFF8000],
                           dtype=torch.int64)
    special = (special - ((special >> 31) << 32)).to(torch.int32).view(torch.float32)
    k = min(n, len(special))
    x[torch.randperm(n, generator=g)[:k]] = special[:k]
    return x


def bits16(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("n", [1, 7, 1030, 70001])
def test_cast_bf16(ext, n):
    x = rounding_values(n, n)
    src = x.to(DEV)
    out = R.canary(1, 1, n, n, dtype=torch.bfloat16).to(DEV)
    ext.cast_bf16(src.data_ptr(), n, out.ptr(), S())
    torch.cuda.synchronize()
    assert torch.equal(bits16(out.view()[0, 0].cpu()), bits16(x.bfloat16()))
    R.check_canary(out, "cast_bf16")


@pytest.mark.parametrize("Rr,Cc", [(1, 1), (3, 70), (65, 129), (130, 67)])
def test_transpose_bf16(ext, Rr, Cc):
    x = rounding_values(Rr * Cc, Rr * Cc).view(Rr, Cc)
    src = x.to(DEV)
    out = R.canary(1, Cc, Rr, Rr, dtype=torch.bfloat16).to(DEV)
    ext.transpose_bf16(src.data_ptr(), Rr, Cc, out.ptr(), S())
    torch.cuda.synchronize()
    assert torch.equal(bits16(out.view()[0].cpu()), bits16(x.T.contiguous().bfloat16()))
    R.check_canary(out, "transpose_bf16")


@pytest.mark.parametrize("n,splits", [(1, 1), (7, 3), (1030, 4), (70001, 3)])
def test_reduce_slabs(ext, n, splits):
    g = torch.Generator(device="cpu").manual_seed(n)
    x = torch.randint(-(1 << 20), 1 << 20, (splits, n), generator=g).double() * 0.125     # sums < 2^23 lsbs: exact
    src = x.float().to(DEV)
    out = R.canary(1, 1, n, n).to(DEV)
    ext.reduce_slabs(src.data_ptr(), splits, n, out.ptr(), S())
    torch.cuda.synchronize()
    R.compare(out.view()[0, 0], x.sum(0).float(), "reduce_slabs")
    R.check_canary(out, "reduce_slabs")


@pytest.mark.parametrize("Rr,K", [(3, 70), (1, 1), (64, 512), (1030, 1024)])   # 1030 x 1024 > 4096 blocks x 256
def test_split_bf16x3(ext, Rr, K):
    """dst [R][3K] = [hi | lo | hi], hi = bf16(x), lo = bf16(x - hi), bitwise."""
    x = rounding_values(Rr * K, Rr + K).view(Rr, K)
    src = x.to(DEV)
    out = R.canary(1, Rr, 3 * K, 3 * K, dtype=torch.bfloat16).to(DEV)
    ext.split_bf16x3(src.data_ptr(), Rr, K, out.ptr(), S())
    torch.cuda.synchronize()
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    assert torch.equal(bits16(out.view()[0].cpu()), bits16(torch.cat([hi, lo, hi], 1)))
    R.check_canary(out, "split_bf16x3")

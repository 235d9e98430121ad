"""The optimiser tail (misc.hip + optim_dev.h) per element against fp64: the fused Adam/SGD +
bf16-refresh launch, the plain Adam kernel, global-norm clipping, the slab reductions, the loss sum
and the sharded optimiser's bias pack -- through raw-kernel bindings, and once more through
HipTrainer.

Reference: fp64 torch.  The hyper-parameters are the fp32-rounded values promoted to double (the
device holds them as float), lr_t comes from cpu_ref.lr_at, and every step's reference starts from
the device's own pre-step p, m, v, so each step is judged on its own and no bound needs an
accumulation term.

Bounds (eps32 = 2^-24 is the fp32 unit round-off; gs = g * gscale):
  v = b2*v0 + (1-b2)*gs*gs: every term is positive, so the error is relative to v itself.  Roundings:
      gs, (1-b2)*gs, *gs, b2*v0, the sum (1 - b2 is exact in fp32) -- at most 3 of them on any one
      term plus the sum, 4 eps32 = 2^-22 worst case, 2^-20 leaves 4x; atol 1e-37 for results in the
      fp32 denormal range.
  m = b1*m0 + (1-b1)*gs: the two terms may cancel, so the bound is relative to their magnitudes:
      gs and (1-b1)*gs round (2 eps32 on that term), b1*m0 rounds (1 eps32), the sum rounds
      (1 eps32 of |m| <= both terms): within 2^-22 * (|b1*m0| + |(1-b1)*gs|).
  p (Adam) = p0 - lr_t*u, u = m^/(sqrt(v^) + eps) + wd*p0: one rounding of the result (2^-24 |p|,
      2^-23 allowed) plus lr_t * |du|; du <= (1 + |u|) * (8e-6 + 2^-22 / (1 - b2^t)): the first term
      for the roundings of m, v, the corrections, sqrtf, the division and lr_t itself (cosf, powf, FMA
      contraction; an fp32 emulation in the kernel's operation order measured 1.8e-6), the second for
      the cancellation in 1 - powf(b2, t) (an error of 4 ulp(1) relative to 1 - b2^t).
  p (SGD) = p0 - lr_t*(gs + wd*p0): 2^-23 |p| + lr_t * 2^-22 * (|gs| + |wd*p0|).
Worst err / tol measured on an MI355X over every case here: v 0.25, m 0.63, p (Adam) 0.48, p (SGD) 0.52
(each check prints its own).

Every buffer is over-allocated and filled with NaN (fp32) or a sentinel bit pattern (bf16, ints)
between the jobs and past the end; untouched memory is asserted untouched.
"""
import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import cpu_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT16 = 0x5A5A     # bf16 sentinel (as int16)
NAN_BITS = 0x7FC00000


def S():
    return torch.cuda.current_stream().cuda_stream


def f32(x):
    """The fp32-rounded value as a Python double: what the device holds."""
    return float(np.float32(x))


SCHEDS = {   # name -> OptimArgs schedule fields (warm-up at t <= warmup)
    "const": dict(sched=0, warmup=0, total=0, lr_min=0.0),
    "cosine": dict(sched=1, warmup=2, total=6, lr_min=f32(1e-4)),
    "linear": dict(sched=2, warmup=2, total=6, lr_min=f32(1e-4)),
}


def hyper(sgd=0, wd=0.0, sched="const", lr=1e-3):
    hp = dict(lr=f32(lr), b1=f32(0.9), b2=f32(0.999), eps=f32(1e-8), wd=f32(wd), sgd=int(sgd))
    hp.update(SCHEDS[sched])
    return hp


def lr_ref(hp, t):
    cfg = GRUConfig(lr=hp["lr"], lr_sched=cpu_ref.LR_SCHEDS[hp["sched"]], warmup_steps=hp["warmup"],
                    total_steps=hp["total"], lr_min=hp["lr_min"])
    return cpu_ref.lr_at(cfg, t)


def _le(err, tol, what, tag):
    """err <= tol per element (a NaN fails); prints the worst err / tol first."""
    ok = err <= tol
    ratio = float((err / tol.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max()) if err.numel() else 0.0
    print(f"[optim] {tag} {what}: worst err/tol {ratio:.3g} over {err.numel()} elements")
    if not bool(ok.all()):
        i = int((~ok).nonzero()[0])
        raise AssertionError(f"{tag} {what}: {int((~ok).sum())} of {err.numel()} elements out of bound, first at {i}: "
                             f"err {float(err[i]):.3e} > tol {float(tol[i]):.3e} (worst err/tol {ratio:.3g})")
    return ratio


def check_update(p, m, v, p0, g, m0, v0, t, hp, sc, tag):
    """One optimiser step per element against fp64.  p, m, v: after the step; p0, g, m0, v0: the
    device's values before it (fp32, any device); sc: the gradient scale as a double."""
    d = lambda x: x.detach().double().cpu().reshape(-1)
    p, p0, g = d(p), d(p0), d(g)
    lr_t, b1, b2, eps, wd = lr_ref(hp, t), hp["b1"], hp["b2"], hp["eps"], hp["wd"]
    gs = g * sc
    if hp["sgd"]:
        p64 = p0 - lr_t * (gs + wd * p0)
        _le((p - p64).abs(), 2.0 ** -23 * p64.abs() + lr_t * 2.0 ** -22 * (gs.abs() + (wd * p0).abs()), "p(sgd)", tag)
        return
    m, v, m0, v0 = d(m), d(v), d(m0), d(v0)
    m64 = b1 * m0 + (1 - b1) * gs
    v64 = b2 * v0 + (1 - b2) * gs * gs
    u64 = (m64 / (1 - b1 ** t)) / ((v64 / (1 - b2 ** t)).sqrt() + eps) + wd * p0
    p64 = p0 - lr_t * u64
    _le((v - v64).abs(), 2.0 ** -20 * v64.abs() + 1e-37, "v", tag)
    _le((m - m64).abs(), 2.0 ** -22 * ((b1 * m0).abs() + ((1 - b1) * gs).abs()), "m", tag)
    _le((p - p64).abs(), 2.0 ** -23 * p64.abs() + lr_t * (1 + u64.abs()) * (8e-6 + 2.0 ** -22 / (1 - b2 ** t)), "p(adam)", tag)


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).reshape(-1)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def sent16(n, pad=64):
    """bf16 output buffer of n elements (+ pad) holding the sentinel, as int16."""
    return torch.full((n + pad,), SENT16, dtype=torch.int16, device=DEV)


def assert_bf16(buf, ref, what):
    """buf[:n] holds ref (a bf16 tensor) bitwise and the sentinel after it."""
    r = bits(ref)
    assert torch.equal(buf[:r.numel()], r), what
    assert bool((buf[r.numel():] == SENT16).all()), f"{what}: wrote past the end"


class Flat:
    """Flat fp32 p / g / m / v buffers, NaN outside the jobs' spans and past the end.

    Gradients: magnitudes 10^U(-9, 1) (fixed per element) times a fresh normal, every 97th exactly 0:
    |g| ~ 1e-9 makes the placement of eps = 1e-8 decide the update.  zero = (start, len): a block with
    p = g = m = v = 0 that must stay bitwise 0."""

    def __init__(self, spans, seed, zero=None, pad=64):
        self.spans, self.zero = spans, zero
        self.n = max(o + n for o, n in spans)
        self.alloc = self.n + pad
        self.gen = torch.Generator().manual_seed(seed)
        live = torch.zeros(self.alloc, dtype=torch.bool)
        for o, n in spans:
            assert not live[o:o + n].any()
            live[o:o + n] = True
        self.live_cpu = live
        self.live = live.to(DEV)
        self.mag = 10.0 ** (torch.rand(self.alloc, generator=self.gen, dtype=torch.float64) * 10 - 9)
        self.p = self._fill(torch.randn(self.alloc, generator=self.gen) * 0.1)
        self.m = self._fill(torch.zeros(self.alloc))
        self.v = self._fill(torch.zeros(self.alloc))
        self.g = torch.full((self.alloc,), float("nan"), device=DEV)
        self.step = torch.tensor([0, -7], dtype=torch.int32, device=DEV)
        self.new_grad()

    def _fill(self, vals):
        out = torch.full((self.alloc,), float("nan"))
        out[self.live_cpu] = vals.float()[self.live_cpu]
        if self.zero:
            out[self.zero[0]:self.zero[0] + self.zero[1]] = 0.0
        return out.to(DEV)

    def new_grad(self):
        g = self.mag * torch.randn(self.alloc, generator=self.gen, dtype=torch.float64)
        g[::97] = 0.0
        self.g.copy_(self._fill(g))
        return self.g

    def moments_like_a_run(self):
        """m, v as after a few steps of gradients of the same per-element magnitudes."""
        g = (self.mag * torch.randn(self.alloc, generator=self.gen, dtype=torch.float64))
        self.m.copy_(self._fill(0.3 * g))
        self.v.copy_(self._fill(0.01 * g * g))

    def opt(self, hp, t, gscale=0, err=0, err_host=0, keep_g=1, null_mv=False):
        self.step[0] = t
        d = dict(hp)
        d.update(p=self.p.data_ptr(), g=self.g.data_ptr(), m=0 if null_mv else self.m.data_ptr(),
                 v=0 if null_mv else self.v.data_ptr(), n=self.n, step=self.step.data_ptr(), gscale=gscale,
                 err=err, err_host=err_host, keep_g=keep_g)
        return d

    def snapshot(self):
        return self.p.clone(), self.g.clone(), self.m.clone(), self.v.clone()

    def check(self, before, t, hp, sc, tag, g=None):
        """Live elements against fp64, everything else bitwise as before, the zero block bitwise 0."""
        torch.cuda.synchronize()
        p0, g0, m0, v0 = before
        L = self.live
        check_update(self.p[L], self.m[L], self.v[L], p0[L], (g0 if g is None else g)[L], m0[L], v0[L], t, hp, sc, tag)
        for name, now, was in (("p", self.p, p0), ("m", self.m, m0), ("v", self.v, v0)):
            assert torch.equal(bits(now)[~L], bits(was)[~L]), f"{tag}: {name} written outside the jobs"
            if hp["sgd"] and name != "p":
                assert same_bits(now, was), f"{tag}: SGD touched {name}"
        assert self.step.tolist() == [t, -7], f"{tag}: step word changed"
        if self.zero:
            z = slice(self.zero[0], self.zero[0] + self.zero[1])
            for name, now in (("p", self.p), ("m", self.m), ("v", self.v)):
                assert bool((bits(now)[z] == 0).all()), f"{tag}: zero block of {name} moved"


def dev_scalar(x):
    return torch.tensor([x], dtype=torch.float32, device=DEV)


# ------------------------------------------------------------------ 1. the update rule
STEPS = (1, 2, 3, 10, 1000)


@pytest.mark.parametrize("sched", ["const", "cosine", "linear"])
@pytest.mark.parametrize("gs", [None, 0.37])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("sgd", [0, 1])
def test_adam_cast_multi_update_rule(ext, sgd, wd, gs, sched):
    """Four jobs in the trainer's order (matrix, matrix, flat, matrix) in one launch, steps 1, 2, 3, 10
    and 1000 written to the device step word: p, m, v per element, the row-major / transposed copies
    of the matrices, the gaps (4 to 64 floats) between the jobs."""
    shapes = [(64, 64), (192, 64), (0, 768), (64, 256)]
    gaps = [64, 4, 64, 12]
    jobs, spans, off = [], [], 0
    for (R, C), gap in zip(shapes, gaps):
        off += gap
        n = R * C if R else C
        jobs.append(dict(off=off, R=R, C=C))
        spans.append((off, n))
        off += n
    fl = Flat(spans, seed=1 + sgd + 2 * (wd > 0) + 4 * (gs is not None), zero=(spans[1][0], 64))
    copies = []
    for j, (o, n) in zip(jobs, spans):
        if j["R"]:
            d, dT = sent16(n), sent16(n)
            j.update(dst=d.data_ptr(), dstT=dT.data_ptr())
            copies.append((j, d, dT))
    hp = hyper(sgd, wd, sched)
    scale = dev_scalar(gs) if gs is not None else None
    sc = f32(gs) if gs is not None else 1.0
    for i, t in enumerate(STEPS):
        if i:
            fl.new_grad()
        before = fl.snapshot()
        # SGD never reads m / v: null pointers on every other step, real buffers (checked untouched) else
        null_mv = bool(sgd) and i % 2 == 1
        ext.adam_cast_multi(fl.opt(hp, t, gscale=scale.data_ptr() if scale is not None else 0, null_mv=null_mv), jobs, S())
        tag = f"sgd={sgd} wd={wd} gs={gs} {sched} t={t}"
        fl.check(before, t, hp, sc, tag)
        assert same_bits(fl.g, before[1]), f"{tag}: gradient buffer written"
        for j, d, dT in copies:
            P = fl.p[j["off"]:j["off"] + j["R"] * j["C"]].view(j["R"], j["C"]).bfloat16()
            assert_bf16(d, P, f"{tag}: dst of {j['R']}x{j['C']}")
            assert_bf16(dT, P.T.contiguous(), f"{tag}: dstT of {j['R']}x{j['C']}")


# ------------------------------------------------------------------ 2. the bf16 copies
OUTSETS = {"all": ("dst", "dstT", "dstF", "dstTF"), "dst+dstT": ("dst", "dstT"), "ft": ("dstF", "dstTF"),
           "dstT": ("dstT",), "none": ()}


@pytest.mark.parametrize("outs", sorted(OUTSETS))
@pytest.mark.parametrize("R,C", [(64, 64), (64, 192), (192, 64), (256, 128)])
def test_adam_cast_multi_copies(ext, R, C, outs):
    """Every written copy is a layout of the device's own updated p, bitwise.  The copies leave
    through the swizzled LDS tile (rows 32..63 swap 4-column groups): random, asymmetric contents whose
    rows 32..63 differ from rows 0..31, so a missed swizzle or a transposed write shows."""
    from gru_mpi_cuda_amd.ops import ft_layout
    n = R * C
    spans = [(64, 256), (64 + 256 + 4, n)]   # a flat job first: the matrix's blocks start at 1
    fl = Flat(spans, seed=R + C)
    fl.moments_like_a_run()
    off = spans[1][0]
    P0 = fl.p[off:off + n].view(R, C)
    assert not torch.equal(P0[:32].bfloat16(), P0[32:64].bfloat16()) and not torch.equal(P0[:, :64].bfloat16(), P0[:64, :].T.bfloat16())
    bufs = {k: sent16(n) for k in OUTSETS["all"]}
    job = dict(off=off, R=R, C=C)
    job.update({k: bufs[k].data_ptr() for k in OUTSETS[outs]})
    hp = hyper(0, 0.01)
    before = fl.snapshot()
    ext.adam_cast_multi(fl.opt(hp, 3), [dict(off=64, R=0, C=256), job], S())
    fl.check(before, 3, hp, 1.0, f"copies {R}x{C} {outs}")
    P = fl.p[off:off + n].view(R, C).bfloat16()
    assert not same_bits(fl.p[off:off + n], before[0][off:off + n])   # the update happened
    want = {"dst": P, "dstT": P.T.contiguous(), "dstF": ft_layout(P), "dstTF": ft_layout(P.T.contiguous())}
    for k, buf in bufs.items():
        if k in OUTSETS[outs]:
            assert_bf16(buf, want[k], f"{k} of {R}x{C} ({outs})")
        else:
            assert bool((buf == SENT16).all()), f"{k} written though not asked for"


# ------------------------------------------------------------------ 3. slabs, flat jobs, the gate
def seq_sum(slabs):
    """fp32 sum in slab order 0, 1, 2, ... (what sum_slabs4 and the tail loops compute, bitwise)."""
    ref = slabs[0].clone()
    for k in range(1, slabs.shape[0]):
        ref += slabs[k]
    return ref


def make_slabs(nsl, n, seed, pad=64):
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((nsl * n + pad,), float("nan"))
    buf[:nsl * n] = torch.randn(nsl * n, generator=g) * (10.0 ** (torch.rand(nsl * n, generator=g) * 4 - 3))
    buf = buf.to(DEV)
    return buf, buf[:nsl * n].view(nsl, n)


@pytest.mark.parametrize("nsl", [1, 2, 8, 9, 10, 17])
@pytest.mark.parametrize("kind", ["matrix", "flat"])
def test_adam_cast_multi_slabs(ext, kind, nsl):
    """A job's gradient summed from nsl slabs inside the launch (1 slab + rounds of 8 in flight):
    keep_g = 1 leaves the fp32 sum in slab order in g, bitwise; keep_g = 0 does not write g; the
    update is the same bitwise, and right per element against fp64."""
    R, C = (64, 128) if kind == "matrix" else (0, 1028)
    n = R * C if R else C
    off = 68
    hp = hyper(0, 0.01)
    raw, slabs = make_slabs(nsl, n, seed=nsl)
    gsum = seq_sum(slabs)
    runs = []
    for keep_g in (1, 0):
        fl = Flat([(off, n)], seed=7)
        fl.moments_like_a_run()
        fl.g.fill_(float("nan"))
        before = fl.snapshot()
        gfull = torch.zeros_like(fl.g)
        gfull[off:off + n] = gsum
        ext.adam_cast_multi(fl.opt(hp, 4, keep_g=keep_g), [dict(off=off, R=R, C=C, gsl=slabs.data_ptr(), nsl=nsl)], S())
        fl.check(before, 4, hp, 1.0, f"slabs {kind} nsl={nsl} keep_g={keep_g}", g=gfull)
        if keep_g:
            assert torch.equal(fl.g[off:off + n], gsum), "g is not the slab sum in order 0, 1, 2, ..."
            assert bool((bits(fl.g)[~fl.live] == NAN_BITS).all()), "g written outside the job"
        else:
            assert bool((bits(fl.g) == NAN_BITS).all()), "keep_g = 0 wrote the gradient buffer"
        runs.append(fl)
    for name in ("p", "m", "v"):
        assert same_bits(getattr(runs[0], name), getattr(runs[1], name)), f"{name} differs between keep_g = 1 and 0"
    assert bool(raw[nsl * n:].isnan().all())


@pytest.mark.parametrize("with_dst", [False, True])
@pytest.mark.parametrize("C", [4, 256, 1024, 1028, 1536])
def test_adam_cast_multi_flat_jobs(ext, C, with_dst):
    """Two flat jobs of C elements (1024 per block, guarded by t * 1024 + 4 * tid < C), 4 NaN floats
    apart, between two matrix jobs in one launch (blocks dealt by the blk_start prefix sum); with dst,
    the flat bf16 mirror dst[i - off] = bf16(p[i])."""
    oA = 64 + 4096 + 8
    oB = oA + C + 4
    oM = oB + C + 60
    spans = [(64, 4096), (oA, C), (oB, C), (oM, 4096)]
    fl = Flat(spans, seed=C, zero=(oA, 4))
    fl.moments_like_a_run()
    dA, dB = sent16(C), sent16(C)
    jobs = [dict(off=64, R=64, C=64), dict(off=oA, R=0, C=C), dict(off=oB, R=0, C=C), dict(off=oM, R=64, C=64)]
    if with_dst:
        jobs[1]["dst"], jobs[2]["dst"] = dA.data_ptr(), dB.data_ptr()
    gs = dev_scalar(0.37)
    hp = hyper(0, 0.01, "cosine")
    before = fl.snapshot()
    ext.adam_cast_multi(fl.opt(hp, 3, gscale=gs.data_ptr()), jobs, S())
    fl.check(before, 3, hp, f32(0.37), f"flat C={C} dst={with_dst}")
    for o, d in ((oA, dA), (oB, dB)):
        if with_dst:
            assert_bf16(d, fl.p[o:o + C].bfloat16(), f"flat mirror at {o}")
        else:
            assert bool((d == SENT16).all())


@pytest.mark.parametrize("errv", [5, 0])
def test_adam_cast_multi_error_gate(ext, errv):
    """A set step error word skips the whole update -- p, m, v, g and every copy stay bitwise -- and is
    mirrored to err_host; a clear word lets the update through and mirrors 0."""
    n = 64 * 64
    oF = 64 + n + 4
    fl = Flat([(64, n), (oF, 256)], seed=3)
    fl.moments_like_a_run()
    raw, slabs = make_slabs(3, n, seed=5)
    fl.g[64:64 + n] = float("nan")   # comes from the slabs
    bufs = {k: sent16(n) for k in OUTSETS["all"]}
    dflat = sent16(256)
    jobs = [dict(off=64, R=64, C=64, gsl=slabs.data_ptr(), nsl=3, **{k: b.data_ptr() for k, b in bufs.items()}),
            dict(off=oF, R=0, C=256, dst=dflat.data_ptr())]
    err = torch.tensor([errv, -3], dtype=torch.int32, device=DEV)
    err_host = torch.tensor([-1, -1], dtype=torch.int32, device=DEV)
    hp = hyper(0, 0.01)
    before = fl.snapshot()
    ext.adam_cast_multi(fl.opt(hp, 2, err=err.data_ptr(), err_host=err_host.data_ptr()), jobs, S())
    torch.cuda.synchronize()
    assert err_host.tolist() == [errv, -1] and err.tolist() == [errv, -3]
    if errv:
        for name, now, was in zip("pgmv", (fl.p, fl.g, fl.m, fl.v), before):
            assert same_bits(now, was), f"{name} changed on a failed step"
        for k, b in list(bufs.items()) + [("flat dst", dflat)]:
            assert bool((b == SENT16).all()), f"{k} written on a failed step"
        return
    gfull = before[1].clone()
    gfull[64:64 + n] = seq_sum(slabs)
    fl.check(before, 2, hp, 1.0, "gate open", g=gfull)
    assert torch.equal(fl.g[64:64 + n], gfull[64:64 + n])
    P = fl.p[64:64 + n].view(64, 64).bfloat16()
    assert_bf16(bufs["dst"], P, "dst")
    assert_bf16(dflat, fl.p[oF:oF + 256].bfloat16(), "flat dst")


# ------------------------------------------------------------------ 4. the plain Adam kernel
@pytest.mark.parametrize("sgd,wd,gs", [(0, 0.0, None), (0, 0.01, 0.37), (1, 0.01, 0.37)])
@pytest.mark.parametrize("n", [4, 5, 6, 7, 4096, 4099, 65540])
def test_adam_step(ext, n, sgd, wd, gs):
    """adam_kernel (the fallback for shapes off the 64-grid) at every n, the n % 4 tail included."""
    fl = Flat([(0, n)], seed=n)
    hp = hyper(sgd, wd, "linear")
    scale = dev_scalar(gs) if gs is not None else None
    for i, t in enumerate((1, 2, 1000)):
        if i:
            fl.new_grad()
        before = fl.snapshot()
        ext.adam_step(fl.opt(hp, t, gscale=scale.data_ptr() if scale is not None else 0), S())
        fl.check(before, t, hp, f32(gs) if gs is not None else 1.0, f"adam_step n={n} sgd={sgd} wd={wd} gs={gs} t={t}")
        assert same_bits(fl.g, before[1])


# ------------------------------------------------------------------ 5. global-norm clipping
@pytest.mark.parametrize("nparts", [1, 256])
@pytest.mark.parametrize("n", [4, 1023, 65536, (1 << 20) + 3])
def test_grad_clip_scale(ext, n, nparts):
    """sumsq_partials + clip_scale_finalize: norm and scale against fp64 (fp32 partial sums of at most
    4096 terms per thread chain: well inside rtol 1e-5), scale exactly 1 when the norm is under the clip
    or zero; then the fused Adam launch reads the device scale as its gscale."""
    fl = Flat([(0, n)], seed=n + nparts)
    # norm ~ 3: far above the 1e-6 the kernel adds to it, or "exactly 1 under the clip" would not hold
    fl.g[:n] *= 3.0 / float(fl.g[:n].double().norm())
    parts =torch.full((nparts + 64,), float("nan"), device=DEV)
    scale = torch.full((2 + 64,), float("nan"), device=DEV)
    norm64 = float(fl.g[:n].double().norm())

    def run(x, clip):
        ext.grad_clip_scale(dict(x=x.data_ptr(), n=n, parts=parts.data_ptr(), nparts=nparts, clip=clip,
                                 scale=scale.data_ptr()), S())
        torch.cuda.synchronize()
        assert bool(parts[:nparts].isfinite().all()) and bool((bits(parts)[nparts:] == NAN_BITS).all())
        assert bool((bits(scale)[2:] == NAN_BITS).all())
        return float(scale[0]), float(scale[1])

    clip = f32(norm64 / 2)
    s, nrm = run(fl.g, clip)
    print(f"[optim] clip n={n} nparts={nparts}: norm rel err {abs(nrm - norm64) / norm64:.3g}")
    assert abs(nrm - norm64) <= 1e-5 * norm64
    want = min(1.0, clip / (norm64 + 1e-6))
    assert want < 1 and abs(s - want) <= 1e-5 * want
    s1, _ = run(fl.g, f32(norm64 * 2))
    assert s1 == 1.0
    sz, nz = run(torch.zeros(n + 64, device=DEV), clip)
    assert sz == 1.0 and nz == 0.0
    # the clipped update: one flat job over the 4-aligned prefix, gscale = the device's own scale
    C = n // 4 * 4
    s, _ = run(fl.g, clip)
    hp = hyper(0, 0.01)
    before = fl.snapshot()
    fl.live[C:] = False   # the n % 4 tail is no job: it stays as it is
    ext.adam_cast_multi(fl.opt(hp, 1, gscale=scale.data_ptr()), [dict(off=0, R=0, C=C)], S())
    fl.check(before, 1, hp, s, f"clipped adam n={n}")


# ------------------------------------------------------------------ 6. / 7. slab and partial sums
def test_reduce_slabs_multi(ext):
    """Seven jobs in one launch: the n < 4 wave path (the loss), the n % 4 tail, 17 slabs, the 512-block
    cap and two cast jobs; bump incremented exactly once per launch, left alone when null."""
    plain = [(1, 200), (3, 5), (7, 9), (1024, 17), (600004, 2)]
    cast = [(16, 64, 1), (48, 192, 3)]
    jobs, checks = [], []
    for i, (n, splits) in enumerate(plain):
        raw, src = make_slabs(splits, n, seed=10 + i)
        if n < 4:   # lane-strided wave sums are not sequential: positive terms (loss partials), no cancellation
            src.abs_().add_(0.5)
        dst = torch.full((n + 64,), float("nan"), device=DEV)
        jobs.append(dict(src=src.data_ptr(), splits=splits, n=n, dst=dst.data_ptr()))
        checks.append((n, src, dst, raw))
    cbufs = []
    for i, (R, C, splits) in enumerate(cast):
        raw, src = make_slabs(splits, R * C, seed=20 + i)
        dst = torch.full((R * C + 64,), float("nan"), device=DEV)
        bf, bT = sent16(R * C), sent16(R * C)
        jobs.append(dict(src=src.data_ptr(), splits=splits, R=R, C=C, dst=dst.data_ptr(), bf=bf.data_ptr(), bfT=bT.data_ptr()))
        cbufs.append((R, C, src, dst, bf, bT))
    bump = torch.tensor([41, -9], dtype=torch.int32, device=DEV)

    def verify():
        torch.cuda.synchronize()
        for n, src, dst, raw in checks:
            assert bool((bits(dst)[n:] == NAN_BITS).all()), f"n={n}: wrote past the end"
            if n < 4:   # <= 6 wave-sum levels + 4 strided adds of positive terms: 10 * 2^-24 < 1e-6
                ref = src.double().sum(0)
                assert bool(((dst[:n].double() - ref).abs() <= 1e-6 * ref.abs()).all()), f"n={n}"
            else:       # float4 body and tail: sequential from slab 0, bitwise
                assert torch.equal(dst[:n], seq_sum(src)), f"n={n}"
        for R, C, src, dst, bf, bT in cbufs:
            ref = seq_sum(src)
            assert torch.equal(dst[:R * C], ref) and bool((bits(dst)[R * C:] == NAN_BITS).all())
            assert_bf16(bf, ref.view(R, C).bfloat16(), f"bf {R}x{C}")
            assert_bf16(bT, ref.view(R, C).bfloat16().T.contiguous(), f"bfT {R}x{C}")

    ext.reduce_slabs_multi(jobs, bump.data_ptr(), S())
    verify()
    assert bump.tolist() == [42, -9]
    for _, _, dst, _ in checks:
        dst.fill_(float("nan"))
    ext.reduce_slabs_multi(jobs, 0, S())
    verify()
    assert bump.tolist() == [42, -9]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256])
def test_sum_partials(ext, n):
    """One wave, lane-strided then a wave sum: against fp64 (positive terms: <= 4 + 6 roundings,
    10 * 2^-24 < 1e-6), bump once per launch or not at all, bitwise the same on a second launch."""
    g = torch.Generator().manual_seed(n)
    parts = torch.full((n + 64,), float("nan"))
    parts[:n] = torch.rand(n, generator=g) * 5 + 0.1
    parts = parts.to(DEV)
    out = torch.full((2,), float("nan"), device=DEV)
    bump = torch.tensor([6, -9], dtype=torch.int32, device=DEV)
    ext.sum_partials(parts.data_ptr(), n, out.data_ptr(), bump.data_ptr(), S())
    torch.cuda.synchronize()
    first = out.clone()
    ref = float(parts[:n].double().sum())
    assert abs(float(out[0]) - ref) <= 1e-6 * ref and int(bits(out)[1]) == NAN_BITS
    assert bump.tolist() == [7, -9]
    out.fill_(float("nan"))
    ext.sum_partials(parts.data_ptr(), n, out.data_ptr(), 0, S())
    torch.cuda.synchronize()
    assert same_bits(out, first) and bump.tolist() == [7, -9]


# ------------------------------------------------------------------ 8. the bias pack of the sharded optimiser
def test_flat_pack_u32_two_ranks(ext):
    """pack on two emulated ranks ([lo, hi) cut inside the second range), integer-add the packs (the
    all-reduce), unpack below `tail` (inside the third range): bit-exact, specials included."""
    ranges = [(1024, 768), (4096, 768), (8192, 256)]
    total = sum(n for _, n in ranges)
    N = 8192 + 256 + 64
    g = torch.Generator().manual_seed(8)
    src = torch.full((N,), float("nan"))
    idx = torch.cat([torch.arange(o, o + n) for o, n in ranges])
    src[idx] = torch.randn(total, generator=g)
    sb = src.view(torch.int32)
    for o, n in ranges:   # -0.0, a denormal, inf, a NaN with a payload, in every range
        sb[o + 1], sb[o + 5], sb[o + n - 2], sb[o + n - 1] = -0x80000000, 0x00000123, 0x7F800000, 0x7FC12345
    src = src.to(DEV)
    before = src.clone()
    cut, tail = 4096 + 384, 8192 + 128
    packs = []
    for lo, hi in ((0, cut), (cut, tail)):
        pack = torch.full((total + 64,), 0x0BADBEEF, dtype=torch.int32, device=DEV)
        ext.flat_pack_u32(src.data_ptr(), pack.data_ptr(), ranges, lo, hi, tail, 0, S())
        torch.cuda.synchronize()
        own = ((idx >= lo) & (idx < hi)).to(DEV)
        want = torch.where(own, bits(src)[idx.to(DEV)], torch.zeros(total, dtype=torch.int32, device=DEV))
        assert torch.equal(pack[:total], want) and bool((pack[total:] == 0x0BADBEEF).all())
        packs.append(pack)
    assert same_bits(src, before)   # packing reads only
    summed = packs[0].clone()
    summed[:total] += packs[1][:total]
    dst = torch.full((N,), 0x7FC00BAD, dtype=torch.int32, device=DEV)
    ext.flat_pack_u32(dst.data_ptr(), summed.data_ptr(), ranges, 0, 0, tail, 1, S())
    torch.cuda.synchronize()
    inr = torch.zeros(N, dtype=torch.bool)
    inr[idx] = True
    wrote = (inr & (torch.arange(N) < tail)).to(DEV)
    assert torch.equal(dst[wrote], bits(src)[wrote])
    assert bool((dst[~wrote] == 0x7FC00BAD).all())


def test_optimiser_bindings_reject_bad_shapes(ext):
    """Every raw optimiser binding throws on a shape its kernel cannot take (nothing is launched)."""
    fl = Flat([(0, 64 * 64 + 64)], seed=0)
    o = fl.opt(hyper(), 1)
    bad = [dict(off=2, R=0, C=64), dict(off=0, R=32, C=64), dict(off=0, R=64, C=96), dict(off=0, R=0, C=6),
           dict(off=128, R=64, C=64), dict(off=0, R=0, C=64, gsl=fl.g.data_ptr(), nsl=0)]
    for job in bad:
        with pytest.raises(RuntimeError, match="adam_cast_multi"):
            ext.adam_cast_multi(o, [job], S())
    with pytest.raises(RuntimeError, match="at most 32"):
        ext.adam_cast_multi(o, [dict(off=0, R=0, C=4)] * 33, S())
    with pytest.raises(RuntimeError, match="m and v"):
        ext.adam_step(fl.opt(hyper(), 1, null_mv=True), S())
    with pytest.raises(RuntimeError, match="at most 24"):
        ext.reduce_slabs_multi([dict(src=fl.g.data_ptr(), splits=1, n=4, dst=fl.p.data_ptr())] * 25, 0, S())
    with pytest.raises(RuntimeError, match="R % 16"):
        ext.reduce_slabs_multi([dict(src=fl.g.data_ptr(), splits=1, R=8, C=64, bf=fl.p.data_ptr())], 0, S())
    with pytest.raises(RuntimeError, match="at most 16"):
        ext.flat_pack_u32(fl.p.data_ptr(), fl.g.data_ptr(), [(0, 4)] * 17, 0, 4, 4, 0, S())
    with pytest.raises(RuntimeError, match="nparts"):
        ext.grad_clip_scale(dict(x=fl.g.data_ptr(), n=4, parts=fl.p.data_ptr(), nparts=0, clip=1.0, scale=fl.m.data_ptr()), S())


# ------------------------------------------------------------------ 9. the trainer's optimiser
def _trainer_cfg(layers, hidden=128, **kw):
    return GRUConfig(vocab=256, embed=64, hidden=hidden, layers=layers, batch=32, seq=4, seed=21, keep_grads=True, **kw)


def _batches(cfg, n=3):
    from gru_mpi_cuda_amd.utils.data import NameStream
    ds = NameStream(cfg.batch, cfg.seq, seed=4)
    return [ds.next() for _ in range(n)]


def _first_norm(cfg):
    """The first step's gradient norm, measured by a trainer whose clip (1e-3) is far below it."""
    from gru_mpi_cuda_amd.engine.trainer import HipTrainer
    from gru_mpi_cuda_amd.models.params import init_params
    tr = HipTrainer(cfg.replace(clip_norm=1e-3), params=init_params(cfg))
    tr.step(*_batches(cfg, 1)[0])
    torch.cuda.synchronize()
    N = tr.t.read_grad_norm()
    assert np.isfinite(N) and N > 1e-2
    return N


@pytest.fixture(scope="module")
def first_norm():
    cache = {}

    def get(cfg):
        key = (cfg.layers, cfg.embed, cfg.hidden)
        if key not in cache:
            cache[key] = _first_norm(cfg)
        return cache[key]
    return get


def _hp_of(cfg):
    hp = dict(lr=f32(cfg.lr), b1=f32(cfg.beta1), b2=f32(cfg.beta2), eps=f32(cfg.eps), wd=f32(cfg.weight_decay),
              sgd=int(cfg.optimizer == "sgd"))
    hp.update(SCHEDS["const"])
    return hp


def _run_steps(tr, batches, path, clip, tag):
    """Three steps; each against fp64 Adam on the device's own pre-step p, m, v and its gradient."""
    hp = _hp_of(tr.cfg)
    for i, (x, y) in enumerate(batches):
        p0, m0, v0 = tr.params.clone(), tr.m.clone(), tr.v.clone()
        if path == "step":
            tr.step(x, y)
        else:
            tr.forward_backward(x, y)
            tr.optimizer_step()
        torch.cuda.synchronize()
        t = tr.t.get_step()
        assert t == i + 1
        g = tr.grads.clone()
        sc = sc64 = 1.0
        if clip:
            norm64 = float(g.double().norm())
            sc64 = min(1.0, f32(clip) / (norm64 + 1e-6))
            got = np.float32(tr.t.read_grad_norm())
            print(f"[optim] {tag} step {t}: device norm rel err {abs(float(got) - norm64) / norm64:.3g}")
            assert abs(float(got) - norm64) <= 1e-5 * norm64, f"{tag}: device norm {got} vs {norm64}"
            # The per-element reference multiplies by the scale the device used: clip_final_kernel's
            # expression on the device's own norm word, in fp32 (bit-exact: + and / round correctly).
            # With the scale from the fp64 norm instead, m missed its bound on 40 % of the elements of
            # the two-layer clipped runs (step 1: worst err / tol 1.39, v 0.71): the device norm was off
            # by 1.9e-7 relative there (fp32 sums; up to 3.5e-7 over all the runs here, held to 1e-5
            # above), a common factor on every g * sc, and the m bound (2^-22 = 2.4e-7 of the terms)
            # has no room for it -- it is derived for a scale that is an exact input of the step.
            # With the device's scale the worst m err / tol over all the trainer runs is 0.48.
            sc = float(min(np.float32(1), np.float32(clip) / (got + np.float32(1e-6))))
            assert abs(sc - sc64) <= 1e-5 * sc64
        check_update(tr.params, tr.m, tr.v, p0, g, m0, v0, t, hp, sc, f"{tag} step {t}")
        if hp["sgd"]:
            assert same_bits(tr.m, m0) and same_bits(tr.v, v0)
        yield sc64


@pytest.mark.parametrize("path", ["step", "phased"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("opt", ["adam", "sgd"])
@pytest.mark.parametrize("layers", [1, 2])
def test_trainer_optimiser_matches_fp64(first_norm, layers, opt, clip, wd, path):
    """HipTrainer's optimiser -- the one-graph step() and forward_backward() + optimizer_step() -- per
    element, every tensor, three steps; the clip is half the first step's norm, so it bites (the scale
    from the fp64 norm is < 1 on every step).  The device norm is held to the fp64 norm at 1e-5; the
    per-element reference then uses the scale the device derived from its own norm (see _run_steps).
    At this shape every configuration runs the per-step plan (printed)."""
    from gru_mpi_cuda_amd.engine.trainer import HipTrainer
    from gru_mpi_cuda_amd.models.params import init_params
    cfg = _trainer_cfg(layers, optimizer=opt, weight_decay=wd)
    c = first_norm(cfg) / 2 if clip else 0.0
    cfg = cfg.replace(clip_norm=c)
    tr = HipTrainer(cfg, params=init_params(cfg))
    tag = f"trainer L={layers} {opt} clip={c:.4g} wd={wd} {path}"
    print(f"[optim] {tag}: plan {tr.t.plan()}")
    for sc in _run_steps(tr, _batches(cfg), path, c, tag):
        assert (sc < 1.0) if clip else (sc == 1.0)


@pytest.mark.parametrize("path", ["step", "phased"])
@pytest.mark.parametrize("layers", [1, 2])
def test_trainer_optimiser_persistent_plan(first_norm, layers, path):
    """The same at hidden = 256, where the trainer plans the persistent sequence kernels (the clipped
    one-graph step reduces every slab before the norm instead of inside the Adam launch)."""
    from gru_mpi_cuda_amd.engine.trainer import HipTrainer
    from gru_mpi_cuda_amd.models.params import init_params
    cfg = _trainer_cfg(layers, hidden=256, weight_decay=0.01)
    cfg = cfg.replace(clip_norm=first_norm(cfg) / 2)
    tr = HipTrainer(cfg, params=init_params(cfg))
    tag = f"trainer L={layers} H=256 adam clip={cfg.clip_norm:.4g} wd=0.01 {path}"
    print(f"[optim] {tag}: plan {tr.t.plan()}")
    assert tr.t.uses_persistent(), tr.t.plan()
    for sc in _run_steps(tr, _batches(cfg), path, cfg.clip_norm, tag):
        assert sc < 1.0


@pytest.mark.parametrize("layers", [1, 2])
def test_trainer_inactive_clip_is_bitwise_no_clip(layers):
    """clip_norm = 1e6: the scale is exactly 1, the weights bitwise those of the run without clipping."""
    from gru_mpi_cuda_amd.engine.trainer import HipTrainer
    from gru_mpi_cuda_amd.models.params import init_params
    cfg = _trainer_cfg(layers, weight_decay=0.01)
    a = HipTrainer(cfg, params=init_params(cfg))
    b = HipTrainer(cfg.replace(clip_norm=1e6), params=init_params(cfg))
    for x, y in _batches(cfg):
        a.step(x, y)
    for sc in _run_steps(b, _batches(cfg), "step", 1e6, f"trainer L={layers} clip=1e6"):
        assert sc == 1.0
    torch.cuda.synchronize()
    for name in ("params", "m", "v"):
        assert same_bits(getattr(a, name), getattr(b, name)), name


def test_trainer_padded_entries_stay_put(first_norm):
    """embed = 40, hidden = 96 run zero-padded to (64, 128): after three clipped steps with weight
    decay every padded entry of params, m and v is bitwise where it started (zero stays zero)."""
    from gru_mpi_cuda_amd.engine.trainer import HipTrainer
    from gru_mpi_cuda_amd.models.params import init_params, pad_params, to_flat
    cfg = GRUConfig(vocab=256, embed=40, hidden=96, layers=1, batch=32, seq=4, seed=21, keep_grads=True,
                    weight_decay=0.01)
    cfg = cfg.replace(clip_norm=first_norm(cfg) / 2)
    tr = HipTrainer(cfg, params=init_params(cfg))
    assert tr.padded
    ones = {k: torch.ones_like(v) for k, v in init_params(cfg).items()}
    pad = (to_flat(tr.icfg, pad_params(ones, cfg, tr.icfg, masked_bias=False)) == 0).to(DEV)   # padding + alignment gaps
    assert 0 < int(pad.sum()) < pad.numel()
    start = [t.clone() for t in (tr.params, tr.m, tr.v)]
    assert all(bool((s[pad] == 0).all()) for s in start)
    for sc in _run_steps(tr, _batches(cfg), "step", cfg.clip_norm, "trainer padded"):
        assert sc < 1.0
    for name, now, was in zip(("params", "m", "v"), (tr.params, tr.m, tr.v), start):
        assert torch.equal(bits(now)[pad], bits(was)[pad]), f"padded entries of {name} moved"
        assert not same_bits(now, was)

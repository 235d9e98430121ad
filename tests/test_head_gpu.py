"""Per-element tests of the FC / softmax-xent head against the float64 reference of
models/head_ref.py: fc_xent (generic kernel, eight-wave V = 256 kernel, fc_xent_fl), softmax_xent,
the FC consumers of gru_fwd_seq_fc and fc_sample (both kernels), each launched on its own through
the raw bindings.

Every output starts as NaN (dl^T: a sentinel, so the columns outside its window show a stray write),
every launch runs twice and must repeat bit for bit, and every tolerance is imported from head_ref
(measured there on the CPU as emulator - reference; tests/test_head_ref.py).  Inputs: the planted set
(head_ref.planted_inputs: labels and row maxima in every slab, +-100 rows, spikes, chunk maxima
that rise, fall and jump, one fully ignored 32-row block) and one random seed, M = 64.  The float64
reference runs once per input set on the CPU and is shared by the cases that use it.  Each
comparison prints its err / tol before it asserts.

Kernel -> cases:
  fc_xent_kernel<1>            (64, 32) one wave; (128, 96) two waves, fc_dh_tile<1> only
  fc_xent_kernel<2>            (256, 64); (256, 320) tiles <4> + <1>; (512, 128) eight waves, 76.5 KB of LDS
  fc_xent_kernel<4>            (256, 256)
  fc_xent_v256_kernel<H, DH>   H in (512, 1024) x DH in (true, false)
  fc_xent_fl_kernel            H = 512 with fc_flash = 1
  softmax_xent_kernel          V = 256 fast path; V in (64, 128, 320, 512) general path
  gru_fwd_seq_kernel<4, 2, true>  T in (3, 33) x allow_local in (1, 0)
  fc_sample_kernel<1>          (64, 32)
  fc_sample_kernel<2>          (256, 128); (512, 64) 68 KB of LDS
  fc_sample_v256_kernel<H>     H in (512, 1024)
"""
import functools

import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.models import head_ref as hr
from gru_mpi_cuda_amd.models import seq_ref as sr

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")
M = hr.M_ROWS
LDT, COLT = M + 16, 8
SENTINEL = 12352.0     # exact in bf16


def S():
    return torch.cuda.current_stream().cuda_stream


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def close(got, ref, family, what, inv=1.0):
    """Print the figure, then assert it (normalised by inv)."""
    print(f"HEAD {family:8s} err/tol {hr.err_over_tol(got, ref, family, inv):9.3e}  {what}")
    m = hr.mismatch(got, ref, family, inv)
    assert m is None, f"{what}: {m}"


def gemm_close(got, A, B, depth, what, family="dy_gemm"):
    print(f"HEAD {family:8s} err/tol {hr.gemm_err_over_bound(got, A, B, depth):9.3e}  {what}")
    m = hr.gemm_mismatch(got, A, B, depth)
    assert m is None, f"{what}: {m}"


@pytest.fixture
def variants(ext):
    saved = ext.step_lds_variants()
    yield ext
    ext.set_step_lds_variants(saved)


@functools.lru_cache(maxsize=None)
def _case(kind, V, H, wscale=1.0):
    """(inputs, float64 reference) of one input set, on the CPU; shared and never modified."""
    d = hr.inputs(kind, V, H, seed=0, wscale=wscale)
    return d, hr.head_ref(d["X"], d["W"], d["b"], d["labels"], d["inv"])


# ====================================================================================== fc_xent
def _launch_xent(ext, d, V, H, want_dl, want_dy, ft):
    from gru_mpi_cuda_amd.ops import ft_layout
    X, W = d["X"].to(DEV, BF).contiguous(), d["W"].to(DEV, BF).contiguous()
    b, y, inv = d["b"].to(DEV), d["labels"].to(DEV), d["inv"].reshape(1).to(DEV)
    WT = W.T.contiguous()
    keep = [X, W, b, y, inv, WT]
    o = dict(dlT=torch.full((V, LDT), SENTINEL, device=DEV, dtype=BF), lp=nans(M // 32))
    a = dict(X=X.data_ptr(), W=W.data_ptr(), b=b.data_ptr(), labels=y.data_ptr(), inv_count=inv.data_ptr(),
             dlT=o["dlT"].data_ptr(), loss_part=o["lp"].data_ptr(), M=M, H=H, V=V, ldT=LDT, colT=COLT)
    if want_dl:
        o["dl"] = nans(M, V, dtype=BF)
        a["dl"] = o["dl"].data_ptr()
    if want_dy:
        o["dy"] = nans(M, H)
        a.update(dy=o["dy"].data_ptr(), WT=WT.data_ptr())
    if ft:
        Wf, WTf = ft_layout(W), ft_layout(WT)
        keep += [Wf, WTf]
        a.update(Wf=Wf.data_ptr(), WTf=WTf.data_ptr())
    ext.fc_xent(a, S())
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


def _check_head(o, o2, d, ref, what, flash=False):
    """The common checks of one head launch: o, o2 = two launches' outputs (dlT, lp and dl / dy where
    asked for), d / ref = inputs and float64 reference."""
    inv, lab = float(d["inv"]), d["labels"]
    V = d["W"].shape[0] if d.get("W") is not None else ref["dl"].shape[1]
    for k in o:
        assert same_bits(o[k], o2[k]), f"{what}: {k} differs between two launches"
    # dl^T: the window, and nothing outside it
    fill = torch.full((V, LDT), SENTINEL, dtype=BF)
    assert same_bits(o["dlT"][:, :COLT], fill[:, :COLT]) and same_bits(o["dlT"][:, COLT + M:], fill[:, COLT + M:]), \
        f"{what}: dl^T written outside its window"
    dlT = hr.dlt_decode(o["dlT"], M, COLT)
    close(dlT, ref["dl"], "dl", what + " dlT", inv)
    if "dl" in o:
        assert same_bits(dlT.contiguous(), o["dl"]), f"{what}: dl^T differs from dl"
        close(o["dl"], ref["dl"], "dl", what + " dl", inv)
    ign = lab < 0
    assert not bool(dlT[ign].float().abs().any()), f"{what}: dl of an ignored row is not exactly 0"
    close(o["lp"], ref["loss_part"], "loss", what + " loss_part", inv)
    blocks = ign.reshape(-1, 32).all(1)
    assert bool((o["lp"][blocks] == 0).all()), f"{what}: the loss partial of an all-ignored block is not exactly 0"
    if "dy" in o:
        assert not bool(torch.isnan(o["dy"]).any()), f"{what}: dy not fully written"
        assert bool((o["dy"][ign] == 0).all()), f"{what}: dy of an ignored row is not exactly 0"
        c0 = d["dy_from"]
        close(o["dy"][:, c0:], ref["dy"][:, c0:], "dy_flash" if flash else "dy", what + " dy end to end", inv)
        if not flash:   # the product alone: the kernel's own bf16 dl times W
            gemm_close(o["dy"], dlT.float(), d["W"], V, what + " dy = dl . W")


XENT_CASES = [(V, H, mode) for V, H in hr.XENT_SHAPES for mode in ("dl", "dy") if mode == "dl" or V % 128 == 0]


@pytest.mark.parametrize("kind", ["planted", "random"])
@pytest.mark.parametrize("V,H,mode", XENT_CASES)
def test_fc_xent_generic(ext, V, H, mode, kind):
    """fc_xent_kernel<KB> without the FT copies: row-major dl ("dl"), or the fused dy = dl . W_fc and no
    row-major dl ("dy", where fc_xent allows it: V % 128 == 0 and H % (V / 4) == 0)."""
    d, ref = _case(kind, V, H)
    run = lambda: _launch_xent(ext, d, V, H, want_dl=mode == "dl", want_dy=mode == "dy", ft=False)
    _check_head(run(), run(), d, ref, f"fc_xent V={V} H={H} {mode} {kind}")


def test_fc_xent_generic_refuses_fused_dy_at_v64(ext):
    d, _ = _case("random", 64, 32)
    with pytest.raises(RuntimeError, match="fused dH"):
        _launch_xent(ext, d, 64, 32, want_dl=False, want_dy=True, ft=False)


@pytest.mark.parametrize("kind", ["planted", "random"])
@pytest.mark.parametrize("dh", [True, False])
@pytest.mark.parametrize("H", hr.V256_H)
def test_fc_xent_v256(variants, H, dh, kind):
    """The eight-wave V = 256 kernel on the FT copies: DH = true (dy, no row-major dl) and DH = false (dl only)."""
    variants.set_step_lds_variants(dict(fc_flash=0))
    d, ref = _case(kind, 256, H)
    run = lambda: _launch_xent(variants, d, 256, H, want_dl=not dh, want_dy=dh, ft=True)
    _check_head(run(), run(), d, ref, f"fc_xent_v256 H={H} DH={int(dh)} {kind}")


@pytest.mark.parametrize("kind", ["planted", "random"])
def test_fc_xent_flash(variants, kind):
    """fc_xent_fl (fc_flash = 1, H = 512): online softmax over four chunks; dy held to the flash bound."""
    V, H = hr.FLASH_SHAPE
    variants.set_step_lds_variants(dict(fc_flash=1))
    d, ref = _case(kind, V, H)
    run = lambda: _launch_xent(variants, d, V, H, want_dl=False, want_dy=True, ft=True)
    _check_head(run(), run(), d, ref, f"fc_xent_fl {kind}", flash=True)


# ====================================================================================== softmax_xent
@functools.lru_cache(maxsize=None)
def _softmax_case(kind, V):
    d = dict(hr.inputs(kind, V, hr.SOFTMAX_H, seed=0))
    lg = hr.emulate(d["X"], d["W"], d["b"], d["labels"], d["inv"])["logits"].contiguous()   # fp32
    ref = hr.head_ref(None, None, None, d["labels"], d["inv"], logits=lg)
    d["W"] = None
    return d, lg, ref


def _launch_softmax(ext, lg, d, V, want_dl, ldT=LDT, colT=COLT):
    L, y, inv = lg.to(DEV), d["labels"].to(DEV), d["inv"].reshape(1).to(DEV)
    o = dict(dlT=torch.full((V, LDT), SENTINEL, device=DEV, dtype=BF), lp=nans(M // 32))
    a = dict(labels=y.data_ptr(), inv_count=inv.data_ptr(), dlT=o["dlT"].data_ptr(), loss_part=o["lp"].data_ptr(),
             M=M, V=V, ldT=ldT, colT=colT)
    if want_dl:
        o["dl"] = nans(M, V, dtype=BF)
        a["dl"] = o["dl"].data_ptr()
    ext.softmax_xent(L.data_ptr(), a, S())
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


@pytest.mark.parametrize("kind", ["planted", "random"])
@pytest.mark.parametrize("want_dl", [1, 0])
@pytest.mark.parametrize("V", hr.SOFTMAX_V)
def test_softmax_xent(ext, V, want_dl, kind):
    """softmax_xent on fp32 logits (the head of the large-H plans): V = 256 takes the four-per-lane fast
    path, the rest the general per = V / 64 path (V = 320: per = 5).  Reference: float64 on the same logits."""
    d, lg, ref = _softmax_case(kind, V)
    run = lambda: _launch_softmax(ext, lg, d, V, bool(want_dl))
    _check_head(run(), run(), d, ref, f"softmax_xent V={V} dl={want_dl} {kind}")


@pytest.mark.parametrize("V,ldT,colT", [(96, LDT, COLT), (576, LDT, COLT), (256, LDT + 4, COLT), (256, LDT, COLT + 4),
                                        (256, M, COLT)])
def test_softmax_xent_refuses_what_it_does_not_serve(ext, V, ldT, colT):
    d, lg, _ = _softmax_case("random", 256)
    with pytest.raises(RuntimeError, match="softmax_xent"):
        _launch_softmax(ext, lg, d, V, True, ldT=ldT, colT=colT)


# ====================================================================================== gru_fwd_seq_fc
def _seq_fc_inputs(T):
    H, V, Bp = hr.SEQ_FC["H"], hr.SEQ_FC["V"], hr.SEQ_FC["Bp"]
    inp = sr.fwd_inputs(H, Bp, T, seed=0, V=V)
    hd = hr.random_inputs(V, H, M=T * Bp, seed=0)
    lab = hd["labels"].clone()
    lab[Bp + 32:Bp + 64] = -1                       # step 1, row block 1: fully ignored
    inv = torch.tensor(1.0 / int((lab >= 0).sum()), dtype=torch.float32)
    return inp, hd["W"], hd["b"], lab, inv


@pytest.mark.parametrize("T,local", [(3, 1), (3, 0), (33, 1), (33, 0)])
def test_fwd_seq_fc(ext, T, local):
    """The FC consumers inside the persistent forward: T = 3 leaves most of the 32 consumers per row
    block without an item, T = 33 gives consumer 0 two.  The recurrence has its own tests, so the head is
    referenced from the kernel's own HSb bits; HSb / HSf must equal the plain gru_fwd_seq's."""
    from gru_mpi_cuda_amd.ops import ft_layout
    H, V, Bp = hr.SEQ_FC["H"], hr.SEQ_FC["V"], hr.SEQ_FC["Bp"]
    if not ext.fwd_seq_fc_supported(H, Bp, V):
        print(f"HEAD gru_fwd_seq_fc T={T}: NOT RUN (shape not co-resident)")
        pytest.skip("gru_fwd_seq_fc: shape not co-resident")
    inp, W, b, lab, inv = _seq_fc_inputs(T)
    nrb, Mt = Bp // 32, T * Bp
    g = {k: v.to(DEV) for k, v in inp.items()}
    Whh = g["Whh"].to(BF).contiguous()
    Wb = W.to(DEV, BF).contiguous()
    Wf, WTf = ft_layout(Wb), ft_layout(Wb.T.contiguous())
    bd, yd, invd = b.to(DEV), lab.to(DEV), inv.reshape(1).to(DEV)
    h0b = g["h0"].to(BF)

    def launch(fc):
        o = dict(HSb=nans(T + 1, Bp, H, dtype=BF), HSf=nans(T + 1, Bp, H), HF=nans(T + 1, Bp * H, dtype=BF),
                 xch=nans(T, Bp * H, dtype=BF))
        o["HSb"][0], o["HSf"][0], o["HF"][0] = h0b, g["h0"], sr.hf_encode(h0b[None])
        sv = [nans(T, Bp, H) for _ in range(4)]
        cnt = torch.zeros(ext.seq_flag_words(H, Bp), device=DEV, dtype=torch.int32)
        err = torch.zeros(16, device=DEV, dtype=torch.int32)
        a = dict(HSb=o["HSb"].data_ptr(), HSf=o["HSf"].data_ptr(), HF=o["HF"].data_ptr(), xch=o["xch"].data_ptr(),
                 sr=sv[0].data_ptr(), sz=sv[1].data_ptr(), sn=sv[2].data_ptr(), sghn=sv[3].data_ptr(),
                 Whh=Whh.data_ptr(), bhh=g["bhh"].data_ptr(), P=g["P"].data_ptr(), ids=g["ids"].data_ptr(),
                 h0=g["h0"].data_ptr(), cnt=cnt.data_ptr(), err=err.data_ptr(), allow_local=local, T=T, Bp=Bp, H=H)
        if fc:
            f = dict(dy=nans(Mt, H), dlF=nans(Mt * V, dtype=BF), lp=nans(Mt // 32), dW=nans(nrb, V, H), db=nans(nrb, V))
            ext.fwd_seq_fc(a, dict(Wf=Wf.data_ptr(), WTf=WTf.data_ptr(), b=bd.data_ptr(), labels=yd.data_ptr(),
                                   inv_count=invd.data_ptr(), dy=f["dy"].data_ptr(), dlF=f["dlF"].data_ptr(),
                                   loss_part=f["lp"].data_ptr(), dW=f["dW"].data_ptr(), db=f["db"].data_ptr(), V=V), S())
            o.update(f)
        else:
            ext.fwd_seq(a, S())
        torch.cuda.synchronize()
        assert int(err[0]) == 0, "a cross-workgroup wait hit its spin limit"
        return {k: v.cpu() for k, v in o.items()}

    o, o2, plain = launch(True), launch(True), launch(False)
    what = f"fwd_seq_fc T={T} local={local}"
    print(f"HEAD gru_fwd_seq_fc T={T} local={local}: RAN")
    for k in o:
        if k != "xch":
            assert same_bits(o[k], o2[k]), f"{what}: {k} differs between two launches"
    for k in ("HSb", "HSf", "HF"):
        assert same_bits(o[k], plain[k]), f"{what}: {k} differs from the plain gru_fwd_seq"
    assert same_bits(sr.hf_decode(o["HF"], T + 1, Bp, H)[1:], o["HSb"][1:]), "HF differs from HSb"
    X = o["HSb"][1:].reshape(Mt, H).float()                     # the kernel's own h_t bits
    ref = hr.head_ref(X, W, b, lab, inv, T=T, Bp=Bp)
    invf = float(inv)
    for k in ("dy", "dlF", "lp", "dW", "db"):
        assert not bool(torch.isnan(o[k].float()).any()), f"{what}: {k} not fully written"
    dl = hr.dlf_decode(o["dlF"], T, Bp, V).reshape(Mt, V)
    close(dl, ref["dl"], "dl", what + " dlF", invf)
    ign = lab < 0
    assert not bool(dl[ign].float().abs().any()) and bool((o["dy"][ign] == 0).all()), f"{what}: ignored rows not exactly 0"
    close(o["lp"], ref["loss_part"], "loss", what + " loss_part", invf)
    blocks = ign.reshape(-1, 32).all(1)
    assert int(blocks.sum()) == 1 and bool((o["lp"][blocks] == 0).all()), f"{what}: all-ignored block's loss partial"
    close(o["dy"], ref["dy"], "dy", what + " dy end to end", invf)
    gemm_close(o["dy"], dl.float(), W, V, what + " dy = dl . W")
    # dW / db per row block from the kernel's own dlF and HSb bits: sums of 32 T exact products
    d4 = dl.float().reshape(T, nrb, 32, V).permute(1, 0, 2, 3).reshape(nrb, T * 32, V)
    x4 = X.reshape(T, nrb, 32, H).permute(1, 0, 2, 3).reshape(nrb, T * 32, H)
    for rb in range(nrb):
        gemm_close(o["dW"][rb], d4[rb].T, x4[rb], 32 * T, f"{what} dW[{rb}]", "dW")
        gemm_close(o["db"][rb][:, None], d4[rb].T, torch.ones(32 * T, 1), 32 * T, f"{what} db[{rb}]", "db")


# ====================================================================================== fc_sample
N_LIVE, ML, STEP = 50, 6, 2


@pytest.mark.parametrize("kind", ["planted", "random"])
@pytest.mark.parametrize("V,H", hr.SAMPLE_SHAPES)
def test_fc_sample_exact(ext, V, H, kind):
    """probs against float64, and -- the uniforms moved 1e-5 off the float64 CDF edges -- every row's
    index equal to the float64 inverse-CDF choice, no allowance.  Row 7 draws 1.5 (above the fp32 total:
    V - 1), row 3 is dead, the EOS is row 5's choice, rows >= N are padding."""
    from gru_mpi_cuda_amd.ops import ft_layout
    d, ref = _case(kind, V, H, 3.0)
    p64 = ref["probs"].numpy()
    rng = np.random.RandomState(V + H)
    r = rng.rand(N_LIVE).astype(np.float32)
    r[7] = 1.5
    r, want = hr.clear_uniforms(p64[:N_LIVE], r)
    assert want[7] == V - 1
    eos = int(want[5])
    X, W, b = d["X"].to(DEV, BF).contiguous(), d["W"].to(DEV, BF).contiguous(), d["b"].to(DEV)
    rf = np.full((N_LIVE, ML), 0.5, np.float32)
    rf[:, STEP] = r
    rf = torch.from_numpy(rf).to(DEV)
    keep = [X, W, b, rf]

    def launch():
        ids = torch.full((M,), -1, device=DEV, dtype=torch.int32)
        alive = torch.ones(M, device=DEV, dtype=torch.int32)
        alive[3] = 0
        out = torch.full((M, ML + 1), 7, device=DEV, dtype=torch.uint8)   # N rows are the kernel's; the rest must stay
        probs = nans(M, V)
        a = dict(X=X.data_ptr(), W=W.data_ptr(), b=b.data_ptr(), rf=rf.data_ptr(), ids=ids.data_ptr(), out=out.data_ptr(),
                 alive=alive.data_ptr(), probs=probs.data_ptr(), N=N_LIVE, Bp=M, H=H, V=V, step=STEP, max_len=ML, eos=eos)
        if H >= 512:
            Wf = ft_layout(W)
            keep.append(Wf)
            a["Wf"] = Wf.data_ptr()
        ext.fc_sample(a, S())
        torch.cuda.synchronize()
        return dict(ids=ids.cpu(), alive=alive.cpu(), out=out.cpu(), probs=probs.cpu())

    o, o2 = launch(), launch()
    what = f"fc_sample V={V} H={H} {kind}"
    for k in o:
        assert same_bits(o[k], o2[k]), f"{what}: {k} differs between two launches"
    close(o["probs"], ref["probs"], "probs", what + " probs")
    want_t = torch.from_numpy(np.asarray(want)).int()
    got = o["ids"][:N_LIVE]
    bad = (got != want_t).nonzero().flatten().tolist()
    assert not bad, f"{what}: rows {bad} chose {got[bad].tolist()}, the float64 CDF chooses {want_t[bad].tolist()}"
    assert bool((o["ids"][N_LIVE:] == -1).all()), f"{what}: padding rows wrote ids"
    live = torch.ones(N_LIVE, dtype=torch.bool)
    live[3] = False
    exp_out = torch.full((M, ML + 1), 7, dtype=torch.uint8)
    exp_out[:N_LIVE][live, STEP] = want_t[live].to(torch.uint8)
    assert torch.equal(o["out"], exp_out), f"{what}: out (a dead row, another step or a padding row written)"
    exp_alive = torch.ones(M, dtype=torch.int32)
    exp_alive[:N_LIVE][want_t == eos] = 0
    exp_alive[3] = 0
    assert int(exp_alive[5]) == 0 and torch.equal(o["alive"], exp_alive), f"{what}: alive"

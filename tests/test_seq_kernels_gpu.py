"""Per-element tests of the persistent sequence kernels against the float64 reference of
models/seq_ref.py: gru_fwd_seq, gru_bwd_seq (all eight variants), gru_bwd_seq16 and gru_bwd_seq_big,
each launched on its own through the raw bindings.

Every output buffer starts as NaN (what the kernel does not write stays visible), the flag blocks
start as zero, the error word must read 0, and every tolerance is imported from seq_ref (measured
there on the CPU as the emulator-vs-reference deviation; tests/test_seq_ref.py).  The float64
reference runs in torch on the device, once per (shape, T, inputs) and shared by the cases that
use it.

Kernel variant -> cases (the dispatch tables of gru_seq.hip, gru_seq16.hip, gru_seq_big.hip):
  gru_fwd_seq_kernel<1, 2>   H = 256           FWD_CASES with H = 256 (Bp = 64, 96)
  gru_fwd_seq_kernel<2, 2>   H = 512           FWD_CASES with H = 512 (Bp = 64; Bp = 256: row-block-fast map)
  gru_fwd_seq_kernel<8, 1>   H = 1024          FWD_CASES with H = 1024
    (FWD_VARIANTS also lists <2, 1>, <4, 1>, <4, 2>; fwd_rs() picks RS = 2 up to H = 512 and RS = 1
     above, so the host can launch only the three above)
  gru_bwd_seq_kernel<3, 2, 2>   H = 256, dW_hh + dP    BWD_CASES (256, *, "wp")
  gru_bwd_seq_kernel<3, 2, 0>   H = 256, dW_hh         BWD_CASES (256, *, "w")
  gru_bwd_seq_kernel<3, 0, 0>   H = 256                BWD_CASES (256, *, "none")
  gru_bwd_seq_kernel<6, 4, 2>   H = 512, dW_hh + dP    BWD_CASES (512, *, "wp")
  gru_bwd_seq_kernel<6, 4, 0>   H = 512, dW_hh         BWD_CASES (512, *, "w")
  gru_bwd_seq_kernel<6, 0, 0>   H = 512                BWD_CASES (512, *, "none")
  gru_bwd_seq_kernel<12, 0, 2>  H = 1024, dP           BWD_CASES (1024, *, "p")
  gru_bwd_seq_kernel<12, 0, 0>  H = 1024               BWD_CASES (1024, *, "none")
  gru_bwd_seq16_kernel<12, 2>   fused dP               BWD16_CASES with p = 1
  gru_bwd_seq16_kernel<12, 0>                          BWD16_CASES with p = 0
  gru_bwd_seq_big_kernel<false>                        BIG_CASES with fdy = 0
  gru_bwd_seq_big_kernel<true>  fused dy               BIG_CASES with fdy = 1
"""
import functools

import pytest
import torch

from gru_mpi_cuda_amd.models import seq_ref as sr

pytestmark = pytest.mark.gpu

DEV = "cuda"
V = 256
BF = torch.bfloat16
NAN = float("nan")


def S():
    return torch.cuda.current_stream().cuda_stream


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def all_nan(t):
    return bool(torch.isnan(t).all())


def no_nan(t):
    return not bool(torch.isnan(t).any())


def close(got, ref, family, what):
    """Print the figure, then assert it: |got - ref| - rtol |ref| at its worst against the family's atol."""
    print(f"{what}: deviation {sr.deviation(got, ref, sr.RTOL[family]):.3e} (atol {sr.ATOL[family]:.3e}, {family})")
    sr.assert_close(got, ref, family, what)


class Flags:
    """Zeroed flag block sized by seq_flag_words, the error word, and a block of ones standing for
    the next kernel's flags (zero_next), with a guard tail that must stay ones."""
    ZW = 1000

    def __init__(self, ext, H, Bp, words=None):
        self.cnt = torch.zeros(words or ext.seq_flag_words(H, Bp), device=DEV, dtype=torch.int32)
        self.err = torch.zeros(16, device=DEV, dtype=torch.int32)
        self.nxt = torch.ones(self.ZW + 64, device=DEV, dtype=torch.int32)

    def args(self, zero_next=True):
        d = dict(cnt=self.cnt.data_ptr(), err=self.err.data_ptr())
        if zero_next:
            d.update(zero_next=self.nxt.data_ptr(), zero_words=self.ZW)
        return d

    def rearm(self):
        self.cnt.zero_()
        self.nxt.fill_(1)

    def check(self, zero_next=True):
        assert int(self.err[0]) == 0, "a cross-workgroup wait hit its spin limit"
        if zero_next:
            assert not self.nxt[:self.ZW].any(), "zero_next block not zeroed"
            assert bool((self.nxt[self.ZW:] == 1).all()), "zero_next wrote past zero_words"

    def epochs(self, lines):
        """Word 0 of the first ``lines`` 64-byte flag lines."""
        return self.cnt[:lines * 16].view(lines, 16)[:, 0]


# ====================================================================================== forward
@functools.lru_cache(maxsize=4)
def _fwd_reference(H, Bp, T, mode, use_h0):
    d = {k: v.to(DEV) for k, v in sr.fwd_inputs(H, Bp, T, seed=0).items()}
    kw = dict(P=d["P"], ids=d["ids"]) if mode == "ids" else dict(Gi=d["Gi"])
    ref = sr.fwd_ref(d["Whh"], d["bhh"], T, Bp, h0=d["h0"] if use_h0 else None, **kw)
    return d, ref


# (H, Bp, T, input, h0, xring, allow_local, s16).  Bp = 256 (Bp/32 % 8 == 0) takes the row-block-fast
# workgroup map and, with allow_local, the L2-local hand-off; the other shapes the unit-tile-fast
# map.  Every value of every axis appears under both maps; T = 9 is no multiple of a ring, T < xring
# leaves the ring partly used.
FWD_CASES = [
    (512, 256, 9, "ids", 1, 4, 1, 0), (512, 256, 9, "gi", 0, 2, 0, 1), (512, 256, 2, "gi", 1, 0, 1, 1),
    (512, 256, 1, "ids", 0, 0, 0, 0), (512, 256, 1, "gi", 1, 2, 1, 0),
    (256, 64, 9, "ids", 1, 2, 1, 0), (256, 64, 2, "gi", 0, 4, 0, 1), (256, 64, 1, "ids", 0, 0, 1, 1),
    (256, 96, 9, "gi", 1, 4, 0, 0), (256, 96, 2, "ids", 0, 2, 1, 1),
    (512, 64, 9, "ids", 0, 0, 0, 1), (512, 64, 1, "gi", 1, 4, 1, 0),
    (1024, 128, 9, "ids", 1, 2, 1, 1), (1024, 128, 9, "gi", 0, 4, 0, 0), (1024, 128, 2, "ids", 1, 0, 1, 0),
    (1024, 128, 1, "gi", 0, 2, 0, 1),
]


@pytest.mark.parametrize("H,Bp,T,mode,use_h0,xring,local,s16", FWD_CASES)
def test_fwd_seq(ext, H, Bp, T, mode, use_h0, xring, local, s16):
    if not ext.fwd_seq_supported(H, Bp):
        pytest.skip("shape not co-resident")
    inp, ref = _fwd_reference(H, Bp, T, mode, bool(use_h0))
    ldT = (T + 1) * Bp + 64
    HSb, HSf = nans(T + 1, Bp, H, dtype=BF), nans(T + 1, Bp, H)
    HT, HF, xch = nans(H, ldT, dtype=BF), nans(T + 1, Bp * H, dtype=BF), nans(T, Bp * H, dtype=BF)
    if use_h0:   # as the trainer does: the bf16 copies of h_init are the caller's
        h0b = inp["h0"].to(BF)
        HSb[0], HSf[0], HF[0] = h0b, inp["h0"], sr.hf_encode(h0b[None])
    before = (HSb[0].clone(), HSf[0].clone(), HF[0].clone())
    sv = [nans(T, Bp, H) for _ in range(4)]
    sv16 = nans(T, Bp, H, 4, dtype=BF)
    Whh = inp["Whh"].to(BF).contiguous()
    fl = Flags(ext, H, Bp)
    d = dict(HSb=HSb.data_ptr(), HSf=HSf.data_ptr(), HT=HT.data_ptr(), ldT=ldT, HF=HF.data_ptr(), xch=xch.data_ptr(),
             Whh=Whh.data_ptr(), bhh=inp["bhh"].data_ptr(), allow_local=local, xring=xring, T=T, Bp=Bp, H=H, **fl.args())
    if s16:
        d["s16"] = sv16.data_ptr()
    else:
        d.update(sr=sv[0].data_ptr(), sz=sv[1].data_ptr(), sn=sv[2].data_ptr(), sghn=sv[3].data_ptr())
    if mode == "ids":
        d.update(P=inp["P"].data_ptr(), ids=inp["ids"].data_ptr())
    else:
        d["Gi"] = inp["Gi"].data_ptr()
    if use_h0:
        d["h0"] = inp["h0"].data_ptr()
    ext.fwd_seq(d, S())
    torch.cuda.synchronize()
    fl.check()
    nrb, nunit = Bp // 32, H // 16
    assert bool((fl.epochs(nrb * nunit) == T).all()), "every producer's flag ends at epoch T"
    # slot 0 of the state buffers is the caller's
    for got, was in zip((HSb[0], HSf[0], HF[0]), before):
        assert same_bits(got, was)
    close(HSf[1:], ref["HS"][1:], "f32_state", "HSf")
    close(HSb[1:], ref["HS"][1:], "bf16_copy", "HSb")
    # transposed copy: h_t at column (t + 1) * Bp + b -- the same bf16 values; column block 0 and the pad untouched
    assert same_bits(sr.ht_decode(HT, T + 1, Bp)[1:], HSb[1:]), "HT differs from HSb"
    close(sr.ht_decode(HT, T + 1, Bp)[1:], ref["HS"][1:], "bf16_copy", "HT")
    assert all_nan(HT[:, :Bp]) and all_nan(HT[:, (T + 1) * Bp:]), "HT written outside its steps"
    # fragment-tiled copy, blocks 1 .. T
    hf = sr.hf_decode(HF, T + 1, Bp, H)
    assert same_bits(hf[1:], HSb[1:]), "HF differs from HSb"
    close(hf[1:], ref["HS"][1:], "bf16_copy", "HF")
    names = ("r", "z", "n", "ghn")
    if s16:
        for k, got in zip(names, sr.s16_decode(sv16)):
            close(got, ref[k], "bf16_copy", "s16 " + k)
        assert all(all_nan(x) for x in sv)
    else:
        for k, got in zip(names, sv):
            close(got, ref[k], "f32_state", k)
        assert all_nan(sv16)
        # the kernel's own saves reproduce its own state: h = n + z (h_prev - n)
        hprev = torch.cat([(inp["h0"] if use_h0 else torch.zeros(Bp, H, device=DEV))[None], HSf[1:-1]])
        torch.testing.assert_close(sv[2] + sv[1] * (hprev - sv[2]), HSf[1:], atol=sr.F32_BLEND_ATOL, rtol=0)
    # exchange: step t in slot t % xring (T slots without a ring); the slots beyond stay untouched
    used = min(xring, T) if xring >= 2 else T
    assert no_nan(xch[:used]) and all_nan(xch[used:]), "exchange slots"


# ====================================================================================== backward
@functools.lru_cache(maxsize=3)
def _bwd_reference(H, Bp, T, rows, one_id, s16, fdy, big):
    d = sr.bwd_inputs(H, Bp, T, seed=0, one_id=one_id)
    if s16:
        d = sr.bwd_inputs_s16(d)
    d = {k: v.to(DEV) for k, v in d.items()}
    kw = dict(rows=rows, fuse_w=not big and rows == 32 and H <= 512)
    if not big:
        kw.update(ids=d["ids"], V=V)
    if fdy:
        kw.update(dl=d["dl"], Wfc=d["Wfc"])
    ref = sr.bwd_ref(None if fdy else d["dy"], d["r"], d["z"], d["n"], d["ghn"], d["HS"], d["Whh"], **kw)
    return d, ref


def _run_bwd(ext, kind, H, Bp, T, fuse="none", xring=0, local=1, hsrc=None, one_id=False, s16=False,
             n_only=False, fdy=False):
    """One persistent-backward case: launch twice (flags re-zeroed, outputs re-filled with NaN),
    require bitwise-equal results, compare the first with the reference."""
    rows = 16 if kind == "rows16" else 32
    big = kind == "big"
    fuse_w, fuse_p = "w" in fuse, "p" in fuse
    inp, ref = _bwd_reference(H, Bp, T, rows, one_id, bool(s16 or fdy), bool(fdy), big)
    H3, ldG, nrb = 3 * H, T * Bp + 64, Bp // rows
    WhhT = inp["Whh"].to(BF).T.contiguous()                      # [H][3H]
    HSf = inp["HS"].contiguous()
    hsb = HSf.to(BF)
    keep = [WhhT, HSf]
    fl = Flags(ext, H, Bp, words=8192 if big else None)
    d = dict(HSf=HSf.data_ptr(), WhhT=WhhT.data_ptr(), ldG=ldG, allow_local=local, xring=xring, T=T, Bp=Bp, H=H,
             **fl.args(zero_next=not big))
    if fdy:
        dl, WfcT = inp["dl"].to(BF).contiguous(), inp["Wfc"].to(BF).T.contiguous()   # [T*Bp][V], [H][V]
        d.update(dl=dl.data_ptr(), WfcT=WfcT.data_ptr(), V=V)
        keep += [dl, WfcT]
    else:
        dy = inp["dy"].contiguous()
        d["dy"] = dy.data_ptr()
        keep.append(dy)
    if s16 or fdy:
        p16 = sr.s16_encode(inp["r"], inp["z"], inp["n"], inp["ghn"])
        assert all(torch.equal(a.float(), inp[k]) for a, k in zip(sr.s16_decode(p16), ("r", "z", "n", "ghn")))
        d["s16"] = p16.data_ptr()
        keep.append(p16)
    else:
        svs = [inp[k].contiguous() for k in ("r", "z", "n", "ghn")]
        d.update(sr=svs[0].data_ptr(), sz=svs[1].data_ptr(), sn=svs[2].data_ptr(), sghn=svs[3].data_ptr())
        keep += svs
    if fuse_w:
        if hsrc == "HF":
            hop = sr.hf_encode(hsb)
            d["HF"] = hop.data_ptr()
        else:   # h_{t-1} at column t * Bp + b
            hop = sr.ht_encode(hsb, (T + 1) * Bp + 64)
            d.update(HT=hop.data_ptr(), ldT=(T + 1) * Bp + 64)
        keep.append(hop)
    if fuse_p:
        ids = inp["ids"].contiguous()
        d.update(ids=ids.data_ptr(), V=V)
        keep.append(ids)
    if kind == "rows16":
        d["rows16"] = 1
    if big:
        d["big"] = 1
    if n_only:
        d["dgiT_n_only"] = 1

    def launch():
        o = dict(xbuf=nans(T, Bp * H3, dtype=BF), dghT=nans(H3, ldG, dtype=BF), dgiT=nans(H3, ldG, dtype=BF),
                 dgi=nans(T, Bp, H3, dtype=BF), dbhh_part=nans(nrb, H3), dbih_part=nans(nrb, H3))
        if fuse_w:
            o["dWhh_part"] = nans(nrb, H3, H)
        if fuse_p:
            o["dP_part"] = nans(nrb, V, H3)
        if big:
            o["part"] = nans(ext.bwd_seq_big_part_floats(H, Bp))
        fl.rearm()
        ext.bwd_seq(dict(d, **{k: v.data_ptr() for k, v in o.items()}), S())
        torch.cuda.synchronize()
        fl.check(zero_next=not big)
        o["flags"] = fl.cnt.clone()
        return o

    o, o2 = launch(), launch()
    for k in o:
        if k not in ("part", "flags"):
            assert same_bits(o[k], o2[k]), f"{k} differs between two launches"
    # flags: every dGh producer published all its steps (the large-H kernel publishes nothing at t = 0)
    if big:
        assert bool((fl.epochs(256) == T - 1).all())
    else:
        nunit = H // 16 if rows == 32 else H // 32              # producers per row block
        assert bool((fl.epochs(nrb * nunit) == T).all())
    # row-major dGi and the transposed copies (pad columns untouched)
    close(o["dgi"], ref["dgi"], "bf16_grad", "dgi")
    gT, iT = sr.ht_decode(o["dghT"], T, Bp), sr.ht_decode(o["dgiT"], T, Bp)
    assert all_nan(o["dghT"][:, T * Bp:]) and all_nan(o["dgiT"][:, T * Bp:]), "pad columns written"
    close(gT, ref["dgh"], "bf16_grad", "dghT")         # n rows: dan * r
    if n_only:
        assert all_nan(iT[..., :2 * H]), "dgiT r/z rows written with dgiT_n_only"
    else:
        assert same_bits(iT[..., :2 * H], o["dgi"][..., :2 * H]), "dgiT r/z rows differ from dgi"
    assert same_bits(iT[..., 2 * H:], o["dgi"][..., 2 * H:]), "dgiT n rows differ from dgi"
    close(iT[..., 2 * H:], ref["dgi"][..., 2 * H:], "bf16_grad", "dgiT n rows")   # dan, not dan * r
    assert same_bits(gT[..., :2 * H], o["dgi"][..., :2 * H]), "dghT r/z rows differ from dgi"
    # partial sums: each row block against the reference restricted to its rows, then the total
    for k in ("dbhh_part", "dbih_part", "dWhh_part", "dP_part"):
        if k in o:
            close(o[k], ref[k], "f32_part", k + " per row block")
            close(o[k].sum(0), ref[k].sum(0), "f32_part", k + " total")
    # exchange: dGh_t in slot t % xring (one per step without a ring); the slots beyond stay untouched
    used = min(xring, T) if xring >= 2 else T
    assert all_nan(o["xbuf"][used:]), "exchange slots beyond the ring written"
    if big:   # [slots][Bp][3H] row-major; step 0 is not published
        for t in range(1, T):
            assert same_bits(o["xbuf"][t % (xring if xring >= 2 else T)].view(Bp, H3), gT[t].contiguous()), "exchange slot"
        if xring < 2:
            assert all_nan(o["xbuf"][0])
    else:
        assert no_nan(o["xbuf"][:used])


# (H, Bp, T, fused ("w" dW_hh, "p" dP), xring, allow_local, h operand of the fused dW_hh, all ids equal, s16)
BWD_CASES = [
    (256, 64, 7, "wp", 2, 1, "HF", 0, 0), (256, 64, 2, "w", 0, 0, "HT", 0, 0), (256, 64, 1, "none", 2, 1, None, 0, 0),
    (256, 256, 7, "w", 2, 1, "HF", 0, 0), (256, 256, 7, "none", 0, 0, None, 0, 1), (256, 256, 2, "wp", 0, 1, "HT", 0, 0),
    (256, 256, 1, "wp", 2, 0, "HF", 0, 0),
    (512, 64, 7, "w", 0, 1, "HT", 0, 0), (512, 64, 7, "wp", 2, 0, "HF", 0, 0), (512, 64, 1, "none", 0, 1, None, 0, 0),
    (512, 256, 7, "wp", 2, 1, "HT", 0, 0), (512, 256, 7, "wp", 2, 1, "HF", 1, 0), (512, 256, 2, "none", 2, 0, None, 0, 0),
    (512, 256, 2, "w", 2, 0, "HF", 0, 1), (512, 256, 1, "w", 0, 1, "HT", 0, 0),
    (1024, 64, 7, "p", 2, 1, None, 0, 0), (1024, 64, 2, "none", 0, 0, None, 0, 0),
    (1024, 128, 7, "none", 2, 1, None, 0, 0), (1024, 128, 7, "p", 0, 0, None, 0, 0), (1024, 128, 2, "p", 2, 0, None, 0, 0),
    (1024, 128, 1, "p", 2, 1, None, 0, 0),
]


@pytest.mark.parametrize("H,Bp,T,fuse,xring,local,hsrc,one_id,s16", BWD_CASES)
def test_bwd_seq(ext, H, Bp, T, fuse, xring, local, hsrc, one_id, s16):
    if not ext.bwd_seq_supported(H, Bp, "w" in fuse, "p" in fuse):
        pytest.skip("shape not co-resident")
    _run_bwd(ext, "rows32", H, Bp, T, fuse=fuse, xring=xring, local=local, hsrc=hsrc, one_id=bool(one_id), s16=bool(s16))


# (Bp, T, fused dP, s16, xring, allow_local, dgiT_n_only): H = 1024; Bp = 128 is 8 row blocks of 16
# (row-block-fast map), Bp = 80 is 5 (unit-tile-fast map)
BWD16_CASES = [
    (128, 5, 1, 0, 2, 1, 0), (128, 5, 0, 1, 0, 1, 0), (128, 1, 1, 1, 2, 0, 0), (128, 1, 0, 0, 0, 1, 0),
    (128, 5, 0, 1, 2, 1, 1),
    (80, 5, 1, 1, 2, 1, 0), (80, 5, 0, 0, 0, 0, 0), (80, 1, 1, 0, 0, 1, 0),
]


@pytest.mark.parametrize("Bp,T,p,s16,xring,local,n_only", BWD16_CASES)
def test_bwd_seq_rows16(ext, Bp, T, p, s16, xring, local, n_only):
    if not ext.bwd_seq16_supported(1024, Bp, bool(p)):
        pytest.skip("shape not co-resident")
    _run_bwd(ext, "rows16", 1024, Bp, T, fuse="p" if p else "none", xring=xring, local=local, s16=bool(s16),
             n_only=bool(n_only))


# (H, Bp, T, xring, s16, dgiT_n_only, fused dy): the two shapes with (H/128)(Bp/128) = 64
BIG_CASES = [
    (1024, 1024, 3, 2, 0, 0, 0), (1024, 1024, 3, 0, 1, 1, 0), (1024, 1024, 1, 2, 1, 0, 1), (1024, 1024, 3, 2, 1, 1, 1),
    (1024, 1024, 1, 0, 0, 1, 0),
    (2048, 512, 3, 0, 0, 1, 0), (2048, 512, 3, 2, 1, 0, 1), (2048, 512, 1, 2, 0, 0, 0), (2048, 512, 1, 0, 1, 1, 1),
    (2048, 512, 3, 2, 1, 0, 0),
]


@pytest.mark.parametrize("H,Bp,T,xring,s16,n_only,fdy", BIG_CASES)
def test_bwd_seq_big(ext, H, Bp, T, xring, s16, n_only, fdy):
    if not ext.bwd_seq_big_supported(H, Bp):
        pytest.skip("shape not co-resident")
    _run_bwd(ext, "big", H, Bp, T, xring=xring, s16=bool(s16), n_only=bool(n_only), fdy=bool(fdy))


def test_bwd_seq_big_unsupported_shape_raises(ext):
    """big = 1 at a shape with (H/128)(Bp/128) != 64 throws before anything is launched."""
    with pytest.raises(RuntimeError, match="gru_bwd_seq_big"):
        ext.bwd_seq(dict(big=1, H=1024, Bp=512, T=2, ldG=1024), 0)

"""Per-element tests of the two-layer wavefront forward (gru_seq.hip gru_fwd_seq2_kernel) against the
float64 reference of models/step_ref.py (wave_ref: two seq_ref.fwd_ref layers, layer hi fed with
bf16(h_lo(t+1)) . W_ih^T + b_ih), launched on its own through the raw binding.

Kernel variant -> cases (FWD2_VARIANTS of gru_seq.hip: one instantiation per H):
  gru_fwd_seq2_kernel<1>   H = 256    WAVE_CASES with H = 256  (the staging area is the padded NKS = 4 one)
  gru_fwd_seq2_kernel<2>   H = 512    WAVE_CASES with H = 512
  gru_fwd_seq2_kernel<4>   H = 1024   WAVE_CASES with H = 1024 (Bp <= 128: 64 unit tiles x Bp/32 row blocks
                                      must be co-resident, so Bp = 256 and the row-block-fast map do not exist here)

Bp = 256 (Bp/32 % 8 == 0) takes the row-block-fast workgroup map and, with allow_local, the L2-local
hand-off; Bp = 64, 96, 128 the unit-tile-fast map.  Every value of T, h0, lo's input, the saves of
each layer, the optional outputs and allow_local appears under both maps; xring = 2 and 4 on one
case per H.  As in test_seq_kernels_gpu.py: one zeroed flag block per layer, a zero_next block of
ones with a guard tail per layer, the error word must read 0, every output starts as NaN (slot 0
of a layer without h0 too: the kernel must not read it), every comparison prints its deviation and
atol first.  The tolerance is step_ref's wave_f32_state (measured on the CPU, tests/test_step_ref.py).
"""
import functools

import pytest
import torch

from gru_mpi_cuda_amd.models import seq_ref as sr
from gru_mpi_cuda_amd.models import step_ref as st
from test_seq_kernels_gpu import BF, DEV, Flags, S, all_nan, nans, no_nan, same_bits

pytestmark = pytest.mark.gpu

SAVES = ("r", "z", "n", "ghn")


def close(got, ref, what):
    fam = "wave_f32_state"
    print(f"{what}: deviation {sr.deviation(got, ref):.3e} (atol {st.ATOL[fam]:.3e}, {fam})")
    st.assert_close(got, ref, fam, what)


@functools.lru_cache(maxsize=2)
def _reference(H, Bp, T, mode, h0):
    d = {k: v.to(DEV).contiguous() for k, v in st.wave_inputs(H, Bp, T, seed=0).items()}
    ref = st.wave_ref(**st.wave_kw(d, T, Bp, mode, h0))
    for k in ("Whh_lo", "Wih_hi", "Whh_hi"):
        d[k + "_bf"] = d[k].to(BF).contiguous()
    return d, ref


class Layer:
    """One layer's buffers for one launch, NaN-prefilled; slot 0 of the state copies holds h0 where
    the layer has one (as the trainer leaves it) and NaN where not."""

    def __init__(self, ext, H, Bp, T, h0, s16, HT, HF):
        self.T, self.Bp, self.H, self.h0, self.s16, self.hasHT, self.hasHF = T, Bp, H, h0, s16, HT, HF
        self.ldT = (T + 1) * Bp + 64
        self.HSb, self.HSf = nans(T + 1, Bp, H, dtype=BF), nans(T + 1, Bp, H)
        self.HT, self.HF = nans(H, self.ldT, dtype=BF), nans(T + 1, Bp * H, dtype=BF)
        self.xch = nans(T, Bp * H, dtype=BF)
        self.sv, self.sv16 = [nans(T, Bp, H) for _ in range(4)], nans(T, Bp, H, 4, dtype=BF)
        if h0 is not None:
            h0b = h0.to(BF)
            self.HSb[0], self.HSf[0], self.HF[0] = h0b, h0, sr.hf_encode(h0b[None])
        self.before = (self.HSb[0].clone(), self.HSf[0].clone(), self.HF[0].clone())
        self.fl = Flags(ext, H, Bp)

    def args(self, Whh, bhh, local, xring):
        d = dict(HSb=self.HSb.data_ptr(), HSf=self.HSf.data_ptr(), xch=self.xch.data_ptr(), ldT=self.ldT,
                 Whh=Whh.data_ptr(), bhh=bhh.data_ptr(), allow_local=local, xring=xring, T=self.T, Bp=self.Bp,
                 H=self.H, **self.fl.args())
        if self.hasHT:
            d["HT"] = self.HT.data_ptr()
        if self.hasHF:
            d["HF"] = self.HF.data_ptr()
        if self.s16:
            d["s16"] = self.sv16.data_ptr()
        else:
            d.update(sr=self.sv[0].data_ptr(), sz=self.sv[1].data_ptr(), sn=self.sv[2].data_ptr(), sghn=self.sv[3].data_ptr())
        if self.h0 is not None:
            d["h0"] = self.h0.data_ptr()
        return d

    def outputs(self):
        return [self.HSb, self.HSf, self.HT, self.HF, self.sv16] + self.sv


def _launch(ext, inp, H, Bp, T, mode, h0, s16, opt, local, xring):
    """s16, opt = per layer (lo, hi): packed saves?, (HT?, HF?)."""
    lo = Layer(ext, H, Bp, T, inp["h0_lo"] if h0 in ("lo", "both") else None, s16[0], *opt[0])
    hi = Layer(ext, H, Bp, T, inp["h0_hi"] if h0 in ("hi", "both") else None, s16[1], *opt[1])
    dl = lo.args(inp["Whh_lo_bf"], inp["bhh_lo"], local, xring)
    dh = hi.args(inp["Whh_hi_bf"], inp["bhh_hi"], local, xring)
    dl.update(dict(P=inp["P"].data_ptr(), ids=inp["ids"].data_ptr()) if mode == "ids" else dict(Gi=inp["Gi"].data_ptr()))
    ext.fwd_seq2(dl, dh, inp["Wih_hi_bf"].data_ptr(), inp["bih_hi"].data_ptr(), S())
    torch.cuda.synchronize()
    return lo, hi


# (H, Bp, T, h0, lo's input, packed saves (lo, hi), (HT, HF) of lo, (HT, HF) of hi, allow_local, xring)
WAVE_CASES = [
    # row-block-fast map
    (512, 256, 9, "both", "ids", (0, 1), (1, 1), (1, 1), 1, 0), (512, 256, 9, "none", "gi", (1, 0), (1, 0), (0, 1), 0, 2),
    (256, 256, 2, "lo", "gi", (0, 0), (0, 0), (0, 0), 1, 0), (256, 256, 1, "hi", "ids", (1, 1), (1, 1), (1, 1), 0, 0),
    (256, 256, 9, "hi", "ids", (0, 1), (0, 1), (1, 0), 1, 4), (512, 256, 2, "lo", "ids", (1, 0), (1, 1), (1, 1), 0, 0),
    (512, 256, 1, "both", "gi", (0, 1), (0, 1), (1, 0), 1, 0), (256, 256, 2, "none", "ids", (1, 1), (1, 1), (0, 0), 1, 0),
    # unit-tile-fast map
    (256, 64, 9, "both", "ids", (0, 0), (1, 1), (1, 1), 1, 0), (256, 96, 9, "none", "gi", (1, 1), (1, 0), (0, 1), 0, 2),
    (256, 64, 2, "hi", "gi", (0, 1), (0, 0), (0, 0), 1, 0), (256, 96, 1, "lo", "ids", (1, 0), (1, 1), (1, 1), 0, 0),
    (512, 64, 9, "lo", "gi", (1, 0), (1, 1), (1, 1), 1, 4), (512, 96, 2, "both", "ids", (0, 1), (0, 1), (1, 0), 0, 0),
    (512, 64, 1, "none", "ids", (0, 0), (1, 1), (1, 1), 1, 0),
    (1024, 128, 9, "hi", "ids", (1, 1), (1, 1), (1, 1), 1, 0), (1024, 96, 9, "both", "gi", (0, 0), (1, 0), (0, 1), 0, 2),
    (1024, 64, 2, "none", "ids", (0, 1), (1, 1), (1, 1), 0, 0), (1024, 128, 1, "lo", "gi", (1, 0), (0, 0), (0, 0), 1, 4),
]


@pytest.mark.parametrize("H,Bp,T,h0,mode,s16,opt_lo,opt_hi,local,xring", WAVE_CASES)
def test_fwd_seq2(ext, H, Bp, T, h0, mode, s16, opt_lo, opt_hi, local, xring):
    if not ext.fwd_seq2_supported(H, Bp):
        print(f"NOT RUN: H={H} Bp={Bp}: the wavefront grid is not co-resident on this device")
        pytest.skip("shape not co-resident")
    inp, ref = _reference(H, Bp, T, mode, h0)
    run = lambda s: _launch(ext, inp, H, Bp, T, mode, h0, s, (opt_lo, opt_hi), local, xring)
    first, again, plain = run(s16), run(s16), run((0, 0))    # the case, the case once more, fp32 saves on both layers
    nrb, nunit = Bp // 32, H // 16
    used = min(xring, T) if xring >= 2 else T
    for name, y, y2, f, s in zip(("lo", "hi"), first, again, plain, s16):
        r = ref[name]
        y.fl.check()
        # lo's step t signals t + 1 in iteration t, hi's in iteration t + 1: every producer line of both ends at T
        assert bool((y.fl.epochs(nrb * nunit) == T).all()), f"{name}: a producer's flag does not end at epoch T"
        y2.fl.check()
        for a, b in zip(y.outputs(), y2.outputs()):
            assert same_bits(a, b), f"{name}: two launches differ"
        for got, was in zip((y.HSb[0], y.HSf[0], y.HF[0]), y.before):
            assert same_bits(got, was), f"{name}: slot 0 of a state copy written"
        close(y.HSf[1:], r["HS"][1:], f"{name} HSf")
        assert same_bits(y.HSb[1:], y.HSf[1:].to(BF)), f"{name}: HSb is not bf16(HSf)"
        if y.hasHT:   # h_t at column (t + 1) * Bp + b; column block 0 and the pad untouched
            assert same_bits(sr.ht_decode(y.HT, T + 1, Bp)[1:], y.HSb[1:]), f"{name}: HT differs from HSb"
            assert all_nan(y.HT[:, :Bp]) and all_nan(y.HT[:, (T + 1) * Bp:]), f"{name}: HT written outside its steps"
        else:
            assert all_nan(y.HT)
        if y.hasHF:
            assert same_bits(sr.hf_decode(y.HF, T + 1, Bp, H)[1:], y.HSb[1:]), f"{name}: HF differs from HSb"
        else:
            assert all_nan(y.HF[1:])   # block 0 is the caller's (checked above)
        # the fp32 saves of the all-fp32 launch against the reference; the state does not depend on the save format
        assert same_bits(f.HSf, y.HSf) and same_bits(f.HSb, y.HSb), f"{name}: HSf differs between save formats"
        for k, got in zip(SAVES, f.sv):
            close(got, r[k], f"{name} {k}")
        if s:
            for k, got, f32 in zip(SAVES, sr.s16_decode(y.sv16), f.sv):
                assert same_bits(got, f32.to(BF)), f"{name}: s16 {k} is not bf16 of the fp32 save"
            assert all(all_nan(x) for x in y.sv), f"{name}: fp32 saves written beside s16"
        else:
            assert all(same_bits(a, b) for a, b in zip(y.sv, f.sv)) and all_nan(y.sv16)
        # the kernel's own saves reproduce its own state: h = n + z (h_prev - n)
        hprev = torch.cat([(y.h0 if y.h0 is not None else torch.zeros(Bp, H, device=DEV))[None], f.HSf[1:-1]])
        torch.testing.assert_close(f.sv[2] + f.sv[1] * (hprev - f.sv[2]), f.HSf[1:], atol=sr.F32_BLEND_ATOL, rtol=0)
        # exchange: step t in slot t % xring of both layers (lo's ring length serves both)
        assert no_nan(y.xch[:used]) and all_nan(y.xch[used:]), f"{name}: exchange slots"


def test_fwd_seq2_rejects_inconsistent_layers(ext):
    """hi aliasing lo's exchange or flags, or another shape, throws before anything is launched."""
    a = dict(HSb=256, HSf=256, xch=256, cnt=256, Whh=256, bhh=256, T=2, Bp=64, H=256, Gi=256)
    if not ext.fwd_seq2_supported(256, 64):
        pytest.skip("shape not co-resident")
    with pytest.raises(RuntimeError, match="inconsistent layer arguments"):
        ext.fwd_seq2(a, dict(a), 256, 256, 0)
    with pytest.raises(RuntimeError, match="inconsistent layer arguments"):
        ext.fwd_seq2(a, dict(a, xch=512, cnt=512, T=3), 256, 256, 0)

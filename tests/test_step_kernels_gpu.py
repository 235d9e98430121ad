"""Per-element tests of the per-step GRU kernels (gru_step.hip, gru_step_lds.hip) against the float64
reference of models/step_ref.py, each kernel launched on its own through the raw bindings.

Kernel variant -> cases (step_ref.FWD_STEP_CASES / BWD_STEP_CASES; every case asserts the kernel it
claims through fwd_step_variant / bwd_step_variant, the plan the launcher itself switches on):
  gru_fwd_step_kernel<1, false>   reg, ks 2 / ks 4     H = 64, 128; table and Gi input
  gru_fwd_step_kernel<2, false>   reg, ks 8            H = 512
  gru_fwd_step_kernel<4, false>   reg, ks 8            H = 1024; H = 1024, Bp = 512 with colT % 8 != 0
  gru_fwd_step_kernel<1, true>    reg, fused           H = 64, 128 (Kin = H, and Kin = 256 at H = 128)
  gru_fwd_step_kernel<2, true>    reg, fused           H = 512 (Kin = 512; Kin = 64: ks shrinks to 1; Kin = 256)
  gru_fwd_step_kernel<4, true>    reg, fused           H = 1024 (Kin = 1024; Kin = 256: ks shrinks to 2)
  gru_fwd_step_lds64_kernel<3>          lds64          H = 256, Bp = 128 and H = 320, Bp = 256, algo 2
  gru_fwd_step_lds64_kernel<3, true>    lds64, fused   the same shapes, Kin = H and 64
  gru_fwd_step_lds_kernel<false, 2>     lds128         the same shapes under fwd64 = 0; H = 2048, Bp = 1024 by default
  gru_fwd_step_lds_kernel<true, 2>      lds128, fused  the same; H = 1024, Bp = 3840 (the big tile's neighbour)
  gru_fwd_step_big_kernel<true>         big            H = 1024, Bp = 4096, Kin = 64 and 1024
    (gru_fwd_step_big_kernel<false> has no launch site: the big tile is taken with the fused input only)
  gru_bwd_step_kernel<1>          reg, ks 4 / ks 8     H = 128, 256
  gru_bwd_step_kernel<2>          reg, ks 8            H = 512
  gru_bwd_step_kernel<4>          reg, ks 8            H = 1024
  gru_bwd_step_lds8_kernel        lds8                 H = 256, Bp = 128; H = 320, Bp = 256; H = 1024, Bp = 128;
                                                       and every split-K case with a workspace too small
  gru_bwd_step_sk_kernel<4, 4, true>   sk4, sk_map 1   H = 1024, Bp = 768
  gru_bwd_step_sk_kernel<2>            sk2, sk_map 1   H = 1024, Bp = 1536
  gru_bwd_step_sk_kernel<2>            sk2, sk_map 0   H = 1280, Bp = 1536
    (which split-K kernel a shape takes depends on the device's occupancy: a case whose claim the
     device does not confirm prints NOT RUN and skips)

Every output buffer starts as NaN, every comparison prints its deviation and its atol before it
asserts, the tolerances are step_ref's (measured on the CPU, tests/test_step_ref.py), and the float64
reference runs in torch on the device, once per input set.
"""
import functools

import pytest
import torch

from gru_mpi_cuda_amd.models import seq_ref as sr
from gru_mpi_cuda_amd.models import step_ref as st

pytestmark = pytest.mark.gpu

DEV = "cuda"
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


def close(got, ref, family, what):
    """Print the figure, then assert it."""
    print(f"{what}: deviation {sr.deviation(got, ref, st.RTOL[family]):.3e} (atol {st.ATOL[family]:.3e}, {family})")
    st.assert_close(got, ref, family, what)


def only_columns_written(T_, col, Bp):
    """A transposed copy [rows][ld]: nothing outside columns [col, col + Bp) was written."""
    return all_nan(T_[:, :col]) and all_nan(T_[:, col + Bp:])


@pytest.fixture
def step_variants(ext):
    saved = ext.step_lds_variants()
    yield ext
    ext.set_step_lds_variants(saved)


# ====================================================================================== forward
@functools.lru_cache(maxsize=2)
def _fwd_reference(H, Bp, mode, Kin):
    d = {k: v.to(DEV) for k, v in st.fwd_step_inputs(H, Bp, Kin, seed=0).items()}
    d["Whh_bf"], d["hprev_bf"] = d["Whh"].to(BF).contiguous(), d["hprev"].to(BF).contiguous()
    if Kin:
        d["x_bf"], d["Wih_bf"] = d["x"].to(BF).contiguous(), d["Wih"].to(BF).contiguous()
    return d, st.fwd_step_ref(d["Whh"], d["bhh"], d["hprev"], **st.fwd_step_kw(d, mode))


def _fwd_args(d, H, Bp, mode, Kin, algo):
    a = dict(hprev_bf=d["hprev_bf"].data_ptr(), hprev_f=d["hprev"].data_ptr(), Whh=d["Whh_bf"].data_ptr(),
             bhh=d["bhh"].data_ptr(), Bp=Bp, H=H, algo=algo)
    if mode == "table":
        a.update(P=d["P"].data_ptr(), ids=d["ids"].data_ptr())
    elif mode == "gi":
        a["Gi"] = d["Gi"].data_ptr()
    else:
        a.update(x_bf=d["x_bf"].data_ptr(), Wih=d["Wih_bf"].data_ptr(), bih=d["bih"].data_ptr(), Kin=Kin)
    return a


def _fwd_launch(ext, base, H, Bp, ldT, colT, saves, with_hT=True):
    """One launch into fresh NaN buffers.  saves: "f32", "s16" or None."""
    o = dict(h_f=nans(Bp, H), h_bf=nans(Bp, H, dtype=BF), hT=nans(H, ldT, dtype=BF),
             sv=[nans(Bp, H) for _ in range(4)], s16=nans(Bp, H, 4, dtype=BF))
    a = dict(base, h_f=o["h_f"].data_ptr(), h_bf=o["h_bf"].data_ptr(), ldT=ldT, colT=colT)
    if with_hT:
        a["hT"] = o["hT"].data_ptr()
    if saves == "f32":
        a.update(sr=o["sv"][0].data_ptr(), sz=o["sv"][1].data_ptr(), sn=o["sv"][2].data_ptr(), sghn=o["sv"][3].data_ptr())
    elif saves == "s16":
        a["s16"] = o["s16"].data_ptr()
    ext.fwd_step(a, S())
    torch.cuda.synchronize()
    return o


# (ks, kb) of the register-direct forward by pick_split and the fused shrink loops: H -> plain / Kin = H
REG_FWD_SPLIT = {64: (2, 1), 128: (4, 1), 512: (8, 2), 1024: (8, 4)}
REG_FWD_SPLIT_KIN = {(128, 256): (4, 1), (1024, 256): (2, 4), (512, 64): (1, 2)}


@pytest.mark.parametrize("name,H,Bp,mode,Kin,algo,fwd64,coff", st.FWD_STEP_CASES)
def test_fwd_step(step_variants, name, H, Bp, mode, Kin, algo, fwd64, coff):
    ext = step_variants
    ext.set_step_lds_variants(dict(fwd64=fwd64))
    inp, ref = _fwd_reference(H, Bp, mode, Kin)
    ldT, colT = 3 * Bp + 64, Bp + coff
    base = _fwd_args(inp, H, Bp, mode, Kin, algo)
    var = ext.fwd_step_variant(dict(base, ldT=ldT, colT=colT))
    print(f"variant {var}")
    assert var["name"] == name
    if name == "reg" and not coff:
        want = REG_FWD_SPLIT_KIN[(H, Kin)] if Kin and Kin != H else REG_FWD_SPLIT[H]
        assert (var["ks"], var["kb"]) == want
    # ---- fp32 saves + the transposed copy
    o = _fwd_launch(ext, base, H, Bp, ldT, colT, "f32")
    close(o["h_f"], ref["h"], "f32_state", "h_f")
    for k, got in zip(("r", "z", "n", "ghn"), o["sv"]):
        close(got, ref[k], "f32_state", k)
    assert same_bits(o["h_bf"], o["h_f"].to(BF)), "h_bf is not bf16(h_f)"
    assert same_bits(o["hT"][:, colT:colT + Bp], o["h_bf"].T), "hT differs from h_bf^T"
    assert only_columns_written(o["hT"], colT, Bp), "hT written outside its columns"
    assert all_nan(o["s16"])
    # ---- packed saves instead
    if name == "reg":
        with pytest.raises(RuntimeError, match="packed bf16 saves"):
            _fwd_launch(ext, base, H, Bp, ldT, colT, "s16")
    else:
        p = _fwd_launch(ext, base, H, Bp, ldT, colT, "s16")
        assert same_bits(p["h_f"], o["h_f"]) and same_bits(p["h_bf"], o["h_bf"]), "s16 launch changed h"
        for k, got, f32 in zip(("r", "z", "n", "ghn"), sr.s16_decode(p["s16"]), o["sv"]):
            assert same_bits(got, f32.to(BF)), f"s16 {k} is not bf16 of the fp32 save"
        assert all(all_nan(x) for x in p["sv"]), "fp32 saves written beside s16"
        assert same_bits(p["hT"], o["hT"])
    # ---- as the generator launches it: no saves, no transposed copy
    q = _fwd_launch(ext, base, H, Bp, ldT, colT, None, with_hT=False)
    assert same_bits(q["h_f"], o["h_f"]) and same_bits(q["h_bf"], o["h_bf"]), "launch without saves / hT changed h"
    assert all_nan(q["hT"]) and all(all_nan(x) for x in q["sv"]) and all_nan(q["s16"])


def test_fwd_step_lds_request_with_unaligned_colT_raises(ext):
    """algo = 2 where the LDS kernels' 16-byte transposed stores cannot be used throws before a launch."""
    H, Bp = 1024, 512
    with pytest.raises(RuntimeError, match="LDS kernel requested"):
        ext.fwd_step_variant(dict(H=H, Bp=Bp, algo=2, ldT=3 * Bp + 64, colT=Bp + 4))
    with pytest.raises(RuntimeError, match="LDS kernel requested"):
        ext.fwd_step(dict(H=H, Bp=Bp, algo=2, ldT=3 * Bp + 64, colT=Bp + 4), 0)
    assert ext.fwd_step_variant(dict(H=H, Bp=Bp, algo=0, ldT=3 * Bp + 64, colT=Bp))["name"] == "lds64"
    # gru_step_lds_ok wants whole 128-row tiles, also for the 64-row kernels: H = 320 runs at Bp = 256, not 192
    for query in (ext.fwd_step_variant, ext.bwd_step_variant):
        with pytest.raises(RuntimeError, match="LDS kernel requested"):
            query(dict(H=320, Bp=192, algo=2, ldT=3 * 192 + 64, colT=192))
        assert query(dict(H=320, Bp=192, algo=0, ldT=3 * 192 + 64, colT=192))["name"] == "reg"


# ====================================================================================== backward
@functools.lru_cache(maxsize=2)
def _bwd_reference(H, Bp, first):
    d = {k: v.to(DEV).contiguous() for k, v in st.bwd_step_inputs(H, Bp, seed=0).items()}
    d["WhhT_bf"] = d["Whh"].to(BF).T.contiguous()                 # [H][3H]
    d["dgh_next_bf"] = d["dgh_next"].to(BF).contiguous()
    a, kw = st.bwd_step_args(d, first)
    return d, st.bwd_step_ref(*a, **kw)


def _bwd_args(d, H, Bp, algo, first, ldT, colT):
    a = dict(WhhT=d["WhhT_bf"].data_ptr(), dy=d["dy"].data_ptr(), r=d["r"].data_ptr(), z=d["z"].data_ptr(),
             n=d["n"].data_ptr(), ghn=d["ghn"].data_ptr(), hprev=d["hprev"].data_ptr(), ldT=ldT, colT=colT,
             Bp=Bp, H=H, algo=algo)
    if not first:
        a.update(dgh_next=d["dgh_next_bf"].data_ptr(), carry_in=d["carry_in"].data_ptr())
    return a


def _bwd_launch(ext, base, H, Bp, ldT, dgi=True, dgiT=True, n_only=False):
    o = dict(carry_out=nans(Bp, H), dgh=nans(Bp, 3 * H, dtype=BF), dgi=nans(Bp, 3 * H, dtype=BF),
             dghT=nans(3 * H, ldT, dtype=BF), dgiT=nans(3 * H, ldT, dtype=BF))
    a = dict(base, carry_out=o["carry_out"].data_ptr(), dgh=o["dgh"].data_ptr(), dghT=o["dghT"].data_ptr())
    if dgi:
        a["dgi"] = o["dgi"].data_ptr()
    if dgiT:
        a["dgiT"] = o["dgiT"].data_ptr()
    if n_only:
        a["dgiT_n_only"] = 1
    ext.bwd_step(a, S())
    torch.cuda.synchronize()
    return o


def _check_bwd(o, ref, H, Bp, colT):
    close(o["carry_out"], ref["carry_out"], "f32_carry", "carry_out")
    close(o["dgh"], ref["dgh"], "bf16_grad", "dgh")
    close(o["dgi"], ref["dgi"], "bf16_grad", "dgi")
    assert same_bits(o["dgi"][:, :2 * H], o["dgh"][:, :2 * H]), "dgi r/z columns differ from dgh"
    assert same_bits(o["dghT"][:, colT:colT + Bp], o["dgh"].T), "dghT differs from dgh^T"
    assert same_bits(o["dgiT"][:, colT:colT + Bp], o["dgi"].T), "dgiT differs from dgi^T"
    assert only_columns_written(o["dghT"], colT, Bp) and only_columns_written(o["dgiT"], colT, Bp), "pad columns written"


REG_BWD_SPLIT = {128: (4, 1), 256: (8, 1), 512: (8, 2), 1024: (8, 4)}


@pytest.mark.parametrize("first", [False, True])
@pytest.mark.parametrize("name,H,Bp,algo", st.BWD_STEP_CASES)
def test_bwd_step(step_variants, name, H, Bp, algo, first):
    ext = step_variants
    sk = name in ("sk2", "sk4")
    ldT, colT = 3 * Bp + 64, Bp
    inp, ref = _bwd_reference(H, Bp, first)
    base = _bwd_args(inp, H, Bp, algo, first, ldT, colT)
    if sk:
        # the split count is the device's: occupancy x CUs against the tile count (gru_bwd_step_sk_splits)
        ext.set_step_lds_variants(dict(bwd_sk_min_h=1024))
        S_ = ext.bwd_step_sk_splits(H, Bp)
        if S_ != int(name[2]):
            print(f"NOT RUN: {name} at H={H} Bp={Bp}: gru_bwd_step_sk_splits gives {S_} on this device")
            pytest.skip(f"the device takes {S_} splits here, not {name}")
        tiles = (H // 128) * (Bp // 128)
        part = nans(H * Bp * S_)
        cnt = torch.cat([torch.zeros(tiles * 16, dtype=torch.int32), torch.ones(64, dtype=torch.int32)]).to(DEV)
        err = torch.zeros(16, device=DEV, dtype=torch.int32)
        ws = dict(sk_part=part.data_ptr(), sk_part_floats=part.numel(), sk_cnt=cnt.data_ptr(),
                  sk_cnt_words=tiles * 16, err=err.data_ptr())
        base.update(ws)
    var = ext.bwd_step_variant(base)
    print(f"variant {var}")
    assert var["name"] == name
    if name == "reg":
        assert (var["ks"], var["kb"]) == REG_BWD_SPLIT[H]
    if sk:
        assert var["splits"] == S_ and var["sk_map"] == (1 if (H // 128) % (8 // S_) == 0 else 0)
        assert var["sk_map"] == (0 if H == 1280 else 1)
    o = _bwd_launch(ext, base, H, Bp, ldT)
    _check_bwd(o, ref, H, Bp, colT)
    if sk:
        # three launches on one workspace: deterministic, counters monotonic, nothing past them touched
        for _ in range(2):
            o2 = _bwd_launch(ext, base, H, Bp, ldT)
            for k in o:
                assert same_bits(o[k], o2[k]), f"{k} differs between launches"
        assert int(err[0]) == 0, "a split-K wait hit its spin limit"
        counters = cnt[:tiles * 16].view(tiles, 16)[:, 0]
        # the first step has no product: nothing is exchanged and the counters are not touched
        assert bool((counters == (0 if first else 3 * S_)).all()), counters
        assert bool((cnt[tiles * 16:] == 1).all()), "counter guard tail written"
        assert not bool(cnt[:tiles * 16].view(tiles, 16)[:, 1:].any()), "words beside the counters written"
    # ---- dgiT_n_only: the r / z rows of dgiT are left alone, everything else as before
    p = _bwd_launch(ext, base, H, Bp, ldT, n_only=True)
    assert all_nan(p["dgiT"][:2 * H]), "dgiT r/z rows written with dgiT_n_only"
    assert same_bits(p["dgiT"][2 * H:], o["dgiT"][2 * H:]), "dgiT n rows differ with dgiT_n_only"
    for k in ("carry_out", "dgh", "dgi", "dghT"):
        assert same_bits(p[k], o[k]), f"{k} differs with dgiT_n_only"
    # ---- nullable outputs: the trainer's layer 0 passes no dgi
    for dgi, dgiT in ((False, True), (True, False), (False, False)):
        p = _bwd_launch(ext, base, H, Bp, ldT, dgi=dgi, dgiT=dgiT)
        for k in ("carry_out", "dgh", "dghT") + (("dgi",) if dgi else ()) + (("dgiT",) if dgiT else ()):
            assert same_bits(p[k], o[k]), f"{k} differs with dgi={dgi} dgiT={dgiT}"
        assert dgi or all_nan(p["dgi"])
        assert dgiT or all_nan(p["dgiT"])
    if sk:
        # a workspace one float or one counter word too small: the launcher's host-side fall-back to
        # the 64 x 64 kernel, visible through the query, and still correct
        for short in (dict(sk_part_floats=part.numel() - 1), dict(sk_cnt_words=tiles * 16 - 1)):
            b = dict(base, **short)
            assert ext.bwd_step_variant(b)["name"] == "lds8"
            before = cnt.clone()
            p = _bwd_launch(ext, b, H, Bp, ldT)
            _check_bwd(p, ref, H, Bp, colT)
            assert torch.equal(cnt, before), "the fall-back touched the split-K counters"
        assert ext.bwd_step_variant(dict(base, sk_part=0))["name"] == "lds8"


def test_bwd_step_below_sk_min_h_takes_lds8(step_variants):
    """bwd_sk_min_h gates the split-K kernel per call: above H it is the 64 x 64 kernel."""
    ext = step_variants
    H, Bp = 1024, 768
    d = dict(H=H, Bp=Bp, algo=2, ldT=3 * Bp + 64, colT=Bp, sk_part=256, sk_part_floats=H * Bp * 4, sk_cnt=256,
             sk_cnt_words=(H // 128) * (Bp // 128) * 16)
    ext.set_step_lds_variants(dict(bwd_sk_min_h=2048))
    assert ext.bwd_step_sk_splits(H, Bp) == 0 and ext.bwd_step_variant(d)["name"] == "lds8"

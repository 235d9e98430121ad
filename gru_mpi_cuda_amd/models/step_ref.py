"""Per-element reference of the per-step GRU kernels (gru_step.hip, gru_step_lds.hip) and of the
two-layer wavefront forward (gru_seq.hip gru_fwd_seq2_kernel), in plain torch, next to
``seq_ref.py`` whose gate formulas, rounding, deviation / mismatch helpers and layout decoders it
reuses.

* ``fwd_step_ref`` / ``bwd_step_ref``: ONE timestep in float64 in the kernels' operand precision --
  the MFMA operands (h_{t-1}, x, dGh_{t+1}) are rounded to bf16 as the kernels read them, the blend
  operand h_{t-1}, the input projection and the gate math stay unrounded.  ``exact=True`` turns the
  rounding off; the result then equals ``torch.autograd`` (tests/test_step_ref.py).
* ``emulate_fwd_step`` / ``emulate_bwd_step``: the same in float32 with every bf16-stored output
  rounded once and a ``mut`` hook that plants one of the bugs the tolerances must catch.
* ``wave_ref`` / ``emulate_wave``: two stacked layers composed from ``seq_ref.fwd_ref`` /
  ``seq_ref.emulate_fwd``: layer ``hi`` takes Gi[t] = bf16(h_lo(t+1)) . W_ih^T + b_ih.
* seeded input makers and the case tables of tests/test_step_kernels_gpu.py and
  tests/test_wave_kernel_gpu.py, which the tolerance measurement below runs on the CPU.

Every function runs on the device of its inputs.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import seq_ref as sr
from .seq_ref import _gates, _ident, bf16_round, deviation

Out = Dict[str, torch.Tensor]

# ------------------------------------------------------------------------------ tolerances
# |got - ref| <= ATOL + RTOL |ref| per family, by seq_ref's rule:
#   f32_state : h_f and the four fp32 saves of a forward step
#   f32_carry : carry_out of a backward step
#   bf16_grad : dgh, dgi of a backward step (bf16-stored: rtol = 2^-7, as in seq_ref)
# MEASURED_DEV is the largest deviation emulator - reference (|emu - ref| - RTOL |ref|) over every
# case of FWD_STEP_CASES / BWD_STEP_CASES (first and middle step) and seeds 0, 1, 2, produced by
#     python -m gru_mpi_cuda_amd.models.step_ref
# (figures rounded up to three digits).  One step on identical bf16 operands has no compounding:
# the forward and carry deviations are fp32 rounding of the K-long dot products (K up to 2048
# forward, 3 x 1280 = 3840 backward); what is left of a bf16 gate gradient after rtol took the
# rounding of the stored value is the fp32 error of dh on the few elements where dy + carry + the
# product cancel.  ATOL = 4 x measured: the margin seq_ref gives for the MFMA summation order and
# the device __expf / rcp, which the emulator does not model.
RTOL = {"f32_state": 0.0, "f32_carry": 0.0, "bf16_grad": 2.0 ** -7}
MEASURED_DEV = {
    "f32_state": 1.63e-06,
    "f32_carry": 2.36e-06,
    "bf16_grad": 3.78e-07,
}
ATOL = {k: 4.0 * v for k, v in MEASURED_DEV.items()}
# The wavefront: emulate_wave against wave_ref over WAVE_SHAPES at T = WAVE_T, table and Gi input,
# seeds 0, 1, 2 (the same command prints it), over HSf and the fp32 saves.  Not every deviation is
# within seq_ref.MEASURED_DEV["f32_state"] = 1.36e-3: layer lo alone reaches 1.74e-3 on these inputs
# (seq_ref's one-layer forward on other seeds and on shapes its own measurement does not hold, such
# as H = 256 at Bp = 256), and layer hi, which inherits lo's bf16 flips through its input projection
# on top of its own, 2.00e-3.  So the wavefront has a family of its own, wave_f32_state, for both
# layers; seq_ref's figures are not touched.
WAVE_MEASURED_DEV = {
    "wave_f32_state": 2.00e-03,
}
WAVE_MEASURED_LO = 1.74e-03     # layer lo alone, for the record
RTOL["wave_f32_state"] = 0.0
ATOL.update({k: 4.0 * v for k, v in WAVE_MEASURED_DEV.items()})


def mismatch(got, ref, family) -> Optional[str]:
    return sr.mismatch(got, ref, family, ATOL, RTOL)


def assert_close(got, ref, family, what="") -> None:
    sr.assert_close(got, ref, family, what, ATOL, RTOL)


# ------------------------------------------------------------------------------ forward step
def _fwd_step(Whh, bhh, hprev, P, ids, Gi, x, Wih, bih, dtype, rnd, mut=None) -> Out:
    H = Whh.shape[1]
    c = lambda t: t.to(dtype)
    W, b, hp = c(Whh), c(bhh), c(hprev)
    op = rnd(hp)
    if mut == "drop_k_fragment":                       # one 8-element K fragment left out of the product
        op = op.clone()
        op[:, H // 2:H // 2 + 8] = 0
    gh = op @ W.T + b
    fused = x is not None
    if fused:
        gi = rnd(c(x)) @ c(Wih).T + c(bih)
    else:
        gi = c(P)[ids.long()] if ids is not None else c(Gi)
    hb = rnd(hp) if mut == "blend_from_bf16_hprev" else hp
    if mut == "bhn_outside_r":                         # n = tanh(gi_n + r (gh_n - b_hn) + b_hn)
        h, r, z, n, ghn = _gates(gi + torch.cat([torch.zeros_like(b[:2 * H]), b[2 * H:]]),
                                 gh - torch.cat([torch.zeros_like(b[:2 * H]), b[2 * H:]]), hb)
        ghn = gh[:, 2 * H:]
    elif mut == "fused_n_summed_before_r":             # n = tanh(r (gi_n + gh_n)): one accumulator for both
        assert fused
        s = gi + gh
        r, z = torch.sigmoid(s[:, :H]), torch.sigmoid(s[:, H:2 * H])
        n = torch.tanh(r * s[:, 2 * H:])
        h, ghn = n + z * (hb - n), gh[:, 2 * H:]
    else:
        h, r, z, n, ghn = _gates(gi, gh, hb)
    if mut == "rz_saves_swapped":
        r, z = z, r
    return dict(h=h, r=r, z=z, n=n, ghn=ghn)


def fwd_step_ref(Whh, bhh, hprev_f, P=None, ids=None, Gi=None, x=None, Wih=None, bih=None, exact=False) -> Out:
    """One forward step in float64.  gh = bf16(h_prev) . Whh^T + b_hh (Whh [3H][H] holds bf16 values);
    gi = P[ids] (P [V][3H], ids [Bp]), Gi [Bp][3H], or fused bf16(x) . Wih^T + b_ih (x [Bp][Kin],
    Wih [3H][Kin] bf16 values); r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r gh_n),
    h = n + z (h_prev - n) with the UNROUNDED fp32 h_prev.  Returns h, r, z, n, ghn [Bp][H]."""
    assert (ids is not None) + (Gi is not None) + (x is not None) == 1
    return _fwd_step(Whh, bhh, hprev_f, P, ids, Gi, x, Wih, bih, torch.float64, _ident if exact else bf16_round)


def emulate_fwd_step(Whh, bhh, hprev_f, P=None, ids=None, Gi=None, x=None, Wih=None, bih=None, mut=None) -> Out:
    """fwd_step_ref as a correct kernel computes it: float32, plus the bf16-stored outputs
    (h_bf, and the packed saves r16 .. ghn16), each rounded once."""
    o = _fwd_step(Whh, bhh, hprev_f, P, ids, Gi, x, Wih, bih, torch.float32, bf16_round, mut)
    o["h_bf"] = bf16_round(o["h"])
    for k in ("r", "z", "n", "ghn"):
        o[k + "16"] = bf16_round(o[k])
    return o


# ------------------------------------------------------------------------------ backward step
def _bwd_step(dy, r, z, n, ghn, hprev, Whh, dgh_next, carry_in, dtype, rnd, rnd_out, mut=None) -> Out:
    c = lambda t: t.to(dtype)
    dh = c(dy)
    prod = None
    if dgh_next is not None:
        prod = rnd(c(dgh_next)) @ c(Whh)                          # [Bp][3H] . [3H][H]
        dh = dh + prod + (c(carry_in) if carry_in is not None else 0)
    rt, zt, nt, gt, hp = c(r), c(z), c(n), c(ghn), c(hprev)
    dn = dh * (1 - zt)
    dz = dh * (hp - nt)
    dan = dn * (1 - nt * nt)
    dar = dan * gt * rt * (1 - rt)
    daz = dz * zt * (zt if mut == "daz_uses_z" else 1 - zt)
    dgh = torch.cat([dar, daz, dan if mut == "dgh_n_without_r" else dan * rt], 1)
    dgi = torch.cat([dar, daz, dan], 1)
    carry = zt * (dh - prod if mut == "carry_without_product" and prod is not None else dh)
    return dict(carry_out=carry, dgh=rnd_out(dgh), dgi=rnd_out(dgi))


def bwd_step_ref(dy, r, z, n, ghn, hprev, Whh, dgh_next=None, carry_in=None, exact=False) -> Out:
    """One BPTT step in float64 from given saves.  dh = dy (+ dgh_next . Whh + carry_in; dgh_next
    [Bp][3H] holds bf16 values, Whh [3H][H]); then seq_ref._bwd's formulas: dn = dh (1 - z),
    dz = dh (h_prev - n), dan = dn (1 - n^2), dar = dan gh_n r (1 - r), daz = dz z (1 - z),
    dgh = [dar, daz, dan r], dgi = [dar, daz, dan], carry_out = z dh.  Unrounded outputs."""
    return _bwd_step(dy, r, z, n, ghn, hprev, Whh, dgh_next, carry_in, torch.float64,
                     _ident if exact else bf16_round, _ident)


def emulate_bwd_step(dy, r, z, n, ghn, hprev, Whh, dgh_next=None, carry_in=None, mut=None) -> Out:
    """bwd_step_ref as a correct kernel computes it: float32, dgh / dgi rounded to bf16 as stored."""
    return _bwd_step(dy, r, z, n, ghn, hprev, Whh, dgh_next, carry_in, torch.float32, bf16_round, bf16_round, mut)


# ------------------------------------------------------------------------------ wavefront
def _wave(fwd, lo_key, rnd_x, dtype, Whh_lo, bhh_lo, Wih_hi, bih_hi, Whh_hi, bhh_hi, T, Bp, P, ids, Gi, h0_lo, h0_hi,
          mut=None, **kw):
    lo = fwd(Whh_lo, bhh_lo, T, Bp, P=P, ids=ids, Gi=Gi, h0=h0_lo, **kw)
    H = Whh_lo.shape[1]
    x = rnd_x(lo[lo_key].to(dtype))                               # [T+1][Bp][H]; hi's step t reads h_lo(t+1)
    x = x[:-1] if mut == "hi_reads_stale_h_lo" else x[1:]         # planted: h_lo(t), one step stale
    W, b = Wih_hi.to(dtype), bih_hi.to(dtype)
    prod = x @ W.T
    if mut == "hi_r_gate_without_input":
        prod[..., :H] = 0
    Gi_hi = prod if mut == "hi_b_ih_dropped" else prod + b
    hi = fwd(Whh_hi, bhh_hi, T, Bp, Gi=Gi_hi, h0=h0_hi, **kw)
    return dict(lo=lo, hi=hi)


def wave_ref(Whh_lo, bhh_lo, Wih_hi, bih_hi, Whh_hi, bhh_hi, T, Bp, P=None, ids=None, Gi=None, h0_lo=None,
             h0_hi=None, exact=False) -> Dict[str, Out]:
    """Two stacked layers in float64: lo = seq_ref.fwd_ref(...); Gi_hi[t] = bf16(h_lo(t+1)) . Wih_hi^T
    + b_ih; hi = seq_ref.fwd_ref(Gi = Gi_hi, ...).  Returns {"lo": .., "hi": ..} of fwd_ref's outputs."""
    return _wave(sr.fwd_ref, "HS", _ident if exact else bf16_round, torch.float64, Whh_lo, bhh_lo, Wih_hi, bih_hi,
                 Whh_hi, bhh_hi, T, Bp, P, ids, Gi, h0_lo, h0_hi, exact=exact)


def emulate_wave(Whh_lo, bhh_lo, Wih_hi, bih_hi, Whh_hi, bhh_hi, T, Bp, P=None, ids=None, Gi=None, h0_lo=None,
                 h0_hi=None, xring=0, mut=None) -> Dict[str, Out]:
    """The same with seq_ref.emulate_fwd (float32); hi's input is the emulator's own HSb of lo."""
    return _wave(sr.emulate_fwd, "HSb", _ident, torch.float32, Whh_lo, bhh_lo, Wih_hi, bih_hi, Whh_hi, bhh_hi, T, Bp,
                 P, ids, Gi, h0_lo, h0_hi, mut=mut, xring=xring)


# planted bugs the tolerances must catch: name -> (family of functions, mut)
MUTATIONS = {
    "fwd_b_hn_added_outside_r": ("fwd", "bhn_outside_r"),
    "fwd_k_fragment_dropped": ("fwd", "drop_k_fragment"),
    "fwd_blend_from_bf16_h_prev": ("fwd", "blend_from_bf16_hprev"),
    "fwd_fused_n_parts_summed_before_r": ("fwd_fused", "fused_n_summed_before_r"),
    "fwd_r_and_z_saves_swapped": ("fwd", "rz_saves_swapped"),
    "bwd_dgh_n_row_without_r": ("bwd", "dgh_n_without_r"),
    "bwd_carry_out_without_product": ("bwd", "carry_without_product"),
    "bwd_daz_with_z_for_one_minus_z": ("bwd", "daz_uses_z"),
    "wave_hi_reads_h_lo_one_step_stale": ("wave", "hi_reads_stale_h_lo"),
    "wave_hi_b_ih_dropped": ("wave", "hi_b_ih_dropped"),
    "wave_hi_r_gate_without_input_part": ("wave", "hi_r_gate_without_input"),
}


# ------------------------------------------------------------------------------ test inputs
# Seeded CPU generators (asymmetric operands, MFMA operands rounded to bf16), shared by the CPU
# measurement and the GPU tests.  Magnitudes are those of tests/test_kernels_gpu.py and seq_ref.
def fwd_step_inputs(H: int, Bp: int, Kin: int = 0, seed: int = 0, V: int = 256) -> Out:
    g = torch.Generator(device="cpu").manual_seed(3000 + seed)
    R = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    d = dict(Whh=bf16_round(R(3 * H, H, sc=H ** -0.5)), bhh=R(3 * H, sc=0.1), hprev=R(Bp, H, sc=0.5).clamp(-1, 1),
             P=R(V, 3 * H, sc=0.5), ids=torch.randint(0, V, (Bp,), generator=g, dtype=torch.int32),
             Gi=R(Bp, 3 * H, sc=0.5))
    if Kin:
        d.update(x=bf16_round(R(Bp, Kin)), Wih=bf16_round(R(3 * H, Kin, sc=Kin ** -0.5)), bih=R(3 * H, sc=0.1))
    return d


def fwd_step_kw(d: Out, mode: str) -> Out:
    """The input-projection arguments of fwd_step_ref / emulate_fwd_step for ``mode``."""
    if mode == "table":
        return dict(P=d["P"], ids=d["ids"])
    if mode == "gi":
        return dict(Gi=d["Gi"])
    return dict(x=d["x"], Wih=d["Wih"], bih=d["bih"])


def bwd_step_inputs(H: int, Bp: int, seed: int = 0) -> Out:
    """Saves drawn as test_bwd_step draws them (r, z in (0, 1), n in (-1, 1), gh_n ~ N(0, 1),
    h_prev = tanh(N(0, 1))).  dy, carry_in and dgh_next are drawn at scale 1, not test_bwd_step's 0.1:
    dh is then of order 1 and all but a few gate gradients lie orders of magnitude above the atol
    (a few 1e-7), so it is the relative bar of 2^-7 that decides, not the absolute one."""
    g = torch.Generator(device="cpu").manual_seed(4000 + seed)
    R = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    return dict(Whh=bf16_round(R(3 * H, H, sc=H ** -0.5)), dy=R(Bp, H), carry_in=R(Bp, H),
                dgh_next=bf16_round(R(Bp, 3 * H)), r=torch.sigmoid(R(Bp, H)), z=torch.sigmoid(R(Bp, H)),
                n=torch.tanh(R(Bp, H)), ghn=R(Bp, H), hprev=torch.tanh(R(Bp, H)))


def bwd_step_args(d: Out, first: bool):
    a = (d["dy"], d["r"], d["z"], d["n"], d["ghn"], d["hprev"], d["Whh"])
    return a, ({} if first else dict(dgh_next=d["dgh_next"], carry_in=d["carry_in"]))


def wave_inputs(H: int, Bp: int, T: int, seed: int = 0, V: int = 256) -> Out:
    g = torch.Generator(device="cpu").manual_seed(5000 + seed)
    R = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    W = lambda: bf16_round(R(3 * H, H, sc=H ** -0.5))
    return dict(Whh_lo=W(), Wih_hi=W(), Whh_hi=W(), bhh_lo=R(3 * H, sc=0.1), bih_hi=R(3 * H, sc=0.1),
                bhh_hi=R(3 * H, sc=0.1), P=R(V, 3 * H, sc=0.5),
                ids=torch.randint(0, V, (T, Bp), generator=g, dtype=torch.int32), Gi=R(T, Bp, 3 * H, sc=0.5),
                h0_lo=R(Bp, H, sc=0.5), h0_hi=R(Bp, H, sc=0.5))


def wave_kw(d: Out, T: int, Bp: int, mode: str, h0: str) -> Out:
    """Arguments of wave_ref / emulate_wave; h0 in {"none", "lo", "hi", "both"}."""
    kw = {k: d[k] for k in ("Whh_lo", "bhh_lo", "Wih_hi", "bih_hi", "Whh_hi", "bhh_hi")}
    kw.update(T=T, Bp=Bp, h0_lo=d["h0_lo"] if h0 in ("lo", "both") else None,
              h0_hi=d["h0_hi"] if h0 in ("hi", "both") else None)
    kw.update(dict(P=d["P"], ids=d["ids"]) if mode == "ids" else dict(Gi=d["Gi"]))
    return kw


# ------------------------------------------------------------------------------ case tables
# Forward step: (claimed kernel, H, Bp, input mode, Kin, algo, fwd64, colT offset).  The GPU test
# asserts the claimed kernel through fwd_step_variant.  colT = Bp + offset, ldT = 3 Bp + 64.
def _fwd_step_cases():
    cases = []
    for H in (64, 128, 512, 1024):                 # register-direct: ks 2 | ks 4, kb 1 | kb 2 | kb 4
        for Bp in (32, 96):
            cases += [("reg", H, Bp, "table", 0, 0, 1, 0), ("reg", H, Bp, "gi", 0, 0, 1, 0),
                      ("reg", H, Bp, "fused", H, 0, 1, 0)]
    cases += [("reg", 128, 96, "fused", 256, 0, 1, 0), ("reg", 1024, 32, "fused", 256, 0, 1, 0),
              ("reg", 512, 96, "fused", 64, 0, 1, 0)]          # Kin = 64: the loops that shrink ks and kb
    for f64, name in ((1, "lds64"), (0, "lds128")):
        for H, Bp in ((256, 128), (320, 256)):
            cases += [(name, H, Bp, "table", 0, 2, f64, 0), (name, H, Bp, "gi", 0, 2, f64, 0),
                      (name, H, Bp, "fused", H, 2, f64, 0), (name, H, Bp, "fused", 64, 2, f64, 0)]
    cases += [("lds128", 2048, 1024, "table", 0, 0, 1, 0), ("lds128", 2048, 1024, "fused", 256, 0, 1, 0)]
    cases += [("big", 1024, 4096, "fused", 64, 0, 1, 0), ("big", 1024, 4096, "fused", 1024, 0, 1, 0),
              ("lds128", 1024, 3840, "fused", 64, 0, 1, 0)]    # the neighbour must not take the big tile
    cases += [("reg", 1024, 512, "gi", 0, 0, 1, 4)]            # colT % 8 != 0: algo 0 falls to the register tile
    return cases


FWD_STEP_CASES = _fwd_step_cases()
# Backward step: (claimed kernel, H, Bp, algo).  The split-K rows name the kernel gru_bwd_step_sk_splits
# picks on a 256-CU device with one workgroup per CU; the GPU test asks the device.
BWD_STEP_CASES = ([("reg", H, Bp, 0) for H in (128, 256, 512, 1024) for Bp in (32, 96)] +
                  [("lds8", 256, 128, 2), ("lds8", 320, 256, 2), ("lds8", 1024, 128, 2)] +
                  [("sk4", 1024, 768, 0), ("sk2", 1024, 1536, 0), ("sk2", 1280, 1536, 0)])
# Wavefront shapes (H, Bp) and the longest T of tests/test_wave_kernel_gpu.py
WAVE_SHAPES = [(256, 64), (256, 96), (256, 256), (512, 64), (512, 96), (512, 256), (1024, 64), (1024, 96),
               (1024, 128), (1024, 256)]
WAVE_T = 9


# ------------------------------------------------------------------------------ measurement
def fwd_step_case(H, Bp, mode, Kin, seed, mut=None, device="cpu"):
    d = {k: v.to(device) for k, v in fwd_step_inputs(H, Bp, Kin, seed).items()}
    kw = fwd_step_kw(d, mode)
    return (emulate_fwd_step(d["Whh"], d["bhh"], d["hprev"], mut=mut, **kw),
            fwd_step_ref(d["Whh"], d["bhh"], d["hprev"], **kw))


def bwd_step_case(H, Bp, first, seed, mut=None, device="cpu"):
    d = {k: v.to(device) for k, v in bwd_step_inputs(H, Bp, seed).items()}
    a, kw = bwd_step_args(d, first)
    return emulate_bwd_step(*a, mut=mut, **kw), bwd_step_ref(*a, **kw)


def wave_case(H, Bp, T, mode, h0, seed, xring=0, mut=None, device="cpu"):
    d = {k: v.to(device) for k, v in wave_inputs(H, Bp, T, seed).items()}
    kw = wave_kw(d, T, Bp, mode, h0)
    return emulate_wave(xring=xring, mut=mut, **kw), wave_ref(**kw)


_FWD_FAMILY = {k: "f32_state" for k in ("h", "r", "z", "n", "ghn")}
_BWD_FAMILY = {"carry_out": "f32_carry", "dgh": "bf16_grad", "dgi": "bf16_grad"}
_WAVE_KEYS = ("HS", "r", "z", "n", "ghn")


def step_pairs(emu: Out, ref: Out, families):
    for k, fam in families.items():
        yield k, fam, emu[k], ref[k]


def wave_pairs(emu, ref):
    for ly in ("lo", "hi"):
        for k in _WAVE_KEYS:
            yield f"{ly}.{k}", "wave_f32_state", emu[ly][k], ref[ly][k]


def _fold(out, pairs):
    for _, fam, a, b in pairs:
        out[fam] = max(out.get(fam, 0.0), deviation(a, b, RTOL[fam]))


def measure_deviations(seeds=(0, 1, 2), fwd_cases=None, bwd_cases=None, wave_shapes=None, verbose=False):
    """Largest deviation emulator - reference per family over the GPU case tables and ``seeds``."""
    out: Dict[str, float] = {}
    say = (lambda *a: print(*a, flush=True)) if verbose else (lambda *a: None)
    for seed in seeds:
        seen = set()
        for _, H, Bp, mode, Kin, *_ in (FWD_STEP_CASES if fwd_cases is None else fwd_cases):
            if (H, Bp, mode, Kin) not in seen:
                seen.add((H, Bp, mode, Kin))
                _fold(out, step_pairs(*fwd_step_case(H, Bp, mode, Kin, seed), _FWD_FAMILY))
                say("fwd", H, Bp, mode, Kin, seed, f"{out['f32_state']:.3e}")
        for _, H, Bp, _ in (BWD_STEP_CASES if bwd_cases is None else bwd_cases):
            for first in (True, False):
                _fold(out, step_pairs(*bwd_step_case(H, Bp, first, seed), _BWD_FAMILY))
            say("bwd", H, Bp, seed, f"{out['f32_carry']:.3e} {out['bf16_grad']:.3e}")
        for H, Bp in (WAVE_SHAPES if wave_shapes is None else wave_shapes):
            for mode, h0 in (("ids", "both"), ("gi", "none")):
                emu, ref = wave_case(H, Bp, WAVE_T, mode, h0, seed)
                _fold(out, wave_pairs(emu, ref))
                lo = max(deviation(emu["lo"][k], ref["lo"][k]) for k in _WAVE_KEYS)
                out["wave_lo_f32_state"] = max(out.get("wave_lo_f32_state", 0.0), lo)
            say("wave", H, Bp, seed, f"{out['wave_f32_state']:.3e} lo {out['wave_lo_f32_state']:.3e}")
    return out


if __name__ == "__main__":
    for k, v in measure_deviations(verbose=True).items():
        print(f'    "{k}": {v:.3e},')

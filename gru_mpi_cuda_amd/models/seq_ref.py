"""Per-element reference of the persistent sequence kernels (gru_seq.hip, gru_seq16.hip,
gru_seq_big.hip): one GRU layer over T steps, forward and BPTT, in plain torch.

Three things live here, next to ``cpu_ref.py`` (the whole-model oracle):

* ``fwd_ref`` / ``bwd_ref``: float64, in the kernels' *exchange precision* -- the operand that
  crosses workgroups (h_{t-1} forward, dGh_{t+1} backward) and the weight-gradient operands are
  rounded to bf16 as the kernels round them, everything else (carried state, gate math, bias
  sums) stays unrounded.  ``exact=True`` turns the rounding off: the result is then plain BPTT
  and must equal ``torch.autograd`` (tests/test_seq_ref.py).
* ``emulate_fwd`` / ``emulate_bwd``: the same recurrences in float32 with every value the
  kernels store as bf16 rounded there, the exchange modelled as an explicit ring of slots, and
  a ``mut`` hook that plants one of the bugs the tolerances must catch.  It is the CPU stand-in
  for "a correct kernel"; its deviation from the reference is what the tolerances are made of.
* pure-index decoders (and their inverses) of the tiled layouts documented in kernels.h.

Every function runs on the device of its inputs, so a GPU test may evaluate the float64
reference with torch on the device while the CPU tests run it on the host.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

Out = Dict[str, torch.Tensor]


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    """x rounded to bf16 (round-to-nearest-even from fp32, as f2bf in common.h), in x's dtype."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def _ident(x: torch.Tensor) -> torch.Tensor:
    return x


# ------------------------------------------------------------------------------ tolerances
# The comparison is |got - ref| <= ATOL + RTOL |ref| per output family:
#   fp32 state and saves : HSf, r, z, n, gh_n                      (forward)
#   bf16 copies          : HSb, HT, HF, packed saves               (forward)
#   bf16 gate gradients  : dgi, dghT, dgiT                         (backward)
#   fp32 partial sums    : dbhh / dbih / dWhh / dP partials        (backward)
# bf16-stored outputs get rtol = 2^-7 (two bf16 ulps: the rounding of the stored value); fp32
# outputs get no rtol.
RTOL = {"f32_state": 0.0, "bf16_copy": 2.0 ** -7, "bf16_grad": 2.0 ** -7, "f32_part": 0.0}
# Measured, not guessed: ``python -m gru_mpi_cuda_amd.models.seq_ref`` (measure_deviations below)
# runs, on the CPU, every shape of tests/test_seq_kernels_gpu.py (FWD_SHAPES at T = 9, table and
# Gi input; BWD_SHAPES at their longest T, 32- and 16-row blocks, fp32 and packed saves, with and
# without the fused dy) for seeds 0, 1, 2 and takes the largest deviation emulate - ref of each
# family: the largest |emulate - ref| - RTOL |ref|, i.e. what is left for atol once rtol has
# taken the rounding of the stored value.  (For the fp32 families, RTOL = 0, that is the largest
# |emulate - ref| itself.  For the bf16 families the plain largest |emulate - ref|, MEASURED_RAW,
# is the bf16 rounding of the largest value -- 2^-9 x 4 for gh_n, 2^-9 x 1 for a gate gradient --
# and an atol of 4 x that would pass a gate gradient that is a third off.)  The fp32 deviations
# are not fp32 rounding: where the fp32 and the fp64 value of an exchanged operand straddle a bf16
# rounding boundary the two runs exchange different values, and those flips compound over the steps;
# the fp32 partial sums' worst case is one such flip in a dP bucket that holds a single token.
# tests/test_seq_ref.py re-measures the quick shapes against these numbers and checks that every
# planted bug (MUTATIONS) fails at the resulting tolerances.
MEASURED_DEV = {
    "f32_state": 1.36e-03,
    "bf16_copy": 1.27e-03,
    "bf16_grad": 1.36e-04,
    "f32_part": 1.96e-03,
}
MEASURED_RAW = {   # largest |emulate - ref| without rtol's share, for the record
    "f32_state": 1.36e-03,
    "bf16_copy": 7.80e-03,
    "bf16_grad": 1.91e-03,
    "f32_part": 1.96e-03,
}
# atol = 4 x the measured deviation: the margin covers the MFMA summation order (and the bf16
# roundings it flips), which the emulator does not reproduce.  (The recorded figures are the
# measured ones rounded up to three digits.)
ATOL = {k: 4.0 * v for k, v in MEASURED_DEV.items()}
# h = n + z (h_prev - n) recomputed in fp32 from the kernel's own fp32 saves against its HSf:
# three fp32 operations on magnitudes < 2 (each within 2^-24 * 2 = 1.2e-7, contracted or not),
# so 4e-7 at most; 1e-6 leaves room for nothing else.
F32_BLEND_ATOL = 1e-6


def deviation(got: torch.Tensor, ref: torch.Tensor, rtol: float = 0.0) -> float:
    """Largest |got - ref| - rtol |ref|, floored at 0: the atol the comparison needs once rtol has
    taken its share (inf when got holds a NaN).  rtol = 0 gives the plain largest |got - ref|."""
    r = ref.to(torch.float64)
    d = (got.to(torch.float64) - r).abs() - rtol * r.abs()
    if torch.isnan(d).any():
        return float("inf")
    return max(float(d.max()), 0.0) if d.numel() else 0.0


def mismatch(got: torch.Tensor, ref: torch.Tensor, family: str, ATOL=None, RTOL=None) -> Optional[str]:
    """None when |got - ref| <= ATOL[family] + RTOL[family] |ref| everywhere, else a description
    of the worst element.  A NaN in ``got`` is a mismatch.  ATOL / RTOL: another module's tables
    (step_ref's families) instead of the ones above."""
    ATOL = globals()["ATOL"] if ATOL is None else ATOL
    RTOL = globals()["RTOL"] if RTOL is None else RTOL
    g, r = got.to(torch.float64), ref.to(torch.float64)
    if g.shape != r.shape:
        return f"shape {tuple(g.shape)} vs reference {tuple(r.shape)}"
    d = (g - r).abs()
    bad = ~(d <= ATOL[family] + RTOL[family] * r.abs())
    if not bool(bad.any()):
        return None
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    i = int(torch.argmax(torch.where(bad, d, torch.full_like(d, -1.0))))
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), d.shape))
    return (f"{int(bad.sum())} of {bad.numel()} elements off ({family}: atol {ATOL[family]:.3g}, rtol "
            f"{RTOL[family]:.3g}); worst at {idx}: got {float(g[idx]):.6g}, reference {float(r[idx]):.6g}")


def assert_close(got: torch.Tensor, ref: torch.Tensor, family: str, what: str = "", ATOL=None, RTOL=None) -> None:
    m = mismatch(got, ref, family, ATOL, RTOL)
    assert m is None, f"{what}: {m}"


# ------------------------------------------------------------------------------ layout decoders
def hf_decode(HF: torch.Tensor, T1: int, Bp: int, H: int) -> torch.Tensor:
    """SeqFwdArgs::HF -> [T1][Bp][H].  Block (t, unit tile u, row block rb) of 512 elements at
    ((t * H/16 + u) * Bp/32 + rb) * 512; lane l's 8 elements are unit 16u + (l & 15), rows
    32rb + 8(l >> 4) .. +8."""
    v = HF.reshape(T1, H // 16, Bp // 32, 4, 16, 8)          # [t][u][rb][l >> 4][l & 15][e]
    return v.permute(0, 2, 3, 5, 1, 4).reshape(T1, Bp, H)    # [t][rb][l >> 4][e][u][l & 15]


def hf_encode(HS: torch.Tensor) -> torch.Tensor:
    """Inverse of hf_decode: [T1][Bp][H] -> flat HF."""
    T1, Bp, H = HS.shape
    v = HS.reshape(T1, Bp // 32, 4, 8, H // 16, 16)
    return v.permute(0, 4, 1, 2, 5, 3).contiguous().reshape(-1)


def s16_decode(s16: torch.Tensor) -> Tuple[torch.Tensor, ...]:
    """Packed saves [T][Bp][H][4] (st_save16 in common.h: r | z << 16, n | gh_n << 16, little
    endian) -> (r, z, n, gh_n), each [T][Bp][H]."""
    return tuple(s16[..., k] for k in range(4))


def s16_encode(r: torch.Tensor, z: torch.Tensor, n: torch.Tensor, ghn: torch.Tensor) -> torch.Tensor:
    return torch.stack([r, z, n, ghn], -1).to(torch.bfloat16).contiguous()


def ht_decode(HT: torch.Tensor, T1: int, Bp: int) -> torch.Tensor:
    """Transposed copy [rows][ld] with step t at columns t * Bp .. -> [T1][Bp][rows]; the pad
    columns beyond T1 * Bp are dropped."""
    rows = HT.shape[0]
    return HT[:, :T1 * Bp].reshape(rows, T1, Bp).permute(1, 2, 0)


def ht_encode(X: torch.Tensor, ld: int, fill: float = float("nan")) -> torch.Tensor:
    """Inverse of ht_decode with the pad columns set to ``fill``."""
    T1, Bp, rows = X.shape
    out = torch.full((rows, ld), fill, dtype=X.dtype, device=X.device)
    out[:, :T1 * Bp] = X.permute(2, 0, 1).reshape(rows, T1 * Bp)
    return out


# ------------------------------------------------------------------------------ forward
def _gates(gi, gh, hp):
    """The gate formulas of _gates_ref in tests/test_kernels_gpu.py."""
    H = hp.shape[1]
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    return n + z * (hp - n), r, z, n, gh[:, 2 * H:]


def _fwd(Whh, bhh, T, Bp, P, ids, Gi, h0, dtype, rnd, xring=0, mut=None) -> Out:
    H = Whh.shape[1]
    dev = Whh.device
    W, b = Whh.to(dtype), bhh.to(dtype)
    h = torch.zeros(Bp, H, dtype=dtype, device=dev) if h0 is None else h0.to(dtype)
    xr = xring if xring >= 2 else max(T, 1)
    xch = torch.zeros(xr, Bp, H, dtype=dtype, device=dev)     # slot t % xr holds bf16(h_t)
    hist = [rnd(h)]                                           # exchange operand of every step so far
    HS, sv = [h], [[], [], [], []]
    kind = mut[0] if mut else None
    for t in range(T):
        gi = (P[ids[t].long()] if ids is not None else Gi[t]).to(dtype)
        if t == 0:
            op = rnd(h)
            if kind == "no_h0":                               # (h) h0 left out of step 0's product
                op = torch.zeros_like(op)
        else:
            op = xch[(t - 1) % xr].clone()
            if kind == "stale_tile" and t == mut[1]:          # (g) one 16-unit tile reads h_{t-2}
                u = mut[2]
                op[:, 16 * u:16 * u + 16] = hist[t - 1][:, 16 * u:16 * u + 16]
        gh = op @ W.T + b
        h, r, z, n, ghn = _gates(gi, gh, h)
        xch[t % xr] = rnd(h)
        hist.append(rnd(h))
        HS.append(h)
        for lst, v in zip(sv, (r, z, n, ghn)):
            lst.append(v)
    st = lambda l: torch.stack(l) if l else torch.zeros(0, Bp, H, dtype=dtype, device=dev)
    return dict(HS=torch.stack(HS), r=st(sv[0]), z=st(sv[1]), n=st(sv[2]), ghn=st(sv[3]))


def fwd_ref(Whh, bhh, T, Bp, P=None, ids=None, Gi=None, h0=None, exact=False) -> Out:
    """One GRU layer over T steps in float64.  Whh [3H][H] holds bf16 values; the input
    projection is P[ids[t]] (P [V][3H], ids [T][Bp]) or Gi[t] ([T][Bp][3H]); h0 [Bp][H] optional.
    The recurrent operand is bf16(h_{t-1}); the carried state and the gate math are unrounded.
    Returns HS [T+1][Bp][H] (HS[0] = h0) and r, z, n, ghn [T][Bp][H]."""
    assert (ids is None) != (Gi is None)
    return _fwd(Whh, bhh, T, Bp, P, ids, Gi, h0, torch.float64, _ident if exact else bf16_round)


def emulate_fwd(Whh, bhh, T, Bp, P=None, ids=None, Gi=None, h0=None, xring=0, mut=None) -> Out:
    """fwd_ref's recurrence as a correct kernel computes it: float32, the h exchange as a ring
    of ``xring`` slots, plus the bf16-stored outputs (HSb, and the packed saves r16 .. ghn16)."""
    o = _fwd(Whh, bhh, T, Bp, P, ids, Gi, h0, torch.float32, bf16_round, xring, mut)
    o["HSb"] = bf16_round(o["HS"])
    for k in ("r", "z", "n", "ghn"):
        o[k + "16"] = bf16_round(o[k])
    return o


# ------------------------------------------------------------------------------ backward
def _bwd(dy, r, z, n, ghn, HS, Whh, ids, V, dl, Wfc, rows, fuse_w, dtype, rnd, rnd_out, xring=0, mut=None) -> Out:
    T, Bp, H = r.shape
    dev = r.device
    W = Whh.to(dtype)                                          # [3H][H]: dh = dGh . W_hh
    c = lambda x: x.to(dtype)
    if dl is not None:                                         # fused dy = dl . W_fc
        dy = (c(dl) @ c(Wfc)).reshape(T, Bp, H)
    nrb = Bp // rows
    xr = xring if xring >= 2 else max(T, 1)
    xch = torch.zeros(xr, Bp, 3 * H, dtype=dtype, device=dev)  # slot t % xr holds bf16(dGh_t)
    kind = mut[0] if mut else None
    carry = torch.zeros(Bp, H, dtype=dtype, device=dev)
    dbhh = torch.zeros(nrb, 3 * H, dtype=dtype, device=dev)
    dbih = torch.zeros_like(dbhh)
    dW = torch.zeros(nrb, 3 * H, H, dtype=dtype, device=dev) if fuse_w else None
    dP = torch.zeros(nrb, V, 3 * H, dtype=dtype, device=dev) if ids is not None else None
    dgi_all, dgh_all = [None] * T, [None] * T
    for t in range(T - 1, -1, -1):
        dh = c(dy[t]) + (torch.zeros_like(carry) if kind == "drop_carry" and t == mut[1] else carry)
        if t < T - 1:
            src = xch[(t + 1) % xr]
            if kind == "stale_block":                          # (a) one row block reads slot t, not t + 1
                src = src.clone()
                rb = mut[1]
                src[rb * rows:(rb + 1) * rows] = xch[t % xr][rb * rows:(rb + 1) * rows]
            dh = dh + src @ W
        rt, zt, nt, gt, hp = c(r[t]), c(z[t]), c(n[t]), c(ghn[t]), c(HS[t])
        dn = dh * (1 - zt)
        dz = dh * (hp - nt)
        dan = dn * (1 - nt * nt)
        dar = dan * gt * rt * (1 - rt)
        daz = dz * zt * (1 - zt)
        dgh = torch.cat([dar, daz, dan * rt], 1)
        dgi = torch.cat([dar, daz, dan * rt if kind == "dgi_n_times_r" else dan], 1)   # (e)
        carry = zt * dh
        # (b) the ring slot reused one step early: the write of step t lands in step t - 1's slot
        xch[((t - 1) if kind == "early_reuse" else t) % xr] = rnd(dgh)
        bh, bi = dgh.reshape(nrb, rows, 3 * H).sum(1), dgi.reshape(nrb, rows, 3 * H).sum(1)
        if kind == "skip_block_partials":                      # (d) one row block missing from the sums
            bh[mut[1]] = 0
            bi[mut[1]] = 0
        dbhh += bh
        dbih += bi
        if dW is not None and not (kind == "dw_skip_last" and t == T - 1):   # (f)
            dW += torch.bmm(rnd(dgh).reshape(nrb, rows, 3 * H).transpose(1, 2), rnd(hp).reshape(nrb, rows, H))
        if dP is not None:
            oh = torch.nn.functional.one_hot(ids[t].long(), V).to(dtype).reshape(nrb, rows, V)
            if kind == "skip_block_partials":
                oh[mut[1]] = 0
            dP += torch.bmm(oh.transpose(1, 2), rnd(dgi).reshape(nrb, rows, 3 * H))
        dgi_all[t], dgh_all[t] = rnd_out(dgi), rnd_out(dgh)
    out = dict(dgi=torch.stack(dgi_all), dgh=torch.stack(dgh_all), dbhh_part=dbhh, dbih_part=dbih,
               dh0=carry + dgh @ W, dy=dy)
    if dW is not None:
        out["dWhh_part"] = dW
    if dP is not None:
        out["dP_part"] = dP
    return out


def bwd_ref(dy, r, z, n, ghn, HS, Whh, ids=None, V=0, dl=None, Wfc=None, rows=32, fuse_w=True, exact=False) -> Out:
    """BPTT of one layer in float64 from given saves -- exactly what gru_bwd_seq_kernel computes.
    dy, r, z, n, ghn [T][Bp][H], HS [T+1][Bp][H] (HS[t] = h_{t-1}), Whh [3H][H] bf16 values.  For
    t = T-1 .. 0: dh = dy_t + carry + bf16(dGh_{t+1}) . W_hh (no product at t = T-1), dn = dh(1-z),
    dz = dh(h_{t-1} - n), dan = dn(1 - n^2), dar = dan gh_n r(1-r), daz = dz z(1-z),
    dGh_t = [dar, daz, dan r], dGi_t = [dar, daz, dan], carry = z dh.  Returns, unrounded:
    dgi, dgh [T][Bp][3H]; per ``rows``-row block (summing to the full gradient) dbhh_part,
    dbih_part [Bp/rows][3H] over the unrounded gate gradients, dWhh_part [Bp/rows][3H][H] =
    sum_t bf16(dGh_t)^T bf16(h_{t-1}) and, with ids [T][Bp], dP_part [Bp/rows][V][3H] =
    sum over (t, b) with ids = v of bf16(dGi_t[b]); dh0; and the dy it used.  With dl
    [T*Bp][V] and Wfc [V][H] (bf16 values) dy = dl . W_fc instead."""
    rnd = _ident if exact else bf16_round
    return _bwd(dy, r, z, n, ghn, HS, Whh, ids, V, dl, Wfc, rows, fuse_w, torch.float64, rnd, _ident)


def emulate_bwd(dy, r, z, n, ghn, HS, Whh, ids=None, V=0, dl=None, Wfc=None, rows=32, fuse_w=True, xring=0,
                mut=None) -> Out:
    """bwd_ref's recurrence as a correct kernel computes it: float32, dgi / dgh rounded to bf16
    as stored, the dGh exchange as a ring of ``xring`` slots."""
    return _bwd(dy, r, z, n, ghn, HS, Whh, ids, V, dl, Wfc, rows, fuse_w, torch.float32, bf16_round, bf16_round,
                xring, mut)


# planted bugs the tolerances must catch: name -> (direction, mut builder from (T, Bp, H))
MUTATIONS = {
    "a_stale_exchange_slot_one_row_block": ("bwd", lambda T, Bp, H: ("stale_block", Bp // 32 - 1)),
    "b_ring_slot_reused_one_step_early": ("bwd", lambda T, Bp, H: ("early_reuse",)),
    "c_carry_dropped_at_one_step": ("bwd", lambda T, Bp, H: ("drop_carry", T // 2)),
    "d_row_block_missing_from_partials": ("bwd", lambda T, Bp, H: ("skip_block_partials", Bp // 32 - 1)),
    "e_dgi_n_rows_hold_dan_r": ("bwd", lambda T, Bp, H: ("dgi_n_times_r",)),
    "f_dwhh_skips_last_step": ("bwd", lambda T, Bp, H: ("dw_skip_last",)),
    "g_fwd_tile_reads_h_two_steps_back": ("fwd", lambda T, Bp, H: ("stale_tile", T // 2, H // 16 - 1)),
    "h_fwd_h0_left_out_of_step_0": ("fwd", lambda T, Bp, H: ("no_h0",)),
}


# ------------------------------------------------------------------------------ test inputs
# Seeded CPU generators in the style of tests/test_kernels_gpu.py (asymmetric operands, MFMA
# operands rounded to bf16), shared by the CPU tolerance measurement and the GPU tests so both
# see the same numbers.
def fwd_inputs(H: int, Bp: int, T: int, seed: int = 0, V: int = 256) -> Out:
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    R = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    return dict(Whh=bf16_round(R(3 * H, H, sc=H ** -0.5)), bhh=R(3 * H, sc=0.1), P=R(V, 3 * H, sc=0.5),
                ids=torch.randint(0, V, (T, Bp), generator=g, dtype=torch.int32), Gi=R(T, Bp, 3 * H, sc=0.5),
                h0=R(Bp, H, sc=0.5))


def char_ids(T: int, Bp: int, g: torch.Generator, one: bool = False) -> torch.Tensor:
    """Char-like ids [T][Bp]: lower-case letters, id 0 every 17th (end of name / padding), and a
    heavy bucket of 48 consecutive tokens (one and a half 32-row blocks) with id 7."""
    if one:
        return torch.full((T, Bp), 101, dtype=torch.int32)
    ids = torch.randint(97, 123, (T * Bp,), generator=g, dtype=torch.int32)
    ids[::17] = 0
    ids[:48] = 7
    return ids.reshape(T, Bp)


def bwd_inputs(H: int, Bp: int, T: int, seed: int = 0, V: int = 256, one_id: bool = False,
               grad_scale: float = 0.1) -> Out:
    """Saves drawn as test_bwd_step draws them: r, z in (0, 1), n in (-1, 1), gh_n ~ N(0, 1),
    HS = tanh(N(0, 1)), dy ~ 0.1 N(0, 1); dl / Wfc for the fused dy give a dy of the same size."""
    g = torch.Generator(device="cpu").manual_seed(2000 + seed)
    R = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    d = dict(Whh=bf16_round(R(3 * H, H, sc=H ** -0.5)), dy=R(T, Bp, H, sc=grad_scale),
             r=torch.sigmoid(R(T, Bp, H)), z=torch.sigmoid(R(T, Bp, H)), n=torch.tanh(R(T, Bp, H)),
             ghn=R(T, Bp, H), HS=torch.tanh(R(T + 1, Bp, H)))
    d["ids"] = char_ids(T, Bp, g, one_id)
    d["dl"] = bf16_round(R(T * Bp, V, sc=grad_scale * (H / V) ** 0.5))
    d["Wfc"] = bf16_round(R(V, H, sc=H ** -0.5))
    return d


def bwd_inputs_s16(d: Out) -> Out:
    """The same inputs with the four saves rounded to bf16 (what a packed-saves kernel reads)."""
    e = dict(d)
    for k in ("r", "z", "n", "ghn"):
        e[k] = bf16_round(d[k])
    return e


# shapes of tests/test_seq_kernels_gpu.py (the tolerance measurement covers all of them)
FWD_SHAPES = [(256, 64), (256, 96), (512, 64), (512, 256), (1024, 128)]
FWD_T = 9
# (H, Bp, T, rows per block, fused dy)
BWD_SHAPES = [(256, 64, 7, 32, False), (256, 256, 7, 32, False), (512, 64, 7, 32, False), (512, 256, 7, 32, False),
              (1024, 64, 7, 32, False), (1024, 128, 7, 32, False), (1024, 128, 5, 16, False),
              (1024, 80, 5, 16, False), (1024, 1024, 3, 32, False), (2048, 512, 3, 32, False),
              (1024, 1024, 3, 32, True), (2048, 512, 3, 32, True)]

_FWD_FAMILY = {"HS": "f32_state", "r": "f32_state", "z": "f32_state", "n": "f32_state", "ghn": "f32_state",
               "HSb": "bf16_copy", "r16": "bf16_copy", "z16": "bf16_copy", "n16": "bf16_copy", "ghn16": "bf16_copy"}
_BWD_FAMILY = {"dgi": "bf16_grad", "dgh": "bf16_grad", "dbhh_part": "f32_part", "dbih_part": "f32_part",
               "dWhh_part": "f32_part", "dP_part": "f32_part"}


def fwd_pairs(emu: Out, ref: Out):
    """(name, family, emulated / kernel value, reference value) of every forward output."""
    for k, fam in _FWD_FAMILY.items():
        yield k, fam, emu[k], ref["HS" if k == "HSb" else k[:-2] if k.endswith("16") else k]


def bwd_pairs(emu: Out, ref: Out):
    for k, fam in _BWD_FAMILY.items():
        if k in emu and k in ref:
            yield k, fam, emu[k], ref[k]


def fwd_case_deviation(H, Bp, T, seed, mode="ids", use_h0=True, xring=0, mut=None, device="cpu") -> Dict[str, float]:
    d = {k: v.to(device) for k, v in fwd_inputs(H, Bp, T, seed).items()}
    kw = dict(P=d["P"], ids=d["ids"]) if mode == "ids" else dict(Gi=d["Gi"])
    h0 = d["h0"] if use_h0 else None
    ref = fwd_ref(d["Whh"], d["bhh"], T, Bp, h0=h0, **kw)
    emu = emulate_fwd(d["Whh"], d["bhh"], T, Bp, h0=h0, xring=xring, mut=mut, **kw)
    dev: Dict[str, float] = {}
    for _, fam, a, b in fwd_pairs(emu, ref):
        dev[fam] = max(dev.get(fam, 0.0), deviation(a, b, RTOL[fam]))
        dev[fam + "_raw"] = max(dev.get(fam + "_raw", 0.0), deviation(a, b))
    return dev


def bwd_case(H, Bp, T, seed, rows=32, fdy=False, s16=False, fuse_w=None, xring=0, mut=None, one_id=False,
             grad_scale=0.1, device="cpu") -> Tuple[Out, Out]:
    """(emulated, reference) backward outputs of one generated case."""
    d = bwd_inputs(H, Bp, T, seed, one_id=one_id, grad_scale=grad_scale)
    if s16 or fdy:
        d = bwd_inputs_s16(d)
    d = {k: v.to(device) for k, v in d.items()}
    fw = (rows == 32 and H <= 512) if fuse_w is None else fuse_w
    big = H >= 2048 or Bp >= 512
    kw = dict(ids=None if big else d["ids"], V=256, rows=rows, fuse_w=fw)
    if fdy:
        kw.update(dl=d["dl"], Wfc=d["Wfc"])
    args = (None if fdy else d["dy"], d["r"], d["z"], d["n"], d["ghn"], d["HS"], d["Whh"])
    return emulate_bwd(*args, xring=xring, mut=mut, **kw), bwd_ref(*args, **kw)


def bwd_case_deviation(*a, **kw) -> Dict[str, float]:
    emu, ref = bwd_case(*a, **kw)
    dev: Dict[str, float] = {}
    for _, fam, x, y in bwd_pairs(emu, ref):
        dev[fam] = max(dev.get(fam, 0.0), deviation(x, y, RTOL[fam]))
        dev[fam + "_raw"] = max(dev.get(fam + "_raw", 0.0), deviation(x, y))
    return dev


def measure_deviations(seeds=(0, 1, 2), fwd_shapes=None, bwd_shapes=None, verbose=False) -> Dict[str, float]:
    """Largest |emulate - ref| per output family over the GPU test shapes and ``seeds``."""
    out: Dict[str, float] = {}

    def take(dev, tag):
        for k, v in dev.items():
            out[k] = max(out.get(k, 0.0), v)
        if verbose:
            print(tag, {k: f"{v:.3e}" for k, v in dev.items()}, flush=True)

    for seed in seeds:
        for H, Bp in (FWD_SHAPES if fwd_shapes is None else fwd_shapes):
            for mode, use_h0 in (("ids", True), ("gi", False)):
                take(fwd_case_deviation(H, Bp, FWD_T, seed, mode, use_h0), f"fwd H={H} Bp={Bp} {mode} seed={seed}")
        for H, Bp, T, rows, fdy in (BWD_SHAPES if bwd_shapes is None else bwd_shapes):
            for s16 in ((True,) if fdy else (False, True)):
                take(bwd_case_deviation(H, Bp, T, seed, rows=rows, fdy=fdy, s16=s16),
                     f"bwd H={H} Bp={Bp} T={T} rows={rows} fdy={fdy} s16={s16} seed={seed}")
    return out


if __name__ == "__main__":
    res = measure_deviations(verbose=True)
    for k, v in res.items():
        print(f'    "{k}": {v:.3e},')

"""Per-element reference of the FC / softmax-xent head (fc.hip: fc_xent, fc_xent_v256, fc_xent_fl,
softmax_xent, fc_sample; gru_seq.hip: the FC consumers of gru_fwd_seq_fc), in plain torch, in the
style of ``seq_ref.py``.

* ``head_ref``: float64 -- logits, probs, per-row nll, per-32-row loss partials, dl = (softmax -
  onehot) * inv on the labelled rows, dy = dl . W and, given T / Bp, the per-row-block dW / db.
  It equals ``torch.autograd`` of ``cross_entropy(sum) * inv`` (tests/test_head_ref.py).
* ``emulate``: the same head in float32 with the kernels' rounding points, in two forms: ``dl``
  (fc_xent, fc_xent_v256, softmax_xent, the FC consumers: dy = bf16(dl) . W) and ``flash``
  (fc_xent_fl: online softmax over 64-column chunks, dy = scale (U / s - W[y])).  A ``mut`` hook
  plants one of the bugs the tolerances must catch (MUTATIONS).  It is the CPU stand-in for "a
  correct kernel"; its deviation from the reference is what the measured tolerances are made of.
* pure-index encoders / decoders of the dl^T window and of the dlF fragment blocks.
* seeded inputs: random ones, and *planted* ones whose per-row logits are set exactly through a
  one-hot selector in the first 32 hidden units (planted_inputs).

Everything that scales with 1 / count is compared in the normalised domain (divided by inv in
float64), so one number serves every M.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from .seq_ref import bf16_round, deviation

Out = Dict[str, torch.Tensor]

# ------------------------------------------------------------------------------ tolerances
# |got - ref| <= ATOL + RTOL |ref| per element, got and ref divided by inv (probs: as they are).
#   dl       : dl, dlT, dlF (bf16) against the float64 dl.  rtol = two bf16 ulps, the rounding of the
#              stored value; atol never under 2^-20: the emulator's exact exp and division carry
#              none of the error of __expf / v_rcp_f32 (about 1e-7 of a probability near 1).
#   loss     : per-32-row loss partials (fp32)
#   probs    : fc_sample's probabilities (fp32), not normalised
#   dy       : dy end to end for the dl form: float64 dy against bf16(dl) . W in fp32
#   dy_flash : dy end to end for the flash form
RTOL = {"dl": 2.0 ** -7, "loss": 0.0, "probs": 0.0, "dy": 0.0, "dy_flash": 0.0}
# Measured, not guessed: ``python -m gru_mpi_cuda_amd.models.head_ref`` (measure_deviations below)
# runs, on the CPU, every case of tests/test_head_gpu.py (the shape lists below, planted and random
# inputs) for seeds 0, 1, 2 and takes the largest |emulate - ref| - RTOL |ref| of each family.  The
# dy figures are the bf16 rounding of dl (and, flash, of e) carried through the product with W; the
# loss and probs figures are fp32 rounding of logits as large as 200.  (The recorded figures are the
# measured ones rounded up to three digits.)
MEASURED_DEV = {
    "dl": 5.00e-10,
    "loss": 3.97e-05,
    "probs": 6.13e-06,
    "dy": 1.65e-03,
    "dy_flash": 4.68e-05,
}
DL_ATOL_FLOOR = 2.0 ** -20
# atol = 4 x the measured deviation (the margin covers the MFMA summation order and the fast exp /
# reciprocal, which the emulator does not reproduce)
ATOL = {k: 4.0 * v for k, v in MEASURED_DEV.items()}
ATOL["dl"] = max(ATOL["dl"], DL_ATOL_FLOOR)

# shapes of tests/test_head_gpu.py (the tolerance measurement covers all of them), M = 64
XENT_SHAPES = [(64, 32), (128, 96), (256, 64), (256, 320), (256, 256), (512, 128)]   # (V, H): generic fc_xent
V256_H = [512, 1024]                                                                 # eight-wave V = 256 kernel
FLASH_SHAPE = (256, 512)
SOFTMAX_V = [64, 128, 256, 320, 512]
SOFTMAX_H = 64                      # the planted logits of softmax_xent come from a head of this H
SAMPLE_SHAPES = [(64, 32), (256, 128), (512, 64), (256, 512), (256, 1024)]
SEQ_FC = dict(H=512, V=256, Bp=64, T=(3, 33))
M_ROWS = 64


def mismatch(got: torch.Tensor, ref: torch.Tensor, family: str, inv: float = 1.0) -> Optional[str]:
    """None when |got - ref| / inv <= ATOL[family] + RTOL[family] |ref| / inv everywhere, else a
    description of the worst element.  A NaN in ``got`` is a mismatch."""
    g, r = got.to(torch.float64) / inv, ref.to(torch.float64) / inv
    if g.shape != r.shape:
        return f"shape {tuple(g.shape)} vs reference {tuple(r.shape)}"
    d = (g - r).abs()
    bad = ~(d <= ATOL[family] + RTOL[family] * r.abs())
    if not bool(bad.any()):
        return None
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    i = int(torch.argmax(torch.where(bad, d, torch.full_like(d, -1.0))))
    idx = tuple(int(v) for v in np.unravel_index(i, tuple(d.shape)))
    return (f"{int(bad.sum())} of {bad.numel()} elements off ({family}: atol {ATOL[family]:.3g}, rtol "
            f"{RTOL[family]:.3g}, normalised); worst at {idx}: got {float(g[idx]):.6g}, reference {float(r[idx]):.6g}")


def err_over_tol(got: torch.Tensor, ref: torch.Tensor, family: str, inv: float = 1.0) -> float:
    """Largest |got - ref| / (atol + rtol |ref|) in the normalised domain (inf for a NaN)."""
    g, r = got.to(torch.float64) / inv, ref.to(torch.float64) / inv
    q = (g - r).abs() / (ATOL[family] + RTOL[family] * r.abs())
    if torch.isnan(q).any():
        return float("inf")
    return float(q.max()) if q.numel() else 0.0


def gemm_mismatch(got: torch.Tensor, A: torch.Tensor, B: torch.Tensor, depth: int) -> Optional[str]:
    """got against the float64 product A . B of exactly representable operands: per element within
    depth * 2^-24 * (|A| . |B|), the first-order bound of a fp32 sum of ``depth`` exact products in any
    order.  Where the bound is 0 the element must be exactly 0."""
    A64, B64 = A.to(torch.float64), B.to(torch.float64)
    ref, bound = A64 @ B64, depth * 2.0 ** -24 * (A64.abs() @ B64.abs())
    d = (got.to(torch.float64) - ref).abs()
    bad = ~(d <= bound)
    if not bool(bad.any()):
        return None
    idx = tuple(int(v) for v in bad.nonzero()[0])
    return (f"{int(bad.sum())} of {bad.numel()} elements beyond {depth} x 2^-24 x |A|.|B|; first at {idx}: got "
            f"{float(got[idx]):.8g}, product {float(ref[idx]):.8g}, bound {float(bound[idx]):.3g}")


def gemm_err_over_bound(got: torch.Tensor, A: torch.Tensor, B: torch.Tensor, depth: int) -> float:
    A64, B64 = A.to(torch.float64), B.to(torch.float64)
    ref, bound = A64 @ B64, depth * 2.0 ** -24 * (A64.abs() @ B64.abs())
    d = (got.to(torch.float64) - ref).abs()
    q = torch.where(bound > 0, d / bound.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), d))
    return float(torch.nan_to_num(q, nan=float("inf")).max())


# ------------------------------------------------------------------------------ layouts
def dlt_encode(dl: torch.Tensor, ldT: int, colT: int, fill: float = float("nan")) -> torch.Tensor:
    """dl [M][V] -> the dl^T buffer [V][ldT] with row m at column colT + m; the rest is ``fill``."""
    M, V = dl.shape
    out = torch.full((V, ldT), fill, dtype=dl.dtype, device=dl.device)
    out[:, colT:colT + M] = dl.T
    return out


def dlt_decode(dlT: torch.Tensor, M: int, colT: int) -> torch.Tensor:
    """The window of the dl^T buffer [V][ldT] -> dl [M][V]."""
    return dlT[:, colT:colT + M].T


def dlf_decode(dlF: torch.Tensor, T: int, Bp: int, V: int) -> torch.Tensor:
    """SeqFcArgs::dlF -> dl [T][Bp][V].  Block (t, row block rb, vocab tile vt) of 512 elements at
    ((t * Bp/32 + rb) * V/16 + vt) * 512; lane L's 8 elements are rows 32 rb + 8 (L >> 4) .. +8 of
    vocab column 16 vt + (L & 15)."""
    v = dlF.reshape(T, Bp // 32, V // 16, 4, 16, 8)           # [t][rb][vt][L >> 4][L & 15][e]
    return v.permute(0, 1, 3, 5, 2, 4).reshape(T, Bp, V)      # [t][rb][L >> 4][e][vt][L & 15]


def dlf_encode(dl: torch.Tensor) -> torch.Tensor:
    """Inverse of dlf_decode: dl [T][Bp][V] -> flat dlF."""
    T, Bp, V = dl.shape
    v = dl.reshape(T, Bp // 32, 4, 8, V // 16, 16)
    return v.permute(0, 1, 4, 2, 5, 3).contiguous().reshape(-1)


# ------------------------------------------------------------------------------ float64 reference
def head_ref(X, W, b, labels, inv, T: int = 0, Bp: int = 0, logits=None) -> Out:
    """The head in float64.  X [M][H] and W [V][H] hold bf16 values, b [V], labels [M] (-1 = ignored),
    inv the loss scale (1 / #labelled rows in training).  With ``logits`` [M][V] given they replace
    X . W^T + b (softmax_xent).  Returns logits, probs, nll [M] (0 on ignored rows), loss_part [M/32],
    dl [M][V] = (probs - onehot) inv on labelled rows and 0 elsewhere, dy = dl . W and, with T and Bp
    (M = T Bp, row t Bp + b), dW [Bp/32][V][H] = sum_t dl_t[rows of rb]^T X_t[rows of rb] and db
    [Bp/32][V]."""
    f = torch.float64
    inv = float(inv)
    W64 = W.to(f) if W is not None else None
    lg = logits.to(f) if logits is not None else X.to(f) @ W64.T + b.to(f)
    M, V = lg.shape
    y = labels.long()
    valid = y >= 0
    yc = y.clamp_min(0)
    m = lg.max(1, keepdim=True).values
    e = torch.exp(lg - m)
    s = e.sum(1, keepdim=True)
    p = e / s
    oh = torch.nn.functional.one_hot(yc, V).to(f)
    nll = torch.where(valid, (torch.log(s) + m).squeeze(1) - lg.gather(1, yc[:, None]).squeeze(1),
                      torch.zeros(M, dtype=f, device=lg.device)) * inv
    dl = (p - oh) * valid[:, None].to(f) * inv
    out = dict(logits=lg, probs=p, nll=nll, loss_part=nll.reshape(M // 32, 32).sum(1), dl=dl)
    if W64 is not None:
        out["dy"] = dl @ W64
    if T and X is not None:
        nrb, H = Bp // 32, X.shape[1]
        d4 = dl.reshape(T, nrb, 32, V).permute(1, 0, 2, 3).reshape(nrb, T * 32, V)
        x4 = X.to(f).reshape(T, nrb, 32, H).permute(1, 0, 2, 3).reshape(nrb, T * 32, H)
        out["dW"] = torch.bmm(d4.transpose(1, 2), x4)
        out["db"] = d4.sum(1)
    return out


# ------------------------------------------------------------------------------ float32 emulators
# The emulator's float32 steps are written so that they give the same bits on every host: a product is
# accumulated in fp32 over k-steps of 32, each k-step's 32 exact products summed in float64 first (the
# MFMA's shape; a BLAS fp32 matmul sums in an order that depends on the machine), and exp, log and the row
# sums are the float64 results rounded to fp32.  MEASURED_DEV therefore reproduces anywhere.
def _mm32(A: torch.Tensor, B: torch.Tensor, acc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """acc + A [M][K] . B [K][N] in fp32, A and B holding bf16 values."""
    A64, B64 = A.to(torch.float64), B.to(torch.float64)
    out = torch.zeros(A.shape[0], B.shape[1], dtype=torch.float32) if acc is None else acc
    for k in range(0, A.shape[1], 32):
        out = out + (A64[:, k:k + 32] @ B64[k:k + 32]).to(torch.float32)
    return out


def _exp32(x: torch.Tensor) -> torch.Tensor:
    return torch.exp(x.to(torch.float64)).to(torch.float32)


def _log32(x: torch.Tensor) -> torch.Tensor:
    return torch.log(x.to(torch.float64)).to(torch.float32)


def _rowsum32(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.float64).sum(1, keepdim=True).to(torch.float32)


def emulate(X, W, b, labels, inv, form: str = "dl", mut: Optional[str] = None, logits=None) -> Out:
    """The head as a correct kernel computes it, float32 with the kernels' rounding points.

    form "dl" (fc_xent, fc_xent_v256, softmax_xent, the FC consumers of gru_fwd_seq_fc): fp32
    accumulation of the exact bf16 products (+ bias), fp32 exp(x - max), sum and reciprocal, dl
    rounded to bf16, dy = bf16(dl) . W in fp32.
    form "flash" (fc_xent_fl): the vocabulary in chunks of 64 columns with a running max m and
    alpha = exp(m_old - m_new); s = alpha s + sum e, U = alpha U + bf16(e) . W_c; at the end
    dy = scale (U / s - W[y]); dl from the logits, the final max and s, as the dl form.
    ``mut``: one of MUTATIONS."""
    f = torch.float32
    inv32 = torch.tensor(float(inv), dtype=f)
    Wf = W.to(f) if W is not None else None
    lg = logits.to(f) if logits is not None else _mm32(X, Wf.T) + b.to(f)
    M, V = lg.shape
    y = labels.long()
    valid = y >= 0
    yc = y.clamp_min(0)
    col = torch.arange(V)
    hot = (yc + 1) % V if mut == "onehot_at_y_plus_1" else yc
    oh = torch.nn.functional.one_hot(hot, V).to(f)
    scale = torch.where(valid, inv32, torch.zeros((), dtype=f))[:, None]
    if mut == "ignored_rows_not_zeroed":
        scale = inv32.expand(M, 1)
    if mut == "inv_applied_twice":
        scale = scale * inv32
    slab = col // 64
    nslab = V // 64
    if form == "dl":
        if mut == "no_max_subtraction":
            m = torch.zeros(M, 1, dtype=f)
        elif mut == "max_over_own_slab_only":   # each wave subtracts the maximum of its own 64 columns
            m = torch.cat([lg[:, 64 * k:64 * k + 64].max(1, keepdim=True).values.expand(M, 64) for k in range(nslab)], 1)
        else:
            m = lg.max(1, keepdim=True).values
        e = _exp32(lg - m)
        s = _rowsum32(e[:, slab != nslab - 1] if mut == "slab_missing_from_row_sum" else e)
        p = e * (1.0 / s)
        mrow = lg.max(1, keepdim=True).values if mut == "max_over_own_slab_only" else m
        U = None
    else:
        assert Wf is not None and V % 64 == 0
        H = Wf.shape[1]
        mo = torch.full((M, 1), float("-inf"), dtype=f)
        s = torch.zeros(M, 1, dtype=f)
        U = torch.zeros(M, H, dtype=f)
        for c in range(nslab):
            xc = lg[:, 64 * c:64 * c + 64]
            mn = torch.maximum(mo, xc.max(1, keepdim=True).values)
            alpha = _exp32(mo - mn)                            # 0 on the first chunk
            ec = _exp32(xc - mn)
            s = alpha * s + _rowsum32(ec)
            U = _mm32(bf16_round(ec), Wf[64 * c:64 * c + 64], U if mut == "flash_alpha_not_applied_to_U" else alpha * U)
            mo = mn
        mrow = mo
        p = _exp32(lg - mrow) * (1.0 / s)
    if mut == "uniform_softmax":
        p = torch.full_like(p, 1.0 / V)
    d = (p - oh) * scale
    if mut == "dl_zero_below_1e-4":
        d = torch.where(d.abs() < 1e-4, torch.zeros_like(d), d)
    dl = bf16_round(d)
    nll = torch.where(valid, (_log32(s) + mrow).squeeze(1) - lg.gather(1, yc[:, None]).squeeze(1),
                      torch.zeros(M, dtype=f)) * inv32
    out = dict(logits=lg, probs=p, nll=nll, loss_part=_rowsum32(nll.reshape(M // 32, 32)).squeeze(1), dl=dl)
    dlT = dl
    if mut == "dlT_row_pairs_swapped":   # the XOR-2 staging of fc_xent_v256 not undone: columns with bit 3
        sw = dl[torch.arange(M) ^ 2]     # set hold row r at r ^ 2
        dlT = torch.where(((col >> 3) & 1).bool()[None, :], sw, dl)
    out["dlT"] = dlT
    if Wf is not None:
        if form == "dl":
            k = V - 32 if mut == "dy_last_k_step_dropped" else V
            out["dy"] = _mm32(dl[:, :k], Wf[:k])
        else:
            wy = Wf[yc]
            out["dy"] = (U * (1.0 / s) - wy) * scale if mut != "flash_label_row_not_scaled" else U * (1.0 / s) * scale - wy
    return out


# planted bugs the tolerances must catch: name -> form
MUTATIONS = {
    "no_max_subtraction": "dl",
    "slab_missing_from_row_sum": "dl",
    "max_over_own_slab_only": "dl",
    "onehot_at_y_plus_1": "dl",
    "ignored_rows_not_zeroed": "dl",
    "inv_applied_twice": "dl",
    "dlT_row_pairs_swapped": "dl",
    "dy_last_k_step_dropped": "dl",
    "flash_alpha_not_applied_to_U": "flash",
    "flash_label_row_not_scaled": "flash",
    "uniform_softmax": "dl",
    "dl_zero_below_1e-4": "dl",
}


# ------------------------------------------------------------------------------ inputs
def _finish(X, W, b, labels) -> Out:
    n = int((labels >= 0).sum())
    return dict(X=X, W=W, b=b, labels=labels, inv=torch.tensor(1.0 / max(n, 1), dtype=torch.float32), dy_from=0)


def _randn(g: torch.Generator, *shape) -> torch.Tensor:
    """Near-normal fp32 values of unit variance from integer draws alone (the sum of four uniform 16-bit
    integers, centred and scaled): torch.randn's values depend on the host's vector width in the last
    bit, and a bf16 rounding that flips with it would move the measured deviations from host to host."""
    u = torch.randint(0, 1 << 16, (4,) + tuple(shape), generator=g, dtype=torch.int64).sum(0)
    return ((u - 2 * 65535).to(torch.float64) / (65536.0 / 3.0 ** 0.5)).to(torch.float32)


def random_inputs(V: int, H: int, M: int = M_ROWS, seed: int = 0, wscale: float = 1.0, hidden: bool = False) -> Out:
    """Seeded random head inputs in the style of tests/test_kernels_gpu.py: X ~ N(0, 1) (_randn; ``hidden``:
    tanh of it, like a GRU state), W ~ wscale N(0, 1/H), b ~ 0.5 N(0, 1), every 7th label -1."""
    g = torch.Generator(device="cpu").manual_seed(3000 + seed)
    X = _randn(g, M, H)
    X = bf16_round(torch.tanh(X.double()).float() if hidden else X)
    W = bf16_round(_randn(g, V, H) * (wscale * H ** -0.5))
    b = _randn(g, V) * 0.5
    labels = torch.randint(0, V, (M,), generator=g, dtype=torch.int32)
    labels[::7] = -1
    return _finish(X, W, b, labels)


def planted_table(V: int):
    """The [32][V] table of planted logits (integers, exact in bf16) and the labels of its rows.
    ns = V/32 slabs (the eight-wave kernels' wave columns), nc = V/64 chunks (the generic kernels'
    wave columns, the flash chunks).
      rows 0-15  label in slab i % ns, a +8 row maximum in another slab (every slab over the 16 rows)
      row 16/17  label at column 0 / V-1
      row 18/19  +100 / -100 in every column (exp overflows without the max subtraction)
      row 20/21  a +30 spike on / off the label
      row 22/23  chunk c at +24 c (maxima rising) / +24 (nc-1-c) (falling)
      row 24     +60 at one column of the last chunk
      row 25     one chunk 100 below the rest
      rows 26-28 label -1 (scattered ignored rows), small +-2 pattern
      rows 29-31 +-4 checkerboards, labelled"""
    ns, nc = V // 32, V // 64
    t = torch.zeros(32, V)
    y = torch.zeros(32, dtype=torch.int32)
    col = torch.arange(V)
    for i in range(16):
        y[i] = 32 * (i % ns) + (5 * i + 3) % 32
        t[i, 32 * ((i + ns // 2) % ns) + (11 * i + 1) % 32] = 8
    y[16], y[17] = 0, V - 1
    t[18], t[19] = 100, -100
    y[18], y[19] = V // 2 + 1, V // 2 - 2
    y[20], y[21] = 37 % V, 12
    t[20, int(y[20])] = 30
    t[21, V - 7] = 30
    t[22] = 24.0 * (col // 64)
    t[23] = 24.0 * (nc - 1 - col // 64)
    y[22], y[23] = V - 3, 5                      # each in its row's highest chunk
    t[24, V - 20] = 60
    y[24] = 9
    t[25, 64 * (1 % nc):64 * (1 % nc) + 64] = -100
    y[25] = (64 * (1 % nc) + 70) % V
    for i in (26, 27, 28):
        t[i] = 2.0 * (((col + i) % 3) - 1)
        y[i] = -1
    for i in (29, 30, 31):
        t[i] = 4.0 * (((col // (i - 28)) % 2) * 2 - 1)
        y[i] = (41 * i) % V
    return t, y


def planted_inputs(V: int, H: int, M: int = M_ROWS, seed: int = 0, wscale: float = 1.0) -> Out:
    """Head inputs whose logits carry planted_table exactly: the first 32 hidden units of X are the
    one-hot selector of row % 32 and W[:, :32] holds the table, so row m's logits are the random
    part (hidden units 32 .., seeded) plus table[m % 32].  Row block 0 takes the table's labels,
    every other row block is all -1 (a fully ignored block).  ``dy_from`` = 32: dy is compared end to
    end from hidden unit 32 on -- in the selector's columns |W| reaches 168, so the bf16 rounding of
    dl alone moves dy by 0.5 there (normalised) and an atol made of it would pass anything in the
    other columns; the selector's columns are held by the product bound (gemm_mismatch), which
    scales with |W|."""
    assert H >= 32 and M % 32 == 0
    d = random_inputs(V, H, M, seed, wscale)
    t, y = planted_table(V)
    X, W = d["X"], d["W"]
    X[:, :32] = torch.eye(32).repeat(M // 32, 1)
    W[:, :32] = t.T
    labels = torch.full((M,), -1, dtype=torch.int32)
    labels[:32] = y
    out = _finish(X, W, d["b"], labels)
    out["dy_from"] = 32
    return out


def inputs(kind: str, V: int, H: int, M: int = M_ROWS, seed: int = 0, wscale: float = 1.0) -> Out:
    return planted_inputs(V, H, M, seed, wscale) if kind == "planted" else random_inputs(V, H, M, seed, wscale)


# ------------------------------------------------------------------------------ sampling
def clear_uniforms(probs64, r):
    """A uniform within 1e-5 of an fp64 CDF edge moves to the midpoint of its interval (or, where that
    interval is too narrow to clear the edges, of the widest one).  Returns (r, expected index): the
    first index whose fp64 running sum exceeds r, else the last index with a probability.  (The helper
    of tests/test_sampling_ctl_gpu.py.)"""
    r = np.asarray(r, np.float32).copy()
    V = probs64.shape[1]
    cdf = np.cumsum(probs64, -1)
    for i in range(len(r)):
        if r[i] >= 1 or np.abs(cdf[i] - float(r[i])).min() >= 1e-5:
            continue
        j = min(int(np.searchsorted(cdf[i], float(r[i]), side="right")), V - 1)
        if probs64[i, j] < 4e-5:
            j = int(probs64[i].argmax())
        r[i] = np.float32(cdf[i, j] - 0.5 * probs64[i, j])
        assert np.abs(cdf[i] - float(r[i])).min() >= 1e-5
    hit = cdf > r.astype(np.float64)[:, None]
    last = V - 1 - (probs64 > 0)[:, ::-1].argmax(1)
    return r, np.where(hit.any(1), hit.argmax(1), last)


# ------------------------------------------------------------------------------ measurement
def case_deviation(d: Out, form: str = "dl", logits_only: bool = False, mut: Optional[str] = None) -> Dict[str, float]:
    """Deviation emulate - head_ref of one input set per family, normalised by inv.  ``logits_only``:
    the softmax_xent case (both sides start from the emulator's fp32 logits)."""
    inv = float(d["inv"])
    lg = emulate(d["X"], d["W"], d["b"], d["labels"], inv)["logits"] if logits_only else None
    W = None if logits_only else d["W"]
    ref = head_ref(d["X"], W, d["b"], d["labels"], inv, logits=lg)
    emu = emulate(d["X"], W, d["b"], d["labels"], inv, form=form, mut=mut, logits=lg)
    dev = {"dl": max(deviation(emu["dl"] / inv, ref["dl"] / inv, RTOL["dl"]),
                     deviation(emu["dlT"] / inv, ref["dl"] / inv, RTOL["dl"])),
           "loss": deviation(emu["loss_part"] / inv, ref["loss_part"] / inv),
           "probs": deviation(emu["probs"], ref["probs"])}
    if "dy" in emu:
        c0 = int(d.get("dy_from", 0))
        dev["dy_flash" if form == "flash" else "dy"] = deviation(emu["dy"][:, c0:] / inv, ref["dy"][:, c0:] / inv)
    return dev


def measure_deviations(seeds=(0, 1, 2), verbose: bool = False) -> Dict[str, float]:
    """Largest deviation per family over every case of tests/test_head_gpu.py and ``seeds``."""
    out: Dict[str, float] = {}

    def take(dev, tag, only=None):
        for k, v in dev.items():
            if only is None or k in only:
                out[k] = max(out.get(k, 0.0), v)
        if verbose:
            print(tag, {k: f"{v:.3e}" for k, v in dev.items()}, flush=True)

    for seed in seeds:
        for kind in ("planted", "random"):
            for V, H in XENT_SHAPES + [(256, h) for h in V256_H]:
                take(case_deviation(inputs(kind, V, H, seed=seed)), f"fc_xent {kind} V={V} H={H} seed={seed}",
                     ("dl", "loss", "dy"))
            V, H = FLASH_SHAPE
            take(case_deviation(inputs(kind, V, H, seed=seed), form="flash"), f"flash {kind} seed={seed}",
                 ("dl", "loss", "dy_flash"))
            for V in SOFTMAX_V:
                take(case_deviation(inputs(kind, V, SOFTMAX_H, seed=seed), logits_only=True),
                     f"softmax_xent {kind} V={V} seed={seed}", ("dl", "loss"))
            for V, H in SAMPLE_SHAPES:
                take(case_deviation(inputs(kind, V, H, seed=seed, wscale=3.0)), f"fc_sample {kind} V={V} H={H} seed={seed}",
                     ("probs",))
        take(case_deviation(random_inputs(SEQ_FC["V"], SEQ_FC["H"], 3 * SEQ_FC["Bp"], seed, hidden=True)),
             f"fwd_seq_fc hidden-state X seed={seed}", ("dl", "loss", "dy"))
    return out


if __name__ == "__main__":
    res = measure_deviations(verbose=True)
    for k in MEASURED_DEV:
        print(f'    "{k}": {res[k]:.3e},')

"""Exact per-element reference of the product kernels (gemm.hip, gemm_lds.hip, gemm_small.hip,
gemm256.hip, onehot.hip and gemm_f32_nt of gen_f32.hip).  CPU only: numpy / torch, no GPU import.

A GEMM allows a stronger test than a tolerance: choose the operands so that the result is *exact*.

* ``grid_operands``: operands on a dyadic grid -- small integers times a per-row power of two.  Every
  product a * b and every partial sum of a dot product is then a multiple of the output element's lsb
  2^(ea[m] + eb[n]) and, the integer ranges being sized from the K-slice depth, below 2^24 of them:
  representable in fp32.  An fp32-accumulating MFMA chain then returns the same value whatever its
  summation order, pipeline, split or tile shape, and that value is the exact one.
* ``product_ref``: the product in float64 (exact: every sum is far below 2^53 lsbs) per split-K slab,
  with the bias where the contract puts it, the accumulate term, the row sums of A per slab, one-hot
  A from ids, and the B / B2 row split.  It *asserts* the exactness condition for every output
  element (``GridError`` otherwise), so a case can never silently become inexact: the zero tolerance
  of ``compare`` is derived, not measured.  ``mutate=`` plants one of the wrong results the tests
  must catch (MUTATIONS).
* ``padded`` / ``canary`` / ``check_canary``: operands embedded in buffers whose padding is NaN (a
  read of padding poisons the result), outputs in buffers filled with a fixed 32-bit pattern whose
  padding columns and guard rows are compared bitwise after the launch.
* ``compare``: value equality in every element (0 == -0; any NaN / inf fails) with a message that
  names the slab, the first bad element, the count and the 64 x 64 tile histogram.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

# exponents of the per-row powers of two: A rows in [-3, 0], B rows in [0, 3] (every value's exponent
# in [-3, 3]); a bias element sits on the coarsest A grid (EA_MAX) so it is a multiple of every lsb
# of its column
EA_MIN, EA_MAX = -3, 0
EB_MIN, EB_MAX = 0, 3
LIMIT = 2.0 ** 24          # |integer| < 2^24: every integer below it is an fp32 value
PATTERN = 0xC0FFEE42 - (1 << 32)   # the canary word, as int32 (as fp32: a finite -7.99..)
PATTERN16 = 0xC0FF - (1 << 16)     # 2-byte outputs (bf16 companions): as int16

MUTATIONS = ("swap_k_ranges", "bias_every_slab", "drop_kblock", "transpose_subtile", "rowsum_wrong_slab",
             "padding_as_data", "a32_trans_ignored", "a32_truncated", "id_M_matches_last")


class GridError(ValueError):
    """The exactness condition does not hold for the case."""


def ceil_log2(n: int) -> int:
    return max(0, int(n - 1).bit_length())


def operand_bits(kdepth: int, max_bits: int = 8, a_bits: Optional[int] = None):
    """Significant bits (p for A, q for B) so that kdepth products sum below 2^23 lsbs: p + q =
    23 - ceil(log2 kdepth), each at most max_bits, p >= q.  (2^22 + 2^22 are left to bias and C0.)"""
    budget = 23 - ceil_log2(kdepth)
    if a_bits is None and max_bits > 8:      # fp32 operands: A as wide as max_bits allows, B the rest
        p = min(max_bits, budget - 7)
        q = min(max_bits, budget - p)
    elif a_bits is None:
        p = min(max_bits, (budget + 1) // 2)
        q = min(max_bits, budget - p)
        p = min(max_bits, budget - q)
    else:
        p, q = a_bits, min(max_bits, budget - a_bits)
    if p < 1 or q < 1:
        raise GridError(f"no grid for a K-slice of {kdepth} (budget {budget} bits)")
    return p, q


@dataclass
class Operands:
    A: Optional[torch.Tensor]      # [M][K] float64 values on the grid (None for one-hot A)
    B: torch.Tensor                # [N][K] float64
    ea: torch.Tensor               # [M] int: A[m] / 2^ea[m] are integers
    eb: torch.Tensor               # [N] int
    bias: Optional[torch.Tensor] = None   # [N] float64
    C0: Optional[torch.Tensor] = None     # [M][N] float64
    A32: Optional[torch.Tensor] = None    # [M][K] float32; its bf16 rounding is A
    ids: Optional[torch.Tensor] = None    # [K] int32 (one-hot A: A[m][k] = ids[k] == m)
    bits: tuple = (0, 0)


def _ints(g, shape, bits, kblock=64):
    """Nonzero integers of up to `bits` significant bits: mostly positive (sums grow towards the
    fp32 limit instead of cancelling), a third with the top and the lowest bit set (all `bits` are
    used), and a sign pattern that differs per row and per k-block."""
    hi = (1 << bits) - 1
    v = torch.randint(1, hi + 1, shape, generator=g, dtype=torch.int64)
    full = torch.rand(shape, generator=g) < 1.0 / 3
    v = torch.where(full, v | (1 << (bits - 1)) | 1, v)
    neg = torch.rand(shape, generator=g) < 0.2
    if len(shape) == 2:
        r = torch.arange(shape[0])[:, None]
        kb = torch.arange(shape[1])[None, :] // kblock
        neg = neg ^ ((r * 5 + kb * 3) % 7 == 0)
    return torch.where(neg, -v, v)


def grid_operands(M, N, K, seed, kdepth=None, bias=False, c0=False, a32=False, onehot=None, max_bits=8,
                  exps=True, onehot_kt=64) -> Operands:
    """Grid operands for C[M][N] = A[M][K] . B[N][K]^T.  kdepth: the K-slice depth the integer ranges
    are sized from (K / splits; default K).  max_bits: 8 for bf16 operands, up to 12 for the fp32
    GEMM.  a32: also the fp32 A32 whose bf16 rounding (RNE) is A.  onehot: an id distribution name
    (onehot_ids, `holes` per onehot_kt tokens) -- A is then the one-hot matrix of the ids and only B is drawn.  exps = False: every
    exponent 0 (an A32 that is read both plain and transposed has no per-row grid)."""
    g = torch.Generator(device="cpu").manual_seed(1000003 * seed + 7919 * M + 104729 * N + K)
    kdepth = kdepth or K
    if exps:
        ea = torch.randint(EA_MIN, EA_MAX + 1, (M,), generator=g)
        eb = torch.randint(EB_MIN, EB_MAX + 1, (N,), generator=g)
    else:
        ea, eb = torch.zeros(M, dtype=torch.int64), torch.zeros(N, dtype=torch.int64)
    if onehot is not None:
        ids = onehot_ids(onehot, M, K, g, onehot_kt)
        ea = torch.zeros(M, dtype=torch.int64)
        p, q = 1, min(max_bits, 23 - ceil_log2(kdepth) - 1)
        ib = _ints(g, (N, K), q)
        return Operands(None, ib.double() * torch.exp2(eb.double())[:, None], ea, eb, ids=ids, bits=(p, q))
    # A32 rounds to integers in [128, 256]: bf16's ulp there is 1 grid unit, and |a| <= 2^8 keeps the bound
    p, q = operand_bits(kdepth, max_bits, a_bits=8 if a32 else None)
    out = Operands(None, None, ea, eb, bits=(p, q))
    sa = torch.exp2(ea.double())[:, None]
    if a32:
        mag = torch.randint(129, 256, (M, K), generator=g, dtype=torch.int64)
        # below the tie, above it, exact ties (to even: both ways, by the parity of mag) and 255.5,
        # which rounds up into the next binade (256)
        frac = torch.tensor([0.0, 0.25, -0.25, 0.375, 0.5, -0.5, 0.4375, -0.46875])[
            torch.randint(0, 8, (M, K), generator=g)]
        mag = torch.where(torch.rand((M, K), generator=g) < 1 / 64, torch.full_like(mag, 255), mag)
        x = mag.double() + frac.double()
        x[0, 0], x[0, 1], x[0, 2], x[0, 3] = 255.5, 128.5, 129.5, 254.5   # the named cases, always present
        sign = torch.where(torch.rand((M, K), generator=g) < 0.2, -1.0, 1.0).double()
        out.A32 = (x * sign * sa).float()
        assert torch.equal(out.A32.double(), x * sign * sa)               # needs <= 24 bits: exact in fp32
        out.A = out.A32.bfloat16().double()
    else:
        out.A = _ints(g, (M, K), p).double() * sa
    out.B = _ints(g, (N, K), q).double() * torch.exp2(eb.double())[:, None]
    if bias:   # |bias| < 2^15 coarse units = 2^(15 + EA_MAX - EA_MIN) <= 2^21 of the finest lsb
        out.bias = _ints(g, (N,), 15).double() * torch.exp2(eb.double() + EA_MAX)
    if c0:
        out.C0 = _ints(g, (M, N), 21).double() * sa * torch.exp2(eb.double())[None, :]
    return out


def onehot_ids(dist, M, K, g, kt=64):
    """Token ids for a one-hot A of M vocabulary rows.  uniform; names (a few dozen letters and a
    heavy 0); tile (all in one 16-row tile); invalid (nothing matches: -1, M, values whose low 8 bits
    are valid, far out); holes (per `kt` tokens the ids leave some wave's four 16-row tiles -- rows
    64w .. 64w + 63 -- without a match while the other waves have some)."""
    if dist == "uniform":
        ids = torch.randint(0, M, (K,), generator=g)
    elif dist == "names":
        ids = torch.randint(97, 123, (K,), generator=g) % M
        ids[::17] = 0
    elif dist == "tile":
        ids = 16 * (M // 32) + torch.randint(0, 16, (K,), generator=g)
    elif dist == "invalid":
        pool = torch.tensor([-1, M, M + 5, 256 + 7, 512 + 100, -256 + 3, -(1 << 31), (1 << 31) - 1, 65536 + 9, 1 << 20])
        ids = pool[torch.randint(0, len(pool), (K,), generator=g)]
        ids[0], ids[1 % K] = -1, M
    elif dist == "holes":
        ids = torch.empty(K, dtype=torch.int64)
        nq = max(1, M // 64)
        for t in range((K + kt - 1) // kt):
            absent = t % nq
            q = torch.randint(0, nq - 1, (kt,), generator=g) if nq > 1 else torch.zeros(kt, dtype=torch.int64)
            q = q + (q >= absent).long() if nq > 1 else q
            v = q * 64 + torch.randint(0, min(64, M), (kt,), generator=g)
            ids[t * kt:(t + 1) * kt] = v[:min(kt, K - t * kt)]
    else:
        raise ValueError(dist)
    return ids.to(torch.int32)


def onehot_matrix(ids, M, mutate=None):
    """[M][K] float64: A[m][k] = (ids[k] == m); ids outside [0, M) match nothing."""
    ids = ids.long()
    A = (ids[None, :] == torch.arange(M)[:, None]).double()
    if mutate == "id_M_matches_last":
        A[M - 1] += (ids == M).double()
    return A


def bf16_trunc(x32):
    return (x32.contiguous().view(torch.int32) & -65536).view(torch.float32)


@dataclass
class Ref:
    C: torch.Tensor        # [splits][M][N] float32 (exact)
    rowsum: torch.Tensor   # [splits][M] float32 (exact) row sums of the slab's A


def _exact_or_raise(absum, lsb, what):
    """absum / lsb < 2^24 in every element (absum: the sum of the magnitudes of everything added into
    the element; lsb: the power of two all of them are multiples of)."""
    worst = float((absum / lsb).max())
    if not worst < LIMIT:
        raise GridError(f"{what}: sum of magnitudes reaches {worst:.0f} lsbs (>= 2^24): not exact in fp32")


def product_ref(op: Operands, splits=1, bias_in="unsplit", B2=None, b2_row=0, accumulate=False,
                a32_trans_storage=None, mutate=None) -> Ref:
    """Per-slab exact product.  bias_in: where op.bias goes -- "unsplit" (the bf16 kernels: only when
    splits == 1), "slab0" (gemm_f32_nt), "none".  B2 / b2_row: rows >= b2_row of B come from B2.
    accumulate: op.C0 is added to every slab (the kernels do C += in each slab).
    a32_trans_storage: the [K][M] fp32 array the kernel reads with a32_trans (for the mutation that
    ignores the flag; M == K).  Raises GridError unless every output is exact in fp32."""
    M, N = len(op.ea), len(op.eb)
    if op.ids is not None:
        A = onehot_matrix(op.ids, M, mutate)
    else:
        A = op.A.clone()
    B = op.B.clone()
    if B2 is not None:
        B[b2_row:] = B2[b2_row:]
    K = A.shape[1]
    assert K % splits == 0 and A.shape == (M, K) and B.shape == (N, K)
    kper = K // splits
    sa, sb = torch.exp2(op.ea.double()), torch.exp2(op.eb.double())
    lsb = sa[:, None] * sb[None, :]
    # the grid itself is a checked condition: every operand value is an integer number of its lsbs
    for name, t, s in (("A", A, sa[:, None]), ("B", B, sb[:, None]), ("C0", op.C0 if accumulate else None, lsb),
                       ("bias", op.bias, sb * 2.0 ** EA_MAX)):
        if t is not None and not torch.equal(torch.floor(t / s), t / s):
            raise GridError(f"{name} is off its grid")
    if mutate == "a32_truncated":
        A = bf16_trunc(op.A32).double()
    if mutate == "a32_trans_ignored":
        A = a32_trans_storage.bfloat16().double()         # [K][M] read as [M][K]
    if mutate == "padding_as_data":
        A[M // 2, K - 1] = float("nan")
    if mutate == "drop_kblock":
        A[:, 64:128] = 0
    order = list(range(splits))
    if mutate == "swap_k_ranges":
        order[0], order[1] = order[1], order[0]
    C = torch.empty(splits, M, N, dtype=torch.float64)
    rs = torch.empty(splits, M, dtype=torch.float64)
    for s in range(splits):
        ks = slice(order[s] * kper, (order[s] + 1) * kper)
        As, Bs = A[:, ks], B[:, ks]
        C[s] = As @ Bs.T
        rs[s] = As.sum(1)
        extra = torch.zeros(M, N, dtype=torch.float64)
        with_bias = op.bias is not None and ((bias_in == "unsplit" and splits == 1) or (bias_in == "slab0" and s == 0)
                                             or mutate == "bias_every_slab")
        if with_bias:
            C[s] += op.bias[None, :]
            extra += op.bias.abs()[None, :]
        if accumulate:
            C[s] += op.C0
            extra += op.C0.abs()
        if mutate is None:
            # cheap sufficient bound first (max |a| max |b| kper), the per-element sum only if it fails
            bound = As.abs().amax(1)[:, None] * Bs.abs().amax(1)[None, :] * kper + extra
            if not float((bound / lsb).max()) < LIMIT:
                _exact_or_raise(As.abs() @ Bs.abs().T + extra, lsb, f"C slab {s}")
            _exact_or_raise(As.abs().sum(1), sa, f"row sums slab {s}")
    if mutate == "transpose_subtile":
        C[0, 16:32, 32:48] = C[0, 16:32, 32:48].T.clone()
    if mutate == "rowsum_wrong_slab":
        rs = rs.roll(1, 0)
    C32, rs32 = C.float(), rs.float()
    if mutate is None:
        assert torch.equal(C32.double(), C) and torch.equal(rs32.double(), rs)
    return Ref(C32, rs32)


# ------------------------------------------------------------------------------ buffers
@dataclass
class Padded:
    """A [rows][cols] (or slabs of them) array inside a larger buffer: `guard` rows before and after,
    leading dimension ld >= cols, slab s at row offset s * slab_rows."""
    buf: torch.Tensor          # [guard + nslab * slab_rows + guard][ld]
    guard: int
    nslab: int
    rows: int
    cols: int
    slab_rows: int

    @property
    def ld(self):
        return self.buf.shape[1]

    def view(self):
        """[nslab][rows][cols] view of the payload (2-D input: index [0])."""
        body = self.buf[self.guard:self.guard + self.nslab * self.slab_rows]
        return body.view(self.nslab, self.slab_rows, self.ld)[:, :self.rows, :self.cols]

    def ptr(self):
        return self.view().data_ptr()

    def to(self, dev):
        return Padded(self.buf.to(dev), self.guard, self.nslab, self.rows, self.cols, self.slab_rows)


def padded(t, ld, guard_rows=2, fill=float("nan")) -> Padded:
    """Operand t ([R][C] or [S][R][C]) embedded with leading dimension ld; every padding element is
    `fill` (NaN: a read of padding poisons the result)."""
    t3 = t if t.dim() == 3 else t[None]
    S, R, Cn = t3.shape
    assert ld >= Cn
    buf = torch.full((2 * guard_rows + S * R, ld), fill, dtype=t.dtype)
    p = Padded(buf, guard_rows, S, R, Cn, R)
    p.view().copy_(t3)
    return p


def _bits(t):
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int16)


def canary(nslab, rows, cols, ld, guard_rows=2, slab_rows=None, dtype=torch.float32) -> Padded:
    """Output buffer filled with the canary pattern (the 32-bit word PATTERN; PATTERN16 for 2-byte types)."""
    slab_rows = slab_rows or rows
    assert ld >= cols and slab_rows >= rows
    buf = torch.empty(2 * guard_rows + nslab * slab_rows, ld, dtype=dtype)
    _bits(buf).fill_(PATTERN if buf.element_size() == 4 else PATTERN16)
    return Padded(buf, guard_rows, nslab, rows, cols, slab_rows)


def check_canary(p: Padded, what="output"):
    """Everything outside the payload still holds the canary pattern, bitwise."""
    buf = p.buf.detach().cpu().contiguous()
    ok = _bits(buf) == (PATTERN if buf.element_size() == 4 else PATTERN16)
    inside = torch.zeros_like(ok)
    body = inside[p.guard:p.guard + p.nslab * p.slab_rows].view(p.nslab, p.slab_rows, -1)
    body[:, :p.rows, :p.cols] = True
    bad = ~ok & ~inside
    if bad.any():
        r, c = [int(x) for x in bad.nonzero()[0]]
        raise AssertionError(f"{what}: {int(bad.sum())} stray writes outside the payload; first at buffer row {r} "
                             f"(payload starts at {p.guard}), column {c} (payload {p.cols} of ld {p.ld})")


# ------------------------------------------------------------------------------ comparison
def compare(got, ref, what="C"):
    """Value equality in every element of every slab.  got / ref: [S][M][N], [M][N] or [S][M] (row
    sums: pass them with a trailing unit axis or as 2-D with what="rowsum")."""
    got = got.detach().cpu()
    ref = ref.detach().cpu()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} against {tuple(ref.shape)}"
    while got.dim() < 3:
        got, ref = got[None], ref[None]
    finite = torch.isfinite(got)
    bad = ~finite | (got != ref)
    if not bad.any():
        return
    s, r, c = [int(x) for x in bad.nonzero()[0]]
    per_slab = bad.flatten(1).sum(1).tolist()
    S, R, Cn = bad.shape
    tr, tc = (R + 63) // 64, (Cn + 63) // 64
    hist = torch.zeros(tr * 64, tc * 64, dtype=torch.int64)
    hist[:R, :Cn] = bad.sum(0)
    hist = hist.view(tr, 64, tc, 64).sum((1, 3))
    tiles = {f"({i},{j})": int(hist[i, j]) for i in range(tr) for j in range(tc) if hist[i, j]}
    shown = dict(list(tiles.items())[:24])
    raise AssertionError(
        f"{what}: {int(bad.sum())} of {bad.numel()} elements differ (non-finite: {int((~finite).sum())}); "
        f"first at slab {s} (row {r}, col {c}): got {got[s, r, c].item()!r}, expected {ref[s, r, c].item()!r}; "
        f"bad per slab {per_slab}; bad per 64x64 tile (row, col) {shown}{' ...' if len(tiles) > 24 else ''}")

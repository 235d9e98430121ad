"""CPU reference path (BASELINE config #1) and the numerical oracle for the HIP engine.

Math is the reference's forward step (/root/reference/namegensf.cu:664-872,
SURVEY §3.3), in PyTorch gate convention:

    r = σ(W_ir x + b_ir + W_hr h + b_hr)          namegensf.cu:676-695
    z = σ(W_iz x + b_iz + W_hz h + b_hz)          namegensf.cu:702-721
    n = tanh(W_in x + b_in + r ⊙ (W_hn h + b_hn)) namegensf.cu:729-749
    h' = (1 − z) ⊙ n + z ⊙ h = n + z ⊙ (h − n)    namegensf.cu:754-763
    p = softmax(W_fc h_top + b_fc)                namegensf.cu:861-872

with a *correct* (max-subtracted, race-free) softmax -- the reference's K9 kernel
races on its atomic sum (namegensf.cu:294-300).

The training half (loss, BPTT, optimiser) has no reference counterpart;
``manual_backward`` is the exact formula set the HIP backward kernels implement and
is checked against ``torch.autograd`` in tests/test_cpu_ref.py.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from ..config import GRUConfig

Params = Dict[str, torch.Tensor]


def _gates(gi: torch.Tensor, gh: torch.Tensor, h: torch.Tensor):
    H = h.shape[-1]
    r = torch.sigmoid(gi[..., :H] + gh[..., :H])
    z = torch.sigmoid(gi[..., H:2 * H] + gh[..., H:2 * H])
    ghn = gh[..., 2 * H:]
    n = torch.tanh(gi[..., 2 * H:] + r * ghn)
    hn = n + z * (h - n)
    return hn, (r, z, n, ghn)


# Training dropout on the non-recurrent connections (Zaremba et al. 2014; docs/DESIGN.md §3.5).  With
# cfg.dropout = p every layer's output h_l[t, b, j] reaches its consumer above (the FC head, or layer l + 1's
# input projection) as d = m h / (1 - p); layer 0's input, the recurrent path and a carried state are never
# masked.  m = 1 iff word j & 3 of Philox-4x32-10(key = cfg.seed, counter = (j >> 2, b_global,
# (layer << 24) | t, step)) is >= thr = floor(p 2^32) (formed in double): j the unit, b_global the sequence's
# index in the GLOBAL batch (rank * local_batch + b, so a data-parallel step draws the single-GPU step's
# masks), step the optimiser step counter when the step's forward runs (0 for the first step).  The backward
# multiplies the gradient arriving at h_l[t] from above by the same m / (1 - p) before the layer's BPTT adds
# the recurrent carry.  The device (csrc/kernels/dropout.hip) follows this rule bit for bit: its forward
# scales the bf16 saved state by s = float32(1 / (1 - p)) with one rounding to bf16, its backward the fp32
# gradient by the same s; a dropped element is +0.
def dropout_threshold(p: float) -> int:
    """thr of the mask rule: a unit is kept iff its 32-bit Philox word is >= thr."""
    return int(math.floor(float(p) * 4294967296.0))


def dropout_scale(p: float) -> np.float32:
    """s of the mask rule as the device forms it: 1 / (1 - p) in double, rounded to float32."""
    return np.float32(1.0 / (1.0 - float(p)))


def dropout_mask(cfg: GRUConfig, layer: int, step: int, b_global, T: int) -> np.ndarray:
    """The keep mask of ``layer``'s output at optimiser step ``step``: bool [B, T, H] for the sequences with
    global batch indices ``b_global`` (array-like of B indices; an int is one sequence)."""
    bg = np.atleast_1d(np.asarray(b_global, dtype=np.int64)).astype(np.uint64)
    if bg.ndim != 1:
        raise ValueError("dropout_mask: b_global is an index or a 1-D list of indices")
    if not (0 <= int(layer) < 256 and 0 < int(T) <= (1 << 24)):
        raise ValueError("dropout_mask: the counter holds layers < 256 and T <= 2^24")
    B, H = bg.shape[0], cfg.hidden
    nb = (H + 3) // 4
    seed = int(cfg.seed) & 0xFFFFFFFFFFFFFFFF
    ctr = np.zeros((B, int(T), nb, 4), np.uint64)
    ctr[..., 0] = np.arange(nb, dtype=np.uint64)[None, None, :]
    ctr[..., 1] = (bg & _U32)[:, None, None]
    ctr[..., 2] = (np.uint64(int(layer) << 24) | np.arange(int(T), dtype=np.uint64))[None, :, None]
    ctr[..., 3] = np.uint64(int(step) & 0xFFFFFFFF)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)
    words = philox4x32(ctr, key).reshape(B, int(T), nb * 4)[..., :H]
    return words >= np.uint32(dropout_threshold(cfg.dropout))   # (thr = 0 at p = 0: all ones)


def _dropout_factor(cfg: GRUConfig, layer: int, step: int, b0: int, B: int, T: int, dt) -> torch.Tensor:
    """m / (1 - p) of ``layer``'s output in the oracle dtype, [B, T, H]."""
    m = dropout_mask(cfg, layer, step, b0 + np.arange(B), T)
    return torch.from_numpy(m).to(dt) / (1.0 - float(cfg.dropout))


def forward(params: Params, cfg: GRUConfig, x: torch.Tensor, h0: Optional[List[torch.Tensor]] = None,
            keep_cache: bool = False, dropout_step: Optional[int] = None, b0: int = 0):
    """x: [B, T] int ids.  Returns logits [B, T, V] (and per-layer caches if asked).

    dropout_step: None (every inference caller, and training without dropout) applies no mask; an int applies
    cfg.dropout's masks of that optimiser step to every layer's output as its consumer sees it, the batch's
    rows being sequences b0 .. b0 + B of the global batch."""
    B, T = x.shape
    drop = dropout_step is not None and cfg.dropout > 0
    H = cfg.hidden
    dt = params["fc.weight"].dtype
    inp = params["embedding"][x.long()]                       # [B, T, E]
    caches = []
    for l in range(cfg.layers):
        W_ih, W_hh = params[f"weight_ih_l{l}"], params[f"weight_hh_l{l}"]
        b_ih, b_hh = params[f"bias_ih_l{l}"], params[f"bias_hh_l{l}"]
        gi_all = inp @ W_ih.T + b_ih                          # hoisted input projection [B,T,3H]
        h = torch.zeros(B, H, dtype=dt) if h0 is None else h0[l]
        hs, rs, zs, ns, ghns, hprev = [], [], [], [], [], []
        for t in range(T):
            gh = h @ W_hh.T + b_hh
            hprev.append(h)
            h, (r, z, n, ghn) = _gates(gi_all[:, t], gh, h)
            hs.append(h); rs.append(r); zs.append(z); ns.append(n); ghns.append(ghn)
        out = torch.stack(hs, 1)                              # [B, T, H]
        if keep_cache:
            caches.append(dict(inp=inp, hprev=torch.stack(hprev, 1), r=torch.stack(rs, 1),
                               z=torch.stack(zs, 1), n=torch.stack(ns, 1), ghn=torch.stack(ghns, 1),
                               out=out))
        inp = out
        if drop:   # the consumer above reads d = m h / (1 - p); the recurrence above kept the unmasked h
            f = _dropout_factor(cfg, l, dropout_step, b0, B, T, dt)
            inp = out * f
            if keep_cache:
                caches[-1]["drop"] = f
                caches[-1]["dout"] = inp
    logits = inp @ params["fc.weight"].T + params["fc.bias"]
    return (logits, caches) if keep_cache else logits


def xent(logits: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """Mean next-char cross-entropy over valid (label >= 0) positions."""
    valid = y >= 0
    lp = torch.log_softmax(logits, -1)
    nll = -lp.gather(-1, y.clamp_min(0).long().unsqueeze(-1)).squeeze(-1)
    return (nll * valid).sum() / valid.sum().clamp_min(1)


def manual_backward(params: Params, cfg: GRUConfig, x: torch.Tensor, y: torch.Tensor,
                    h0: Optional[List[torch.Tensor]] = None, state_out: Optional[list] = None,
                    dropout_step: Optional[int] = None, b0: int = 0) -> Tuple[torch.Tensor, Params]:
    """Explicit BPTT. Returns (loss, grads) with grads keyed like params.

    h0: optional per-layer initial states (truncated BPTT: treated as constants, no gradient
    flows into them).  state_out: if a list, receives the per-layer final states h_{T-1}.
    dropout_step / b0: as in ``forward`` (None: no dropout); the gradient arriving at a layer's output from
    above is multiplied by the forward's m / (1 - p) before the BPTT."""
    logits, caches = forward(params, cfg, x, h0=h0, keep_cache=True, dropout_step=dropout_step, b0=b0)
    if state_out is not None:
        state_out[:] = [c["out"][:, -1].detach().clone() for c in caches]
    B, T, V = logits.shape
    H = cfg.hidden
    valid = (y >= 0)
    cnt = valid.sum().clamp_min(1)
    p = torch.softmax(logits, -1)
    onehot = torch.zeros_like(p).scatter_(-1, y.clamp_min(0).long().unsqueeze(-1), 1.0)
    dlog = (p - onehot) * (valid.unsqueeze(-1).to(p.dtype) / cnt.to(p.dtype))
    loss = xent(logits, y)
    g: Params = {}
    top = caches[-1].get("dout", caches[-1]["out"])   # what the head read
    g["fc.weight"] = dlog.reshape(-1, V).T @ top.reshape(-1, H)
    g["fc.bias"] = dlog.sum((0, 1))
    dy = dlog @ params["fc.weight"]                           # [B, T, H]
    for l in reversed(range(cfg.layers)):
        c = caches[l]
        if "drop" in c:
            dy = dy * c["drop"]
        W_hh = params[f"weight_hh_l{l}"]
        dgi = torch.zeros(B, T, 3 * H, dtype=dy.dtype)
        dgh = torch.zeros_like(dgi)
        dh_carry = torch.zeros(B, H, dtype=dy.dtype)          # z_{t+1}⊙dh_{t+1} + dGh_{t+1} W_hh
        for t in reversed(range(T)):
            dh = dy[:, t] + dh_carry
            r, z, n, ghn, hp = c["r"][:, t], c["z"][:, t], c["n"][:, t], c["ghn"][:, t], c["hprev"][:, t]
            dn = dh * (1 - z)
            dz = dh * (hp - n)
            dan = dn * (1 - n * n)
            dr = dan * ghn
            dar = dr * r * (1 - r)
            daz = dz * z * (1 - z)
            dgi[:, t] = torch.cat([dar, daz, dan], -1)
            dgh[:, t] = torch.cat([dar, daz, dan * r], -1)
            dh_carry = z * dh + dgh[:, t] @ W_hh
        g[f"weight_hh_l{l}"] = dgh.reshape(-1, 3 * H).T @ c["hprev"].reshape(-1, H)
        g[f"bias_hh_l{l}"] = dgh.sum((0, 1))
        g[f"weight_ih_l{l}"] = dgi.reshape(-1, 3 * H).T @ c["inp"].reshape(-1, c["inp"].shape[-1])
        g[f"bias_ih_l{l}"] = dgi.sum((0, 1))
        dy = dgi @ params[f"weight_ih_l{l}"]                  # grad wrt this layer's input
    demb = torch.zeros_like(params["embedding"])
    demb.index_add_(0, x.reshape(-1).long(), dy.reshape(-1, dy.shape[-1]))
    g["embedding"] = demb
    return loss, g


def autograd_grads(params: Params, cfg: GRUConfig, x: torch.Tensor, y: torch.Tensor,
                   h0: Optional[List[torch.Tensor]] = None, dropout_step: Optional[int] = None, b0: int = 0):
    ps = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    h0 = None if h0 is None else [h.detach() for h in h0]
    loss = xent(forward(ps, cfg, x, h0=h0, dropout_step=dropout_step, b0=b0), y)
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in ps.items()}


# --------------------------------------------------------------------------- optimiser
LR_SCHEDS = ("const", "cosine", "linear")


def lr_at(cfg: GRUConfig, t: int) -> float:
    """Learning rate of update t (1-based): linear warm-up over ``warmup_steps``, then constant,
    cosine or linear decay from ``lr`` to ``lr_min`` at ``total_steps`` -- the host twin of the
    device schedule in the Adam kernels (csrc/kernels/misc.hip sched_lr)."""
    if cfg.lr_sched not in LR_SCHEDS:
        raise ValueError(f"lr_sched must be one of {LR_SCHEDS}, got {cfg.lr_sched!r}")
    if cfg.warmup_steps > 0 and t <= cfg.warmup_steps:
        return cfg.lr * t / cfg.warmup_steps
    if cfg.lr_sched == "const" or cfg.total_steps <= cfg.warmup_steps:
        return cfg.lr
    p = min(1.0, (t - cfg.warmup_steps) / (cfg.total_steps - cfg.warmup_steps))
    f = 0.5 * (1.0 + math.cos(math.pi * p)) if cfg.lr_sched == "cosine" else 1.0 - p
    return cfg.lr_min + (cfg.lr - cfg.lr_min) * f


class Adam:
    """Functional Adam/SGD on a dict of fp32 tensors -- same update rule as the HIP
    ``optim`` kernel (bias-corrected Adam, decoupled weight decay, optional global
    norm clipping)."""

    def __init__(self, cfg: GRUConfig, params: Params):
        self.cfg = cfg
        self.step_n = 0
        self.m = {k: torch.zeros_like(v) for k, v in params.items()}
        self.v = {k: torch.zeros_like(v) for k, v in params.items()}

    def step(self, params: Params, grads: Params, advance: bool = True) -> None:
        """advance=False: a further part of the SAME step (the pipelined data-parallel tail updates
        the FC pair in a second launch with the step counter of the first)."""
        c = self.cfg
        scale = 1.0
        if c.clip_norm > 0:
            if not advance:
                raise ValueError("a split optimiser step cannot clip (needs the global norm)")
            norm = torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())).item()
            scale = min(1.0, c.clip_norm / (norm + 1e-6))
        if advance:
            self.step_n += 1
        lr = lr_at(c, self.step_n)
        if c.optimizer == "sgd":
            for k in params:
                params[k] -= lr * (grads[k] * scale + c.weight_decay * params[k])
            return
        b1, b2 = c.beta1, c.beta2
        bc1 = 1 - b1 ** self.step_n
        bc2 = 1 - b2 ** self.step_n
        for k in params:
            gk = grads[k] * scale
            self.m[k].mul_(b1).add_(gk, alpha=1 - b1)
            self.v[k].mul_(b2).addcmul_(gk, gk, value=1 - b2)
            upd = (self.m[k] / bc1) / (torch.sqrt(self.v[k] / bc2) + c.eps)
            if c.weight_decay:
                upd = upd + c.weight_decay * params[k]
            params[k] -= lr * upd


# --------------------------------------------------------------------------- scoring
def score_inputs(cfg: GRUConfig, rows: np.ndarray):
    """Teacher-forced schedule of output rows ([N, MAX_LEN+1] or flat uint8, the ``generate`` format).

    ``n_tok`` = index of the first EOS byte among c[0..ML-1] plus one, or ML when there is none -- the
    generator's stopping rule (EOS written, then stop), which also covers ``eos == 0`` where EOS and
    the NUL padding are the same byte.  Step l < n_tok has input SOS (l = 0) or c[l-1] and target
    c[l]; later bytes are ignored.  Returns (rows [N, ML+1], n_tok [N] int32, x [N, ML] int64 with
    masked steps = SOS, tgt [N, ML] int64 with masked steps = -1).  A byte >= vocab at an unmasked
    position is a caller error (ValueError)."""
    ML = cfg.max_len
    rows = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, ML + 1)
    if not 0 <= cfg.sos < cfg.vocab:
        raise ValueError(f"sos {cfg.sos} outside the vocabulary of {cfg.vocab}")
    c = rows[:, :ML].astype(np.int64)
    is_eos = c == cfg.eos
    n_tok = np.where(is_eos.any(1), is_eos.argmax(1) + 1, ML).astype(np.int32)
    mask = np.arange(ML)[None, :] < n_tok[:, None]
    if (c[mask] >= cfg.vocab).any():
        b = int(np.argwhere(mask & (c >= cfg.vocab))[0][0])
        raise ValueError(f"row {b} holds a byte >= vocab ({cfg.vocab}) among its {int(n_tok[b])} scored positions")
    tgt = np.where(mask, c, -1)
    x = np.full_like(c, cfg.sos)
    x[:, 1:] = np.where(mask[:, 1:], c[:, :-1], cfg.sos)
    return rows, n_tok, x, tgt


def score(params: Params, cfg: GRUConfig, rows: np.ndarray, temperature=None, top_k=None, top_p=None, prefix=None,
          constraints=None, logit_bias=None, presence_penalty=None, frequency_penalty=None, soft=None):
    """log P of output rows under the model, teacher-forced from a zero hidden state (score_inputs).

    Returns numpy (tok_logp [N, ML], name_logp [N], n_tok [N] int32, rank [N, ML] int32) in the dtype
    of ``params`` (fp64 params: the oracle).  tok_logp[l] = log softmax(logits_l)[c[l]]; rank[l] = the
    number of j with logit_j > logit_target, or equal and j < target (0: the arg-max is the target);
    name_logp = the tokens' sum in step order.  Masked positions: tok_logp 0, rank -1.
    exp(name_logp) is the probability that ``generate`` emits exactly that row.

    ``temperature`` / ``top_k`` / ``top_p`` / ``prefix`` / ``constraints`` (``generate``'s keywords, scalars or
    one value per row; docs/DESIGN.md §4f): any that is not None -- a neutral value too -- scores the row
    under the distribution ``generate`` samples from with these settings, and a fifth array is returned,
    n_kept [N, ML] int32 (masked -1).  At step l with target t:
      * forced (l < plen): tok_logp 0 if t == prefix[l], else -inf; n_kept 1;
      * greedy (T == 0): 0 if t is the lowest index of the maximum over the allowed set, else -inf; n_kept 1;
      * else K = the kept set of steps 3-6 above ``Controls`` inside the step's allowed set, n_kept = |K|,
        tok_logp = (y_t - max_K y) - log sum_K exp(y_j - max_K y) for t in K and exactly -inf outside.
    Never NaN; name_logp is the step-order sum, so one -inf makes it -inf: exp(name_logp) is the
    probability that ``generate`` with these settings emits exactly this row.  rank stays the model's
    rank on the raw logits, n_tok is read from the row alone.

    ``logit_bias`` / ``presence_penalty`` / ``frequency_penalty`` or ``soft`` (``generate``'s; docs/DESIGN.md
    §4h): they take the controlled rule too, on v = (x + bias) - pen with the counts of the scored row's
    bytes before the position; n_kept is the adjusted kept set's size, rank stays the model's."""
    ctl = cons = None
    soft_given = soft is not None or any(v is not None for v in (logit_bias, presence_penalty, frequency_penalty))
    if constraints is not None or soft_given or any(v is not None for v in (temperature, top_k, top_p, prefix)):
        count = np.ascontiguousarray(rows, dtype=np.uint8).size // (cfg.max_len + 1)
        soft = as_soft(cfg, count, soft, logit_bias, presence_penalty, frequency_penalty)
        cons = as_constraints(cfg, count, constraints)
        ctl = make_controls(cfg, count, temperature, top_k, top_p, prefix)
        check_prefix_allowed(cons, ctl.prefix, ctl.plen)
        if isinstance(cons, Automaton):   # the rows are known: walk them into per-(row, step) lines (§4g)
            cons = cons.for_rows(cfg, rows)
    rows, n_tok, x, tgt = score_inputs(cfg, rows)
    N, ML = tgt.shape
    dt = params["fc.weight"].dtype
    npdt = np.float64 if dt == torch.float64 else np.float32
    if N == 0:
        empty = (np.zeros((0, ML), npdt), np.zeros(0, npdt), n_tok, np.zeros((0, ML), np.int32))
        return empty if ctl is None else empty + (np.zeros((0, ML), np.int32),)
    logits = forward(params, cfg, torch.from_numpy(x))
    if dt != torch.float64:
        logits = logits.to(torch.float32)
    t = torch.from_numpy(tgt)
    mask = t >= 0
    tc = t.clamp_min(0).unsqueeze(-1)
    lp = torch.log_softmax(logits, -1).gather(-1, tc).squeeze(-1)
    lp = torch.where(mask, lp, torch.zeros_like(lp))
    xt = logits.gather(-1, tc)
    j = torch.arange(cfg.vocab).view(1, 1, -1)
    rank = ((logits > xt) | ((logits == xt) & (j < tc))).sum(-1)
    rank = torch.where(mask, rank, torch.full_like(rank, -1))
    n_kept = None
    if ctl is not None:
        lp, n_kept = _score_controlled(logits, tgt, mask, ctl, cons, soft, rows)
    name = torch.zeros(N, dtype=lp.dtype)
    for l in range(ML):   # step order, as the device sums
        name = name + lp[:, l]
    out = (lp.numpy(), name.numpy(), n_tok, rank.numpy().astype(np.int32))
    return out if ctl is None else out + (n_kept,)


def _score_controlled(logits: torch.Tensor, tgt: np.ndarray, mask: torch.Tensor, ctl: "Controls", cons,
                      soft: Optional["Soft"] = None, rows_u8: Optional[np.ndarray] = None):
    """tok_logp [N, ML] (torch) and n_kept [N, ML] int32 of ``score``'s controlled rule: per step the kept
    set of ``_filter`` and the log-softmax over it, formed in the log domain (no log of a rounded
    probability)."""
    N, ML, V = logits.shape
    dt = logits.dtype
    ninf = torch.tensor(-math.inf, dtype=dt)
    lp = torch.zeros(N, ML, dtype=dt)
    n_kept = np.full((N, ML), -1, np.int32)
    inv_t = torch.from_numpy(ctl.inv_temp)
    scale = torch.where(inv_t == 0, torch.ones_like(inv_t), inv_t).to(dt).unsqueeze(-1)
    rows = torch.arange(N)
    for l in range(ML):
        live = mask[:, l]
        if not live.any():
            continue
        t = torch.from_numpy(np.maximum(tgt[:, l], 0))
        xl = logits[:, l] if soft is None else soft_adjust(logits[:, l], soft, rows_u8[:, :l])   # §4h
        _, keep = _filter(xl, ctl.inv_temp, ctl.top_k, ctl.top_p, None if cons is None else cons.allowed(l))
        y = xl * scale                               # _filter's y: rounded once, in the logits' dtype
        # (with everything kept and T == 1 these are the plain call's operations: its bytes)
        ls = torch.log_softmax(torch.where(keep, y, ninf), -1)
        step = torch.where(keep[rows, t], ls[rows, t], ninf)
        nk = keep.sum(-1)
        forced = torch.from_numpy(ctl.plen > l)
        hit = torch.from_numpy(ctl.prefix[:, l].astype(np.int64)) == t
        step = torch.where(forced, torch.where(hit, torch.zeros_like(step), ninf), step)
        nk = torch.where(forced, torch.ones_like(nk), nk)
        lp[:, l] = torch.where(live, step, torch.zeros_like(step))
        n_kept[:, l] = np.where(live.numpy(), nk.numpy(), -1)
    return lp, n_kept


# --------------------------------------------------------------------------- generation
def sample_inverse_cdf(prob: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    """The reference's ``random_select`` (namegensf.cu:322-333): first i with an fp32
    running sum ``psum > r`` in index order, else n-1.  prob [N, V], r [N]."""
    # sequential prefix on CPU: fp32 like the reference, or fp64 for the exact-math oracle.  An explicit
    # loop over the vocabulary (vectorised over the names): torch.cumsum does not promise the strictly
    # left-to-right fp32 rounding of the reference's loop (a hypothesis case: 0.25 + 8.2e-9 + 8.2e-9
    # stays 0.25 sequentially but not in cumsum)
    p = prob if prob.dtype == torch.float64 else prob.to(torch.float32)
    cs = torch.empty_like(p)
    acc = torch.zeros_like(p[..., 0])
    for i in range(p.shape[-1]):
        acc = acc + p[..., i]
        cs[..., i] = acc
    hit = cs > r.unsqueeze(-1)
    idx = hit.to(torch.int64).argmax(-1)
    return torch.where(hit.any(-1), idx, torch.full_like(idx, prob.shape[-1] - 1))


# Sampling controls (docs/DESIGN.md §4b).  Per name: temperature T >= 0, top_k >= 0 (0: off), top_p in
# (0, 1] (1: off) and a prefix pre[0..plen) with plen <= max_len, no EOS byte and no byte >= vocab.
# At step l, with logits x[V]:
#   1. forced: l < plen -> the char is pre[l]; the uniform of the step is ignored (name n still owns
#      rfloats[n*MAX_LEN + l] by position), the char is written and fed back like a sampled one;
#   2. greedy: T == 0 -> the lowest index of the maximum logit; the uniform is ignored;
#   3. temperature: y = x * (1/T), 1/T rounded to fp32 once (T == 1 leaves y bitwise x);
#   4. top-k: keep i iff #{j : y_j > y_i} < k (ties with the k-th value all kept; k == 0 or k >= V: all);
#   5. softmax: q = max-subtracted softmax of y over the kept set, 0 elsewhere;
#   6. top-p: keep i iff sum{q_j : q_j > q_i} < p -- the smallest top set whose mass reaches p, ties
#      at the edge all kept, never empty (the maximum has mass 0 above it); p == 1: all;
#   7. sample: the softmax of y over the final kept set (= q renormalised), the first index in index
#      order whose running sum exceeds r, else the highest kept index (V - 1 with nothing filtered).
# Every rule is a set definition (no sort order), so ties give the same result in fp32 and fp64.
class Controls:
    """Validated per-name controls of ``count`` names: inv_temp float32 (1/T; 0 encodes T == 0),
    top_k int32, top_p float32, plen int32, prefix uint8 [count, max_len] (NUL past plen)."""

    def __init__(self, inv_temp, top_k, top_p, plen, prefix):
        self.inv_temp, self.top_k, self.top_p, self.plen, self.prefix = inv_temp, top_k, top_p, plen, prefix


def encode_prefixes(prefixes, cfg: GRUConfig) -> Tuple[np.ndarray, np.ndarray]:
    """Prefixes -> (rows [N, MAX_LEN] uint8, plen [N] int32).  ``prefixes``: a list of str (taken as
    latin-1) or bytes, or uint8 rows [N, MAX_LEN+1] as ``encode_names`` makes them (chars, then the EOS
    byte unless the row is full).  A prefix longer than max_len, one that holds the EOS byte or a byte
    >= vocab raises ValueError."""
    ML = cfg.max_len
    if isinstance(prefixes, np.ndarray):
        src = np.ascontiguousarray(prefixes, dtype=np.uint8).reshape(-1, ML + 1)[:, :ML]
        is_eos = src == cfg.eos
        plen = np.where(is_eos.any(1), is_eos.argmax(1), ML).astype(np.int32)
        rows = np.where(np.arange(ML)[None, :] < plen[:, None], src, 0).astype(np.uint8)
    else:
        rows = np.zeros((len(prefixes), ML), dtype=np.uint8)
        plen = np.zeros(len(prefixes), dtype=np.int32)
        for i, nm in enumerate(prefixes):
            try:
                b = nm.encode("latin-1") if isinstance(nm, str) else bytes(nm)
            except UnicodeEncodeError as e:
                raise ValueError(f"prefix {i} ({nm!r}) is not latin-1") from e
            if len(b) > ML:
                raise ValueError(f"prefix {i} ({nm!r}) has {len(b)} chars, more than max_len = {ML}")
            rows[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
            plen[i] = len(b)
    mask = np.arange(ML)[None, :] < plen[:, None]
    if (mask & (rows >= cfg.vocab)).any():
        i = int(np.argwhere(mask & (rows >= cfg.vocab))[0][0])
        raise ValueError(f"prefix {i} holds a byte >= vocab ({cfg.vocab})")
    if (mask & (rows == cfg.eos)).any():
        i = int(np.argwhere(mask & (rows == cfg.eos))[0][0])
        raise ValueError(f"prefix {i} contains the EOS byte {cfg.eos}")
    return rows, plen


def _per_name(v, n: int, dtype, what: str) -> np.ndarray:
    a = np.asarray(v, dtype=dtype)
    if a.ndim == 0:
        return np.full(n, a, dtype=dtype)
    if a.shape != (n,):
        raise ValueError(f"{what}: a scalar or {n} values expected, got shape {a.shape}")
    return np.ascontiguousarray(a)


def make_controls(cfg: GRUConfig, count: int, temperature=None, top_k=None, top_p=None, prefix=None) -> Controls:
    """Scalars or per-name arrays of ``count`` entries (None: the neutral value) -> Controls.  ``prefix``:
    one str / bytes for every name, or ``encode_prefixes`` input for ``count`` names.  Raises ValueError
    for T < 0 or not finite (or so extreme that 1/T is not a finite non-zero fp32), top_k < 0, top_p
    outside (0, 1] and a bad prefix."""
    T = _per_name(1.0 if temperature is None else temperature, count, np.float64, "temperature")
    if not np.isfinite(T).all() or (T < 0).any():
        raise ValueError("temperature must be finite and >= 0")
    with np.errstate(divide="ignore", over="ignore", under="ignore"):
        inv = np.where(T == 0, 0.0, 1.0 / np.where(T == 0, 1.0, T)).astype(np.float32)
    if (~np.isfinite(inv)).any() or ((inv == 0) & (T != 0)).any():
        raise ValueError("temperature: 1/T must be a finite non-zero fp32 value (or T == 0 for greedy)")
    kraw = np.asarray(0 if top_k is None else top_k)
    if kraw.dtype.kind == "f" and (kraw != np.floor(kraw)).any():
        raise ValueError("top_k must be an integer")
    k = _per_name(kraw, count, np.int64, "top_k")
    if (k < 0).any():
        raise ValueError("top_k must be >= 0 (0: off)")
    k = np.minimum(k, cfg.vocab).astype(np.int32)   # k >= V keeps everything
    p = _per_name(1.0 if top_p is None else top_p, count, np.float64, "top_p")
    if not ((p > 0) & (p <= 1)).all():
        raise ValueError("top_p must lie in (0, 1] (1: off)")
    p32 = p.astype(np.float32)
    if (p32 <= 0).any():
        raise ValueError("top_p must be a positive fp32 value")
    if prefix is None:
        rows, plen = np.zeros((count, cfg.max_len), np.uint8), np.zeros(count, np.int32)
    else:
        if isinstance(prefix, (str, bytes)):
            prefix = [prefix] * count
        rows, plen = encode_prefixes(prefix, cfg)
        if rows.shape[0] != count:
            raise ValueError(f"prefix: {count} prefixes expected, got {rows.shape[0]}")
    return Controls(inv, k, p32, plen, rows)


# Constraints (docs/DESIGN.md §4e): one more set definition in both rules.  Name n at step l has an
# allowed set A = line idx[n, l] of a table of bit masks (bit c % 32 of word c / 32 = char c); line 0 is
# "everything", so constrained and free names mix in one batch.
#   sampling (steps 2-7 above): y_i = -inf outside A, applied after the temperature scale.  Greedy is
#     the lowest index of the maximum over A; top-k keeps i iff i in A and #{j in A : y_j > y_i} < k (a
#     set smaller than k is kept whole, nothing outside A ever); softmax and top-p run over the kept
#     set; a masked char has probability exactly 0; the fallback is the highest kept index, inside A.
#     A forced step is unchanged.  With A = everything every operation and its order is the one above.
#   beam (step 3 below): a live beam offers c only if c is in A (and, while l < plen, only prefix[l]);
#     carries are not masked; scores stay the model's un-renormalised log-probabilities.
# The forced prefix is the special case of singleton sets.
CONSTRAINT_MAX_ROWS = 1024


class Constraints:
    """Per-position allowed sets of ``count`` names: tab uint32 [M, V/32] (line 0 all ones, lines
    distinct, M <= 1024), idx int32 [count, max_len].  (A vocabulary that is no multiple of 32 -- CPU
    only -- rounds the words up; the spare bits are 0.)"""

    def __init__(self, tab: np.ndarray, idx: np.ndarray, vocab: Optional[int] = None):
        self.tab, self.idx = tab, idx
        self.vocab = int(tab.shape[1]) * 32 if vocab is None else int(vocab)

    @property
    def rows(self) -> int:
        return int(self.tab.shape[0])

    def lines(self) -> np.ndarray:
        """The table as bool [M, V]."""
        bits = (self.tab[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & np.uint32(1)
        return bits.reshape(self.tab.shape[0], -1).astype(bool)[:, :self.vocab]

    def allowed(self, step: Optional[int] = None) -> np.ndarray:
        """bool [count, V] of a step, or [count, max_len, V] of all."""
        ln = self.lines()
        return ln[self.idx] if step is None else ln[self.idx[:, step]]

    def slice(self, start: int, count: int) -> "Constraints":
        """Names start .. start + count - 1 (the table is shared)."""
        return Constraints(self.tab, np.ascontiguousarray(self.idx[start:start + count]), self.vocab)


def _as_bytes(v, what: str) -> bytes:
    try:
        return v.encode("latin-1") if isinstance(v, str) else bytes(v)
    except UnicodeEncodeError as e:
        raise ValueError(f"{what} {v!r} is not latin-1") from e


def _parse_pattern(pat: bytes, cfg: GRUConfig, cs: np.ndarray) -> List[np.ndarray]:
    """One bool [V] set per pattern item.  cs: the charset as bool [V]."""
    V = cfg.vocab
    items = []

    def one(c: int) -> np.ndarray:
        if c >= V:
            raise ValueError(f"pattern {pat!r} names byte {c} >= vocab ({V})")
        if c == cfg.eos:
            raise ValueError(f"pattern {pat!r} names the EOS byte {cfg.eos} (lengths are set by min_len / max_len)")
        s = np.zeros(V, bool)
        s[c] = True
        return s

    i, n = 0, len(pat)
    while i < n:
        c = pat[i]
        if c == 0x5C:                                   # backslash: the next char, literally
            if i + 1 >= n:
                raise ValueError(f"pattern {pat!r} ends in a backslash")
            items.append(one(pat[i + 1]))
            i += 2
        elif c == 0x2E:                                 # .
            items.append(cs.copy())
            i += 1
        elif c == 0x5B:                                 # [ ... ]
            i += 1
            neg = i < n and pat[i] == 0x5E
            if neg:
                i += 1
            s = np.zeros(V, bool)
            members = 0
            while True:
                if i >= n:
                    raise ValueError(f"pattern {pat!r}: a class without its ']'")
                if pat[i] == 0x5D:
                    i += 1
                    break
                if pat[i] == 0x5C:
                    if i + 1 >= n:
                        raise ValueError(f"pattern {pat!r} ends in a backslash")
                    i += 1
                lo = pat[i]
                i += 1
                hi = lo
                if i + 1 < n and pat[i] == 0x2D and pat[i + 1] != 0x5D:   # a-z
                    i += 1
                    if pat[i] == 0x5C:
                        if i + 1 >= n:
                            raise ValueError(f"pattern {pat!r} ends in a backslash")
                        i += 1
                    hi = pat[i]
                    i += 1
                    if hi < lo:
                        raise ValueError(f"pattern {pat!r}: range {chr(lo)}-{chr(hi)} runs backwards")
                for ch in range(lo, hi + 1):
                    s |= one(ch)
                members += 1
            if not members:
                raise ValueError(f"pattern {pat!r}: an empty class")
            items.append(cs & ~s if neg else s)
        elif c == 0x5D:
            raise ValueError(f"pattern {pat!r}: a ']' without its class (write \\])")
        else:
            items.append(one(c))
            i += 1
    return items


def _name_sets(cfg: GRUConfig, pattern, charset, min_len, max_len) -> np.ndarray:
    """bool [max_len, V]: the allowed set of every step of one name (all ones = no constraint)."""
    ML, V, eos = cfg.max_len, cfg.vocab, cfg.eos
    if not 0 <= eos < V:
        raise ValueError(f"eos {eos} outside the vocabulary of {V}")
    cs = np.ones(V, bool)
    if charset is not None:
        b = np.frombuffer(_as_bytes(charset, "charset"), dtype=np.uint8)
        if (b >= V).any():
            raise ValueError(f"charset names a byte >= vocab ({V})")
        if (b == eos).any():
            raise ValueError(f"charset names the EOS byte {eos} (lengths are set by min_len / max_len)")
        cs[:] = False
        cs[b] = True
    cs[eos] = False
    items = [] if pattern is None else _parse_pattern(_as_bytes(pattern, "pattern"), cfg, cs)
    if len(items) > ML:
        raise ValueError(f"pattern {pattern!r} has {len(items)} items, more than max_len = {ML}")
    lo = max(0 if min_len is None else int(min_len), len(items))
    hi = ML if max_len is None else int(max_len)
    if (min_len is not None and int(min_len) < 0) or hi < 0 or hi > ML:
        raise ValueError(f"min_len >= 0 and 0 <= max_len <= {ML} expected, got {min_len!r} and {max_len!r}")
    free = pattern is None and charset is None and lo == 0 and hi == ML
    sets = np.ones((ML, V), bool)
    for l in range(ML):
        if free or l > hi:       # past the forced EOS no step is reached: no constraint
            continue
        if l == hi:              # (hi < ML) only EOS: the name has at most hi chars
            s = np.zeros(V, bool)
        else:
            s = items[l].copy() if l < len(items) else cs.copy()
        s[eos] = l >= lo
        if not s.any():
            raise ValueError(f"no char is allowed at step {l} (pattern {pattern!r}, charset {charset!r}, "
                             f"min_len {lo}, max_len {hi})")
        sets[l] = s
    return sets


def _per_name_obj(v, n: int, what: str) -> list:
    if v is None or isinstance(v, (str, bytes)) or np.ndim(v) == 0:
        return [v] * n
    if len(v) != n:
        raise ValueError(f"{what}: one value or {n} values expected, got {len(v)}")
    return list(v)


def make_constraints(cfg: GRUConfig, count: int, pattern=None, charset=None, min_len=None, max_len=None,
                     regex=None, exclude=None):
    """Each argument: one value for all ``count`` names or one per name (None: no such constraint).
    ``regex`` / ``exclude`` (never with ``pattern``): the result is an ``Automaton`` (``make_automaton``
    below, docs/DESIGN.md §4g) instead of a Constraints object; without them nothing changes.
    ``charset``: the non-EOS chars a name may use (str / bytes; default every char but EOS).  ``pattern``:
    one item per position, no quantifiers -- a literal char, ``\\`` + a literal char, ``.`` (any char of
    charset), ``[abc]`` / ``[a-z]`` / ``[^...]`` classes (a negated class is taken inside charset); P items
    imply min_len >= P and positions past the pattern follow charset.  ``min_len`` = m: no EOS at steps
    < m.  ``max_len`` = M <= cfg.max_len: only EOS at step M (when M < cfg.max_len).  ValueError for an
    empty allowed set at any step, a byte >= vocab, a malformed or too long pattern, and more than 1024
    distinct sets."""
    count = int(count)
    if count < 0:
        raise ValueError("count must be >= 0")
    if regex is not None or exclude is not None:
        if pattern is not None:
            raise ValueError("pattern cannot be combined with regex / exclude (write the pattern as a regex)")
        return make_automaton(cfg, count, regex, exclude, charset, min_len, max_len)
    ML, V = cfg.max_len, cfg.vocab
    cols = [_per_name_obj(v, count, w) for v, w in ((pattern, "pattern"), (charset, "charset"),
                                                    (min_len, "min_len"), (max_len, "max_len"))]
    if count == 0:   # still validate single values
        _name_sets(cfg, *[None if v is not None and not isinstance(v, (str, bytes)) and np.ndim(v) else v
                          for v in (pattern, charset, min_len, max_len)])
    lines: Dict[bytes, int] = {np.ones(V, bool).tobytes(): 0}
    per_name: Dict[tuple, np.ndarray] = {}
    idx = np.zeros((count, ML), np.int32)
    for n in range(count):
        key = tuple(None if v is None else (_as_bytes(v, "pattern / charset") if isinstance(v, (str, bytes)) else int(v))
                    for v in (cols[0][n], cols[1][n], cols[2][n], cols[3][n]))
        row = per_name.get(key)
        if row is None:
            sets = _name_sets(cfg, *key)
            row = np.zeros(ML, np.int32)
            for l in range(ML):
                row[l] = lines.setdefault(sets[l].tobytes(), len(lines))
            per_name[key] = row
        idx[n] = row
    if len(lines) > CONSTRAINT_MAX_ROWS:
        raise ValueError(f"{len(lines)} distinct allowed sets, more than {CONSTRAINT_MAX_ROWS}")
    bits = np.stack([np.frombuffer(k, dtype=bool) for k in lines])            # insertion order = line number
    words = -(-V // 32)
    bits = np.concatenate([bits, np.zeros((len(lines), words * 32 - V), bool)], 1)
    w = (bits.reshape(len(lines), words, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1)
    return Constraints(np.ascontiguousarray(w.astype(np.uint32)), idx, V)


def as_constraints(cfg: GRUConfig, count: int, constraints):
    """None, a Constraints or Automaton object for ``count`` names, or a dict of make_constraints keywords
    (``regex`` / ``exclude`` among them give an Automaton)."""
    if isinstance(constraints, Automaton):
        return _check_automaton(cfg, count, constraints)
    if constraints is None or isinstance(constraints, Constraints):
        c = constraints
    elif isinstance(constraints, dict):
        c = make_constraints(cfg, count, **constraints)
    else:
        raise ValueError("constraints: a Constraints object or a dict of make_constraints keywords expected")
    if isinstance(c, Automaton):
        return _check_automaton(cfg, count, c)
    if c is not None:
        if (c.idx.shape != (count, cfg.max_len) or c.tab.ndim != 2 or c.tab.shape[1] != -(-cfg.vocab // 32)
                or c.vocab != cfg.vocab):
            raise ValueError(f"constraints: idx [{count}, {cfg.max_len}] and tab [M, {-(-cfg.vocab // 32)}] for a vocabulary "
                             f"of {cfg.vocab} expected, got {c.idx.shape}, {c.tab.shape} and {c.vocab}")
        if not 1 <= c.rows <= CONSTRAINT_MAX_ROWS:
            raise ValueError(f"constraints: 1 .. {CONSTRAINT_MAX_ROWS} table lines expected, got {c.rows}")
        if c.idx.size and (c.idx.min() < 0 or c.idx.max() >= c.rows):
            raise ValueError("constraints: an idx entry outside the table")
    return c


def check_prefix_allowed(cons: Optional[Constraints], prefix: np.ndarray, plen: np.ndarray) -> None:
    """ValueError when a forced char is not in its step's set (an Automaton: when the walk from the
    name's start state rejects it)."""
    if cons is None or not len(plen) or not plen.any():
        return
    if isinstance(cons, Automaton):
        lines, state = cons.lines(), cons.start.astype(np.int64)
        for l in range(prefix.shape[1]):
            c = prefix[:, l].astype(np.int64)
            bad = (plen > l) & ~lines[state, c]
            if bad.any():
                n = int(np.flatnonzero(bad)[0])
                raise ValueError(f"prefix {n}: char {int(prefix[n, l])} at position {l} is not allowed by the constraint")
            state = np.where(plen > l, cons.nxt[state, c].astype(np.int64), state)
        return
    ML = prefix.shape[1]
    ok = np.take_along_axis(cons.allowed(), prefix.astype(np.int64)[:, :, None], 2)[:, :, 0]
    bad = (np.arange(ML)[None, :] < plen[:, None]) & ~ok
    if bad.any():
        n, l = (int(v) for v in np.argwhere(bad)[0])
        raise ValueError(f"prefix {n}: char {int(prefix[n, l])} at position {l} is not allowed by the constraint")


# Automaton constraints (docs/DESIGN.md §4g): the allowed set depends on what the name has emitted, not on
# the step number.  A name carries a state q; its set at a step is line q of ``tab`` and after the step's
# char c -- sampled, greedy or forced -- the state is nxt[q][c].  Everything else in the rules above is
# unchanged: Constraints is the special case "state = step".
#   * state 0 is the free state (line all ones, nxt[0][*] = 0): unconstrained names of a mixed batch;
#   * nxt[q][eos] = 0, so a finished row, which keeps stepping, stays in range;
#   * nxt[q][c] = 0 for c outside tab[q]: never taken by the sampler; ``score`` walks known rows on the
#     host and such a row is -inf at that step whatever follows, so its later steps use line 0;
#   * the step counter is folded into the state: the builder takes the product of the language DFA with
#     l = 0 .. max_len and keeps at (q, l) only the chars from whose successor an accepting state is
#     still reachable within the remaining chars and the length bounds.  EOS is allowed iff q accepts and
#     l >= min_len, and at l = max_len - 1 (the config's) a char is allowed iff its successor accepts, as
#     a full-length row has no EOS step.  A name can never reach a dead end.
# beam: a state per beam; a child's state is nxt[parent's state][c], a carried or dead beam's is 0.
AUTOMATON_MAX_STATES = 65535


class Automaton:
    """tab uint32 [S, V/32] (the states' allowed sets, the EOS bit set where the state accepts), nxt
    uint16 [S, V] (the successor), start int32 [count] (the names' start states); S <= 65535."""

    def __init__(self, tab: np.ndarray, nxt: np.ndarray, start: np.ndarray, vocab: Optional[int] = None):
        self.tab, self.nxt, self.start = tab, nxt, start
        self.vocab = int(nxt.shape[1]) if vocab is None else int(vocab)

    @property
    def states(self) -> int:
        return int(self.tab.shape[0])

    rows = states   # the table's lines, as Constraints.rows

    def lines(self) -> np.ndarray:
        """The table as bool [S, V]."""
        bits = (self.tab[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & np.uint32(1)
        return bits.reshape(self.tab.shape[0], -1).astype(bool)[:, :self.vocab]

    def slice(self, start: int, count: int) -> "Automaton":
        """Names start .. start + count - 1 (the tables are shared)."""
        return Automaton(self.tab, self.nxt, np.ascontiguousarray(self.start[start:start + count]), self.vocab)

    def for_rows(self, cfg: GRUConfig, rows: np.ndarray) -> Constraints:
        """The per-(row, step) lines of known output rows, as ``score`` needs them: row n walks from
        start[n]; after a char outside its set (the row is -inf from there) the later steps use line 0.
        The lines used are renumbered into a table of their own (ValueError above 1024 distinct ones)."""
        ML, V = cfg.max_len, cfg.vocab
        c = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, ML + 1)[:, :ML].astype(np.int64)
        if c.shape[0] != self.start.shape[0]:
            raise ValueError(f"constraints for {self.start.shape[0]} rows, {c.shape[0]} rows given")
        state = self.start.astype(np.int64)
        idx = np.zeros((c.shape[0], ML), np.int64)
        for l in range(ML):
            idx[:, l] = state
            state = self.nxt[state, np.minimum(c[:, l], V - 1)].astype(np.int64)   # (0 after EOS: the steps past it are masked)
        seen: Dict[bytes, int] = {self.tab[0].tobytes(): 0}
        used = np.unique(idx)
        remap = np.zeros(self.states, np.int32)
        for u in used:
            remap[u] = seen.setdefault(self.tab[u].tobytes(), len(seen))
        if len(seen) > CONSTRAINT_MAX_ROWS:
            raise ValueError(f"the rows pass through {len(seen)} distinct allowed sets, more than {CONSTRAINT_MAX_ROWS}: "
                             "score them in smaller groups")
        tab = np.stack([np.frombuffer(k, dtype=np.uint32) for k in seen])
        return Constraints(np.ascontiguousarray(tab), remap[idx], V)


def _check_automaton(cfg: GRUConfig, count: int, a: Automaton) -> Automaton:
    words, V = -(-cfg.vocab // 32), cfg.vocab
    if (a.tab.ndim != 2 or a.tab.shape[1] != words or a.nxt.shape != (a.tab.shape[0], V) or a.start.shape != (count,)
            or a.vocab != V):
        raise ValueError(f"constraints: an automaton with tab [S, {words}], nxt [S, {V}] and start [{count}] expected, got "
                         f"{a.tab.shape}, {a.nxt.shape} and {a.start.shape}")
    if not 1 <= a.states <= AUTOMATON_MAX_STATES:
        raise ValueError(f"constraints: 1 .. {AUTOMATON_MAX_STATES} automaton states expected, got {a.states}")
    if (a.start.size and (a.start.min() < 0 or a.start.max() >= a.states)) or int(a.nxt.max()) >= a.states:
        raise ValueError("constraints: a start or nxt entry outside the automaton")
    return a


_RX_SPECIAL = frozenset(b"|()*+?{}[]^$")


def _parse_regex(rx: bytes, cfg: GRUConfig, cs: np.ndarray):
    """Regex -> AST: ("set", bool [V]) | ("cat", [..]) | ("alt", [..]) | ("rep", x, m, n or None).  The
    atoms are ``_parse_pattern``'s (a backslash makes the next byte literal, whatever it is); on top of them
    groups, ``|``, ``* + ?`` and ``{m} {m,} {m,n}``.  Anchors and ``(?`` forms raise."""
    n = len(rx)
    pos = [0]

    def err(msg):
        raise ValueError(f"regex {rx!r}: {msg}")

    def alt():
        parts = [cat()]
        while pos[0] < n and rx[pos[0]] == 0x7C:
            pos[0] += 1
            parts.append(cat())
        return parts[0] if len(parts) == 1 else ("alt", parts)

    def cat():
        items = []
        while pos[0] < n and rx[pos[0]] not in (0x7C, 0x29):
            items.append(rep())
        return ("cat", items)

    def number():
        i = pos[0]
        while pos[0] < n and 0x30 <= rx[pos[0]] <= 0x39:
            pos[0] += 1
        return int(rx[i:pos[0]]) if pos[0] > i else None

    def rep():
        x = atom()
        if pos[0] < n and rx[pos[0]] in b"*+?{":
            c = rx[pos[0]]
            pos[0] += 1
            if c == 0x2A:
                x = ("rep", x, 0, None)
            elif c == 0x2B:
                x = ("rep", x, 1, None)
            elif c == 0x3F:
                x = ("rep", x, 0, 1)
            else:
                m = number()
                if m is None:
                    err("'{' needs a count ({m}, {m,} or {m,n}; write \\{ for the char)")
                hi = m
                if pos[0] < n and rx[pos[0]] == 0x2C:
                    pos[0] += 1
                    hi = number()
                if pos[0] >= n or rx[pos[0]] != 0x7D:
                    err("a '{' without its '}'")
                pos[0] += 1
                if hi is not None and hi < m:
                    err(f"{{{m},{hi}}} runs backwards")
                x = ("rep", x, m, hi)
            if pos[0] < n and rx[pos[0]] in b"*+?{":
                err("a quantifier after a quantifier (group the first: (a*)?)")
        return x

    def atom():
        c = rx[pos[0]]
        if c == 0x28:
            if pos[0] + 1 < n and rx[pos[0] + 1] == 0x3F:
                err("'(?' forms are not supported")
            pos[0] += 1
            x = alt()
            if pos[0] >= n or rx[pos[0]] != 0x29:
                err("a '(' without its ')'")
            pos[0] += 1
            return x
        i = pos[0]
        if c == 0x5C:
            if i + 1 >= n:
                err("ends in a backslash")
            pos[0] += 2
        elif c == 0x5B:
            j = i + 1
            if j < n and rx[j] == 0x5E:
                j += 1
            while j < n and rx[j] != 0x5D:
                j += 2 if rx[j] == 0x5C else 1
            if j >= n:
                err("a class without its ']'")
            pos[0] = j + 1
        elif c in _RX_SPECIAL:
            err(f"a {chr(c)!r} that is no operator here (anchors are not supported; write \\{chr(c)} for the char)")
        else:
            pos[0] += 1
        try:
            return ("set", _parse_pattern(rx[i:pos[0]], cfg, cs)[0])
        except ValueError as e:
            raise ValueError(str(e).replace("pattern", "regex", 1)) from None

    x = alt()
    if pos[0] < n:
        err("a ')' without its '('")
    return x


def _rx_nullable(x) -> bool:
    if x[0] == "set":
        return False
    if x[0] == "cat":
        return all(_rx_nullable(y) for y in x[1])
    if x[0] == "alt":
        return any(_rx_nullable(y) for y in x[1])
    return x[2] == 0 or _rx_nullable(x[1])


def _regex_dfa(rx: bytes, cfg: GRUConfig, cs: np.ndarray):
    """(delta int32 [Q, V] with -1 = no move, accept bool [Q]) of the regex's language, state 0 the start:
    Thompson's construction, then the subset construction over the classes of chars that no set of the
    regex tells apart."""
    ML, V = cfg.max_len, cfg.vocab
    ast = _parse_regex(rx, cfg, cs)
    eps: List[List[int]] = []
    moves: List[List[Tuple[int, int]]] = []
    sets: List[np.ndarray] = []
    set_id: Dict[bytes, int] = {}

    def new() -> int:
        if len(eps) >= 50000:
            raise ValueError(f"regex {rx!r} is too large")
        eps.append([])
        moves.append([])
        return len(eps) - 1

    def build(x, a: int) -> int:
        """x's fragment from state a; returns its end state."""
        if x[0] == "set":
            k = set_id.setdefault(x[1].tobytes(), len(sets))
            if k == len(sets):
                sets.append(x[1])
            b = new()
            moves[a].append((k, b))
            return b
        if x[0] == "cat":
            for y in x[1]:
                a = build(y, a)
            return a
        if x[0] == "alt":
            b = new()
            for y in x[1]:
                s = new()
                eps[a].append(s)
                eps[build(y, s)].append(b)
            return b
        _, y, m, hi = x
        # within max_len chars more copies than that only add empty matches: x{m,n} with n >= max(m, ML) is x{m,}
        if _rx_nullable(y):
            m = 0
        elif m > ML:
            return new()   # too long for any name: a fragment whose end is never reached
        if hi is not None and hi >= max(m, ML):
            hi = None
        for _ in range(m):
            a = build(y, a)
        if hi is None:   # star
            s, b = new(), new()
            eps[a] += [s, b]
            eps[build(y, s)] += [s, b]
            return b
        b = new()
        eps[a].append(b)
        for _ in range(hi - m):
            a = build(y, a)
            eps[a].append(b)
        return b

    s0 = new()
    end = build(ast, s0)
    # chars that lie in the same sets move alike
    if sets:
        _, cls = np.unique(np.stack(sets).T, axis=0, return_inverse=True)
        cls = cls.reshape(-1)
    else:
        cls = np.zeros(V, np.int64)
    ncls = int(cls.max()) + 1
    member = np.zeros((len(sets), ncls), bool)
    for k, st in enumerate(sets):
        member[k, cls[st]] = True

    def closure(states) -> frozenset:
        seen, todo = set(states), list(states)
        while todo:
            for t in eps[todo.pop()]:
                if t not in seen:
                    seen.add(t)
                    todo.append(t)
        return frozenset(seen)

    d0 = closure([s0])
    ids = {d0: 0}
    order = [d0]
    rows = []
    i = 0
    while i < len(order):
        cur = order[i]
        i += 1
        tg: List[set] = [set() for _ in range(ncls)]
        for a in cur:
            for k, b in moves[a]:
                for j in np.flatnonzero(member[k]):
                    tg[j].add(b)
        row = np.full(ncls, -1, np.int32)
        for j in range(ncls):
            if tg[j]:
                d = closure(tg[j])
                if d not in ids:
                    if len(order) >= 200000:
                        raise ValueError(f"regex {rx!r} needs too many states")
                    ids[d] = len(order)
                    order.append(d)
                row[j] = ids[d]
        rows.append(row)
    delta = np.stack(rows)[:, cls]
    return np.ascontiguousarray(delta), np.array([end in d for d in order])


def _exclude_dfa(names, cfg: GRUConfig):
    """(delta, accept) of "every string but these": the names' trie plus a co-accepting sink (the last
    state).  Names longer than max_len cannot be emitted anyway and are skipped."""
    ML, V = cfg.max_len, cfg.vocab
    kids: List[Dict[int, int]] = [{}]
    listed = [False]
    for i, nm in enumerate(names):
        b = _as_bytes(nm, "exclude name")
        if any(c >= V for c in b):
            raise ValueError(f"exclude: name {i} ({nm!r}) holds a byte >= vocab ({V})")
        if cfg.eos in b:
            raise ValueError(f"exclude: name {i} ({nm!r}) contains the EOS byte {cfg.eos}")
        if len(b) > ML:
            continue
        q = 0
        for c in b:
            t = kids[q].get(c)
            if t is None:
                t = kids[q][c] = len(kids)
                kids.append({})
                listed.append(False)
            q = t
        listed[q] = True
    T = len(kids)
    delta = np.full((T + 1, V), T, np.int32)
    for q, kd in enumerate(kids):
        for c, t in kd.items():
            delta[q, c] = t
    return delta, ~np.array(listed + [False])


def _product_dfa(d1, a1, d2, a2):
    """The intersection of two DFAs (the second total), only the pairs reachable from (0, 0)."""
    Q2 = d2.shape[0]
    ids = {0: 0}
    order = [0]
    rows = []
    i = 0
    while i < len(order):
        q1, q2 = divmod(order[i], Q2)
        i += 1
        n1 = d1[q1].astype(np.int64)
        key = np.where(n1 >= 0, n1 * Q2 + d2[q2], -1)
        row = np.full(key.shape, -1, np.int32)
        for k in np.unique(key[key >= 0]):
            t = ids.get(int(k))
            if t is None:
                t = ids[int(k)] = len(order)
                order.append(int(k))
            row[key == k] = t
        rows.append(row)
    o = np.array(order)
    return np.stack(rows), a1[o // Q2] & a2[o % Q2]


def _name_automaton(cfg: GRUConfig, regex, exclude, charset, min_len, max_len):
    """One name's states: (sets bool [S, V], nxt int32 [S, V] with local numbers, -1 = none); state 0 is
    (start, step 0).  The product of the language DFA with the step counter, pruned so that no state is
    a dead end."""
    ML, V, eos = cfg.max_len, cfg.vocab, cfg.eos
    if not 0 <= eos < V:
        raise ValueError(f"eos {eos} outside the vocabulary of {V}")
    cs = np.ones(V, bool)
    if charset is not None:
        b = np.frombuffer(_as_bytes(charset, "charset"), dtype=np.uint8)
        if (b >= V).any():
            raise ValueError(f"charset names a byte >= vocab ({V})")
        if (b == eos).any():
            raise ValueError(f"charset names the EOS byte {eos} (lengths are set by min_len / max_len)")
        cs[:] = False
        cs[b] = True
    cs[eos] = False
    lo = 0 if min_len is None else int(min_len)
    hi = ML if max_len is None else int(max_len)
    if lo < 0 or hi < 0 or hi > ML:
        raise ValueError(f"min_len >= 0 and 0 <= max_len <= {ML} expected, got {min_len!r} and {max_len!r}")
    if regex is None:   # charset*
        delta, acc = np.where(cs, 0, -1).astype(np.int32)[None, :], np.ones(1, bool)
    else:
        delta, acc = _regex_dfa(_as_bytes(regex, "regex"), cfg, cs)
    if exclude is not None:
        delta, acc = _product_dfa(delta, acc, *_exclude_dfa(exclude, cfg))
    what = f"(regex {regex!r}, {0 if exclude is None else len(exclude)} excluded, charset {charset!r}, min_len {lo}, max_len {hi})"
    # ok[l][q]: from q after l chars a name can still end within the bounds
    dc = np.maximum(delta, 0)
    ok = [None] * (hi + 1)
    ok[hi] = acc & (hi >= lo)
    for l in range(hi - 1, -1, -1):
        ok[l] = (acc & (l >= lo)) | ((delta >= 0) & ok[l + 1][dc]).any(1)
    if not ok[0][0]:
        raise ValueError(f"no name is allowed {what}")
    sets, nxts = [], []
    front, base = np.array([0]), 0
    for l in range(hi + 1):
        if l >= ML:   # (hi == ML) a full-length row has no EOS step
            break
        s = np.zeros((len(front), V), bool)
        nx = np.full((len(front), V), -1, np.int64)
        if l < hi:
            d = delta[front]
            s = (d >= 0) & ok[l + 1][np.maximum(d, 0)]
            if l + 1 < ML and l + 1 <= hi:
                nfront = np.unique(d[s])
                nx = np.where(s, base + len(front) + np.searchsorted(nfront, np.where(s, d, nfront[0] if len(nfront) else 0)), -1)
            else:
                nfront = np.zeros(0, np.int64)
        else:
            nfront = np.zeros(0, np.int64)
        s[:, eos] = acc[front] & (l >= lo)
        sets.append(s)
        nxts.append(nx)
        base += len(front)
        front = nfront
        if not len(front):
            break
    return np.concatenate(sets), np.concatenate(nxts)


def _pack_lines(bits: np.ndarray, V: int) -> np.ndarray:
    words = -(-V // 32)
    bits = np.concatenate([bits, np.zeros((bits.shape[0], words * 32 - V), bool)], 1)
    w = (bits.reshape(bits.shape[0], words, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1)
    return np.ascontiguousarray(w.astype(np.uint32))


def _merge_states(tab: np.ndarray, nxt: np.ndarray, start: np.ndarray):
    """States with equal (line, successor row) are one state; repeated until nothing merges.  State 0
    stays state 0 (the survivors keep their order of first appearance)."""
    mix = np.random.default_rng(0).integers(1, 2 ** 62, tab.shape[1] + nxt.shape[1], dtype=np.int64) | 1
    while True:
        key = np.concatenate([tab.astype(np.int64), nxt], 1)
        with np.errstate(over="ignore"):
            h = (key * mix).sum(1)   # a hash first (wrapping int64): sorting whole rows is slow for a large trie
        _, first, inv = np.unique(h, return_index=True, return_inverse=True)
        if not (key == key[first[inv.reshape(-1)]]).all():   # a collision: the exact way
            _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
        if len(first) == tab.shape[0]:
            return tab, nxt, start
        order = np.argsort(first)
        rank = np.empty_like(order)
        rank[order] = np.arange(len(order))
        inv, first = rank[inv.reshape(-1)], first[order]
        tab, nxt, start = tab[first], inv[nxt[first]], inv[start]


def _exclude_key(v):
    if v is None:
        return None
    return tuple(sorted({_as_bytes(x, "exclude name") for x in v}))


def make_automaton(cfg: GRUConfig, count: int, regex=None, exclude=None, charset=None, min_len=None,
                   max_len=None) -> Automaton:
    """``make_constraints(regex=, exclude=)``.  ``regex`` (str / bytes over latin-1 bytes, matched against the
    whole name): ``_parse_pattern``'s atoms -- literals, ``\\c``, ``.`` and classes, ``.`` and negated classes
    inside charset -- plus groups ``( )``, alternation ``|`` and the quantifiers ``* + ? {m} {m,} {m,n}``: a
    subset of Python ``re`` (but for ``\\`` before a letter or digit, which is that byte here).  ``exclude``: a
    list of names none of which may be generated (one list for every name, or a list of lists / None
    per name; names longer than cfg.max_len are skipped).  They combine with each other -- the
    intersection -- and with ``charset`` (alone: the chars a name without a regex may use), ``min_len`` and
    ``max_len``.  A name with none of the five is free (state 0).  ValueError for a language that is empty
    within the bounds, a byte >= vocab, the EOS byte in the regex, charset or a listed name, a malformed
    regex and more than 65535 states after merging."""
    count = int(count)
    ML, V = cfg.max_len, cfg.vocab
    if exclude is not None and not isinstance(exclude, (str, bytes)) and all(isinstance(x, (str, bytes)) for x in exclude):
        ex = [_exclude_key(exclude)] * count
        ex_single = True
    elif exclude is None:
        ex, ex_single = [None] * count, True
    else:
        if isinstance(exclude, (str, bytes)):
            raise ValueError("exclude: a list of names expected")
        if len(exclude) != count:
            raise ValueError(f"exclude: one list of names or {count} lists expected, got {len(exclude)}")
        ex, ex_single = [_exclude_key(x) for x in exclude], False
    given = ((regex, "regex"), (charset, "charset"), (min_len, "min_len"), (max_len, "max_len"))
    cols = [_per_name_obj(v, count, w) for v, w in given]
    if count == 0 and ex_single and all(v is None or isinstance(v, (str, bytes)) or np.ndim(v) == 0 for v, _ in given):
        _name_automaton(cfg, regex, _exclude_key(exclude), charset, min_len, max_len)   # still validate single values
    sets = [np.ones((1, V), bool)]
    nxts = [np.zeros((1, V), np.int64)]
    total = 1
    first: Dict[tuple, int] = {}
    start = np.zeros(count, np.int64)
    for n in range(count):
        key = tuple(None if v is None else (_as_bytes(v, "regex / charset") if isinstance(v, (str, bytes)) else int(v))
                    for v in (cols[0][n], cols[1][n], cols[2][n], cols[3][n])) + (ex[n],)
        if all(v is None for v in key):
            continue   # a free name: state 0
        if key not in first:
            s, nx = _name_automaton(cfg, key[0], key[4], key[1], key[2], key[3])
            first[key] = total
            sets.append(s)
            nxts.append(np.where(nx >= 0, nx + total, 0))
            total += s.shape[0]
        start[n] = first[key]
    tab, nxt, start = _merge_states(_pack_lines(np.concatenate(sets), V), np.concatenate(nxts), start)
    if tab.shape[0] > AUTOMATON_MAX_STATES:
        raise ValueError(f"{tab.shape[0]} automaton states, more than {AUTOMATON_MAX_STATES}")
    return Automaton(tab, np.ascontiguousarray(nxt.astype(np.uint16)), np.ascontiguousarray(start.astype(np.int32)), V)


# Soft controls (docs/DESIGN.md §4h): preferences instead of rules.  A name has a row of V additive logit
# biases, a presence penalty and a frequency penalty.  At a step l that its prefix does not force, with the
# model's logits x (fp32, after the FC bias):
#     n[c] = how often byte c occurs among the row's bytes 0 .. l-1 (forced chars count, SOS is not there)
#     pen  = frequency * float(n[c]);  if n[c] > 0: pen = pen + presence
#     v[c] = (x[c] + bias[c]) - pen            three fp32 operations in this order, never fused
# and v takes x's place in steps 2-7 above: the temperature scale, the mask, greedy, top-k and top-p all
# see the adjusted values.  A forced step reads none of it.  All-zero values leave v bitwise x (x + 0 and
# v - 0 are exact, and the top-k key folds -0 into +0), so neutral soft controls give the call's bytes
# without them.  Every value is finite and at most 1e4 in magnitude: a ban is charset's job, and a finite
# bias never empties an allowed set.  The penalties count bytes, so they need a vocabulary of at most 256.
SOFT_MAX_ROWS = 256
SOFT_MAX_ABS = 1e4


class Soft:
    """Soft controls of ``count`` names: tab float32 [R, V] (line 0 all zero, lines distinct, R <= 256), idx
    int32 [count] (a name's line), presence / frequency float32 [count]."""

    def __init__(self, tab: np.ndarray, idx: np.ndarray, presence: np.ndarray, frequency: np.ndarray):
        self.tab, self.idx, self.presence, self.frequency = tab, idx, presence, frequency

    @property
    def rows(self) -> int:
        return int(self.tab.shape[0])

    @property
    def vocab(self) -> int:
        return int(self.tab.shape[1])

    def bias(self) -> np.ndarray:
        """The names' bias rows, float32 [count, V]."""
        return self.tab[self.idx]

    def slice(self, start: int, count: int) -> "Soft":
        """Names start .. start + count - 1 (the table is shared)."""
        return Soft(self.tab, np.ascontiguousarray(self.idx[start:start + count]),
                    np.ascontiguousarray(self.presence[start:start + count]),
                    np.ascontiguousarray(self.frequency[start:start + count]))


def _soft_value(v, what: str) -> float:
    try:
        f = float(v)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{what}: a number expected, got {v!r}") from e
    if not math.isfinite(f) or abs(f) > SOFT_MAX_ABS:
        raise ValueError(f"{what} must be finite and at most {SOFT_MAX_ABS:g} in magnitude, got {v!r}")
    return f


def _soft_row(cfg: GRUConfig, spec) -> np.ndarray:
    """One name's bias row, float32 [V]: None (zeros), a dict {chars or id: value} (a char named by several
    keys gets their sum) or V values."""
    V = cfg.vocab
    if spec is None:
        return np.zeros(V, np.float32)
    if isinstance(spec, dict):
        row = np.zeros(V, np.float64)
        for key, val in spec.items():
            f = _soft_value(val, f"logit_bias[{key!r}]")
            if isinstance(key, (str, bytes)):
                ids = list(_as_bytes(key, "logit_bias key"))
            elif isinstance(key, (int, np.integer)) and not isinstance(key, bool):
                ids = [int(key)]
            else:
                raise ValueError(f"logit_bias: a key is a str, bytes or an int id, got {key!r}")
            for c in ids:
                if not 0 <= c < V:
                    raise ValueError(f"logit_bias key {key!r} names char {c} outside the vocabulary of {V}")
                row[c] += f
    else:
        try:
            row = np.asarray(spec, dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError(f"logit_bias: a dict or {V} values expected") from e
        if row.shape != (V,):
            raise ValueError(f"logit_bias: {V} values expected, got shape {row.shape}")
    if not np.isfinite(row).all() or (np.abs(row) > SOFT_MAX_ABS).any():
        raise ValueError(f"logit_bias values must be finite and at most {SOFT_MAX_ABS:g} in magnitude")
    return row.astype(np.float32)


def _soft_is_single(lb) -> bool:
    if lb is None or isinstance(lb, dict):
        return True
    if isinstance(lb, np.ndarray):
        return lb.ndim == 1 and lb.dtype != object
    return len(lb) > 0 and all(np.ndim(v) == 0 and v is not None and not isinstance(v, dict) for v in lb)


def make_soft(cfg: GRUConfig, count: int, logit_bias=None, presence_penalty=None, frequency_penalty=None) -> Soft:
    """``logit_bias``: a dict {chars: value} -- keys str / bytes (every char in them) or an int id -- or an
    array of V values, for every name; or a list of ``count`` of those (None: no bias).  ``presence_penalty``
    / ``frequency_penalty``: a scalar or ``count`` values (None: 0).  ValueError for a value that is not
    finite or above 1e4 in magnitude, a wrong length, a key outside the vocabulary, more than 256 distinct
    bias rows, and a non-zero penalty with a vocabulary above 256 (the output row keeps only a char's low
    byte)."""
    count = int(count)
    if count < 0:
        raise ValueError("count must be >= 0")
    V = cfg.vocab
    pres = _per_name(0.0 if presence_penalty is None else presence_penalty, count, np.float64, "presence_penalty")
    freq = _per_name(0.0 if frequency_penalty is None else frequency_penalty, count, np.float64, "frequency_penalty")
    for a, what in ((pres, "presence_penalty"), (freq, "frequency_penalty")):
        if not np.isfinite(a).all() or (np.abs(a) > SOFT_MAX_ABS).any():
            raise ValueError(f"{what} must be finite and at most {SOFT_MAX_ABS:g} in magnitude")
    for v, what in ((presence_penalty, "presence_penalty"), (frequency_penalty, "frequency_penalty")):
        if v is not None and V > 256 and np.any(np.asarray(v, dtype=np.float64) != 0):
            raise ValueError(f"{what} needs vocab <= 256 (got {V}): the output row keeps only a char's low byte")
    lines: Dict[bytes, int] = {np.zeros(V, np.float32).tobytes(): 0}
    idx = np.zeros(count, np.int32)
    if _soft_is_single(logit_bias):
        row = _soft_row(cfg, logit_bias) + np.float32(0)   # (-0 -> +0: one key per value)
        idx[:] = lines.setdefault(row.tobytes(), len(lines))
    else:
        if len(logit_bias) != count:
            raise ValueError(f"logit_bias: one row or {count} rows expected, got {len(logit_bias)}")
        for n in range(count):
            row = _soft_row(cfg, logit_bias[n]) + np.float32(0)
            idx[n] = lines.setdefault(row.tobytes(), len(lines))
    if len(lines) > SOFT_MAX_ROWS:
        raise ValueError(f"{len(lines)} distinct logit_bias rows, more than {SOFT_MAX_ROWS}")
    tab = np.stack([np.frombuffer(k, dtype=np.float32) for k in lines])        # insertion order = line number
    return Soft(np.ascontiguousarray(tab), idx, pres.astype(np.float32), freq.astype(np.float32))


def as_soft(cfg: GRUConfig, count: int, soft=None, logit_bias=None, presence_penalty=None,
            frequency_penalty=None) -> Optional[Soft]:
    """None when nothing is given, a checked ``soft`` object for ``count`` names, or ``make_soft`` of the three
    keywords (a neutral value too: the caller asked for the controlled path)."""
    given = any(v is not None for v in (logit_bias, presence_penalty, frequency_penalty))
    if soft is None:
        return make_soft(cfg, count, logit_bias, presence_penalty, frequency_penalty) if given else None
    if given:
        raise ValueError("soft: give a Soft object or the logit_bias / presence_penalty / frequency_penalty keywords")
    if not isinstance(soft, Soft):
        raise ValueError("soft: a Soft object (make_soft) expected")
    s = soft
    if (s.tab.ndim != 2 or s.tab.shape[1] != cfg.vocab or s.tab.dtype != np.float32 or s.idx.shape != (count,)
            or s.presence.shape != (count,) or s.frequency.shape != (count,)):
        raise ValueError(f"soft: tab float32 [R, {cfg.vocab}] and idx, presence, frequency [{count}] expected, got "
                         f"{s.tab.shape}, {s.idx.shape}, {s.presence.shape} and {s.frequency.shape}")
    if not 1 <= s.rows <= SOFT_MAX_ROWS:
        raise ValueError(f"soft: 1 .. {SOFT_MAX_ROWS} table lines expected, got {s.rows}")
    if s.idx.size and (s.idx.min() < 0 or s.idx.max() >= s.rows):
        raise ValueError("soft: an idx entry outside the table")
    for a in (s.tab, s.presence, s.frequency):
        if not np.isfinite(a).all() or (np.abs(a) > SOFT_MAX_ABS).any():
            raise ValueError(f"soft: values must be finite and at most {SOFT_MAX_ABS:g} in magnitude")
    if cfg.vocab > 256 and (s.presence.any() or s.frequency.any()):
        raise ValueError(f"soft: the penalties need vocab <= 256 (got {cfg.vocab})")
    return s


def soft_adjust(x: torch.Tensor, soft: Soft, emitted: Optional[np.ndarray]) -> torch.Tensor:
    """v of the rule above: logits x [N, V], the rows' Soft and their bytes so far, uint8 [N, l] (None: no
    byte yet).  Three operations in x's dtype, in the rule's order."""
    N, V = x.shape
    dt = x.dtype
    if emitted is None or emitted.shape[1] == 0:
        cnt = np.zeros((N, V), np.int64)
    else:
        e = np.asarray(emitted).reshape(N, -1).astype(np.int64)
        cnt = (e[:, :, None] == np.arange(V)[None, None, :]).sum(1)
    n = torch.from_numpy(cnt).to(dt)
    b = torch.from_numpy(np.ascontiguousarray(soft.bias())).to(dt)
    pen = torch.from_numpy(soft.frequency).to(dt).unsqueeze(-1) * n
    pen = torch.where(n > 0, pen + torch.from_numpy(soft.presence).to(dt).unsqueeze(-1), pen)
    return (x + b) - pen


def _filter(x: torch.Tensor, inv: np.ndarray, top_k: np.ndarray, top_p: np.ndarray,
            allowed: Optional[np.ndarray] = None, soft: Optional[Soft] = None, emitted: Optional[np.ndarray] = None):
    """Steps 2-7 on logits x [N, V] with Controls arrays of N entries (and the rows' allowed sets, bool
    [N, V], None: everything) -> (probs [N, V], keep [N, V]).  ``soft`` (with the rows' bytes so far,
    ``emitted`` uint8 [N, l]): the rule runs on ``soft_adjust``'s values instead of x."""
    N, V = x.shape
    dt = x.dtype
    if soft is not None:
        x = soft_adjust(x, soft, emitted)
    inv_t = torch.from_numpy(inv)
    greedy = inv_t == 0
    y = x * torch.where(greedy, torch.ones_like(inv_t), inv_t).to(dt).unsqueeze(-1)
    keep = torch.ones(N, V, dtype=torch.bool)
    if allowed is not None:
        keep = torch.from_numpy(np.array(allowed, dtype=bool)).reshape(N, V)
        y = torch.where(keep, y, torch.full_like(y, -math.inf))
    k = torch.from_numpy(top_k.astype(np.int64))
    kact = (k > 0) & (k < V)
    if kact.any():   # y_i >= the k-th largest value  <=>  fewer than k values above y_i
        kth = torch.sort(y, -1, descending=True).values.gather(-1, (k.clamp(1, V) - 1).unsqueeze(-1))
        keep = torch.where(kact.unsqueeze(-1), (y >= kth) & keep, keep)   # (& keep: a set smaller than k)
    ninf = torch.full_like(y, -math.inf)
    p = torch.from_numpy(top_p).to(dt)
    pact = p < 1
    if pact.any():
        q = torch.softmax(torch.where(keep, y, ninf), -1)
        qs, order = torch.sort(q, -1, descending=True)
        before = torch.cumsum(qs, -1) - qs                     # mass sorted ahead of each entry
        first = torch.ones_like(keep)
        first[:, 1:] = qs[:, 1:] != qs[:, :-1]                 # an entry's ties share the first one's mass
        above_s = torch.cummax(torch.where(first, before, torch.full_like(before, -1.0)), -1).values
        above = torch.empty_like(above_s).scatter_(-1, order, above_s)
        keep = torch.where(pact.unsqueeze(-1), keep & (above < p.unsqueeze(-1)), keep)
    top = (y == y.max(-1, keepdim=True).values).to(torch.int64).argmax(-1)   # lowest index of the maximum
    keep = torch.where(greedy.unsqueeze(-1), torch.arange(V).unsqueeze(0) == top.unsqueeze(-1), keep)
    return torch.softmax(torch.where(keep, y, ninf), -1), keep


def filter_probs(logits: torch.Tensor, temperature=1.0, top_k=0, top_p=1.0, allowed=None, soft=None,
                 emitted=None) -> torch.Tensor:
    """The distribution step 7 samples from: logits [N, V] (or [V]) in fp32 or fp64 (fp64: the oracle),
    the controls scalars or N values.  T == 0 gives the one-hot row of the lowest arg-max.  ``allowed``:
    bool [N, V] (or [V]), the rows' allowed sets (None: everything).  ``soft`` / ``emitted``: the rows' Soft
    object and their bytes so far (uint8 [N, l]), docs/DESIGN.md §4h."""
    x = logits.unsqueeze(0) if logits.dim() == 1 else logits
    c = make_controls(GRUConfig(vocab=x.shape[-1]), x.shape[0], temperature, top_k, top_p)
    soft = as_soft(GRUConfig(vocab=x.shape[-1]), x.shape[0], soft)
    probs, _ = _filter(x, c.inv_temp, c.top_k, c.top_p, _allowed_rows(allowed, x.shape), soft, emitted)
    return probs[0] if logits.dim() == 1 else probs


def _allowed_rows(allowed, shape) -> Optional[np.ndarray]:
    if allowed is None:
        return None
    a = np.asarray(allowed, dtype=bool)
    a = np.broadcast_to(a, shape) if a.ndim == 1 else a
    if a.shape != tuple(shape):
        raise ValueError(f"allowed: bool {tuple(shape)} expected, got {a.shape}")
    if not a.any(-1).all():
        raise ValueError("allowed: a row with an empty set")
    return a


def sample_controlled(logits: torch.Tensor, r: torch.Tensor, temperature=1.0, top_k=0, top_p=1.0,
                      controls: Optional[Controls] = None, allowed=None, soft: Optional[Soft] = None,
                      emitted: Optional[np.ndarray] = None) -> torch.Tensor:
    """Steps 2-7: logits [N, V], uniforms r [N] (and the rows' allowed sets, bool [N, V]; their Soft object
    and bytes so far, §4h) -> chosen index [N] (int64)."""
    c = controls or make_controls(GRUConfig(vocab=logits.shape[-1]), logits.shape[0], temperature, top_k, top_p)
    probs, keep = _filter(logits, c.inv_temp, c.top_k, c.top_p, _allowed_rows(allowed, logits.shape), soft, emitted)
    V = probs.shape[-1]
    cs = torch.empty_like(probs)
    acc = torch.zeros_like(probs[..., 0])
    for i in range(V):   # strictly left to right, as sample_inverse_cdf
        acc = acc + probs[..., i]
        cs[..., i] = acc
    hit = cs > r.to(probs.dtype).unsqueeze(-1)
    idx = hit.to(torch.int64).argmax(-1)
    last = V - 1 - keep.flip(-1).to(torch.int64).argmax(-1)   # the highest kept index
    return torch.where(hit.any(-1), idx, last)


def generate(params: Params, cfg: GRUConfig, rfloats: np.ndarray, start: int = 0,
             count: Optional[int] = None, temperature=None, top_k=None, top_p=None, prefix=None,
             constraints=None, logit_bias=None, presence_penalty=None, frequency_penalty=None,
             soft=None) -> np.ndarray:
    """Batched version of the reference's per-name loop (namegensf.cu:649-884).

    Names ``start .. start+count-1`` of the global job; name n at step l consumes
    ``rfloats[n*MAX_LEN + l]`` (SURVEY §3.2 invariant) -- the global index, so the
    result is independent of how names are split across ranks.  Returns uint8
    [count, MAX_LEN+1]; the EOS char *is* written before stopping
    (namegensf.cu:877-882) and the rest stays NUL.

    ``temperature`` / ``top_k`` / ``top_p`` / ``prefix`` (see ``make_controls``; scalars or one value per
    generated name, i.e. ``count`` entries): any that is not None takes the controlled sampler above
    (neutral values give the plain path's bytes).  ``constraints``: a Constraints object for the ``count``
    names or a dict of ``make_constraints`` keywords; it takes the controlled sampler too, inside each
    step's allowed set (a table of only line 0 gives the unconstrained bytes).  ``logit_bias`` /
    ``presence_penalty`` / ``frequency_penalty`` (``make_soft``'s arguments) or ``soft`` (its result for the
    ``count`` names): the soft controls of docs/DESIGN.md §4h; any that is not None takes the controlled
    sampler (neutral values give the bytes without them).  fp64 params give the oracle."""
    ML = cfg.max_len
    N = (rfloats.size // ML - start) if count is None else count
    out = np.zeros((N, ML + 1), dtype=np.uint8)
    ctl = None
    cons = as_constraints(cfg, max(N, 0), constraints)
    soft = as_soft(cfg, max(N, 0), soft, logit_bias, presence_penalty, frequency_penalty)
    if cons is not None or soft is not None or any(v is not None for v in (temperature, top_k, top_p, prefix)):
        ctl = make_controls(cfg, max(N, 0), temperature, top_k, top_p, prefix)
        check_prefix_allowed(cons, ctl.prefix, ctl.plen)
    if N <= 0:
        return out
    H = cfg.hidden
    dt = params["fc.weight"].dtype
    rf = torch.from_numpy(np.asarray(rfloats, dtype=np.float32)[start * ML:(start + N) * ML]).view(N, ML)
    hs = [torch.zeros(N, H, dtype=dt) for _ in range(cfg.layers)]
    cur = torch.full((N,), cfg.sos, dtype=torch.int64)
    alive = torch.ones(N, dtype=torch.bool)
    aut = cons if isinstance(cons, Automaton) else None
    if aut is not None:   # §4g: the set is the line of the name's state, which advances with the chosen char
        alines, astate = aut.lines(), aut.start.astype(np.int64)
    for l in range(ML):
        inp = params["embedding"][cur]
        for k in range(cfg.layers):
            gi = inp @ params[f"weight_ih_l{k}"].T + params[f"bias_ih_l{k}"]
            gh = hs[k] @ params[f"weight_hh_l{k}"].T + params[f"bias_hh_l{k}"]
            hs[k], _ = _gates(gi, gh, hs[k])
            inp = hs[k]
        logits = inp @ params["fc.weight"].T + params["fc.bias"]
        if dt != torch.float64:
            logits = logits.to(torch.float32)
        if ctl is None:
            prob = torch.softmax(logits, -1)
            sel = sample_inverse_cdf(prob, rf[:, l].to(prob.dtype))
        else:
            allowed = None if cons is None else (alines[astate] if aut is not None else cons.allowed(l))
            # (§4h: the counts are those of the output row's bytes, as the device reads them)
            sel = sample_controlled(logits, rf[:, l], controls=ctl, allowed=allowed, soft=soft, emitted=out[:, :l])
            forced = torch.from_numpy(ctl.plen > l)
            sel = torch.where(forced, torch.from_numpy(ctl.prefix[:, l].astype(np.int64)), sel)
            if aut is not None:   # every step, a forced one and a finished row's included (nxt[q][eos] = 0)
                astate = aut.nxt[astate, sel.numpy()].astype(np.int64)
        out[alive.numpy(), l] = sel[alive].numpy().astype(np.uint8)
        alive &= sel != cfg.eos
        cur = sel
        if not alive.any():
            break
    return out


# --------------------------------------------------------------------------- beam search
# The W most probable output rows per prefix (docs/DESIGN.md §4d).  A name holds W ordered beams, each
# live (score, hidden states, row so far, last char), finished (it wrote EOS: score and row frozen) or
# dead (score -inf, empty row).  Before step 0 beam 0 is live with score 0, h = 0 and input SOS; the
# others are dead.  Every step l = 0 .. max_len - 1:
#   1. every beam row takes the model's step (finished and dead rows with input SOS, ignored);
#   2. lp = log softmax(logits) per live beam;
#   3. candidates j = b V + c: a live beam offers every c with score s_b + lp[c] -- only c = prefix[l]
#      while l < plen -- a finished beam the carry j = b V with score s_b, a dead beam nothing;
#   4. the new beams are the first W candidates in the total order "score descending, then j
#      ascending", stored in that order; with fewer than W candidates the rest are dead;
#   5. (b, c) copies b's row and appends c; it is finished when c == eos (the byte is written, then
#      the beam stops: the generator's rule), else live with b's post-step states and input c.
# Forced chars add their log-prob: logp is the row's full log-probability, what ``score`` returns.
BEAM_DEAD, BEAM_LIVE, BEAM_FIN = 0, 1, 2
BEAM_MAX_WIDTH = 32


class BeamResult:
    """``HipGenerator.beam_search`` / ``cpu_ref.beam_search`` output for N prefixes of W beams, in order:
    rows [N, W, MAX_LEN+1] uint8 (the ``generate`` format), logp [N, W] (-inf for a dead slot), n_tok
    [N, W] int32, n_beams [N] int32 (the slots that are not dead, always the first ones)."""

    def __init__(self, rows, logp, n_tok, n_beams, eos: int = 0):
        self.rows, self.logp, self.n_tok, self.n_beams, self.eos = rows, logp, n_tok, n_beams, eos

    def names(self) -> List[List[str]]:
        """Per prefix the beams' names in order (the EOS byte dropped, dead slots left out)."""
        out = []
        for n in range(self.rows.shape[0]):
            cur = []
            for k in range(int(self.n_beams[n])):
                b = bytes(self.rows[n, k, :int(self.n_tok[n, k])])
                if b and b[-1] == self.eos:
                    b = b[:-1]
                cur.append(b.decode("latin-1"))
            out.append(cur)
        return out


def beam_inputs(cfg: GRUConfig, prefix=None, width: int = 4, count: Optional[int] = None):
    """Validated (prefix rows [N, MAX_LEN] uint8, plen [N] int32) of a beam search.  ``prefix``: a str /
    bytes, ``encode_prefixes`` input, or None for ``count`` (default 1) empty prefixes.  ValueError for
    a width outside [1, min(32, vocab)], max_len > 64 and bad prefixes."""
    if isinstance(width, bool) or int(width) != width or not 1 <= width <= min(BEAM_MAX_WIDTH, cfg.vocab):
        raise ValueError(f"width must be an integer in [1, {min(BEAM_MAX_WIDTH, cfg.vocab)}], got {width!r}")
    if cfg.max_len > 64:
        raise ValueError(f"beam search needs max_len <= 64 (got {cfg.max_len})")
    if not 0 <= cfg.sos < cfg.vocab:
        raise ValueError(f"sos {cfg.sos} outside the vocabulary of {cfg.vocab}")
    if prefix is None:
        n = 1 if count is None else int(count)
        if n < 0:
            raise ValueError("count must be >= 0")
        return np.zeros((n, cfg.max_len), np.uint8), np.zeros(n, np.int32)
    if isinstance(prefix, (str, bytes)):
        prefix = [prefix]
    rows, plen = encode_prefixes(prefix, cfg)
    if count is not None and count != rows.shape[0]:
        raise ValueError(f"count = {count} but {rows.shape[0]} prefixes given")
    return rows, plen


def beam_select(lp: np.ndarray, score: np.ndarray, state: np.ndarray, forced_char: int = -1, allowed=None):
    """Steps 3-4 for one name: lp [W, V], score [W], state [W] -> the W new beams in order as (parent,
    chr, score, j), parent -1 for a dead slot, chr -1 for a carry or a dead slot.  ``allowed``: bool [V],
    the name's set at this step (None: everything), or bool [W, V], a set per beam: a live beam offers
    only chars in it, carries are not masked."""
    W, V = lp.shape
    cand = np.full((W, V), -np.inf, dtype=lp.dtype)
    offered = np.zeros((W, V), dtype=bool)
    oks = np.ones(V, bool) if allowed is None else np.asarray(allowed, dtype=bool)
    for b in range(W):
        ok = oks[b] if oks.ndim == 2 else oks   # [W, V]: a set per beam (an Automaton, §4g)
        if state[b] == BEAM_LIVE:
            if forced_char >= 0:
                if ok[forced_char]:
                    cand[b, forced_char] = score[b] + lp[b, forced_char]
                    offered[b, forced_char] = True
            else:
                cand[b] = np.where(ok, score[b] + lp[b], -np.inf)
                offered[b] = ok
        elif state[b] == BEAM_FIN:
            cand[b, 0] = score[b]
            offered[b, 0] = True
    js = np.flatnonzero(offered.reshape(-1))
    sc = cand.reshape(-1)[js]
    order = js[np.lexsort((js, -sc))][:W]      # score descending, then j ascending
    out = []
    for j in order:
        b, c = divmod(int(j), V)
        out.append((b, -1 if state[b] == BEAM_FIN else c, cand[b, c], int(j)))
    while len(out) < W:
        out.append((-1, -1, lp.dtype.type(-np.inf), -1))
    return out


def beam_search(params: Params, cfg: GRUConfig, prefix=None, width: int = 4, count: Optional[int] = None,
                constraints=None) -> BeamResult:
    """The rule above in the dtype of ``params`` (fp64 params: the oracle; the CPU path of ``cli beam``).
    ``constraints``: a Constraints object for the N prefixes or a dict of ``make_constraints`` keywords:
    the W most probable names that satisfy it."""
    pre, plen = beam_inputs(cfg, prefix, width, count)
    cons = as_constraints(cfg, pre.shape[0], constraints)
    check_prefix_allowed(cons, pre, plen)
    return beam_search_rule(params, cfg, pre, plen, int(width), cons)


def beam_search_rule(params: Params, cfg: GRUConfig, pre: np.ndarray, plen: np.ndarray, W: int,
                     cons: Optional[Constraints] = None) -> BeamResult:
    """The rule itself on validated inputs (``beam_inputs`` / ``as_constraints``).  It has no width limit
    of its own -- the limits of ``beam_inputs`` are the device's -- so a width that holds every candidate
    makes the search exhaustive (tests/test_constraints.py)."""
    N, ML, V, H = pre.shape[0], cfg.max_len, cfg.vocab, cfg.hidden
    dt = params["fc.weight"].dtype
    npdt = np.float64 if dt == torch.float64 else np.float32
    rows = np.zeros((N, W, ML + 1), np.uint8)
    score = np.full((N, W), -np.inf, npdt)
    state = np.full((N, W), BEAM_DEAD, np.int64)
    ntok = np.zeros((N, W), np.int32)
    if N == 0:
        return BeamResult(rows, score, ntok, np.zeros(0, np.int32), cfg.eos)
    score[:, 0] = 0
    state[:, 0] = BEAM_LIVE
    hs = [torch.zeros(N * W, H, dtype=dt) for _ in range(cfg.layers)]
    cur = torch.full((N * W,), cfg.sos, dtype=torch.int64)
    aut = cons if isinstance(cons, Automaton) else None
    if aut is not None:   # §4g: a state per beam; beam 0 starts in the name's start state, carried and dead beams sit in 0
        alines, astate = aut.lines(), np.zeros((N, W), np.int64)
        astate[:, 0] = aut.start
    for l in range(ML):
        inp = params["embedding"][cur]
        for k in range(cfg.layers):
            gi = inp @ params[f"weight_ih_l{k}"].T + params[f"bias_ih_l{k}"]
            gh = hs[k] @ params[f"weight_hh_l{k}"].T + params[f"bias_hh_l{k}"]
            hs[k], _ = _gates(gi, gh, hs[k])
            inp = hs[k]
        logits = inp @ params["fc.weight"].T + params["fc.bias"]
        if dt != torch.float64:
            logits = logits.to(torch.float32)
        lp = torch.log_softmax(logits, -1).numpy().reshape(N, W, V)
        nastate = None if aut is None else np.zeros_like(astate)
        gather = np.zeros(N * W, np.int64)
        nrows, nscore, nstate, nntok = np.zeros_like(rows), np.full_like(score, -np.inf), np.zeros_like(state), np.zeros_like(ntok)
        nxt = np.full(N * W, cfg.sos, np.int64)
        for n in range(N):
            sel = beam_select(lp[n], score[n], state[n], int(pre[n, l]) if l < plen[n] else -1,
                              None if cons is None else (alines[astate[n]] if aut is not None else cons.allowed(l)[n]))
            for k, (b, c, s, _) in enumerate(sel):
                if b < 0:
                    continue
                gather[n * W + k] = n * W + b
                nrows[n, k] = rows[n, b]
                nntok[n, k] = ntok[n, b]
                nscore[n, k] = s
                if c < 0:
                    nstate[n, k] = BEAM_FIN
                    continue
                nrows[n, k, l] = c
                nntok[n, k] = l + 1
                if aut is not None:
                    nastate[n, k] = aut.nxt[astate[n, b], c]
                nstate[n, k] = BEAM_FIN if c == cfg.eos else BEAM_LIVE
                if c != cfg.eos:
                    nxt[n * W + k] = c
        g = torch.from_numpy(gather)
        hs = [h[g] for h in hs]
        rows, score, state, ntok = nrows, nscore, nstate, nntok
        if aut is not None:
            astate = nastate
        cur = torch.from_numpy(nxt)
    return BeamResult(rows, score, ntok, (state != BEAM_DEAD).sum(1).astype(np.int32), cfg.eos)


# --------------------------------------------------------------------------- distinct names
# Sampling without replacement by stochastic beam search (docs/DESIGN.md §4i; Kool, van Hoof and Welling,
# 2019): the beam loop above, ranked by Gumbel-perturbed log-probabilities.  Per name W ordered slots (live /
# finished / dead as above), each with logq -- the log-probability of its row so far under the SAMPLER's
# distribution (temperature, constraint sets renormalised, forced chars 0: what ``score`` returns with the
# same keywords) -- and G, its perturbed value.  Slot 0 starts live with logq = G = 0.  Per step l:
#   1. every row takes the model's step;
#   2. per live slot b: y = x * inv_T, A = the allowed set, lq[c] = (y[c] - max_A y) - log sum_A exp(y - max_A y);
#      on a forced step the only child is prefix[l] with lq = 0;
#   3. candidate j = b V + c of the name with global index g = start + n gets the 32-bit word j & 3 of
#      Philox-4x32-10(key = seed, counter = (j >> 2, l, g)); u = (2 (word >> 9) + 1) 2^-24, gum = -log(-log u);
#   4. psi = logq_b + lq[c], g = psi + gum, Z = max over the offered c; with d = g - Z
#         v  = (G_b - g) + log1mexp(d)
#         Gt = (G_b - max(0, v)) - log1p(exp(-|v|))
#      i.e. Gt = -log(e^-G_b - e^-Z + e^-g): the children's maximum is moved onto G_b.  A finished slot offers
#      its carry j = b V with Gt = G_b and logq unchanged, a dead slot nothing;
#   5. the first W candidates in the order "Gt descending, then j ascending" are the new slots, in that order.
# The W rows at the end are an exact sample without replacement, in draw order, from the distribution
# ``generate`` samples from with the same temperature / prefix / constraints.
_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PHILOX_W0, _PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_U32 = np.uint64(0xFFFFFFFF)


def philox4x32(ctr: np.ndarray, key: np.ndarray) -> np.ndarray:
    """Philox-4x32-10 (Salmon et al., Random123): ctr [..., 4], key [..., 2] (uint32 values) -> uint32 [..., 4]."""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    for _ in range(10):
        p0, p1 = _PHILOX_M0 * c[0], _PHILOX_M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & _U32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & _U32]
        k = [(k[0] + _PHILOX_W0) & _U32, (k[1] + _PHILOX_W1) & _U32]
    return np.stack(c, -1).astype(np.uint32)


def sbs_uniform(seed: int, g: np.ndarray, step: int, W: int, V: int) -> np.ndarray:
    """Step 3's u, float32 [len(g), W, V] (exact, inside [2^-24, 1 - 2^-24]) for the names with global
    indices ``g`` at ``step``."""
    g = np.asarray(g, dtype=np.uint64).reshape(-1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    nb = (W * V + 3) // 4
    ctr = np.zeros((g.shape[0], nb, 4), np.uint64)
    ctr[:, :, 0] = np.arange(nb, dtype=np.uint64)[None, :]
    ctr[:, :, 1] = np.uint64(int(step) & 0xFFFFFFFF)
    ctr[:, :, 2] = (g & _U32)[:, None]
    ctr[:, :, 3] = (g >> np.uint64(32))[:, None]
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)
    words = philox4x32(ctr, key).reshape(g.shape[0], nb * 4)[:, :W * V]
    u = (2.0 * (words >> np.uint32(9)).astype(np.float64) + 1.0) * 2.0 ** -24
    return u.astype(np.float32).reshape(g.shape[0], W, V)


def _rounded(f, a: np.ndarray) -> np.ndarray:
    """f(a) in a's dtype; float32: evaluated in float64 and rounded once, as a correctly rounded expf /
    logf would (the device's are within an ulp or two of that)."""
    if a.dtype == np.float32:
        return f(a.astype(np.float64)).astype(np.float32)
    return f(a)


def _wave_sum(e: np.ndarray) -> np.ndarray:
    """The sum over the last axis (V entries) in e's dtype, in the device's order when V is a multiple of
    64: a lane adds its V / 64 consecutive entries in index order, then the 64 lane sums are added as a
    balanced tree of neighbours (pairs, quads, eights, the 16-lane rows, two rows, the wave)."""
    V = e.shape[-1]
    if V % 64:
        return e.sum(-1, keepdims=True)
    t = e.reshape(e.shape[:-1] + (64, V // 64))
    acc = t[..., 0]
    for k in range(1, V // 64):
        acc = acc + t[..., k]
    while acc.shape[-1] > 1:
        acc = acc[..., 0::2] + acc[..., 1::2]
    return acc


def sbs_step(x: np.ndarray, logq: np.ndarray, G: np.ndarray, state: np.ndarray, forced: np.ndarray, allowed,
             inv_t: np.ndarray, u: np.ndarray, eos: int, sos: int, mut: Optional[str] = None) -> Dict[str, np.ndarray]:
    """Steps 2-5 for N names at once, in the dtype of ``x`` (float32: the device's operations in its order,
    the row sum included, each rounded once; expf / logf / log1pf / expm1f as correctly rounded functions,
    which the device's are not, so this emulates the kernel, it does not reproduce its bits).  x [N, W, V] logits, logq / G / state [N, W], forced [N] (the forced char, -1 on
    a free step), allowed None / bool [N, V] / bool [N, W, V], inv_t [N] float32, u [N, W, V] float32.
    Returns the new slots -- parent (-1: dead), chr (-1: a carry or dead), state, logq, G, next_id, sel (the
    flat index j, -1) -- and lq / gt [N, W, V] (NaN outside the allowed set / where not offered), zmax [N, W],
    scale [N, W, V] (max(1, exp(Gt - g)): the conditioning of a candidate's truncation), and top / top_gt /
    top_scale / top_row_scale [N, W + 1]: the first W + 1 candidates in order (-1 / NaN where there are fewer;
    row_scale: max(1, exp(G_b - Z)) of the candidate's row, the supremum of its scale).  ``mut``: a planted
    defect (models/sbs_ref.py)."""
    N, W, V = x.shape
    dt = x.dtype.type
    ninf = dt(-np.inf)
    with np.errstate(all="ignore"):
        y = x * inv_t.astype(x.dtype)[:, None, None]
        if allowed is None:
            A = np.ones((N, W, V), bool)
        else:
            A = np.asarray(allowed, bool)
            A = np.broadcast_to(A[:, None, :] if A.ndim == 2 else A, (N, W, V))
        An = np.ones((N, W, V), bool) if mut == "lq_not_renormalised" else A
        mx = np.where(An, y, ninf).max(-1, keepdims=True)
        z = y - mx
        e = np.where(An, _rounded(np.exp, z), dt(0))
        se = _wave_sum(e)
        lq = np.where(A, z - _rounded(np.log, se), dt(np.nan)).astype(x.dtype)
        gum = -_rounded(np.log, -_rounded(np.log, u.astype(x.dtype)))
        live = state == BEAM_LIVE
        fin = state == BEAM_FIN
        isf = (forced >= 0)[:, None, None]
        off = A & live[:, :, None] & (~isf | (np.arange(V)[None, None, :] == forced[:, None, None]))
        lqe = lq if mut == "forced_adds_lp" else np.where(isf, dt(0), lq)
        psi = (logq[:, :, None] + lqe).astype(x.dtype)
        g = psi + gum
        if mut == "z_over_masked":      # every char of a live row, in its set or not
            Z = np.where(live[:, :, None], (logq[:, :, None] + (z - _rounded(np.log, se))) + gum, ninf).max(-1)
        else:
            Z = np.where(off, g, ninf).max(-1)
        d = g - Z[:, :, None]
        l1 = np.where(d > dt(-0.6931), _rounded(np.log, -_rounded(np.expm1, d)), _rounded(np.log1p, -_rounded(np.exp, d)))
        Gb = G[:, :, None]
        v = (Gb - g) + l1
        gt = (Gb - np.maximum(dt(0), v)) - _rounded(np.log1p, _rounded(np.exp, -np.abs(v)))
        if mut == "naive_truncation":
            gt = -_rounded(np.log, (_rounded(np.exp, -Gb) - _rounded(np.exp, -Z[:, :, None])) + _rounded(np.exp, -g))
        if mut == "g_as_key":
            gt = g
        gt = np.where(off, gt, dt(np.nan)).astype(x.dtype)
        psi = np.where(off, psi, dt(np.nan)).astype(x.dtype)
        off = off.copy()
        off[:, :, 0] |= fin
        gt[:, :, 0] = np.where(fin, (logq + gum[:, :, 0]) if mut == "carry_reperturbed" else G, gt[:, :, 0])
        psi[:, :, 0] = np.where(fin, logq, psi[:, :, 0])
        has = off.any(-1) & live
        zmax = np.where(has, Z, dt(np.nan)).astype(x.dtype)
        # the conditioning of a candidate's Gt: |dGt/dg| = exp(Gt - g) (dGt/dZ and dGt/dG_b are no larger); a row's
        # best child (Gt == G_b bitwise) and a carry have none.  Its supremum over a row is exp(G_b - Z).
        scale = np.where(off & (d != 0) & live[:, :, None],
                         np.maximum(1.0, np.exp(np.minimum(gt.astype(np.float64) - g.astype(np.float64), 80.0))), 1.0)
        row_scale = np.where(has, np.maximum(1.0, np.exp(np.minimum(G.astype(np.float64) - Z.astype(np.float64), 80.0))), 1.0)
        keyv = np.where(off, gt, ninf).reshape(N, W * V)
        order = np.argsort(-keyv, axis=1, kind="stable")      # Gt descending, then j ascending
    rows_i = np.arange(N)[:, None]
    # ... offered candidates first: one whose Gt is -inf still ranks before what was not offered
    order = order[rows_i, np.argsort(~off.reshape(N, W * V)[rows_i, order], axis=1, kind="stable")][:, :W + 1]
    cnt = off.reshape(N, -1).sum(1)
    valid = np.arange(W + 1)[None, :] < cnt[:, None]
    top = np.where(valid, order, -1)
    top_gt = np.where(valid, keyv[rows_i, order], np.nan)
    top_scale = np.where(valid, scale.reshape(N, W * V)[rows_i, order], np.nan)
    top_row_scale = np.where(valid, row_scale[rows_i, order // V], np.nan)
    win, wv = order[:, :W], valid[:, :W]
    pb, pc = win // V, win % V
    carried = fin[rows_i, pb] & wv
    parent = np.where(wv, pb, -1).astype(np.int32)
    chrs = np.where(wv & ~carried, pc, -1).astype(np.int32)
    nstate = np.where(wv, np.where(carried | (pc == eos), BEAM_FIN, BEAM_LIVE), BEAM_DEAD).astype(np.int32)
    nlogq = np.where(wv, psi.reshape(N, -1)[rows_i, win], ninf).astype(x.dtype)
    nG = np.where(wv, keyv[rows_i, win], ninf).astype(x.dtype)
    if mut == "logq_from_key":
        nlogq = np.where(wv & ~carried, nG - gum.reshape(N, -1)[rows_i, win], nlogq).astype(x.dtype)
    nxt = np.where(nstate == BEAM_LIVE, pc, sos).astype(np.int32)
    sel = np.where(wv, win, -1).astype(np.int32)
    return dict(parent=parent, chr=chrs, state=nstate, logq=nlogq, G=nG, next_id=nxt, sel=sel, lq=lq, gt=gt, zmax=zmax,
                scale=scale, top=top, top_gt=top_gt, top_scale=top_scale, top_row_scale=top_row_scale)


class DistinctResult:
    """``HipGenerator.sample_distinct`` / ``cpu_ref.sample_distinct`` output for N prefixes of W draws, in
    draw order: rows [N, W, MAX_LEN+1] uint8 (the ``generate`` format), logq [N, W] (the rows' log-probability
    under the sampler, -inf for a dead slot), gumbel [N, W] (the final perturbed values, non-increasing),
    n_tok [N, W] int32, n_found [N] int32 (the slots that are not dead, always the first ones)."""

    def __init__(self, rows, logq, gumbel, n_tok, n_found, eos: int = 0):
        self.rows, self.logq, self.gumbel, self.n_tok, self.n_found, self.eos = rows, logq, gumbel, n_tok, n_found, eos

    def names(self) -> List[List[str]]:
        """Per prefix the draws' names in order (the EOS byte dropped, dead slots left out)."""
        return BeamResult(self.rows, self.logq, self.n_tok, self.n_found, self.eos).names()


def distinct_inputs(cfg: GRUConfig, prefix=None, width: int = 4, count: Optional[int] = None, seed: int = 0,
                    start: int = 0, temperature=None, **excluded):
    """Validated (prefix rows, plen, inv_t [N] float32, seed, start) of ``sample_distinct``.  ValueError for
    what ``beam_inputs`` rejects, a temperature that is not finite and > 0, a seed or start outside
    [0, 2^64), and any of the keywords the rule does not carry (top_k, top_p, the soft controls)."""
    for k, v in excluded.items():
        if k not in ("top_k", "top_p", "logit_bias", "presence_penalty", "frequency_penalty", "soft"):
            raise TypeError(f"sample_distinct: unexpected keyword {k!r}")
        if v is not None:
            raise ValueError(f"sample_distinct does not take {k}: the rule samples without replacement from the "
                             "distribution of temperature, prefix and constraints alone")
    pre, plen = beam_inputs(cfg, prefix, width, count)
    N = pre.shape[0]
    T = _per_name(1.0 if temperature is None else temperature, N, np.float64, "temperature")
    if not np.isfinite(T).all() or (T <= 0).any():
        raise ValueError("sample_distinct: temperature must be finite and > 0 (temperature 0 has one name: use beam_search)")
    with np.errstate(over="ignore", under="ignore"):
        inv = (1.0 / T).astype(np.float32)
    if (~np.isfinite(inv)).any() or (inv == 0).any():
        raise ValueError("temperature: 1/T must be a finite non-zero fp32 value")
    for what, v in (("seed", seed), ("start", start)):
        if isinstance(v, bool) or int(v) != v or not 0 <= int(v) < 2 ** 64:
            raise ValueError(f"{what} must be an integer in [0, 2^64), got {v!r}")
    if int(start) + N > 2 ** 64:
        raise ValueError("start + count must stay below 2^64")
    return pre, plen, inv, int(seed), int(start)


def sample_distinct(params: Params, cfg: GRUConfig, prefix=None, width: int = 4, count: Optional[int] = None, *,
                    seed: int = 0, start: int = 0, temperature=None, constraints=None, **excluded) -> DistinctResult:
    """``width`` distinct names per prefix, an exact sample without replacement in draw order (the rule
    above) in the dtype of ``params`` (fp64 params: the oracle; the CPU path of ``cli distinct``).  Name n
    of the call has the global index ``start + n``: its noise does not depend on how a job is cut up."""
    pre, plen, inv, seed, start = distinct_inputs(cfg, prefix, width, count, seed, start, temperature, **excluded)
    cons = as_constraints(cfg, pre.shape[0], constraints)
    check_prefix_allowed(cons, pre, plen)
    return sample_distinct_rule(params, cfg, pre, plen, int(width), seed, start, inv, cons)


def sample_distinct_rule(params: Params, cfg: GRUConfig, pre: np.ndarray, plen: np.ndarray, W: int, seed: int,
                         start: int, inv_t: np.ndarray, cons=None, mut: Optional[str] = None,
                         trace: Optional[list] = None) -> DistinctResult:
    """The rule itself on validated inputs.  ``trace``: a list that receives every step's ``sbs_step``
    output (models/sbs_ref.py); ``mut``: a planted defect (there too)."""
    N, ML, V, H = pre.shape[0], cfg.max_len, cfg.vocab, cfg.hidden
    dt = params["fc.weight"].dtype
    npdt = np.float64 if dt == torch.float64 else np.float32
    rows = np.zeros((N, W, ML + 1), np.uint8)
    logq = np.full((N, W), -np.inf, npdt)
    G = np.full((N, W), -np.inf, npdt)
    state = np.full((N, W), BEAM_DEAD, np.int32)
    ntok = np.zeros((N, W), np.int32)
    if N == 0:
        return DistinctResult(rows, logq, G, ntok, np.zeros(0, np.int32), cfg.eos)
    logq[:, 0] = G[:, 0] = 0
    state[:, 0] = BEAM_LIVE
    hs = [torch.zeros(N * W, H, dtype=dt) for _ in range(cfg.layers)]
    cur = torch.full((N * W,), cfg.sos, dtype=torch.int64)
    aut = cons if isinstance(cons, Automaton) else None
    if aut is not None:
        alines, astate = aut.lines(), np.zeros((N, W), np.int64)
        astate[:, 0] = aut.start
    gidx = np.arange(N, dtype=np.uint64) + np.uint64(0 if mut == "counter_local_index" else start)
    ni = np.arange(N)[:, None]
    for l in range(ML):
        inp = params["embedding"][cur]
        new = []
        for k in range(cfg.layers):
            gi = inp @ params[f"weight_ih_l{k}"].T + params[f"bias_ih_l{k}"]
            gh = hs[k] @ params[f"weight_hh_l{k}"].T + params[f"bias_hh_l{k}"]
            hk, _ = _gates(gi, gh, hs[k])
            new.append(hk)
            inp = hk
        logits = inp @ params["fc.weight"].T + params["fc.bias"]
        if dt != torch.float64:
            logits = logits.to(torch.float32)
        x = logits.numpy().reshape(N, W, V)
        allowed = None if cons is None else (alines[astate] if aut is not None else cons.allowed(l))
        forced = np.where(plen > l, pre[:, l].astype(np.int64), -1)
        u = sbs_uniform(seed, gidx, 0 if mut == "counter_without_step" else l, W, V)
        s = sbs_step(x, logq, G, state, forced, allowed, inv_t, u, cfg.eos, cfg.sos, mut)
        if trace is not None:
            trace.append(s)
        par = np.maximum(s["parent"], 0)
        alive = s["parent"] >= 0
        app = s["chr"] >= 0
        nrows = np.where(alive[:, :, None], rows[ni, par], 0).astype(np.uint8)
        nrows[:, :, l] = np.where(app, s["chr"], nrows[:, :, l])
        ntok = np.where(alive, np.where(app, l + 1, ntok[ni, par]), 0).astype(np.int32)
        if aut is not None:   # (a carried or dead slot sits in state 0)
            astate = np.where(app, aut.nxt[astate[ni, par], np.maximum(s["chr"], 0)].astype(np.int64), 0)
        gather = torch.from_numpy((ni * W + par).reshape(-1).astype(np.int64))
        dead = torch.from_numpy(~alive.reshape(-1))
        hs = [h[gather].masked_fill(dead[:, None], 0) for h in new]
        rows, logq, G, state = nrows, s["logq"], s["G"], s["state"]
        cur = torch.from_numpy(s["next_id"].reshape(-1).astype(np.int64))
    return DistinctResult(rows, logq, G, ntok, (state != BEAM_DEAD).sum(1).astype(np.int32), cfg.eos)


# --------------------------------------------------------------------------- conditional names
# Sequential Monte Carlo over the constrained sampler (docs/DESIGN.md §4j).  The constrained sampler masks
# the forbidden chars at every step and renormalises, so its law is q(row) = prod_l p(c_l | ...) / m_l with
# m_l the model mass of the allowed set; the model's conditional is p(row | row in L) = p(row) / Z,
# Z = P(row in L).  They differ by the per-row factor prod_l m_l, which the particles below carry as their
# importance weight.  Per name W ordered slots (live / finished / dead as above), each with logw -- its
# unnormalised log importance weight -- and logq, the log-probability of its row under the sampler along its
# own lineage.  Slot 0 starts live with logw = logq = 0, the others dead.  Per step l:
#   1. every row takes the model's step;
#   2. per live slot b: y = x * inv_T, lse_all = max y + log sum exp(y - max y) over the vocabulary, lse_A the
#      same over the allowed set A, logm_b = lse_A - lse_all, lq[c] = y[c] - lse_A.  Forced step: logm_b = 0,
#      lq[prefix[l]] = 0.  Finished slot: logm_b = 0.  No constraint: lse_A is lse_all itself, logm_b == 0;
#   3. the look-ahead weight u_b = logw_b + logm_b (known before the draw);
#   4. over the slots that are not dead, in slot order: e_b = exp(u_b - max u), S = sum e, ESS = S S / sum e e.
#      l == 0: fan-out, a_i = 0, logw_i = u_0.  Else iff ESS < thr W: systematic resampling with the step's
#      uniform U, t_i = (i + U) / W * S, a_i = the first b whose inclusive running sum of e exceeds t_i (none:
#      the last slot), logw_i = max u + log(S / W).  Else a_i = i, logw_i = u_i;
#   5. new slot i carries a finished ancestor (row, length, logq unchanged) or draws one char of a live one:
#      the first allowed c in index order whose running sum of exp(y - max_A y) exceeds r_i times the total
#      (none: the last allowed c; forced: prefix[l]); logq_i = logq_a + lq_a[c]; finished iff c == eos;
#   6. noise: Philox-4x32-10, key = seed, counter = (i, l, g lo, g hi), g = start + n: word 0 is r_i, word 1 of
#      slot 0's block is U, both (2 (word >> 9) + 1) 2^-24.
# Zhat = mean_i exp(logw_i) is an unbiased estimate of Z = P_T(row in L | prefix) at any W, and
# mean_i exp(logw_i) f(row_i) of sum_{row in L} p_T(row | prefix) f(row).
def smc_uniform(seed: int, g: np.ndarray, step: int, W: int) -> np.ndarray:
    """Step 6's uniforms, float32 [len(g), W, 2] (exact, inside [2^-24, 1 - 2^-24]): [:, i, 0] is r_i,
    [:, 0, 1] the step's U, for the names with global indices ``g`` at ``step``."""
    g = np.asarray(g, dtype=np.uint64).reshape(-1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ctr = np.zeros((g.shape[0], W, 4), np.uint64)
    ctr[:, :, 0] = np.arange(W, dtype=np.uint64)[None, :]
    ctr[:, :, 1] = np.uint64(int(step) & 0xFFFFFFFF)
    ctr[:, :, 2] = (g & _U32)[:, None]
    ctr[:, :, 3] = (g >> np.uint64(32))[:, None]
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)
    words = philox4x32(ctr, key)[..., :2]
    return ((2.0 * (words >> np.uint32(9)).astype(np.float64) + 1.0) * 2.0 ** -24).astype(np.float32)


def _slot_cumsum(e: np.ndarray) -> np.ndarray:
    """Inclusive running sums along the last axis in e's dtype, one addition at a time in index order."""
    return np.cumsum(e, axis=-1, dtype=e.dtype)


def smc_step(x: np.ndarray, logw: np.ndarray, logq: np.ndarray, state: np.ndarray, forced: np.ndarray, allowed,
             inv_t: np.ndarray, noise: np.ndarray, thr: float, step: int, eos: int, sos: int,
             mut: Optional[str] = None) -> Dict[str, np.ndarray]:
    """Steps 2-5 for N names at once, in the dtype of ``x`` (float32: the device's operations in its order,
    each rounded once, expf / logf as correctly rounded functions; the running sums one addition at a time
    where the device scans, so this emulates the kernel, it does not reproduce its bits).  x [N, W, V]
    logits, logw / logq / state [N, W], forced [N] (the forced char, -1 on a free step), allowed None / bool
    [N, V] / bool [N, W, V], inv_t [N] float32, noise [N, W, 2] (``smc_uniform``).  Returns the new slots --
    parent (-1: dead), chr (-1: a carry or dead), state, logw, logq, next_id -- resampled [N] bool, ess [N],
    logm [N, W] (NaN: dead), lq [N, W, V] (a live row's y - lse_A, NaN outside the set), and what
    models/smc_ref.py measures: q_ess (ESS / W), q_t [N, W, W] ((running sum_b - t_i) / S, NaN where no
    resampling), q_r [N, W, 2] ((running sum - r_i total) / total at the chosen char and before it, NaN where
    nothing is drawn), clear [N] (the smallest of |ESS - thr W| / W -- not counted where every weight is bitwise
    equal -- |q_t| and |q_r|).  ``mut``: a planted defect
    (models/smc_ref.py)."""
    N, W, V = x.shape
    dt = x.dtype.type
    ninf = dt(-np.inf)
    ni = np.arange(N)[:, None]
    with np.errstate(all="ignore"):
        y = x * inv_t.astype(x.dtype)[:, None, None]
        mx = y.max(-1, keepdims=True)
        se = _wave_sum(_rounded(np.exp, y - mx))
        lse_all = (mx + _rounded(np.log, se))[..., 0]
        if allowed is None:
            A = np.ones((N, W, V), bool)
            mxa, sea, lse_a = mx[..., 0], se[..., 0], lse_all
        else:
            A = np.asarray(allowed, bool)
            A = np.broadcast_to(A[:, None, :] if A.ndim == 2 else A, (N, W, V))
            mxa_k = np.where(A, y, ninf).max(-1, keepdims=True)
            sea_k = _wave_sum(np.where(A, _rounded(np.exp, y - mxa_k), dt(0)))
            mxa, sea = mxa_k[..., 0], sea_k[..., 0]
            lse_a = mxa + _rounded(np.log, sea)
        live, fin, dead = state == BEAM_LIVE, state == BEAM_FIN, state == BEAM_DEAD
        isf = forced >= 0
        credit = live & ~isf[:, None]
        if mut == "forced_adds_logm":
            credit = live
        if mut == "finished_reweighted":
            credit = credit | (fin & ~isf[:, None])
        logm = np.where(credit, lse_a - lse_all, dt(0)).astype(x.dtype)
        u = (logw + logm).astype(x.dtype)
        lq = np.where(A & live[:, :, None], y - lse_a[:, :, None], dt(np.nan)).astype(x.dtype)
        nd = ~dead
        base = logw.astype(x.dtype) if mut == "resample_on_logw" else u   # what ESS and the ancestors are taken from
        mu = np.where(nd, u, ninf).max(1)
        mub = np.where(nd, base, ninf).max(1)
        e = np.where(nd, _rounded(np.exp, base - mub[:, None]), dt(0)).astype(x.dtype)
        cum = _slot_cumsum(e)
        S = cum[:, -1]
        Q = _slot_cumsum(e * e)[:, -1]
        ess = (S * S) / Q
        eu = np.where(nd, _rounded(np.exp, u - mu[:, None]), dt(0)).astype(x.dtype)
        Su = _slot_cumsum(eu)[:, -1]
        fan = step == 0
        res = np.zeros(N, bool) if fan else (ess < dt(thr) * dt(W))
        Uw = noise[:, :, 1].astype(x.dtype)
        Ui = Uw if mut == "u_per_slot" else np.broadcast_to(Uw[:, :1], (N, W))
        t = ((np.arange(W, dtype=x.dtype)[None, :] + Ui) / dt(W) * S[:, None]).astype(x.dtype)
        over = (cum[:, None, :] > t[:, :, None]) & nd[:, None, :]       # [N, i, b]
        last = (W - 1 - np.argmax(nd[:, ::-1], 1))
        a_res = np.where(over.any(-1), np.argmax(over, -1), last[:, None])
        ident = np.broadcast_to(np.arange(W)[None, :], (N, W))
        if fan:
            anc = np.zeros((N, W), np.int64)
            nlogw = np.broadcast_to(u[:, :1], (N, W)).astype(x.dtype)
        else:
            anc = np.where(res[:, None], a_res, ident)
            eq = (mu + _rounded(np.log, Su / dt(W)))[:, None]
            if mut == "weights_not_equalised":
                eq = u[ni, anc]
            nlogw = np.where(res[:, None], eq, u).astype(x.dtype)
        a_live, a_fin = live[ni, anc], fin[ni, anc]
        ya, Aa = y[ni, anc], A[ni, anc]                                  # [N, W, V]
        ex = np.where(Aa, _rounded(np.exp, ya - mxa[ni, anc][:, :, None]), dt(0)).astype(x.dtype)
        run = _slot_cumsum(ex)
        tot = sea[ni, anc]
        target = (noise[:, :, 0].astype(x.dtype) * tot).astype(x.dtype)
        hit = (run > target[:, :, None]) & Aa
        lastc = V - 1 - np.argmax(Aa[:, :, ::-1], -1)
        c = np.where(hit.any(-1), np.argmax(hit, -1), lastc)
        c = np.where(isf[:, None], np.maximum(forced, 0)[:, None], c)
        draws = a_live & ~isf[:, None]
        dl = np.where(draws, np.take_along_axis(ya, c[:, :, None], -1)[..., 0] - lse_a[ni, anc], dt(0)).astype(x.dtype)
        nlogq = np.where(a_live | a_fin, logq[ni, anc] + np.where(a_live, dl, dt(0)), ninf).astype(x.dtype)
        nlogw = np.where(a_live | a_fin, nlogw, ninf).astype(x.dtype)
        parent = np.where(a_live | a_fin, anc, -1).astype(np.int32)
        chrs = np.where(a_live, c, -1).astype(np.int32)
        nstate = np.where(a_fin | (a_live & (c == eos)), BEAM_FIN, np.where(a_live, BEAM_LIVE, BEAM_DEAD)).astype(np.int32)
        nxt = np.where(nstate == BEAM_LIVE, c, sos).astype(np.int32)
        # what the guard is made of (float64 quotients of this precision's values)
        f8 = np.float64
        q_ess = ess.astype(f8) / W
        q_t = np.where(res[:, None, None] & nd[:, None, :], (cum[:, None, :].astype(f8) - t[:, :, None].astype(f8)) /
                       S.astype(f8)[:, None, None], np.nan)
        run_c = np.take_along_axis(run, c[:, :, None], -1)[..., 0].astype(f8)
        ex_c = np.take_along_axis(ex, c[:, :, None], -1)[..., 0].astype(f8)
        q_r = np.stack([(run_c - target.astype(f8)) / tot.astype(f8), (run_c - ex_c - target.astype(f8)) / tot.astype(f8)], -1)
        q_r = np.where(draws[:, :, None], q_r, np.nan)
        # (weights that are all bitwise equal give e = 1, S = Q = the slot count and ESS exactly, in any precision:
        # that decision carries no rounding)
        flat = (np.where(nd, base, mub[:, None]) == mub[:, None]).all(1)
        c_ess = np.full(N, np.inf) if fan else np.where(flat, np.inf, np.abs(ess.astype(f8) - f8(dt(thr)) * W) / W)
        c_t = np.where(np.isnan(q_t), np.inf, np.abs(q_t)).reshape(N, -1).min(1)
        c_r = np.where(np.isnan(q_r), np.inf, np.abs(q_r)).reshape(N, -1).min(1)
        clear = np.minimum(np.minimum(np.where(np.isnan(c_ess), np.inf, c_ess), c_t), c_r)
    counted = res | (np.ones(N, bool) if (mut == "fanout_counted" and fan) else np.zeros(N, bool))
    return dict(parent=parent, chr=chrs, state=nstate, logw=nlogw, logq=nlogq, next_id=nxt, resampled=counted,
                ess=ess.astype(x.dtype), logm=np.where(dead, dt(np.nan), logm).astype(x.dtype), lq=lq, q_ess=q_ess, q_t=q_t,
                q_r=q_r, clear=clear)


class ConditionalResult:
    """``HipGenerator.sample_conditional`` / ``cpu_ref.sample_conditional`` output for N prefixes of R runs
    of W particles, pooled per prefix (P = R W, run r in columns r W .. r W + W - 1):
    rows [N, P, MAX_LEN+1] uint8 (the ``generate`` format), log_weight [N, P] (the unnormalised log
    importance weights), logq [N, P] (the rows' log-probability under the constrained sampler), n_tok [N, P]
    int32, n_resampled [N, R] int32, log_z [N] float64 (the log-mean-exp of the pooled log_weight: the log of
    the estimate of Z = P(the rule | prefix) under the model at the temperature), z_stderr [N] (the standard
    error of exp(log_z) over the runs, NaN at R = 1; like exp(log_z) it is 0 where Z lies below the smallest
    double -- compare z_stderr / exp(log_z) through log_z then), ess [N] (the pool's effective sample size).

    ``exp(log_z)`` is an UNBIASED estimate of Z at any width and any number of runs.  ``weights``,
    ``expectation`` and ``draw`` normalise the weights by their own sum: they are consistent, with a bias of
    order 1 / particles -- use more runs, not a single row, when that matters."""

    def __init__(self, rows, log_weight, logq, n_tok, n_resampled, eos: int = 0):
        self.rows, self.log_weight, self.logq, self.n_tok, self.n_resampled, self.eos = rows, log_weight, logq, n_tok, n_resampled, eos
        N, P = log_weight.shape
        R = max(n_resampled.shape[1], 1) if n_resampled.ndim == 2 else 1
        lw = np.asarray(log_weight, np.float64)
        with np.errstate(all="ignore"):
            m = lw.max(1, keepdims=True) if P else np.zeros((N, 1))
            m = np.where(np.isfinite(m), m, 0.0)
            w = np.exp(lw - m)
            s = w.sum(1)
            self.log_z = (m[:, 0] + np.log(s / max(P, 1)))
            self.ess = np.where(s > 0, s * s / np.maximum((w * w).sum(1), 1e-300), 0.0)
            # the runs' means relative to the pooled maximum, rescaled last: a rule of probability far below the
            # smallest double still has the spread of its runs taken from non-zero numbers (the product underflows
            # only where exp(log_z) itself does)
            zr = w.reshape(N, R, P // R).mean(2) if P else np.zeros((N, R))
            self.z_stderr = np.exp(m[:, 0]) * zr.std(1, ddof=1) / math.sqrt(R) if R > 1 else np.full(N, np.nan)

    def names(self) -> List[List[str]]:
        """Per prefix the particles' names in pool order (the EOS byte dropped)."""
        full = np.full(self.rows.shape[0], self.rows.shape[1], np.int32)
        return BeamResult(self.rows, self.logq, self.n_tok, full, self.eos).names()

    def weights(self) -> np.ndarray:
        """[N, P] float64, the weights normalised per prefix (zeros where every weight is zero)."""
        lw = np.asarray(self.log_weight, np.float64)
        with np.errstate(all="ignore"):
            m = lw.max(1, keepdims=True)
            w = np.exp(lw - np.where(np.isfinite(m), m, 0.0))
            s = w.sum(1, keepdims=True)
            return np.where(s > 0, w / np.where(s > 0, s, 1.0), 0.0)

    def expectation(self, f) -> np.ndarray:
        """[N] self-normalised estimates of E[f(name) | the rule, prefix]; ``f`` maps a name (str) to a number.
        Consistent, bias O(1 / particles)."""
        w = self.weights()
        return np.array([sum(wk * float(f(nm)) for wk, nm in zip(w[n], names)) for n, names in enumerate(self.names())])

    def draw(self, k: int, seed: int = 0) -> List[List[str]]:
        """Per prefix k names drawn from the pool with probability proportional to the weights (multinomial
        resampling on the host): approximate draws from the model's conditional, bias O(1 / particles)."""
        rng = np.random.default_rng(seed)
        w = self.weights()
        out = []
        for n, names in enumerate(self.names()):
            if not w[n].sum() > 0:
                out.append([])
                continue
            out.append([names[j] for j in rng.choice(len(names), size=int(k), p=w[n] / w[n].sum())])
        return out


def conditional_inputs(cfg: GRUConfig, prefix=None, width: int = 16, count: Optional[int] = None, runs: int = 1,
                       seed: int = 0, start: int = 0, temperature=None, ess_threshold: float = 0.5, **excluded):
    """Validated (prefix rows [N R], plen [N R], inv_t [N R] float32, seed, start, thr, N, R) of
    ``sample_conditional``: every prefix repeated ``runs`` times, run r of prefix n at the global index
    start + n R + r; thr is ess_threshold rounded to float32.  ValueError for what ``distinct_inputs`` rejects, runs < 1, a threshold outside [0, 1]."""
    for k, v in excluded.items():
        if k not in ("top_k", "top_p", "logit_bias", "presence_penalty", "frequency_penalty", "soft"):
            raise TypeError(f"sample_conditional: unexpected keyword {k!r}")
        if v is not None:
            raise ValueError(f"sample_conditional does not take {k}: the target is the model's distribution at the "
                             "temperature, conditioned on prefix and constraints alone")
    if isinstance(runs, bool) or int(runs) != runs or runs < 1:
        raise ValueError(f"runs must be an integer >= 1, got {runs!r}")
    thr = float(ess_threshold)
    if not 0.0 <= thr <= 1.0:
        raise ValueError(f"ess_threshold must lie in [0, 1], got {ess_threshold!r}")
    thr = float(np.float32(thr))      # the value the device reads: the rule in any precision compares against it
    try:
        pre, plen, inv, seed, start = distinct_inputs(cfg, prefix, width, count, seed, start, temperature)
    except ValueError as e:
        raise ValueError(str(e).replace("sample_distinct", "sample_conditional")) from None
    N, R = pre.shape[0], int(runs)
    if start + N * R > 2 ** 64:
        raise ValueError("start + count * runs must stay below 2^64")
    return np.repeat(pre, R, 0), np.repeat(plen, R, 0), np.repeat(inv, R, 0), seed, start, thr, N, R


def conditional_constraints(cfg: GRUConfig, N: int, R: int, constraints):
    """``as_constraints`` for the N R names of a call.  A dict's values are one for every name or one per PREFIX
    (N of them, as in ``generate``): per-prefix values are repeated for the prefix's R runs.  A built
    Constraints / Automaton object holds one entry per name and serves R = 1 only."""
    if constraints is None:
        return None
    if not isinstance(constraints, dict):
        if R > 1:
            raise ValueError("sample_conditional with runs > 1 takes constraints as a dict of keywords")
        return as_constraints(cfg, N, constraints)
    kw = dict(constraints)
    if R > 1:
        for k, v in kw.items():
            if v is None or isinstance(v, (str, bytes)) or np.ndim(v) == 0:
                continue
            if k == "exclude" and all(isinstance(x, (str, bytes)) for x in v):      # one list of names for everybody
                continue
            if len(v) != N:
                raise ValueError(f"constraints[{k!r}]: one value or {N} values (one per prefix) expected, got {len(v)}")
            kw[k] = [x for x in v for _ in range(R)]
    return as_constraints(cfg, N * R, kw)


def pool_conditional(rows, logw, logq, ntok, nres, N: int, R: int, W: int, eos: int) -> ConditionalResult:
    """The device's / the rule's [N R, W] outputs pooled per prefix."""
    return ConditionalResult(rows.reshape(N, R * W, rows.shape[-1]), logw.reshape(N, R * W), logq.reshape(N, R * W),
                             ntok.reshape(N, R * W), nres.reshape(N, R), eos)


def sample_conditional(params: Params, cfg: GRUConfig, prefix=None, width: int = 16, count: Optional[int] = None, *,
                       runs: int = 1, seed: int = 0, start: int = 0, temperature=None, constraints=None,
                       ess_threshold: float = 0.5, **excluded) -> ConditionalResult:
    """``runs`` independent systems of ``width`` weighted particles per prefix (the rule above), in the dtype
    of ``params`` (fp64 params: the oracle; the CPU path of ``cli conditional``)."""
    pre, plen, inv, seed, start, thr, N, R = conditional_inputs(cfg, prefix, width, count, runs, seed, start, temperature,
                                                                ess_threshold, **excluded)
    cons = conditional_constraints(cfg, N, R, constraints)
    check_prefix_allowed(cons, pre, plen)
    rows, logw, logq, ntok, nres = sample_conditional_rule(params, cfg, pre, plen, int(width), seed, start, inv, thr, cons)
    return pool_conditional(rows, logw, logq, ntok, nres, N, R, int(width), cfg.eos)


def sample_conditional_rule(params: Params, cfg: GRUConfig, pre: np.ndarray, plen: np.ndarray, W: int, seed: int,
                            start: int, inv_t: np.ndarray, thr: float, cons=None, mut: Optional[str] = None,
                            trace: Optional[list] = None):
    """The rule itself on validated inputs: (rows [M, W, ML+1], logw, logq [M, W], n_tok [M, W], n_resampled
    [M]) for the M names given.  ``trace``: a list that receives every step's ``smc_step`` output
    (models/smc_ref.py); ``mut``: a planted defect (there too)."""
    N, ML, V, H = pre.shape[0], cfg.max_len, cfg.vocab, cfg.hidden
    dt = params["fc.weight"].dtype
    npdt = np.float64 if dt == torch.float64 else np.float32
    rows = np.zeros((N, W, ML + 1), np.uint8)
    logw = np.full((N, W), -np.inf, npdt)
    logq = np.full((N, W), -np.inf, npdt)
    state = np.full((N, W), BEAM_DEAD, np.int32)
    ntok = np.zeros((N, W), np.int32)
    nres = np.zeros(N, np.int32)
    if N == 0:
        return rows, logw, logq, ntok, nres
    logw[:, 0] = logq[:, 0] = 0
    state[:, 0] = BEAM_LIVE
    hs = [torch.zeros(N * W, H, dtype=dt) for _ in range(cfg.layers)]
    cur = torch.full((N * W,), cfg.sos, dtype=torch.int64)
    aut = cons if isinstance(cons, Automaton) else None
    if aut is not None:
        alines, astate = aut.lines(), np.zeros((N, W), np.int64)
        astate[:, 0] = aut.start
    gidx = np.arange(N, dtype=np.uint64) + np.uint64(0 if mut == "counter_local_index" else start)
    ni = np.arange(N)[:, None]
    for l in range(ML):
        inp = params["embedding"][cur]
        new = []
        for k in range(cfg.layers):
            gi = inp @ params[f"weight_ih_l{k}"].T + params[f"bias_ih_l{k}"]
            gh = hs[k] @ params[f"weight_hh_l{k}"].T + params[f"bias_hh_l{k}"]
            hk, _ = _gates(gi, gh, hs[k])
            new.append(hk)
            inp = hk
        logits = inp @ params["fc.weight"].T + params["fc.bias"]
        if dt != torch.float64:
            logits = logits.to(torch.float32)
        x = logits.numpy().reshape(N, W, V)
        allowed = None if cons is None else (alines[astate] if aut is not None else cons.allowed(l))
        forced = np.where(plen > l, pre[:, l].astype(np.int64), -1)
        noise = smc_uniform(seed, gidx, 0 if mut == "counter_without_step" else l, W)
        s = smc_step(x, logw, logq, state, forced, allowed, inv_t, noise, thr, l, cfg.eos, cfg.sos, mut)
        if trace is not None:
            trace.append(s)
        par = np.maximum(s["parent"], 0)
        alive = s["parent"] >= 0
        app = s["chr"] >= 0
        nrows = np.where(alive[:, :, None], rows[ni, par], 0).astype(np.uint8)
        nrows[:, :, l] = np.where(app, s["chr"], nrows[:, :, l])
        ntok = np.where(alive, np.where(app, l + 1, ntok[ni, par]), 0).astype(np.int32)
        if aut is not None:   # (a carried or dead slot sits in state 0)
            astate = np.where(app, aut.nxt[astate[ni, par], np.maximum(s["chr"], 0)].astype(np.int64), 0)
        gather = torch.from_numpy((ni * W + par).reshape(-1).astype(np.int64))
        dead = torch.from_numpy(~alive.reshape(-1))
        hs = [h[gather].masked_fill(dead[:, None], 0) for h in new]
        rows, logw, logq, state = nrows, s["logw"], s["logq"], s["state"]
        nres = nres + s["resampled"].astype(np.int32)
        cur = torch.from_numpy(s["next_id"].reshape(-1).astype(np.int64))
    return rows, logw, logq, ntok, nres

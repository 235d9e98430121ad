"""beam_head_bf16 + beam_merge, and beam_reorder_bf16, alone (csrc/kernels/beam_fast.hip), exact by construction.

h holds values from {-1, -1/2, 0, 1/2, 1}, W_fc and b_fc multiples of 1/4 (a sub-grid of the 1/8 grid) of
magnitude <= 1, score_in multiples of 1/8: every logit is a multiple of 1/8 below 2^9, exact in fp32 in any
summation order, so only the softmax arithmetic separates the kernels from float64.  The last quarter of W_fc's
rows repeats the first (ties inside a row); in every name beam 1 is a bitwise copy of beam 0 (h row, score and
state: exact ties across rows) and beam 3 has beam 2's score (near comparisons across rows).

Reference: the float64 log-softmax and cpu_ref.beam_select per name.  A slot is compared when both gaps to its
neighbours among the first W + 1 float64 candidates are 0 (an exact tie, decided by j) or above beam_ref.GUARD;
at most 1 % of a case's slots may be left out.  Checked on the CPU: on these grids the reference alone leaves out
no slot of any case (two candidates of different rows differ by a multiple of 1/8 plus the difference of two
log-sum-exps, which falls inside the guard about once in 350 pairs)."""
import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.models import beam_ref, cpu_ref

DEV = "cuda"
ML, STEP, SOS, EOS = 6, 2, 1, 5
DEAD, LIVE, FIN = cpu_ref.BEAM_DEAD, cpu_ref.BEAM_LIVE, cpu_ref.BEAM_FIN


def make_inputs(H, V, W, many, forced):
    N = 64 // W + 2 if many else 1          # many: the rows straddle a 64-row tile
    R = N * W
    Bp = (R + 63) // 64 * 64
    rng = np.random.default_rng(H + 7 * V + 131 * W + 2 * many + forced)
    h = rng.integers(-2, 3, size=(Bp, H)) / 2.0
    Wfc = rng.integers(-4, 5, size=(V, H)) / 4.0
    bfc = rng.integers(-4, 5, size=V) / 4.0
    Wfc[3 * V // 4:], bfc[3 * V // 4:] = Wfc[:V // 4], bfc[:V // 4]
    score = -rng.integers(0, 33, R) / 8.0
    state = rng.integers(0, 3, R).astype(np.int32)
    state[::W] = np.where(np.arange(N) % 3 == 2, FIN, LIVE)          # beam 0: never dead
    if many and V == 64:
        state[64:] = np.where(state[64:] == LIVE, FIN, state[64:])   # the second workgroup has no live row
    for n in range(N):
        if W >= 2:
            h[n * W + 1], score[n * W + 1], state[n * W + 1] = h[n * W], score[n * W], state[n * W]
        if W >= 4:
            score[n * W + 3] = score[n * W + 2]
    score[state == DEAD] = -np.inf
    plen = np.full(N, ML if forced else 0, np.int32)
    prefix = rng.integers(0, min(V, 256), (N, ML)).astype(np.uint8)
    prefix[prefix == EOS] = 7
    return dict(N=N, R=R, Bp=Bp, h=h, Wfc=Wfc, bfc=bfc, score=score, state=state, plen=plen, prefix=prefix)


def reference(d, V, W):
    """float64: lp [R][V], the selection per name (cpu_ref.beam_select) and the mask of compared slots."""
    R, N = d["R"], d["N"]
    x = d["h"][:R] @ d["Wfc"].T + d["bfc"]                           # exact
    mx = x.max(-1, keepdims=True)
    lp = (x - mx) - np.log(np.exp(x - mx).sum(-1, keepdims=True))
    out = {k: np.full(R, -1, np.int64) for k in ("parent", "chr", "sel")}
    out.update(score=np.full(R, -np.inf), state=np.full(R, DEAD, np.int64), next_id=np.full(R, SOS, np.int64),
               ok=np.ones(R, bool), lp=lp)
    for n in range(N):
        sl = slice(n * W, (n + 1) * W)
        forced = int(d["prefix"][n, STEP]) if STEP < d["plen"][n] else -1
        if forced >= V:
            forced = 0
        for k, (b, c, s, j) in enumerate(cpu_ref.beam_select(lp[sl], d["score"][sl], d["state"][sl], forced)):
            if b < 0:
                continue
            o = n * W + k
            out["parent"][o], out["chr"][o], out["score"][o], out["sel"][o] = b, c, s, j
            out["state"][o] = FIN if (c < 0 or c == EOS) else LIVE
            out["next_id"][o] = c if (c >= 0 and c != EOS) else SOS
        gaps = beam_ref.select(lp[sl], d["score"][sl], d["state"][sl], forced, EOS, SOS)["gaps"]
        clear = (gaps == 0) | (gaps > beam_ref.GUARD)
        for k in range(W):
            out["ok"][n * W + k] = all(clear[i] for i in (k - 1, k) if 0 <= i < len(clear))
    return out


def launch(ext, d, H, V, W, want_lp=True):
    R, N, Bp = d["R"], d["N"], d["Bp"]
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)
    dev = dict(h=t(d["h"], torch.bfloat16), Wfc=t(d["Wfc"], torch.bfloat16), bfc=t(d["bfc"], torch.float32),
               score_in=t(d["score"], torch.float32), state_in=t(d["state"], torch.int32),
               plen=t(d["plen"], torch.int32), prefix=t(d["prefix"], torch.uint8))
    f = lambda v, dt, n=R: torch.full((n,), v, dtype=dt, device=DEV)
    out = dict(cand_score=f(np.nan, torch.float32, R * W), cand_chr=f(-9, torch.int32, R * W),
               score_out=f(np.nan, torch.float32), parent=f(-9, torch.int32), chr=f(-9, torch.int32),
               state_out=f(-9, torch.int32), next_id=f(-9, torch.int32), sel=f(-9, torch.int32),
               lp=f(np.nan, torch.float32, R * V), err=torch.zeros(4, dtype=torch.int32, device=DEV))
    s = torch.cuda.current_stream().cuda_stream
    ptr = lambda names: {k: (dev.get(k, out.get(k))).data_ptr() for k in names}
    head = ptr(("h", "Wfc", "bfc", "score_in", "state_in", "plen", "prefix", "cand_score", "cand_chr", "err"))
    if want_lp:
        head["lp"] = out["lp"].data_ptr()
    ext.beam_head(dict(head, N=N, W=W, Bp=Bp, H=H, V=V, step=STEP, max_len=ML), s)
    ext.beam_merge(dict(ptr(("cand_score", "cand_chr", "score_in", "state_in", "score_out", "parent", "chr", "state_out",
                             "next_id", "sel")), N=N, W=W, V=V, sos=SOS, eos=EOS), s)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("forced", [0, 1])
@pytest.mark.parametrize("many", [0, 1])
@pytest.mark.parametrize("W", [1, 3, 16, 32])
@pytest.mark.parametrize("V", [64, 256, 512])
@pytest.mark.parametrize("H", [64, 192])        # one k-tile; an odd number that wraps the two-slot ring
def test_head_and_merge_exact_operands(ext, H, V, W, many, forced):
    d = make_inputs(H, V, W, many, forced)
    ref = reference(d, V, W)
    ok = ref["ok"]
    assert (~ok).sum() <= 0.01 * len(ok), f"{int((~ok).sum())} of {len(ok)} slots inside the guard"
    got = launch(ext, d, H, V, W)
    assert int(got["err"][0]) == 0
    for k, g in (("sel", "sel"), ("parent", "parent"), ("chr", "chr"), ("state", "state_out"), ("next_id", "next_id")):
        assert np.array_equal(got[g][ok], ref[k][ok]), k
    gs, rs = got["score_out"].astype(np.float64)[ok], ref["score"][ok]
    assert np.array_equal(np.isneginf(gs), np.isneginf(rs)) and not np.isnan(gs).any()
    fin = np.isfinite(rs)
    dev = float(np.abs(gs[fin] - rs[fin]).max()) if fin.any() else 0.0
    live = d["state"] == LIVE
    dlp = float(np.abs(got["lp"].reshape(d["R"], V)[live].astype(np.float64) - ref["lp"][live]).max())
    print(f"score_out: max |d| {dev:.3e}; lp: max |d| {dlp:.3e}; slots left out {int((~ok).sum())} of {len(ok)}")
    assert dev <= beam_ref.ATOL["cand"] and dlp <= beam_ref.ATOL["lp"]
    again = launch(ext, d, H, V, W, want_lp=False)      # a second launch (without the lp output): the same bytes
    for k in ("cand_score", "cand_chr", "score_out", "parent", "chr", "state_out", "next_id", "sel"):
        assert got[k].tobytes() == again[k].tobytes(), k


@pytest.mark.gpu
def test_forced_byte_outside_the_vocabulary(ext):
    H, V, W = 64, 64, 3
    d = make_inputs(H, V, W, 0, 1)
    d["prefix"][0, STEP] = 200
    ref = reference(d, V, W)                            # the rule: taken as char 0
    got = launch(ext, d, H, V, W)
    assert int(got["err"][0]) & 16 and int(got["err"][1]) == 200
    assert np.array_equal(got["sel"][ref["ok"]], ref["sel"][ref["ok"]])


@pytest.mark.gpu
@pytest.mark.parametrize("L,H,W,N", [(1, 64, 1, 3), (2, 192, 3, 23), (4, 64, 32, 2)])
def test_reorder_bf16_is_an_exact_gather(ext, L, H, W, N):
    rng = np.random.default_rng(L + H + W)
    R = N * W
    hs = [torch.from_numpy(rng.standard_normal((R, H)).astype(np.float32)) for _ in range(L)]
    parent = rng.integers(-1, W, R).astype(np.int32)
    chrs = np.where(parent >= 0, rng.integers(-1, 60, R), -1).astype(np.int32)
    nxt = rng.integers(0, 64, R).astype(np.int32)
    lens = rng.integers(0, ML + 1, R).astype(np.int32)
    rows = rng.integers(1, 255, (R, ML + 1)).astype(np.uint8)
    t = lambda a: torch.from_numpy(a).to(DEV)
    src = [h.to(DEV) for h in hs]
    dst = [torch.full((R, H), np.nan, device=DEV) for _ in range(L)]
    dstb = [torch.full((R, H), np.nan, dtype=torch.bfloat16, device=DEV) for _ in range(L)]
    dev = dict(parent=t(parent), chr=t(chrs), next_id=t(nxt), len_src=t(lens), rows_src=t(rows))
    out = dict(rows_dst=torch.zeros(R, ML + 1, dtype=torch.uint8, device=DEV), len_dst=torch.zeros(R, dtype=torch.int32, device=DEV),
               ids=torch.zeros(R, dtype=torch.int32, device=DEV), n_beams=torch.zeros(N, dtype=torch.int32, device=DEV))
    args = {k: v.data_ptr() for k, v in {**dev, **out}.items()}
    args.update(h_src=[x.data_ptr() for x in src], h_dst=[x.data_ptr() for x in dst], hb_dst=[x.data_ptr() for x in dstb],
                N=N, W=W, L=L, H=H, max_len=ML)
    ext.beam_reorder_bf16(args, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    g = np.arange(R) // W * W + np.maximum(parent, 0)
    alive = parent >= 0
    for l in range(L):
        want = np.where(alive[:, None], hs[l].numpy()[g], 0.0).astype(np.float32)
        assert np.array_equal(dst[l].cpu().numpy(), want)
        # what gru_fwd_step stores beside the parent's fp32 row: its round-to-nearest-even bf16
        assert torch.equal(dstb[l].cpu(), torch.from_numpy(want).to(torch.bfloat16))
    wrows = np.where(alive[:, None], rows[g], 0)
    wlen = np.where(alive, lens[g], 0)
    for r in np.flatnonzero(alive & (chrs >= 0) & (wlen < ML)):
        wrows[r, wlen[r]] = chrs[r]
        wlen[r] += 1
    assert np.array_equal(out["rows_dst"].cpu().numpy(), wrows) and np.array_equal(out["len_dst"].cpu().numpy(), wlen)
    assert np.array_equal(out["ids"].cpu().numpy(), nxt)
    assert np.array_equal(out["n_beams"].cpu().numpy(), alive.reshape(N, W).sum(1))

"""sbs_head_bf16 + sbs_merge alone (csrc/kernels/sbs_fast.hip) against float64 cpu_ref.sbs_step.

h holds values from {-1, -1/2, 0, 1/2, 1}, W_fc and b_fc multiples of 1/4 of magnitude <= 1: every logit is a
multiple of 1/8 below 2^9 and stays exact under 1 / T in {1, 1.25}, in any summation order, so only the
epilogue's arithmetic separates the kernels from float64.  The other inputs are planted as sbs_ref.step_inputs
does: logq on a 2^-7 grid, G = logq + a multiple of 2^-5, every slot state, slot 1 a bitwise copy of slot 0
(exact ties in Gt across rows), a seed and a start index above 2^32.

Reference and assertions: sbs_ref.select_ref (cpu_ref.sbs_step in float64 on the exact logits) and
sbs_ref.check_step -- sel / parent / chr / state / next_id equal wherever the scaled clearance is 0 (a tie) or
at least sbs_ref.GUARD, lq / gt / zmax / G_out / logq_out within sbs_ref.ATOL (gt in units of its scale), a row's
best child keeps G_b and a child's logq_out is logq_b + lq[c], both bitwise.  The inputs are the first of eight
seeds whose reference clears the guard for every name."""
import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.models import cpu_ref, sbs_ref

DEV = "cuda"
ML, STEP, SOS, EOS = 6, 2, 1, 5
DEAD, LIVE, FIN = cpu_ref.BEAM_DEAD, cpu_ref.BEAM_LIVE, cpu_ref.BEAM_FIN


def make_inputs(H, V, W, many, forced, seed=0):
    N = 64 // W + 2 if many else 1          # many: the rows straddle a 64-row tile
    R = N * W
    Bp = (R + 63) // 64 * 64
    rng = np.random.default_rng(1000 * seed + H + 7 * V + 131 * W + 2 * many + forced)
    h = rng.integers(-2, 3, size=(Bp, H)) / 2.0
    Wfc = rng.integers(-4, 5, size=(V, H)) / 4.0
    bfc = rng.integers(-4, 5, size=V) / 4.0
    logq = (-rng.integers(0, 1025, R) / 128.0).astype(np.float32)
    G = (logq + rng.integers(-64, 97, R) / 32.0).astype(np.float32)
    state = rng.integers(0, 3, R).astype(np.int32)
    state[::W] = np.where(np.arange(N) % 3 == 2, FIN, LIVE)          # slot 0: never dead
    if many and V == 64:
        state[64:] = np.where(state[64:] == LIVE, FIN, state[64:])   # the second workgroup has no live row
    if W >= 2:
        for n in range(N):
            h[n * W + 1], logq[n * W + 1], G[n * W + 1], state[n * W + 1] = h[n * W], logq[n * W], G[n * W], state[n * W]
    logq[state == DEAD] = -np.inf
    G[state == DEAD] = -np.inf
    prefix = rng.integers(0, min(V, 256), (N, ML)).astype(np.uint8)
    prefix[prefix == EOS] = 7
    x = (h[:R] @ Wfc.T + bfc).astype(np.float32)                     # exact
    # sbs_ref's step format: the exact logits as one slab
    return dict(V=V, W=W, N=N, R=R, Rp=Bp, H=H, splits=1, logits=x[None], bias=None, h=h, Wfc=Wfc, bfc=bfc, logq=logq, G=G,
                state=state, plen=np.full(N, ML if forced else 0, np.int32), prefix=prefix, step=STEP, ML=ML, sos=SOS,
                eos=EOS, inv_t=np.where(np.arange(N) % 2 == 0, 1.0, 1.25).astype(np.float32),
                seed=(0x9E3779B97F4A7C15 * (seed + 1)) % 2 ** 64, start=2 ** 33 + 5 + seed, allowed=None, astate=None)


def settled_inputs(*shape):
    for seed in range(8):
        d = make_inputs(*shape, seed=seed)
        ref = sbs_ref.select_ref(d)
        if (ref["clear"] >= sbs_ref.GUARD).all():
            return d, ref
    raise AssertionError(f"{shape}: no planted input clears the guard")


def launch(ext, d, debug=True):
    R, N, Bp, V, W = d["R"], d["N"], d["Rp"], d["V"], d["W"]
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)
    words = torch.from_numpy(np.array([d["seed"], d["start"]], np.uint64).view(np.int64)).to(DEV)
    dev = dict(h=t(d["h"], torch.bfloat16), Wfc=t(d["Wfc"], torch.bfloat16), bfc=t(d["bfc"], torch.float32),
               logq_in=t(d["logq"], torch.float32), G_in=t(d["G"], torch.float32), state_in=t(d["state"], torch.int32),
               plen=t(d["plen"], torch.int32), prefix=t(d["prefix"], torch.uint8), inv_t=t(d["inv_t"], torch.float32))
    f = lambda v, dt, n=R: torch.full((n,), v, dtype=dt, device=DEV)
    out = dict(cand_gt=f(np.nan, torch.float32, R * W), cand_chr=f(-9, torch.int32, R * W), cand_psi=f(np.nan, torch.float32, R * W),
               logq_out=f(np.nan, torch.float32), G_out=f(np.nan, torch.float32), parent=f(-9, torch.int32),
               chr=f(-9, torch.int32), state_out=f(-9, torch.int32), next_id=f(-9, torch.int32), sel=f(-9, torch.int32),
               lq=f(np.nan, torch.float32, R * V), gt=f(np.nan, torch.float32, R * V), zmax=f(np.nan, torch.float32),
               err=torch.zeros(4, dtype=torch.int32, device=DEV))
    s = torch.cuda.current_stream().cuda_stream
    ptr = lambda names: {k: (dev.get(k, out.get(k))).data_ptr() for k in names}
    head = ptr(("h", "Wfc", "bfc", "logq_in", "G_in", "state_in", "plen", "prefix", "inv_t", "cand_gt", "cand_chr", "cand_psi",
                "err") + (("lq", "gt", "zmax") if debug else ()))
    ext.sbs_head(dict(head, seed=words.data_ptr(), start=words.data_ptr() + 8, N=N, W=W, Bp=Bp, H=d["H"], V=V, step=STEP,
                      max_len=ML), s)
    ext.sbs_merge(dict(ptr(("cand_gt", "cand_chr", "cand_psi", "logq_in", "G_in", "state_in", "logq_out", "G_out", "parent",
                            "chr", "state_out", "next_id", "sel")), N=N, W=W, V=V, sos=SOS, eos=EOS), s)
    torch.cuda.synchronize()
    o = {k: v.cpu().numpy() for k, v in out.items()}
    o.update(logq=o["logq_out"], G=o["G_out"], state=o["state_out"], lq=o["lq"].reshape(R, V), gt=o["gt"].reshape(R, V))
    return o


@pytest.mark.gpu
@pytest.mark.parametrize("forced", [0, 1])
@pytest.mark.parametrize("many", [0, 1])
@pytest.mark.parametrize("W", [1, 3, 16, 32])
@pytest.mark.parametrize("V", [64, 256, 512])
@pytest.mark.parametrize("H", [64, 192])        # one k-tile; an odd number that wraps the two-slot ring
def test_head_and_merge_exact_operands(ext, H, V, W, many, forced):
    d, ref = settled_inputs(H, V, W, many, forced)
    got = launch(ext, d)
    assert int(got["err"][0]) == 0
    assert sbs_ref.check_step(d, ref, got) == []
    again = launch(ext, d, debug=False)     # a second launch, without the debug outputs: a workgroup without a
    for k in ("cand_gt", "cand_chr", "cand_psi", "logq_out", "G_out", "parent", "chr", "state_out", "next_id", "sel"):
        assert got[k].tobytes() == again[k].tobytes(), k    # live row now skips its product; the same bytes


@pytest.mark.gpu
def test_forced_byte_outside_the_vocabulary(ext):
    d = make_inputs(64, 64, 3, 0, 1)
    d["prefix"][0, STEP] = 200
    ref = sbs_ref.select_ref(d)             # the rule: taken as char 0
    got = launch(ext, d)
    assert int(got["err"][0]) & 16 and int(got["err"][1]) == 200
    assert sbs_ref.check_step(d, ref, got) == []

"""Per-element tests of the generation path's kernels against the float64 references of
models/gen_ref.py, each launched on its own through the raw bindings: the persistent generator
(gen_persist.hip) on a caller-owned workspace, gru_gates_f32 and gen_reset (gen_f32.hip), score_prep
and score_logprob_f32 (score.hip).

A persistent launch keeps every hidden state of every layer at every char, every logit and (more than
16 names) every published id in its exchange workspace (kernels.h, GenPersistArgs::ws), so each of
them is compared per element with the ONE-step float64 reference computed from the kernel's own
stored inputs (gen_ref.step_ref) -- no error piles up over chars or layers.  The uniforms are planted
by the float64 trajectory itself (gen_ref.plant_uniforms: each at least GUARD from every CDF edge),
so the output rows must equal the oracle's bytewise for every name and step.  All checks of a launch
are gen_ref.check_launch, which tests/test_gen_ref.py shows to fail on every planted defect.  The
tolerances are gen_ref.ATOL (measured on the CPU as emulator - reference).  Each comparison prints its
worst deviation before it asserts.

Cases (gen_ref.PERSIST_CASES): a every (H, L) variant at 3 names; b every name-count regime at H = 512;
c the same at H = 1024 (tagged state layout up to 8 names, no rolling prefetch); d the prefetch boundary
and four-layer stacks; e V = 512; f max_len 1, 2, 10; g names that end (states after the EOS, the early
exit with probs == nullptr); h one workspace over launches of alternating parity.
"""
import functools

import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.models import gen_ref as gr

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
I32 = torch.int32
PROBS_CANARY = 0x7FC0A5A5      # a NaN bit pattern
OUT_CANARY = 0xA5


def S():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture
def gp(ext):
    if ext.device_info()["cus"] < 256:
        pytest.skip("the persistent generator needs 256 compute units")
    return ext


def u32(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


# ====================================================================================== persistent launch
@functools.lru_cache(maxsize=2)
def _dev_weights(H, L, V, seed):
    w = gr._weights(H, L, V, seed)
    up = lambda t: None if t is None else t.to(DEV).contiguous()
    return {k: ([up(t) for t in v] if isinstance(v, list) else up(v)) for k, v in w.items() if k != "w64"}


def _ptrs(ts):
    return [0 if t is None else t.data_ptr() for t in ts]


def _new_ws(ext, H, L, V, ML):
    n = ext.gen_persist_ws_floats(H, L, V, ML)
    assert n == 2 * gr.set_floats(H, L, V, ML)
    ws = torch.zeros(n, dtype=I32, device=DEV)
    ext.gen_persist_fill_ws(ws.data_ptr(), H, L, V, ML, S())
    sync = torch.zeros(ext.gen_persist_sync_words(L), dtype=I32, device=DEV)
    torch.cuda.synchronize()
    assert (u32(ws) == gr.EMPTY).all()
    return ws, sync


def _launch(ext, c, ws=None, sync=None, par=0):
    """One launch of case c, fully checked.  Returns (out rows, the words of set par that the launch defines)."""
    H, L, V, N, ML = c.H, c.L, c.V, c.N, c.ML
    assert ext.gen_persist_supported(H, L, V, N, ML), c.name
    d = gr.case_inputs(c)
    orc = gr.plant_uniforms(d, gr.case_plan(c))
    w = _dev_weights(H, L, V, c.seed_off)
    if ws is None:
        ws, sync = _new_ws(ext, H, L, V, ML)
    Np = (N + 15) // 16 * 16
    err = torch.zeros(4, dtype=I32, device=DEV)
    out = torch.full((N + 2, ML + 1), OUT_CANARY, dtype=torch.uint8, device=DEV)
    rf = torch.from_numpy(orc["rf"]).to(DEV).contiguous()
    a = dict(N=N, H=H, L=L, V=V, ML=ML, sos=c.sos, eos=c.eos, par=par, Whh=_ptrs(w["Whh"]), bhh=_ptrs(w["bhh"]),
             Wih=_ptrs(w["Wih"]), bih=_ptrs(w["bih"]), Wfc=w["Wfc"].data_ptr(), bfc=w["bfc"].data_ptr(), P=w["P"].data_ptr(),
             rf=rf.data_ptr(), out=out.data_ptr(), ws=ws.data_ptr(), sync=sync.data_ptr(), err=err.data_ptr())
    probs = None
    if c.probs:
        probs = torch.full((Np + 2, V), PROBS_CANARY, dtype=I32, device=DEV)
        a["probs"] = probs.data_ptr()
    before = u32(ws)
    ext.gen_persist(a, S())
    torch.cuda.synchronize()
    after = u32(ws)
    got = dict(err=u32(err), sync=u32(sync), out=out.cpu().numpy(), out_canary=OUT_CANARY, par=par, ws_before=before, ws_after=after)
    if c.probs:
        got["probs"] = u32(probs).view(np.float32)
        got["probs_before"] = np.full((Np + 2, V), PROBS_CANARY, np.uint32).view(np.float32)
    fails, fig = gr.check_launch(d, orc, got, probs=c.probs)
    T = gr.chars_run(orc["alive_after"], ML, c.probs)
    print(f"GEN {c.name:28s} par {par} chars {T}/{ML} " + " ".join(f"{k} {v:9.3e} (atol {gr.ATOL[k]:.2e})" for k, v in fig.items()))
    assert not fails, f"{c.name}: " + "; ".join(fails)
    sf = gr.set_floats(H, L, V, ML)
    defined = gr.ws_decode(after, par, H, L, V, ML, N, T)["mask"]
    if N > 16:                                                    # rows N .. Np of a plain slot are unspecified
        defined = defined & _rows_below(H, L, V, ML, N)
    return got["out"][:N].copy(), after[par * sf:(par + 1) * sf][defined].copy()


def _rows_below(H, L, V, ML, N):
    """Mask of a set's words in name rows n < N of the plain layout (the rows a launch defines)."""
    m = np.zeros(gr.set_floats(H, L, V, ML), dtype=bool)
    st, lg, idw = gr._views(m, H, L, V, ML)
    st.reshape(L, ML, gr.NMAX, H)[:, :, :N] = True
    lg[:, :N] = True
    idw[:, :N] = True
    return m


@pytest.mark.parametrize("c", gr.CASES_A, ids=lambda c: c.name)
def test_persist_every_variant(gp, c):
    _launch(gp, c)


@pytest.mark.parametrize("c", gr.CASES_B + gr.CASES_C, ids=lambda c: c.name)
def test_persist_every_name_count_regime(gp, c):
    _launch(gp, c)


@pytest.mark.parametrize("c", gr.CASES_D, ids=lambda c: c.name)
def test_persist_prefetch_boundary_and_deep_stacks(gp, c):
    _launch(gp, c)


@pytest.mark.parametrize("c", gr.CASES_E, ids=lambda c: c.name)
def test_persist_vocab_512(gp, c):
    _launch(gp, c)


@pytest.mark.parametrize("c", gr.CASES_F, ids=lambda c: c.name)
def test_persist_max_len(gp, c):
    _launch(gp, c)


@pytest.mark.parametrize("c", gr.CASES_G, ids=lambda c: c.name)
def test_persist_names_that_end(gp, c):
    """ends01: the states after a name's EOS follow the sampled ids while its row stops at the EOS byte.
    all-end with probs == nullptr: the launch stops after char 1 and leaves chars >= 2 untouched; with
    probs set it runs every char."""
    _launch(gp, c)


def test_persist_one_workspace_alternating_parity(gp):
    """Four launches on one workspace with parity 0, 1, 0, 1 (16, 5, 64, 8 names at H = 1024, L = 2: plain
    and tagged state layouts alternate over the same lines, each launch refilling the set the next one
    polls), each fully checked; a fifth repeats the first and reproduces its rows and its workspace
    words bitwise."""
    c0 = gr.CASES_H[0]
    ws, sync = _new_ws(gp, c0.H, c0.L, c0.V, c0.ML)
    kept = [_launch(gp, c, ws, sync, par=i % 2) for i, c in enumerate(gr.CASES_H)]
    out5, words5 = _launch(gp, c0, ws, sync, par=0)
    assert np.array_equal(out5, kept[0][0])
    assert np.array_equal(words5, kept[0][1])


def test_persist_binding_rejects_what_the_kernel_cannot_run(gp):
    assert not gp.gen_persist_supported(512, 2, 256, 65, 3) and not gp.gen_persist_supported(512, 2, 128, 4, 3)
    assert not gp.gen_persist_supported(1024, 3, 256, 4, 3) and not gp.gen_persist_supported(384, 1, 256, 4, 3)
    with pytest.raises(RuntimeError):
        gp.gen_persist(dict(N=4, H=512, L=2, V=256, ML=3, Whh=[0, 0], bhh=[0, 0], Wih=[0, 0], bih=[0, 0]), S())


# ====================================================================================== gru_gates_f32
PAD = 32


def _padded(t: torch.Tensor, fill=NAN):
    """t in the middle of a buffer of ``fill``; returns (buffer, view)."""
    flat = t.reshape(-1)
    buf = torch.full((flat.numel() + 2 * PAD,), fill, dtype=t.dtype, device=DEV)
    buf[PAD:PAD + flat.numel()] = flat.to(DEV)
    return buf, buf[PAD:PAD + flat.numel()]


def _run_gates(ext, d, hsplit):
    Bp, H = d["Bp"], d["H"]
    keep = {}
    a = dict(Bp=Bp, H=H, V=d["V"], gh_splits=d["gh_splits"], gh_slab=d["slab"], gi_splits=d["gi_splits"], gi_slab=d["slab"])
    for k in ("Gh", "Gi", "P", "hprev", "bgh", "bgi"):
        if d.get(k) is not None:
            keep[k] = _padded(d[k].float())
            a[k] = keep[k][1].data_ptr()
    if d["table"]:
        keep["ids"] = d["ids"].to(DEV)
        a["ids"] = keep["ids"].data_ptr()
    err = torch.zeros(4, dtype=I32, device=DEV)
    hout_buf, hout = _padded(torch.full((Bp, H), NAN))
    a.update(hout=hout.data_ptr(), err=err.data_ptr())
    hs_buf = None
    if hsplit:
        hs_buf = torch.full((Bp * 3 * H + 2 * PAD,), 0x7FFF, dtype=torch.int16, device=DEV)
        a["hsplit"] = hs_buf[PAD:].data_ptr()
    ext.gru_gates_f32(a, S())
    torch.cuda.synchronize()
    hb = hout_buf.cpu()
    assert bool(torch.isnan(hb[:PAD]).all()) and bool(torch.isnan(hb[PAD + Bp * H:]).all()), "hout canaries"
    h = hb[PAD:PAD + Bp * H].reshape(Bp, H)
    if hsplit:
        w = hs_buf.cpu()
        assert bool((w[:PAD] == 0x7FFF).all()) and bool((w[PAD + Bp * 3 * H:] == 0x7FFF).all()), "hsplit canaries"
        words = (w[PAD:PAD + Bp * 3 * H].to(torch.int32) & 0xFFFF).reshape(Bp, 3 * H)
        want = gr.hsplit_of(h)                                    # the split of the kernel's OWN h'
        assert torch.equal(words, want), "hsplit is not [hi | hi | lo] of hout"
        hi = (words[:, :H] << 16).to(torch.int32).view(torch.float32)
        lo = (words[:, 2 * H:] << 16).to(torch.int32).view(torch.float32)
        assert float((hi + lo - h).abs().max()) <= 2.0 ** -16
    return h, u32(err)


@pytest.mark.parametrize("k,a", list(enumerate(gr.gates_cases())), ids=lambda v: str(v).replace(" ", ""))
def test_gates_per_element(ext, k, a):
    d = gr.gates_inputs(*a)
    h, err = _run_gates(ext, d, hsplit=k % 2 == 0)
    ref = gr.gates_ref(d)
    dev = gr.deviation(h, ref)
    print(f"GEN gates {a} hsplit {k % 2 == 0}: worst {dev:9.3e} (atol {gr.ATOL['gates']:.2e})")
    assert not err.any()
    assert dev <= gr.ATOL["gates"]


@pytest.mark.parametrize("Bp,H", gr.GATES_SHAPES[1:])
def test_gates_invalid_ids(ext, Bp, H):
    """Ids -1 and V in two rows: bit 4 of err[0], err[1..2] name one of the two (id, row) pairs, those
    rows use table row 0 and every other row is unaffected."""
    d = gr.gates_inputs(Bp, H, True, 3, 1, True, bad_ids=True)
    ids = d["ids"].tolist()
    bad = [(i & 0xFFFFFFFF, b) for b, i in enumerate(ids) if i < 0 or i >= d["V"]]
    assert sorted(i for i, _ in bad) == [d["V"], 0xFFFFFFFF]
    h, err = _run_gates(ext, d, hsplit=True)
    assert err[0] == 16 and (int(err[1]), int(err[2])) in bad, err
    assert gr.deviation(h, gr.gates_ref(d)) <= gr.ATOL["gates"]   # gates_ref reads row 0 for the invalid ids
    good = gr.gates_inputs(Bp, H, True, 3, 1, True)
    for _, b in bad:
        good["ids"][b] = 0
    h2, err2 = _run_gates(ext, good, hsplit=False)
    assert not err2.any() and torch.equal(h2, h)


# ====================================================================================== gen_reset
@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("hb_cols", [None, 1, 3])
@pytest.mark.parametrize("Bp,H,ML", [(1, 64, 10), (33, 256, 10), (96, 1024, 63), (2, 64, 63)])
def test_gen_reset(ext, L, hb_cols, Bp, H, ML):
    """Every buffer starts as junk with canaries after it.  (96, 1024, 63): Bp H is beyond the 65536
    threads of the grid (the grid-stride tail); (2, 64, 63): max_len + 1 = H, the edge of the launcher's
    check."""
    tail = 24
    g = torch.Generator(device="cpu").manual_seed(Bp + H)
    hf = [torch.randn(Bp * H + tail, generator=g).to(DEV) for _ in range(L)]
    hbm = hb_cols or 0
    hb = [torch.full((Bp * hbm * H + tail,), 0x3F80, dtype=torch.int16, device=DEV) for _ in range(L)] if hbm else []
    ids = torch.full((Bp + tail,), 77, dtype=I32, device=DEV)
    alive = torch.full((Bp + tail,), 55, dtype=I32, device=DEV)
    out = torch.full((Bp * (ML + 1) + tail,), 0xA5, dtype=torch.uint8, device=DEV)
    hf0 = [t.cpu().clone() for t in hf]
    a = dict(L=L, Bp=Bp, H=H, ML=ML, sos=9, hf=[t.data_ptr() for t in hf], ids=ids.data_ptr(), alive=alive.data_ptr(),
             out=out.data_ptr())
    if hbm:
        a.update(hb=[t.data_ptr() for t in hb], hb_cols=hbm * H if hbm == 3 else (H if L == 4 else 0))   # 0 means H
    ext.gen_reset(a, S())
    torch.cuda.synchronize()
    for l in range(L):
        t = hf[l].cpu()
        assert not t[:Bp * H].any() and torch.equal(t[Bp * H:], hf0[l][Bp * H:]), f"hf[{l}]"
        if hbm:
            w = hb[l].cpu()
            assert not w[:Bp * hbm * H].any() and bool((w[Bp * hbm * H:] == 0x3F80).all()), f"hb[{l}]"
    i, al, o = ids.cpu(), alive.cpu(), out.cpu()
    assert bool((i[:Bp] == 9).all()) and bool((i[Bp:] == 77).all())
    assert bool((al[:Bp] == 1).all()) and bool((al[Bp:] == 55).all())
    assert not o[:Bp * (ML + 1)].any() and bool((o[Bp * (ML + 1):] == 0xA5).all())


def test_gen_reset_rejects_max_len_beyond_h(ext):
    t = torch.zeros(64 * 66, device=DEV)
    i = torch.zeros(64 * 66, dtype=I32, device=DEV)
    with pytest.raises(RuntimeError):
        ext.gen_reset(dict(L=1, Bp=1, H=64, ML=64, hf=[t.data_ptr()], ids=i.data_ptr(), alive=i.data_ptr(), out=t.data_ptr()), S())


# ====================================================================================== score_prep
def _prep_rows(ML, V, sos, eos, with_bad):
    rows = np.array([[eos, 9, 9, 9, 9, 9, 0],            # EOS at byte 0
                     [4, 6, eos, 7, 7, 7, 0],            # in the middle
                     [4, 6, 8, 10, 12, eos, 0],          # at ML - 1
                     [1, 3, 4, 6, 8, 10, eos],           # absent among the first ML bytes
                     [4, V + 3, 6, eos, V + 9, 1, 0]],   # a byte >= V at a scored position (and one after the EOS)
                    np.uint8)
    assert rows.shape[1] == ML + 1
    return rows if with_bad else rows[:4]


@pytest.mark.parametrize("with_bad", [True, False])
@pytest.mark.parametrize("via_dev", [False, True])
def test_score_prep_exact(ext, with_bad, via_dev):
    ML, V, sos, eos, Bp = 6, 64, 5, 2, 8
    rows = _prep_rows(ML, V, sos, eos, with_bad)
    N = len(rows)
    tail = 16
    drows = torch.from_numpy(rows).to(DEV)
    ids = torch.full((ML * Bp + tail,), -7, dtype=I32, device=DEV)
    tgt = torch.full((ML * Bp + tail,), -7, dtype=I32, device=DEV)
    ntok = torch.full((Bp + tail,), -7, dtype=I32, device=DEV)
    err = torch.zeros(4, dtype=I32, device=DEV)
    a = dict(rows=drows.data_ptr(), ids=ids.data_ptr(), tgt=tgt.data_ptr(), ntok=ntok.data_ptr(), err=err.data_ptr(),
             Bp=Bp, ML=ML, V=V, sos=sos, eos=eos)
    if via_dev:
        n_dev = torch.full((4,), 99, dtype=I32, device=DEV)
        ext.score_set_count(n_dev.data_ptr(), N, S())
        a.update(n_dev=n_dev.data_ptr(), N=Bp)             # the device word wins over the value
    else:
        a["N"] = N
    ext.score_prep(a, S())
    torch.cuda.synchronize()
    if via_dev:
        assert n_dev.cpu().tolist() == [N, 99, 99, 99]
    rids, rtgt, rntok, bad = gr.score_prep_ref(rows, N, Bp, ML, V, sos, eos)
    assert bad == with_bad and int(err.cpu()[0]) == (16 if with_bad else 0) and not err.cpu()[1:].any()
    i, t, n = ids.cpu().numpy(), tgt.cpu().numpy(), ntok.cpu().numpy()
    assert np.array_equal(i[:ML * Bp].reshape(ML, Bp), rids) and (i[ML * Bp:] == -7).all()
    assert np.array_equal(t[:ML * Bp].reshape(ML, Bp), rtgt) and (t[ML * Bp:] == -7).all()
    assert np.array_equal(n[:Bp], rntok) and (n[Bp:] == -7).all()
    assert list(rntok[:4]) == [1, 3, 6, 6]


# ====================================================================================== score_logprob_f32
@pytest.mark.parametrize("V,ML,Bp,splits,bias", gr.SCORE_CASES)
def test_score_logprob_per_element(ext, V, ML, Bp, splits, bias):
    d = gr.score_inputs(V, ML, Bp, splits, bias)
    lg = d["logits"].to(DEV).contiguous()
    tgt, ntok = d["tgt"].to(DEV).contiguous(), d["ntok"].to(DEV).contiguous()
    tail = 8
    lp = torch.full((Bp * ML + tail,), NAN, device=DEV)
    rank = torch.full((Bp * ML + tail,), -9, dtype=I32, device=DEV)
    name = torch.full((Bp + tail,), NAN, device=DEV)
    nout = torch.full((Bp + tail,), -9, dtype=I32, device=DEV)
    a = dict(logits=lg.data_ptr(), splits=splits, slab=d["slab"], tgt=tgt.data_ptr(), ntok=ntok.data_ptr(),
             tok_logp=lp.data_ptr(), rank=rank.data_ptr(), name_logp=name.data_ptr(), ntok_out=nout.data_ptr(), Bp=Bp, V=V, ML=ML)
    if bias:
        b = d["bias"].to(DEV)
        a["bias"] = b.data_ptr()
    ext.score_logprob(a, S())
    torch.cuda.synchronize()
    rlp, rname, rrank, rnt = gr.score_ref(d)
    glp, grank, gname, gnt = lp.cpu(), rank.cpu(), name.cpu(), nout.cpu()
    assert bool(torch.isnan(glp[Bp * ML:]).all()) and bool((grank[Bp * ML:] == -9).all())
    assert bool(torch.isnan(gname[Bp:]).all()) and bool((gnt[Bp:] == -9).all())
    glp, grank, gname, gnt = glp[:Bp * ML].reshape(Bp, ML), grank[:Bp * ML].reshape(Bp, ML), gname[:Bp], gnt[:Bp]
    dl, dn = gr.deviation(glp, rlp), gr.deviation(gname, rname)
    print(f"GEN logp V {V} ML {ML} splits {splits} bias {bias}: tok {dl:9.3e} (atol {gr.ATOL['logp']:.2e}) "
          f"name {dn:9.3e} (atol {gr.ATOL['name_logp']:.2e})")
    assert torch.equal(gnt, rnt) and torch.equal(grank, rrank)
    assert dl <= gr.ATOL["logp"] and dn <= gr.ATOL["name_logp"]
    masked = torch.arange(ML)[None, :] >= rnt[:, None]
    assert not glp[masked].any()                                  # masked positions are 0, not merely small
    seq = np.zeros(Bp, np.float32)
    g = glp.numpy()
    for l in range(ML):
        seq = (seq + g[:, l]).astype(np.float32)                  # masked positions add 0
    assert np.array_equal(seq.view(np.uint32), gname.numpy().view(np.uint32)), "name_logp is not the step-order fp32 sum"

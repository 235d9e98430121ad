"""Beam search on the device (csrc/kernels/beam.hip, Generator::beam) against the float64 rule of
models/beam_ref.py: the selection kernel on planted inputs, the reorder as a bitwise gather, the
whole search against the oracle, its relations to generate / score, graph reuse and the errors."""
import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.models import beam_ref as br
from gru_mpi_cuda_amd.models import cpu_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------- beam_select_f32
CANARY = 3      # rows past the launch's own in every output


def run_select(ext, d, want_lp=True, prefix=None):
    """One launch on the planted inputs ``d``.  Outputs start NaN / -77 filled with CANARY extra rows;
    returns them whole plus the error words."""
    R, V, W, N = d["R"], d["V"], d["W"], d["N"]
    lg, sc, st = t(d["logits"]), t(d["score"]), t(d["state"])
    pl, pre = t(d["plen"]), t(d["prefix"] if prefix is None else prefix)
    out_f = torch.full((R + CANARY,), float("nan"), device=DEV)
    outs = {k: torch.full((R + CANARY,), -77, dtype=torch.int32, device=DEV) for k in ("parent", "chr", "state_out", "next_id", "sel")}
    lp = torch.full((R + CANARY, V), float("nan"), device=DEV)
    err = torch.zeros(4, dtype=torch.int32, device=DEV)
    a = dict(logits=lg.data_ptr(), splits=d["splits"], slab=d["Rp"] * V, score_in=sc.data_ptr(), state_in=st.data_ptr(),
             plen=pl.data_ptr(), prefix=pre.data_ptr(), score_out=out_f.data_ptr(), err=err.data_ptr(),
             N=N, W=W, V=V, step=d["step"], max_len=d["ML"], sos=d["sos"], eos=d["eos"],
             **{k: v.data_ptr() for k, v in outs.items()})
    if not want_lp:
        del a["sel"]
    else:
        a["lp"] = lp.data_ptr()
    keep = [lg, sc, st, pl, pre]
    if d["bias"] is not None:
        b = t(d["bias"])
        keep.append(b)
        a["bias"] = b.data_ptr()
    ext.beam_select(a, stream())
    torch.cuda.synchronize()
    got = dict(score=out_f.cpu().numpy(), parent=outs["parent"].cpu().numpy(), chr=outs["chr"].cpu().numpy(),
               state=outs["state_out"].cpu().numpy(), next_id=outs["next_id"].cpu().numpy(), sel=outs["sel"].cpu().numpy(),
               lp=lp.cpu().numpy(), err=err.cpu().numpy(), logits_after=lg.cpu().numpy())
    return got


@pytest.mark.parametrize("i", range(len(br.STEP_CASES)), ids=lambda i: "-".join(map(str, br.STEP_CASES[i])))
def test_select_matches_fp64_rule(ext, i):
    c = br.STEP_CASES[i]
    d = br.plant_step(br.step_inputs(c, seed=i % 3))
    ref = br.select_ref(d)
    want_lp = i % 4 != 3      # every fourth case without the optional outputs
    got = run_select(ext, d, want_lp)
    R = d["R"]
    own = {k: (v[:R] if k not in ("err", "logits_after") else v) for k, v in got.items()}
    if not want_lp:
        own["lp"] = own["sel"] = None
    dev = np.abs(own["score"][np.isfinite(ref["score"])].astype(np.float64) - ref["score"][np.isfinite(ref["score"])])
    print(f"{c}: score deviation {dev.max() if len(dev) else 0.0:.3e} (atol {br.ATOL['cand']:.3e})",
          "" if not want_lp else f"lp deviation {np.abs(own['lp'].astype(np.float64) - ref['lp']).max():.3e} (atol {br.ATOL['lp']:.3e})")
    assert br.check_step(ref, own) == []
    assert (got["err"] == 0).all()
    # canary rows and the optional outputs that were not asked for: bitwise untouched
    assert np.isnan(got["score"][R:]).all() and np.isnan(got["lp"][R:]).all()
    for k in ("parent", "chr", "state", "next_id", "sel"):
        assert (got[k][R:] == -77).all(), k
    if not want_lp:
        assert np.isnan(got["lp"]).all() and (got["sel"] == -77).all()
    # the pad rows of the logits (NaN) were neither read into a result nor written
    assert np.array_equal(got["logits_after"], d["logits"], equal_nan=True)


def test_select_flags_prefix_byte_outside_vocab(ext):
    c = br.StepCase(64, 3, 3, 1, False, "forced", "live", 5)
    d = br.step_inputs(c, 1)
    pre = d["prefix"].copy()
    pre[1, d["step"]] = 200
    got = run_select(ext, d, prefix=pre)
    assert got["err"][0] == 16 and got["err"][1] == 200 and got["err"][2] == 1 * c.W and got["err"][3] == 0
    pre0 = pre.copy()
    pre0[1, d["step"]] = 0      # the byte is taken as 0
    ref = br.select_ref(dict(d, prefix=pre0))
    assert br.check_step(ref, {k: got[k][:d["R"]] for k in ("score", "parent", "chr", "state", "next_id", "sel", "lp")}) == []


def test_select_rejects_unsupported_shapes(ext):
    z = torch.zeros(4096, device=DEV)
    zi = torch.zeros(4096, dtype=torch.int32, device=DEV)
    base = dict(logits=z.data_ptr(), score_in=z.data_ptr(), state_in=zi.data_ptr(), plen=zi.data_ptr(), prefix=zi.data_ptr(),
                score_out=z.data_ptr() + 2048, parent=zi.data_ptr() + 1024, chr=zi.data_ptr() + 2048, state_out=zi.data_ptr() + 4096,
                next_id=zi.data_ptr() + 8192, N=1, W=2, V=64, step=0, max_len=4, sos=1, eos=0)
    for bad in (dict(V=96), dict(V=576), dict(W=0), dict(W=33), dict(V=64, W=65), dict(step=4)):
        with pytest.raises(RuntimeError):
            ext.beam_select(dict(base, **bad), stream())


# ------------------------------------------------------------------------------- beam_reorder
@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("kind", ["perm", "fan", "identity", "carry"])
def test_reorder_is_a_bitwise_gather(ext, L, kind):
    N, W, H, ML = 3, 5, 64, 6
    R, RT = N * W, 64      # rows of the launch, rows of every buffer
    rng = np.random.default_rng(11 + L)
    hs = [rng.standard_normal((RT, H)).astype(np.float32) for _ in range(L)]
    hd = [rng.standard_normal((RT, H)).astype(np.float32) for _ in range(L)]
    rows_s = rng.integers(1, 200, (RT, ML + 1)).astype(np.uint8)
    rows_d = rng.integers(1, 200, (RT, ML + 1)).astype(np.uint8)
    len_s = rng.integers(0, ML, RT).astype(np.int32)
    for r in range(RT):
        rows_s[r, len_s[r]:] = 0
    len_d = np.full(RT, -5, np.int32)
    ids = np.full(RT, -5, np.int32)
    nb = np.full(N + 2, -5, np.int32)
    if kind == "perm":
        parent = np.concatenate([rng.permutation(W) for _ in range(N)]).astype(np.int32)
    elif kind == "fan":
        parent = np.repeat(rng.integers(0, W, N), W).astype(np.int32)
    else:
        parent = np.tile(np.arange(W), N).astype(np.int32)
    chrs = rng.integers(0, 200, R).astype(np.int32)
    if kind == "carry":
        chrs[::2] = -1
        parent[W - 1::W] = -1      # and a dead slot per name
        chrs[W - 1::W] = -1
    nxt = rng.integers(0, 200, R).astype(np.int32)
    d_hs, d_hd = [t(h) for h in hs], [t(h) for h in hd]
    d_rs, d_rd, d_ls, d_ld, d_ids, d_nb = t(rows_s), t(rows_d), t(len_s), t(len_d), t(ids), t(nb)
    d_p, d_c, d_n = t(parent), t(chrs), t(nxt)
    ext.beam_reorder(dict(h_src=[x.data_ptr() for x in d_hs], h_dst=[x.data_ptr() for x in d_hd], parent=d_p.data_ptr(),
                          chr=d_c.data_ptr(), next_id=d_n.data_ptr(), rows_src=d_rs.data_ptr(), rows_dst=d_rd.data_ptr(),
                          len_src=d_ls.data_ptr(), len_dst=d_ld.data_ptr(), ids=d_ids.data_ptr(), n_beams=d_nb.data_ptr(),
                          N=N, W=W, L=L, H=H, max_len=ML), stream())
    torch.cuda.synchronize()
    # expected: a copy (tolerance 0)
    e_hd = [h.copy() for h in hd]
    e_rd, e_ld, e_ids, e_nb = rows_d.copy(), len_d.copy(), ids.copy(), nb.copy()
    for n in range(N):
        for k in range(W):
            r, p = n * W + k, int(parent[n * W + k])
            if p < 0:
                for l in range(L):
                    e_hd[l][r] = 0
                e_rd[r], e_ld[r] = 0, 0
            else:
                for l in range(L):
                    e_hd[l][r] = hs[l][n * W + p]
                e_rd[r], e_ld[r] = rows_s[n * W + p], len_s[n * W + p]
                if chrs[r] >= 0:
                    e_rd[r, e_ld[r]] = chrs[r]
                    e_ld[r] += 1
            e_ids[r] = nxt[r]
        e_nb[n] = int((parent[n * W:(n + 1) * W] >= 0).sum())
    for l in range(L):
        assert np.array_equal(d_hd[l].cpu().numpy().view(np.uint32), e_hd[l].view(np.uint32))
        assert np.array_equal(d_hs[l].cpu().numpy().view(np.uint32), hs[l].view(np.uint32))      # the source slot: unchanged
    assert np.array_equal(d_rd.cpu().numpy(), e_rd) and np.array_equal(d_rs.cpu().numpy(), rows_s)
    assert np.array_equal(d_ld.cpu().numpy(), e_ld) and np.array_equal(d_ls.cpu().numpy(), len_s)
    assert np.array_equal(d_ids.cpu().numpy(), e_ids) and np.array_equal(d_nb.cpu().numpy(), e_nb)


def test_reorder_refuses_an_in_place_gather(ext):
    z = torch.zeros(4096, device=DEV)
    zi = torch.zeros(4096, dtype=torch.int32, device=DEV)
    a = dict(h_src=[z.data_ptr()], h_dst=[z.data_ptr()], parent=zi.data_ptr(), chr=zi.data_ptr(), next_id=zi.data_ptr(),
             rows_src=zi.data_ptr(), rows_dst=zi.data_ptr() + 4096, len_src=zi.data_ptr(), len_dst=zi.data_ptr() + 8192,
             ids=zi.data_ptr(), n_beams=zi.data_ptr(), N=1, W=2, L=1, H=64, max_len=4)
    with pytest.raises(RuntimeError):
        ext.beam_reorder(a, stream())


def test_reset_state_before_step_zero(ext):
    N, W, L, Bp, H, ML, sos = 5, 3, 2, 64, 64, 6, 9
    h = [torch.full((Bp, H), 3.0, device=DEV) for _ in range(L)]
    ids = torch.full((Bp,), -1, dtype=torch.int32, device=DEV)
    sc = torch.full((Bp,), 7.0, device=DEV)
    st = torch.full((Bp,), -1, dtype=torch.int32, device=DEV)
    ln = torch.full((Bp,), -1, dtype=torch.int32, device=DEV)
    rows = torch.full((Bp + 1, ML + 1), 9, dtype=torch.uint8, device=DEV)
    ext.beam_reset(dict(h=[x.data_ptr() for x in h], ids=ids.data_ptr(), score=sc.data_ptr(), state=st.data_ptr(),
                        len=ln.data_ptr(), rows=rows.data_ptr(), N=N, W=W, L=L, Bp=Bp, H=H, max_len=ML, sos=sos), stream())
    torch.cuda.synchronize()
    first = (np.arange(Bp) < N * W) & (np.arange(Bp) % W == 0)
    assert all((x == 0).all().item() for x in h) and (ids == sos).all().item() and (ln == 0).all().item()
    assert np.array_equal(st.cpu().numpy(), np.where(first, br.LIVE, br.DEAD))
    assert np.array_equal(sc.cpu().numpy(), np.where(first, 0.0, -np.inf).astype(np.float32))
    r = rows.cpu().numpy()
    assert (r[:Bp] == 0).all() and (r[Bp] == 9).all()


# ------------------------------------------------------------------------------- the whole search
_gens = {}


def gen_of(c, precision="fp32", max_batch=4096):
    """One generator per model and precision, shared by the tests (its beam graphs and arena with it)."""
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    cfg, p = br.case_model(c)
    key = (c.V, c.E, c.H, c.L, c.ML, c.eos, c.seed, c.sharp, precision, max_batch)
    if key not in _gens:
        _gens[key] = HipGenerator(cfg, p, precision=precision, max_batch=max_batch)
    return _gens[key]


def check_case(c, got):
    cfg, p = br.case_model(c)
    orc = br.case_oracle(c)
    s64 = br.score64_of(p, cfg, got)
    nb = [int(x) for x in got.n_beams]
    dev = max(float(np.abs(got.logp[n, :nb[n]].astype(np.float64) - s64[n, :nb[n]]).max()) for n in range(len(nb)))
    print(f"{c.name}: settled {int(orc['settled'].sum())} of {len(nb)}, logp vs fp64 score of the rows {dev:.3e} (atol {br.ATOL['logp']:.3e})")
    assert br.check_result(cfg, c.prefixes, orc, got, s64) == []


@pytest.mark.parametrize("c", [c for c in br.TRAJ_CASES if c.name != "m-batches"], ids=lambda c: c.name)
def test_beam_search_matches_fp64_oracle(c):
    got = gen_of(c).beam_search(list(c.prefixes), width=c.W)
    assert got.rows.shape == (len(c.prefixes), c.W, c.ML + 1) and got.logp.dtype == np.float32
    check_case(c, got)


def test_beam_search_single_kinds_of_prefix():
    """Empty, short and full-length prefixes each in a call of their own (and the None / str forms)."""
    c = next(x for x in br.TRAJ_CASES if x.name == "s-L2-ML6-e5-W8")
    cfg, p = br.case_model(c)
    g = gen_of(c)
    for pre in (None, "0", "012345"):
        got = g.beam_search(pre, width=c.W)
        lst = [""] if pre is None else [pre]
        orc = br.oracle(p, cfg, lst, c.W)
        assert br.check_result(cfg, lst, orc, got, br.score64_of(p, cfg, got)) == []
    got = g.beam_search("012345", width=c.W)      # nothing free: one beam, the prefix itself
    assert got.n_beams[0] == 1 and bytes(got.rows[0, 0, :6]) == b"012345"
    assert g.beam_search(None, width=2, count=3).rows.shape == (3, 2, cfg.max_len + 1)


def test_beam_search_split_into_batches():
    c = next(x for x in br.TRAJ_CASES if x.name == "m-batches")
    g = gen_of(c, max_batch=64)      # 8 names of 8 beams per batch: 20 prefixes = 8 + 8 + 4
    check_case(c, g.beam_search(list(c.prefixes), width=c.W))
    assert g.g.beam_graphs() == 2
    with pytest.raises(RuntimeError):
        from gru_mpi_cuda_amd.engine.generator import HipGenerator
        cfg, p = br.case_model(c)
        HipGenerator(cfg, p, max_batch=16).beam_search("", width=32)      # max_batch < width


# ------------------------------------------------------------------------------- relations
def test_relations_to_generate_and_score():
    c = next(x for x in br.TRAJ_CASES if x.name == "m-W8")
    cfg, p = br.case_model(c)
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    from gru_mpi_cuda_amd.utils.data import random_floats
    g = HipGenerator(cfg, p)      # a fresh one: nothing searched yet
    assert g.g.beam_workspace_bytes() == 0
    pre = list(c.prefixes)
    N = len(pre)
    rf = random_floats(N, cfg.max_len, 5)
    before = (g.generate(rf), g.generate(rf, temperature=0.0, prefix=pre), g.generate(rf, temperature=0.7, top_k=5, prefix=pre))
    sc_before = g.score(before[0])
    w8 = g.beam_search(pre, width=8)
    w1 = g.beam_search(pre, width=1)
    assert g.g.beam_workspace_bytes() > 0
    after = (g.generate(rf), g.generate(rf, temperature=0.0, prefix=pre), g.generate(rf, temperature=0.7, top_k=5, prefix=pre))
    sc_after = g.score(before[0])
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert np.array_equal(sc_before.tok_logp.view(np.uint32), sc_after.tok_logp.view(np.uint32))
    assert np.array_equal(sc_before.rank, sc_after.rank)
    # W = 1 is the greedy chain; beam 0 of W = 8 is at least as probable (settled prefixes)
    o1, o8 = br.oracle(p, cfg, pre, 1), br.case_oracle(c)
    greedy = before[1]
    g_logp = g.score(greedy).name_logp
    for n in range(N):
        if o1["settled"][n]:
            assert np.array_equal(w1.rows[n, 0], greedy[n]), n
        if o8["settled"][n] and o1["settled"][n]:
            assert w8.logp[n, 0] >= g_logp[n] - br.ATOL["logp"], n
    # the path is exact fp32 whatever the generator samples with
    gb = HipGenerator(cfg, p, precision="bf16")
    b8 = gb.beam_search(pre, width=8)
    assert np.array_equal(b8.rows, w8.rows) and np.array_equal(b8.logp.view(np.uint32), w8.logp.view(np.uint32))
    assert np.array_equal(b8.n_tok, w8.n_tok) and np.array_equal(b8.n_beams, w8.n_beams)


# ------------------------------------------------------------------------------- graph reuse
def test_graph_reuse_reads_prefixes_from_memory():
    c = next(x for x in br.TRAJ_CASES if x.name == "s-L2-ML6-e5-W3")
    cfg, p = br.case_model(c)
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    g = HipGenerator(cfg, p)
    a_pre = list(c.prefixes)
    b_pre = [s[::-1] for s in a_pre[1:]] + ["!"]      # the same count, other prefixes
    a1 = g.beam_search(a_pre, width=3)
    assert g.g.beam_graphs() == 1
    b1 = g.beam_search(b_pre, width=3)
    a2 = g.beam_search(a_pre, width=3)
    assert g.g.beam_graphs() == 1      # one recording served all three
    for pre, got in ((a_pre, a1), (b_pre, b1)):
        orc = br.oracle(p, cfg, pre, 3)
        assert br.check_result(cfg, pre, orc, got, br.score64_of(p, cfg, got)) == []
    for k in ("rows", "n_tok", "n_beams"):
        assert np.array_equal(getattr(a1, k), getattr(a2, k)), k
    assert np.array_equal(a1.logp.view(np.uint32), a2.logp.view(np.uint32))
    g.beam_search(a_pre, width=8)
    assert g.g.beam_graphs() == 2      # a second width records a second graph


# ------------------------------------------------------------------------------- errors
def test_errors_raise_before_any_launch():
    c = next(x for x in br.TRAJ_CASES if x.name == "s-L1-ML3-e5-W3")
    cfg, p = br.case_model(c)
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    g = HipGenerator(cfg, p)
    for kw in (dict(width=0), dict(width=33), dict(prefix="0" + chr(cfg.eos)), dict(prefix="0123")):
        with pytest.raises(ValueError):
            g.beam_search(**kw)
    from gru_mpi_cuda_amd.config import GRUConfig
    from gru_mpi_cuda_amd.models.params import init_params
    with pytest.raises(ValueError):      # width > vocab needs a vocabulary below 32: never a device model (vocab % 64)
        cpu_ref.beam_inputs(GRUConfig(vocab=16, embed=64, hidden=64, layers=1, max_len=3), None, 17)
    long_cfg = GRUConfig(vocab=64, embed=64, hidden=64, layers=1, max_len=65, sos=0, eos=5, seed=4)
    with pytest.raises(ValueError):
        HipGenerator(long_cfg, init_params(long_cfg)).beam_search("")
    assert g.g.beam_workspace_bytes() == 0 and g.g.beam_graphs() == 0      # nothing was launched
    assert g.g.read_error() == 0

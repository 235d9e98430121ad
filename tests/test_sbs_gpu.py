"""Stochastic beam search on the device (csrc/kernels/sbs.hip, Generator::distinct) against the float64
rule of models/sbs_ref.py: the selection kernel on planted inputs, the whole search against the oracle,
its relation to score, batching, graph reuse, the neighbours it must not disturb and the errors."""
import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models import sbs_ref as sr

pytestmark = pytest.mark.gpu

DEV = "cuda"
CANARY = 3      # rows past the launch's own in every output


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------- sbs_select_f32
def run_select(ext, d, optional=True, prefix=None):
    """One launch on the planted inputs ``d``.  Outputs start NaN / -77 filled with CANARY extra rows;
    returns them whole plus the error words."""
    R, V, W, N = d["R"], d["V"], d["W"], d["N"]
    lg, lq_in, G_in, st = t(d["logits"]), t(d["logq"]), t(d["G"]), t(d["state"])
    pl, pre, inv = t(d["plen"]), t(d["prefix"] if prefix is None else prefix), t(d["inv_t"])
    words = t(np.array([d["seed"], d["start"]], np.uint64).view(np.int64))
    fo = {k: torch.full((R + CANARY,), float("nan"), device=DEV) for k in ("logq_out", "G_out", "zmax")}
    io = {k: torch.full((R + CANARY,), -77, dtype=torch.int32, device=DEV)
          for k in ("parent", "chr", "state_out", "next_id", "sel", "allow_state_out")}
    lq = torch.full((R + CANARY, V), float("nan"), device=DEV)
    gt = torch.full((R + CANARY, V), float("nan"), device=DEV)
    err = torch.zeros(4, dtype=torch.int32, device=DEV)
    a = dict(logits=lg.data_ptr(), splits=d["splits"], slab=d["Rp"] * V, logq_in=lq_in.data_ptr(), G_in=G_in.data_ptr(),
             state_in=st.data_ptr(), plen=pl.data_ptr(), prefix=pre.data_ptr(), seed=words.data_ptr(),
             start=words.data_ptr() + 8, inv_t=inv.data_ptr(), err=err.data_ptr(),
             N=N, W=W, V=V, step=d["step"], max_len=d["ML"], sos=d["sos"], eos=d["eos"],
             **{k: fo[k].data_ptr() for k in ("logq_out", "G_out")},
             **{k: io[k].data_ptr() for k in ("parent", "chr", "state_out", "next_id")})
    if optional:
        a.update(lq=lq.data_ptr(), gt=gt.data_ptr(), zmax=fo["zmax"].data_ptr(), sel=io["sel"].data_ptr())
    keep = [lg, lq_in, G_in, st, pl, pre, inv, words]
    if d["bias"] is not None:
        keep.append(t(d["bias"]))
        a["bias"] = keep[-1].data_ptr()
    if d["tab"] is not None:
        keep.append(t(d["tab"].view(np.int32)))
        a.update(allow_tab=keep[-1].data_ptr(), allow_rows=sr.LINES)
        if d["idx"] is not None:
            keep.append(t(d["idx"]))
            a["allow_idx"] = keep[-1].data_ptr()
        else:
            keep += [t(d["astate"]), t(d["nxt"].view(np.int16))]
            a.update(allow_state_in=keep[-2].data_ptr(), allow_next=keep[-1].data_ptr(),
                     allow_state_out=io["allow_state_out"].data_ptr())
    ext.sbs_select(a, stream())
    torch.cuda.synchronize()
    return dict(logq=fo["logq_out"].cpu().numpy(), G=fo["G_out"].cpu().numpy(), zmax=fo["zmax"].cpu().numpy(),
                parent=io["parent"].cpu().numpy(), chr=io["chr"].cpu().numpy(), state=io["state_out"].cpu().numpy(),
                next_id=io["next_id"].cpu().numpy(), sel=io["sel"].cpu().numpy(), astate=io["allow_state_out"].cpu().numpy(),
                lq=lq.cpu().numpy(), gt=gt.cpu().numpy(), err=err.cpu().numpy(), logits_after=lg.cpu().numpy())


def own_rows(d, got, optional=True):
    R = d["R"]
    own = {k: (v[:R] if k not in ("err", "logits_after") else v) for k, v in got.items()}
    if not optional:
        for k in ("lq", "gt", "zmax", "sel"):
            own[k] = None
    if d["astate"] is None:
        own["astate"] = None
    return own


@pytest.mark.parametrize("i", range(len(sr.STEP_CASES)), ids=lambda i: "-".join(map(str, sr.STEP_CASES[i])))
def test_select_matches_fp64_rule(ext, i):
    c = sr.STEP_CASES[i]
    d = sr.settled_inputs(c, seed=i % 3)
    ref = sr.select_ref(d)
    got = run_select(ext, d, c.optional)
    own = own_rows(d, got, c.optional)
    R = d["R"]
    fin = np.isfinite(ref["logq"])
    print(f"{c}: logq deviation {sr._dev(own['logq'][fin], ref['logq'][fin]):.3e} (atol {sr.ATOL['logq']:.3e}), "
          f"G {sr._dev(own['G'], ref['G'], ref['wscale']):.3e} (atol {sr.ATOL['Gt']:.3e})",
          "" if not c.optional else f"lq {sr._dev(own['lq'], ref['lq']):.3e} (atol {sr.ATOL['lq']:.3e}), "
          f"gt {sr._dev(own['gt'], ref['gt'], ref['scale']):.3e}, zmax {sr._dev(own['zmax'], ref['zmax']):.3e}")
    assert sr.check_step(d, ref, own) == []
    assert (got["err"] == 0).all()
    # canary rows and the optional outputs that were not asked for: bitwise untouched
    for k in ("logq", "G", "zmax"):
        assert np.isnan(got[k][R:]).all(), k
    assert np.isnan(got["lq"][R:]).all() and np.isnan(got["gt"][R:]).all()
    for k in ("parent", "chr", "state", "next_id", "sel", "astate"):
        assert (got[k][R:] == -77).all(), k
    if not c.optional:
        assert np.isnan(got["lq"]).all() and np.isnan(got["gt"]).all() and np.isnan(got["zmax"]).all()
        assert (got["sel"] == -77).all()
    if d["astate"] is None:
        assert (got["astate"] == -77).all()
    # the logits (their NaN pad rows included) were neither changed nor read into a result
    assert np.array_equal(got["logits_after"], d["logits"], equal_nan=True)
    # two launches: identical bytes
    again = run_select(ext, d, c.optional)
    for k in ("logq", "G", "zmax", "lq", "gt"):
        assert np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)), k
    for k in ("parent", "chr", "state", "next_id", "sel", "astate"):
        assert np.array_equal(got[k], again[k]), k


def test_select_covers_every_branch_of_the_case_table():
    cs = sr.STEP_CASES
    assert {c.V for c in cs} == {64, 256, 512} and {c.W for c in cs} == {1, 4, 16, 17, 32} and {c.N for c in cs} == {1, 3}
    assert {c.splits for c in cs} == {1, 2} and {c.bias for c in cs} == {True, False}
    assert {c.mask for c in cs} == {"none", "pos", "auto"} and {c.mode for c in cs} == {"free", "forced", "mixed"}
    assert {c.states for c in cs} == {"mix", "live", "fin", "step0"} and {c.big for c in cs} == {True, False}
    assert sum(not c.optional for c in cs) * 4 >= len(cs) - 3


def test_select_flags_prefix_byte_outside_vocab(ext):
    c = sr.StepCase(64, 4, 3, 1, False, "forced", "live", "none", 5, True, True)
    d = sr.step_inputs(c, 1)
    pre = d["prefix"].copy()
    pre[1, d["step"]] = 200
    got = run_select(ext, d, prefix=pre)
    assert got["err"][0] == 16 and got["err"][1] == 200 and got["err"][2] == 1 * c.W and got["err"][3] == 0
    pre0 = pre.copy()
    pre0[1, d["step"]] = 0      # the byte is taken as 0
    d0 = dict(d, prefix=pre0)
    assert sr.check_step(d0, sr.select_ref(d0), own_rows(d, got)) == []


def test_select_rejects_unsupported_shapes(ext):
    z = torch.zeros(8192, device=DEV)
    zi = torch.zeros(8192, dtype=torch.int32, device=DEV)
    base = dict(logits=z.data_ptr(), logq_in=z.data_ptr(), G_in=z.data_ptr() + 512, state_in=zi.data_ptr(), plen=zi.data_ptr(),
                prefix=zi.data_ptr(), seed=zi.data_ptr(), start=zi.data_ptr() + 8, inv_t=z.data_ptr(),
                logq_out=z.data_ptr() + 2048, G_out=z.data_ptr() + 4096, parent=zi.data_ptr() + 1024, chr=zi.data_ptr() + 2048,
                state_out=zi.data_ptr() + 4096, next_id=zi.data_ptr() + 8192, N=1, W=2, V=64, step=0, max_len=4, sos=1, eos=0)
    for bad in (dict(V=96), dict(V=576), dict(W=0), dict(W=33), dict(V=64, W=65), dict(step=4), dict(seed=0), dict(inv_t=0),
                dict(G_out=z.data_ptr() + 512)):
        with pytest.raises(RuntimeError):
            ext.sbs_select(dict(base, **bad), stream())


# ------------------------------------------------------------------------------- the whole search
_gens = {}


def gen_of(c, precision="fp32", max_batch=4096):
    """One generator per model and precision, shared by the tests (its graphs and arena with it)."""
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    cfg, p = sr.case_model(c)
    key = (c.preset, c.V, c.E, c.H, c.L, c.ML, c.eos, c.seed, precision, max_batch)
    if key not in _gens:
        _gens[key] = HipGenerator(cfg, p, precision=precision, max_batch=max_batch)
    return _gens[key]


def case(name):
    return next(c for c in sr.TRAJ_CASES if c.name == name)


def run_case(g, c):
    return g.sample_distinct(list(c.prefixes), width=c.W, **sr.case_kwargs(c))


def same_bytes(a, b):
    return (np.array_equal(a.rows, b.rows) and np.array_equal(a.logq.view(np.uint32), b.logq.view(np.uint32))
            and np.array_equal(a.gumbel.view(np.uint32), b.gumbel.view(np.uint32)) and np.array_equal(a.n_tok, b.n_tok)
            and np.array_equal(a.n_found, b.n_found))


def check_case(c, got, g=None):
    cfg, p = sr.case_model(c)
    orc = sr.case_oracle(c)
    s64 = sr.score64_of(p, cfg, c.prefixes, got, c.temperature, c.constraints)
    nf = [int(x) for x in got.n_found]
    dev = max(float(np.abs(got.logq[n, :nf[n]].astype(np.float64) - s64[n, :nf[n]]).max()) for n in range(len(nf)))
    print(f"{c.name}: settled {int(orc['settled'].sum())} of {len(nf)}, logq vs fp64 score of the rows {dev:.3e} "
          f"(atol {sr.ATOL['logq']:.3e})")
    assert sr.check_result(cfg, c.prefixes, orc, got, s64) == []
    if g is not None:      # the device's own score of the rows, under the same keywords
        for n in range(len(nf)):
            k = nf[n]
            sc = g.score(got.rows[n, :k], temperature=1.0 if c.temperature is None else c.temperature,
                         prefix=[c.prefixes[n]] * k, constraints=None if c.constraints is None else dict(c.constraints))
            assert np.abs(sc.name_logp.astype(np.float64) - got.logq[n, :k]).max() <= sr.ATOL["logq"], (c.name, n)


@pytest.mark.parametrize("c", sr.TRAJ_CASES, ids=lambda c: c.name)
def test_sample_distinct_matches_fp64_oracle(c):
    g = gen_of(c)
    got = run_case(g, c)
    cfg, _ = sr.case_model(c)
    assert got.rows.shape == (len(c.prefixes), c.W, cfg.max_len + 1) and got.logq.dtype == np.float32
    check_case(c, got, g)


def test_a_language_of_three_names_leaves_one_dead_slot():
    c = case("regex3")
    got = run_case(gen_of(c), c)
    assert (got.n_found == 3).all()
    assert np.isneginf(got.logq[:, 3]).all() and np.isneginf(got.gumbel[:, 3]).all()
    assert np.abs(np.exp(got.logq[:, :3].astype(np.float64)).sum(1) - 1).max() <= sr.ATOL["logq"]
    for names in got.names():
        assert sorted(names) == ["ab", "ac", "ad"]


@pytest.mark.parametrize("name,max_batch", [("h64-L1-n9-W4", 20), ("h64-L1-n9-W4", 12), ("h128-L2-n9-W17", 85)])
def test_batches_do_not_change_the_bytes(name, max_batch):
    """max_batch = 20 / 12 at W = 4: 5 + 4 and 3 + 3 + 3 names; 85 at W = 17: 5 + 4."""
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    c = case(name)
    cfg, p = sr.case_model(c)
    one = run_case(gen_of(c), c)
    cut = run_case(HipGenerator(cfg, p, max_batch=max_batch), c)
    assert same_bytes(one, cut)


def test_start_shifts_the_names_and_seeds_replay_one_recording():
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    c = case("h64-L1-n9-W4")
    cfg, p = sr.case_model(c)
    g = HipGenerator(cfg, p)
    pre = [""] * 9
    whole = g.sample_distinct(pre, width=4, seed=3, start=2 ** 33)
    assert g.g.distinct_graphs() == 1 and g.g.beam_graphs() == 0
    part = g.sample_distinct(pre[:4], width=4, seed=3, start=2 ** 33 + 5)
    assert np.array_equal(part.rows, whole.rows[5:]) and np.array_equal(part.logq.view(np.uint32), whole.logq[5:].view(np.uint32))
    assert np.array_equal(part.gumbel.view(np.uint32), whole.gumbel[5:].view(np.uint32))
    n = g.g.distinct_graphs()
    other = g.sample_distinct(pre, width=4, seed=4, start=2 ** 33, temperature=0.7)
    assert g.g.distinct_graphs() == n and g.g.beam_graphs() == 0      # a seed and a temperature are read from memory
    assert not np.array_equal(other.rows, whole.rows)
    orc = sr.oracle(p, cfg, pre, 4, seed=4, start=2 ** 33, temperature=0.7)
    assert sr.check_result(cfg, pre, orc, other, sr.score64_of(p, cfg, pre, other, 0.7)) == []
    assert same_bytes(whole, g.sample_distinct(pre, width=4, seed=3, start=2 ** 33))


def test_neighbours_are_not_disturbed():
    """beam_search and generate before and after a sample_distinct call: the bytes of a fresh generator."""
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    from gru_mpi_cuda_amd.utils.data import random_floats
    c = case("h128-L2-n3-W4")
    cfg, p = sr.case_model(c)
    pre = list(c.prefixes)
    rf = random_floats(len(pre), cfg.max_len, 5)
    fresh = HipGenerator(cfg, p)
    want_b, want_g = fresh.beam_search(pre, width=4), fresh.generate(rf, temperature=0.8, prefix=pre)
    ws, bg = fresh.g.beam_workspace_bytes(), fresh.g.beam_graphs()
    g = HipGenerator(cfg, p)
    for rnd in range(2):
        b, s = g.beam_search(pre, width=4), g.generate(rf, temperature=0.8, prefix=pre)
        assert np.array_equal(b.rows, want_b.rows) and np.array_equal(b.logp.view(np.uint32), want_b.logp.view(np.uint32))
        assert np.array_equal(b.n_tok, want_b.n_tok) and np.array_equal(b.n_beams, want_b.n_beams)
        assert np.array_equal(s, want_g)
        assert g.g.beam_workspace_bytes() == ws and g.g.beam_graphs() == bg
        if rnd == 0:
            check_case(c, run_case(g, c))
            assert g.g.distinct_graphs() == 1


def test_exact_fp32_whatever_the_generator_samples_with():
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    c = case("h64-L1-n3-W4")
    cfg, p = sr.case_model(c)
    assert same_bytes(run_case(gen_of(c), c), run_case(HipGenerator(cfg, p, precision="bf16x3"), c))


def test_errors_raise_before_any_launch():
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    c = case("h64-L1-n3-W4")
    cfg, p = sr.case_model(c)
    g = HipGenerator(cfg, p)
    for kw in (dict(width=0), dict(width=33), dict(prefix="0" + chr(cfg.eos)), dict(temperature=0), dict(temperature=-1.0),
               dict(temperature=float("nan")), dict(top_k=5), dict(top_p=0.9), dict(logit_bias={"a": 1.0}),
               dict(presence_penalty=0.5), dict(frequency_penalty=0.5), dict(seed=-1), dict(start=2 ** 64),
               dict(prefix="0", constraints=dict(charset="abc"))):
        with pytest.raises(ValueError):
            g.sample_distinct(**kw)
    with pytest.raises(ValueError):
        HipGenerator(cfg, p, precision="bf16").sample_distinct("")
    assert g.g.beam_workspace_bytes() == 0 and g.g.distinct_graphs() == 0      # nothing was launched
    assert g.g.read_error() == 0

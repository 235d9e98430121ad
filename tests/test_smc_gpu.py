"""Sequential Monte Carlo on the device (csrc/kernels/smc.hip, Generator::conditional) against the float64
rule of models/smc_ref.py: the selection kernel on planted inputs, whole trajectories against the oracle,
their relation to score, batching, runs, graph reuse, the law of the estimate, the neighbours it must not
disturb and the errors."""
import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models import smc_ref as sr

pytestmark = pytest.mark.gpu

DEV = "cuda"
CANARY = 3      # rows past the launch's own in every output
FLOATS = ("logw_out", "logq_out", "logm")
INTS = ("parent", "chr", "state_out", "next_id", "allow_state_out")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------- smc_select_f32
def run_select(ext, d, optional=True, prefix=None, thr=None):
    """One launch on the planted inputs ``d``.  Outputs start NaN / -77 filled with CANARY extra rows (names);
    returns them whole plus the error words."""
    R, V, W, N = d["R"], d["V"], d["W"], d["N"]
    lg, lw_in, lq_in, st = t(d["logits"]), t(d["logw"]), t(d["logq"]), t(d["state"])
    pl, pre, inv = t(d["plen"]), t(d["prefix"] if prefix is None else prefix), t(d["inv_t"])
    words = t(np.array([d["seed"], d["start"]], np.uint64).view(np.int64))
    th = t(np.array([d["thr"] if thr is None else thr], np.float32))
    fo = {k: torch.full((R + CANARY,), float("nan"), device=DEV) for k in FLOATS}
    io = {k: torch.full((R + CANARY,), -77, dtype=torch.int32, device=DEV) for k in INTS}
    ess = torch.full((N + CANARY,), float("nan"), device=DEV)
    nres = torch.full((N + CANARY,), 5 if d["step"] > 0 else -77, dtype=torch.int32, device=DEV)
    lq = torch.full((R + CANARY, V), float("nan"), device=DEV)
    err = torch.zeros(4, dtype=torch.int32, device=DEV)
    a = dict(logits=lg.data_ptr(), splits=d["splits"], slab=d["Rp"] * V, logw_in=lw_in.data_ptr(), logq_in=lq_in.data_ptr(),
             state_in=st.data_ptr(), plen=pl.data_ptr(), prefix=pre.data_ptr(), seed=words.data_ptr(),
             start=words.data_ptr() + 8, thr=th.data_ptr(), inv_t=inv.data_ptr(), err=err.data_ptr(), n_res=nres.data_ptr(),
             N=N, W=W, V=V, step=d["step"], max_len=d["ML"], sos=d["sos"], eos=d["eos"],
             **{k: fo[k].data_ptr() for k in ("logw_out", "logq_out")},
             **{k: io[k].data_ptr() for k in ("parent", "chr", "state_out", "next_id")})
    if optional:
        a.update(lq=lq.data_ptr(), logm=fo["logm"].data_ptr(), ess=ess.data_ptr())
    keep = [lg, lw_in, lq_in, st, pl, pre, inv, words, th]
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
    ext.smc_select(a, stream())
    torch.cuda.synchronize()
    nr = nres.cpu().numpy()
    return dict(logw=fo["logw_out"].cpu().numpy(), logq=fo["logq_out"].cpu().numpy(), logm=fo["logm"].cpu().numpy(),
                parent=io["parent"].cpu().numpy(), chr=io["chr"].cpu().numpy(), state=io["state_out"].cpu().numpy(),
                next_id=io["next_id"].cpu().numpy(), astate=io["allow_state_out"].cpu().numpy(), ess=ess.cpu().numpy(),
                n_res=nr, lq=lq.cpu().numpy(), err=err.cpu().numpy(), logits_after=lg.cpu().numpy())


def own_rows(d, got, optional=True):
    R, N = d["R"], d["N"]
    own = {k: v[:R] for k, v in got.items() if k not in ("err", "logits_after", "ess", "n_res")}
    own["ess"] = got["ess"][:N]
    own["resampled"] = (got["n_res"][:N] - (5 if d["step"] > 0 else 0)) != 0     # a later step adds to what was there
    if not optional:
        for k in ("lq", "logm", "ess"):
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
    R, N = d["R"], d["N"]
    print(f"{c}: logw deviation {sr._dev(own['logw'], ref['logw']):.3e} (atol {sr.ATOL['logw']:.3e}), "
          f"logq {sr._dev(own['logq'], ref['logq']):.3e} (atol {sr.ATOL['logq']:.3e})",
          "" if not c.optional else f"logm {sr._dev(own['logm'], ref['logm']):.3e} (atol {sr.ATOL['logm']:.3e}), "
          f"ess / W {sr._dev(own['ess'].astype(np.float64) / c.W, ref['q_ess']):.3e} (atol {sr.ATOL['decide']:.3e})")
    assert sr.check_step(d, ref, own) == []
    assert (got["err"] == 0).all()
    assert set((got["n_res"][:N] - (5 if d["step"] > 0 else 0)).tolist()) <= {0, 1}
    # canary rows and the optional outputs that were not asked for: bitwise untouched
    for k in ("logw", "logq", "logm"):
        assert np.isnan(got[k][R:]).all(), k
    assert np.isnan(got["lq"][R:]).all() and np.isnan(got["ess"][N:]).all()
    assert (got["n_res"][N:] == (5 if d["step"] > 0 else -77)).all()
    for k in ("parent", "chr", "state", "next_id", "astate"):
        assert (got[k][R:] == -77).all(), k
    if not c.optional:
        assert np.isnan(got["lq"]).all() and np.isnan(got["logm"]).all() and np.isnan(got["ess"]).all()
    if d["astate"] is None:
        assert (got["astate"] == -77).all()
    # the logits (their NaN pad rows included) were neither changed nor read into a result
    assert np.array_equal(got["logits_after"], d["logits"], equal_nan=True)
    # two launches: identical bytes
    again = run_select(ext, d, c.optional)
    for k in ("logw", "logq", "logm", "lq", "ess"):
        assert np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)), k
    for k in ("parent", "chr", "state", "next_id", "astate", "n_res"):
        assert np.array_equal(got[k], again[k]), k


def test_select_covers_every_branch_of_the_case_table():
    cs = sr.STEP_CASES
    assert {c.V for c in cs} == {64, 256, 512} and {c.W for c in cs} == {1, 2, 4, 16, 17, 32} and {c.N for c in cs} == {1, 2, 3}
    assert {c.splits for c in cs} == {1, 2} and {c.bias for c in cs} == {True, False}
    assert {c.mask for c in cs} == {"none", "pos", "auto"} and {c.mode for c in cs} == {"free", "forced", "mixed"}
    assert {c.states for c in cs} == {"mix", "live", "fin", "step0"} and {c.big for c in cs} == {True, False}
    assert {c.thr for c in cs} == {0.0, 0.5, 1.0} and {c.weights for c in cs} == {"rand", "last"}
    assert {c.mask for c in cs if c.single} == {"pos", "auto"}
    assert sum(not c.optional for c in cs) * 5 >= len(cs) - 20
    # what the table is there to reach, read from the float64 rule: a step that resamples and one that does not on
    # the same inputs, carried slots, a forced step, the fan-out, the last slot as every ancestor, a row of one char
    res = {}
    seen = set()
    for i, c in enumerate(cs):
        d = sr.settled_inputs(c, seed=i % 3)
        ref = sr.select_ref(d)
        if c.weights == "rand" and c.states == "live" and c.mode == "free" and not c.single and c.thr in (0.0, 1.0):
            res.setdefault((c.V, c.W, c.mask, c.N), {})[c.thr] = bool(np.asarray(ref["resampled"]).all())
        par, ch = ref["parent"].reshape(c.N, c.W), ref["chr"].reshape(c.N, c.W)
        if ((par >= 0) & (ch < 0)).any():
            seen.add("carried")
        if c.mode == "forced" and (ch >= 0).any():
            seen.add("forced")
        if c.states == "step0" and c.W > 1 and (par == 0).all():
            seen.add("fanout")
        if c.weights == "last" and c.thr == 1.0 and c.W > 1 and (par == c.W - 1).all() and np.asarray(ref["resampled"]).all():
            seen.add("last")
        if c.single and (np.isfinite(ref["lq"]).sum(1) == 1).any():
            seen.add("single")
        if c.W == 17 and np.asarray(ref["resampled"]).any() and (par >= 16).any():
            seen.add("second row of a wave")
    pairs = [v for v in res.values() if 0.0 in v and 1.0 in v]
    assert len(pairs) >= 4 and all(v[1.0] and not v[0.0] for v in pairs)
    assert seen == {"carried", "forced", "fanout", "last", "single", "second row of a wave"}, seen


def test_select_flags_prefix_byte_outside_vocab(ext):
    c = sr.StepCase(64, 4, 3, 1, False, "forced", "live", "none", 5, True)
    d = sr.step_inputs(c, 1)
    pre = d["prefix"].copy()
    pre[1, d["step"]] = 200
    got = run_select(ext, d, prefix=pre)
    assert got["err"][0] == 16 and got["err"][1] == 200 and got["err"][2] == 1 * c.W and got["err"][3] == 0
    R = d["R"]
    assert np.isnan(got["logw"][R:]).all() and np.isnan(got["logq"][R:]).all() and (got["chr"][R:] == -77).all()
    assert (got["parent"][R:] == -77).all() and (got["n_res"][d["N"]:] == 5).all()
    pre0 = pre.copy()
    pre0[1, d["step"]] = 0      # the byte is taken as 0
    d0 = dict(d, prefix=pre0)
    assert sr.check_step(d0, sr.select_ref(d0), own_rows(d, got)) == []


def test_select_rejects_unsupported_shapes(ext):
    z = torch.zeros(8192, device=DEV)
    zi = torch.zeros(8192, dtype=torch.int32, device=DEV)
    base = dict(logits=z.data_ptr(), logw_in=z.data_ptr(), logq_in=z.data_ptr() + 512, state_in=zi.data_ptr(), plen=zi.data_ptr(),
                prefix=zi.data_ptr(), seed=zi.data_ptr(), start=zi.data_ptr() + 8, thr=z.data_ptr(), inv_t=z.data_ptr(),
                logw_out=z.data_ptr() + 2048, logq_out=z.data_ptr() + 4096, parent=zi.data_ptr() + 1024, chr=zi.data_ptr() + 2048,
                state_out=zi.data_ptr() + 4096, next_id=zi.data_ptr() + 8192, N=1, W=2, V=64, step=0, max_len=4, sos=1, eos=0)
    for bad in (dict(V=96), dict(V=576), dict(W=0), dict(W=33), dict(V=64, W=65), dict(step=4), dict(seed=0), dict(inv_t=0),
                dict(thr=0), dict(logq_out=z.data_ptr() + 512)):
        with pytest.raises(RuntimeError):
            ext.smc_select(dict(base, **bad), stream())


# ------------------------------------------------------------------------------- whole trajectories
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


def run_case(g, c, **over):
    return g.sample_conditional(list(c.prefixes), width=c.W, **dict(sr.case_kwargs(c), **over))


def same_bytes(a, b):
    return (np.array_equal(a.rows, b.rows) and np.array_equal(a.logq.view(np.uint32), b.logq.view(np.uint32))
            and np.array_equal(a.log_weight.view(np.uint32), b.log_weight.view(np.uint32))
            and np.array_equal(a.n_tok, b.n_tok) and np.array_equal(a.n_resampled, b.n_resampled))


def check_case(c, got):
    cfg, p = sr.case_model(c)
    orc = sr.case_oracle(c)
    s64 = sr.score64_of(p, cfg, c.prefixes, got, c.temperature, c.constraints)
    dq = float(np.abs(got.logq.astype(np.float64) - s64[0]).max())
    print(f"{c.name}: settled {int(orc['settled'].sum())} of {len(c.prefixes)}, logq vs fp64 score of the rows {dq:.3e} "
          f"(atol {sr.ATOL['logq']:.3e}), resamples {got.n_resampled.reshape(-1).tolist()}")
    assert sr.check_result(cfg, c.prefixes, orc, got, s64, c.thr) == []


@pytest.mark.parametrize("c", sr.TRAJ_CASES, ids=lambda c: c.name)
def test_sample_conditional_matches_fp64_oracle(c):
    g = gen_of(c)
    got = run_case(g, c)
    cfg, _ = sr.case_model(c)
    N = len(c.prefixes)
    assert got.rows.shape == (N, c.W, cfg.max_len + 1) and got.logq.dtype == np.float32 and got.log_weight.dtype == np.float32
    assert got.n_resampled.shape == (N, 1) and got.log_z.shape == (N,) and np.isnan(got.z_stderr).all()
    check_case(c, got)


def test_no_constraint_has_no_weights():
    c = case("plain")
    got = run_case(gen_of(c), c)
    assert (got.log_weight.view(np.uint32) == 0).all()      # +0.0 bitwise
    assert (got.n_resampled == 0).all() and (got.log_z == 0).all()
    hot = run_case(gen_of(c), c, ess_threshold=1.0)
    assert (hot.log_weight.view(np.uint32) == 0).all() and (hot.n_resampled == 0).all()
    assert same_bytes(got, hot)


@pytest.mark.parametrize("name,max_batch", [("h64-L1-n9-W4", 20), ("h64-L1-n9-W4", 12), ("h128-L2-n9-W17", 85)])
def test_batches_do_not_change_the_bytes(name, max_batch):
    """max_batch = 20 / 12 at W = 4: 5 + 4 and 3 + 3 + 3 names; 85 at W = 17: 5 + 4."""
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    c = case(name)
    cfg, p = sr.case_model(c)
    one = run_case(gen_of(c), c)
    cut = run_case(HipGenerator(cfg, p, max_batch=max_batch), c)
    assert same_bytes(one, cut)


def test_start_runs_seeds_and_thresholds_on_one_recording():
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    c = case("h64-L1-n9-W4")
    cfg, p = sr.case_model(c)
    g = HipGenerator(cfg, p)
    pre = [""] * 9
    kw = dict(width=4, seed=3, constraints=sr.DIGITS)
    whole = g.sample_conditional(pre, start=2 ** 33, **kw)
    assert g.g.conditional_graphs() == 1 and g.g.beam_graphs() == 0 and g.g.distinct_graphs() == 0
    part = g.sample_conditional(pre[:4], start=2 ** 33 + 5, **kw)
    assert np.array_equal(part.rows, whole.rows[5:]) and np.array_equal(part.logq.view(np.uint32), whole.logq[5:].view(np.uint32))
    assert np.array_equal(part.log_weight.view(np.uint32), whole.log_weight[5:].view(np.uint32))
    assert np.array_equal(part.n_resampled, whole.n_resampled[5:])
    assert not np.array_equal(whole.rows[:4], whole.rows[5:])
    # runs = 3: the three calls with the matching start, pooled
    three = g.sample_conditional(pre[:3], runs=3, start=2 ** 33, **kw)
    assert three.rows.shape == (3, 12, cfg.max_len + 1) and three.n_resampled.shape == (3, 3)
    assert np.array_equal(three.rows.reshape(9, 4, -1), whole.rows)
    assert np.array_equal(three.log_weight.reshape(9, 4).view(np.uint32), whole.log_weight.view(np.uint32))
    assert np.array_equal(three.n_resampled.reshape(9, 1), whole.n_resampled)
    for r in range(3):
        one = g.sample_conditional(pre[:3], start=2 ** 33 + r, **kw)      # names start + n: run r of prefix 0 is its name 0
        assert np.array_equal(one.rows[0], three.rows[0, 4 * r:4 * r + 4])
        assert np.array_equal(one.log_weight[0].view(np.uint32), three.log_weight[0, 4 * r:4 * r + 4].view(np.uint32))
    assert np.isfinite(three.z_stderr).all()
    # another seed, threshold and temperature replay the recordings that exist
    n = g.g.conditional_graphs()
    other = g.sample_conditional(pre, start=2 ** 33, width=4, seed=4, constraints=sr.DIGITS, ess_threshold=1.0, temperature=0.7)
    assert g.g.conditional_graphs() == n and g.g.beam_graphs() == 0
    assert not np.array_equal(other.rows, whole.rows)
    orc = sr.oracle(p, cfg, pre, 4, seed=4, start=2 ** 33, temperature=0.7, constraints=sr.DIGITS, ess_threshold=1.0)
    assert sr.check_result(cfg, pre, orc, other, sr.score64_of(p, cfg, pre, other, 0.7, sr.DIGITS), 1.0) == []
    assert same_bytes(whole, g.sample_conditional(pre, start=2 ** 33, **kw))


def test_neighbours_are_not_disturbed():
    """beam_search, sample_distinct and generate before and after a sample_conditional call: the bytes, graph
    counts and workspace of a fresh generator."""
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    from gru_mpi_cuda_amd.utils.data import random_floats
    c = case("h128-L2-n3-W4")
    cfg, p = sr.case_model(c)
    pre = list(c.prefixes)
    rf = random_floats(len(pre), cfg.max_len, 5)
    fresh = HipGenerator(cfg, p)
    want_b, want_d = fresh.beam_search(pre, width=4), fresh.sample_distinct(pre, width=4, seed=2)
    want_g = fresh.generate(rf, temperature=0.8, prefix=pre)
    ws, bg, dg = fresh.g.beam_workspace_bytes(), fresh.g.beam_graphs(), fresh.g.distinct_graphs()
    g = HipGenerator(cfg, p)
    for rnd in range(2):
        b, d = g.beam_search(pre, width=4), g.sample_distinct(pre, width=4, seed=2)
        s = g.generate(rf, temperature=0.8, prefix=pre)
        assert np.array_equal(b.rows, want_b.rows) and np.array_equal(b.logp.view(np.uint32), want_b.logp.view(np.uint32))
        assert np.array_equal(b.n_tok, want_b.n_tok) and np.array_equal(b.n_beams, want_b.n_beams)
        assert np.array_equal(d.rows, want_d.rows) and np.array_equal(d.logq.view(np.uint32), want_d.logq.view(np.uint32))
        assert np.array_equal(d.gumbel.view(np.uint32), want_d.gumbel.view(np.uint32))
        assert np.array_equal(s, want_g)
        assert g.g.beam_workspace_bytes() == ws and g.g.beam_graphs() == bg and g.g.distinct_graphs() == dg
        if rnd == 0:
            check_case(c, run_case(g, c))
            assert g.g.conditional_graphs() == 1


def test_the_estimate_of_z_follows_the_law():
    """tests/test_smc_ref.py's model and language, 4096 systems of 4 particles in one call at the default
    threshold, where a good third of the systems resamples in mid-trajectory and the others carry unequal
    weights to the end: the mean of exp(log_z) within 5 of its own standard errors of the exact float64 Z."""
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    cfg, p, rows = sr.law_case()
    Z = float(sr.law_exact(cfg, p, rows).sum())
    g = HipGenerator(cfg, p, max_batch=4096)
    got = g.sample_conditional(None, width=4, count=4096, seed=7, constraints=sr.LAW)
    zh = np.exp(got.log_z)
    se = zh.std(ddof=1) / np.sqrt(len(zh))
    print(f"Z {Z:.6e}, mean Zhat {zh.mean():.6e}, standard error {se:.3e} ({(zh.mean() - Z) / se:+.2f} sigma)")
    assert se / Z < 0.05 and abs(zh.mean() - Z) <= 5 * se
    nres = got.n_resampled.reshape(-1)
    print(f"resampling steps per system {nres.mean():.3f}, systems that resample {float((nres > 0).mean()):.3f}")
    assert 0.2 <= float((nres > 0).mean()) <= 0.8 and nres.max() < cfg.max_len - 1      # the adaptive regime
    plain = g.sample_conditional(None, width=4, count=4096, seed=7, constraints=sr.LAW, ess_threshold=0.0)
    assert (plain.n_resampled == 0).all() and not np.array_equal(plain.log_weight, got.log_weight)
    index = {bytes(r) for r in rows}
    assert all(bytes(r) in index for r in got.rows.reshape(-1, cfg.max_len + 1))
    pooled = g.sample_conditional(None, width=4, count=1, runs=4096, seed=7, constraints=sr.LAW)     # the same names, pooled
    assert abs(float(np.exp(pooled.log_z[0])) - zh.mean()) <= 1e-6 * zh.mean()
    assert abs(float(pooled.z_stderr[0]) - se) <= 1e-6 * se


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
               dict(presence_penalty=0.5), dict(frequency_penalty=0.5), dict(seed=-1), dict(start=2 ** 64), dict(runs=0),
               dict(ess_threshold=1.5), dict(ess_threshold=-0.1), dict(prefix="0", constraints=dict(charset="abc"))):
        with pytest.raises(ValueError):
            g.sample_conditional(**kw)
    with pytest.raises(ValueError):
        HipGenerator(cfg, p, precision="bf16").sample_conditional("")
    assert g.g.beam_workspace_bytes() == 0 and g.g.conditional_graphs() == 0      # nothing was launched
    assert g.g.read_error() == 0

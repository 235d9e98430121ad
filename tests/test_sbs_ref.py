"""models/sbs_ref.py and cpu_ref.sample_distinct on the CPU: the Philox twin, the float32 emulator against the
float64 rule, the planted defects, the condition the GPU test relies on (at most one prefix in eight
unsettled), the distribution of the draws, and the validation errors."""
import itertools

import numpy as np
import pytest

from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models import sbs_ref as sr
from gru_mpi_cuda_amd.models.params import init_params


# ------------------------------------------------------------------------------- the noise
def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(v) for v in sr.philox4x32(np.array(ctr, np.uint32), np.array(key, np.uint32))) == want
    ctr = np.array([k[0] for k in kat], np.uint32)
    key = np.array([k[1] for k in kat], np.uint32)
    assert np.array_equal(sr.philox4x32(ctr, key), np.array([k[2] for k in kat], np.uint32))      # batched


def test_uniforms_are_exact_and_inside_the_open_interval():
    g = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 5], np.uint64)
    u = sr.sbs_uniform(0xDEADBEEFCAFEF00D, g, 3, 17, 64)
    assert u.dtype == np.float32 and u.shape == (5, 17, 64)
    k = u.astype(np.float64) * 2.0 ** 24
    assert np.array_equal(k, np.round(k)) and (k.astype(np.int64) % 2 == 1).all()      # odd multiples of 2^-24
    assert u.min() >= np.float32(2.0 ** -24) and u.max() <= np.float32(1 - 2.0 ** -24)
    # the extreme words
    for word, want in ((0, 2.0 ** -24), (0xFFFFFFFF, 1 - 2.0 ** -24)):
        v = np.float32((2.0 * (word >> 9) + 1.0) * 2.0 ** -24)
        assert float(v) == want and np.isfinite(-np.log(-np.log(np.float64(v))))
    # candidate j reads word j & 3 of the block j >> 2; name, step and seed all enter the counter / key
    blk = sr.philox4x32(np.array([5, 3, 1, 0], np.uint32), np.array([0xCAFEF00D, 0xDEADBEEF], np.uint32))
    want = np.float32((2.0 * (int(blk[2]) >> 9) + 1.0) * 2.0 ** -24)
    assert u[1].reshape(-1)[5 * 4 + 2] == want
    assert len({sr.sbs_uniform(s, np.array([gi], np.uint64), l, 2, 64).tobytes()
                for s, gi, l in itertools.product((1, 2 ** 32 + 1), (0, 2 ** 32), (0, 1))}) == 8


# ------------------------------------------------------------------------------- one step
@pytest.mark.parametrize("i", range(len(sr.STEP_CASES)), ids=lambda i: "-".join(map(str, sr.STEP_CASES[i])))
def test_emulator_passes_check_step(i):
    c = sr.STEP_CASES[i]
    d = sr.settled_inputs(c, seed=i % 3)
    ref, emu = sr.select_ref(d), sr.select_emulate(d)
    assert sr.check_step(d, ref, emu) == []
    if not c.optional:
        assert sr.check_step(d, ref, {k: v for k, v in emu.items() if k not in ("lq", "gt", "zmax", "sel")}) == []


@pytest.mark.parametrize("mut", sorted(sr.MUTATIONS))
def test_every_planted_defect_fails(mut):
    hit = tried = 0
    for i, c in enumerate(sr.STEP_CASES):
        if not sr.mutation_applies(mut, c):
            continue
        d = sr.settled_inputs(c, seed=i % 3)
        tried += 1
        hit += bool(sr.check_step(d, sr.select_ref(d), sr.select_emulate(d, mut)))
    assert tried >= 2 and hit == tried, (mut, hit, tried)


def test_measured_deviation_is_the_recorded_one():
    """MEASURED_DEV is a measurement: the step cases (the fast part) stay within it."""
    worst = {k: 0.0 for k in sr.MEASURED_DEV}
    for c in sr.STEP_CASES:
        for seed in (0, 1, 2):
            for k, v in sr.step_deviation(c, seed).items():
                worst[k] = max(worst[k], v)
    for k in ("lq", "Gt"):
        assert 0.5 * sr.MEASURED_DEV[k] <= worst[k] <= sr.MEASURED_DEV[k], (k, worst[k])
    assert worst["logq"] <= sr.MEASURED_DEV["logq"]
    assert sr.GUARD == 8 * sr.MEASURED_DEV["Gt"] and sr.ATOL["Gt"] == 4 * sr.MEASURED_DEV["Gt"]


# ------------------------------------------------------------------------------- the trajectory
@pytest.mark.parametrize("c", sr.TRAJ_CASES, ids=lambda c: c.name)
def test_at_most_one_prefix_in_eight_is_unsettled(c):
    """A condition, not a measurement: tests/test_sbs_gpu.py compares bytes on settled prefixes only."""
    orc = sr.case_oracle(c)
    unsettled = int((~orc["settled"]).sum())
    assert unsettled * 8 <= len(c.prefixes), (c.name, unsettled, orc["clear"].min(1))


@pytest.mark.parametrize("c", [c for c in sr.TRAJ_CASES if c.preset is None and c.W in (4, 17)], ids=lambda c: c.name)
def test_emulator_passes_check_result(c):
    cfg, p = sr.case_model(c)
    emu = sr.emulate(p, cfg, c.prefixes, c.W, **sr.case_kwargs(c))
    s64 = sr.score64_of(p, cfg, c.prefixes, emu, c.temperature, c.constraints)
    assert sr.check_result(cfg, c.prefixes, sr.case_oracle(c), emu, s64) == []
    for mut in ("counter_without_step", "counter_local_index", "forced_adds_lp", "g_as_key"):
        if mut == "counter_local_index" and c.start == 0:
            continue
        if mut == "forced_adds_lp" and (not any(c.prefixes) or c.constraints is not None):      # (a forced char alone in its set has lq = 0)
            continue
        bad = sr.emulate(p, cfg, c.prefixes, c.W, mut=mut, **sr.case_kwargs(c))
        s64 = sr.score64_of(p, cfg, c.prefixes, bad, c.temperature, c.constraints)
        assert sr.check_result(cfg, c.prefixes, sr.case_oracle(c), bad, s64) != [], mut


# ------------------------------------------------------------------------------- the distribution
def chi2_quantile(df: int, z: float = 4.753424) -> float:
    """The 1 - 10^-6 quantile of chi-square at ``df`` degrees of freedom (z: the normal one)."""
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(1 - 1e-6, df))
    except ImportError:
        return df * (1 - 2 / (9 * df) + z * (2 / (9 * df)) ** 0.5) ** 3      # Wilson-Hilferty


def pearson(counts: np.ndarray, expected: np.ndarray):
    """Pearson's statistic over cells of expected count >= 5 (smaller ones pooled, smallest first) and its
    degrees of freedom."""
    order = np.argsort(expected)
    cells = []
    acc_c = acc_e = 0.0
    for i in order:
        acc_c += counts[i]
        acc_e += expected[i]
        if acc_e >= 5:
            cells.append((acc_c, acc_e))
            acc_c = acc_e = 0.0
    if acc_e > 0:      # a last pool below 5: into the largest cell
        cells[-1] = (cells[-1][0] + acc_c, cells[-1][1] + acc_e)
    c, e = np.array(cells).T
    assert abs(c.sum() - counts.sum()) < 1e-6 and abs(e.sum() - expected.sum()) < 1e-6 * expected.sum()
    return float(((c - e) ** 2 / e).sum()), len(cells) - 1


CHARSET = "0123"


@pytest.fixture(scope="module")
def toy():
    cfg = GRUConfig(vocab=64, embed=8, hidden=16, layers=1, max_len=2, sos=0, eos=10, seed=5)
    p = {k: v.double() for k, v in init_params(cfg).items()}
    p["fc.weight"] = p["fc.weight"] * 6
    names = [""] + list(CHARSET) + [a + b for a in CHARSET for b in CHARSET]      # the language: 21 rows
    from gru_mpi_cuda_amd.engine.generator import encode_names
    return cfg, p, names, encode_names(names, cfg)


@pytest.mark.parametrize("temperature", [None, 0.7])
def test_draws_follow_sampling_without_replacement(toy, temperature):
    """One call, 20000 empty prefixes (every name its own noise through its global index), width 2: the first
    draw is a sample from p, the ordered pair (i, j) has probability p_i p_j / (1 - p_i)."""
    cfg, p, names, rows = toy
    N = 20000
    logp = cpu_ref.score(p, cfg, rows, temperature=1.0 if temperature is None else temperature,
                         constraints=dict(charset=CHARSET))[1]
    pr = np.exp(logp)
    assert abs(pr.sum() - 1) < 1e-12 and len(pr) == 21
    res = cpu_ref.sample_distinct(p, cfg, None, 2, N, seed=11, start=5, temperature=temperature,
                                  constraints=dict(charset=CHARSET))
    assert (res.n_found == 2).all()
    index = {bytes(r): i for i, r in enumerate(rows)}
    first = np.array([index[bytes(r)] for r in res.rows[:, 0]])
    second = np.array([index[bytes(r)] for r in res.rows[:, 1]])
    assert (first != second).all()
    assert np.abs(res.logq - logp[np.stack([first, second], 1)]).max() < 1e-12      # logq is the rows' score
    stat, df = pearson(np.bincount(first, minlength=21).astype(float), N * pr)
    print(f"T = {temperature}: first draw chi2 {stat:.1f} at {df} df (bound {chi2_quantile(df):.1f})")
    assert stat < chi2_quantile(df)
    pair = pr[:, None] * pr[None, :] / (1 - pr[:, None])
    np.fill_diagonal(pair, 0)
    assert abs(pair.sum() - 1) < 1e-12
    counts = np.bincount(first * 21 + second, minlength=441).astype(float)
    off = ~np.eye(21, dtype=bool).reshape(-1)
    stat, df = pearson(counts[off], N * pair.reshape(-1)[off])
    print(f"T = {temperature}: ordered pairs chi2 {stat:.1f} at {df} df (bound {chi2_quantile(df):.1f})")
    assert stat < chi2_quantile(df)
    assert (np.diff(res.gumbel, axis=1) <= 0).all() and (res.gumbel[:, 0] == 0).all()


@pytest.mark.parametrize("mut", ["g_as_key", "carry_reperturbed", "counter_without_step"])
def test_the_distribution_check_sees_a_planted_defect(toy, mut):
    """The untruncated key, a re-perturbed carry and noise shared between the steps each miss the first
    draw's law by far: the chi-square above is not a formality."""
    cfg, p, names, rows = toy
    N = 20000
    pr = np.exp(cpu_ref.score(p, cfg, rows, temperature=1.0, constraints=dict(charset=CHARSET))[1])
    pre, plen, inv, seed, start = cpu_ref.distinct_inputs(cfg, None, 2, N, 11, 5)
    cons = cpu_ref.as_constraints(cfg, N, dict(charset=CHARSET))
    res = cpu_ref.sample_distinct_rule(p, cfg, pre, plen, 2, seed, start, inv, cons, mut)
    index = {bytes(r): i for i, r in enumerate(rows)}
    first = np.array([index[bytes(r)] for r in res.rows[:, 0]])
    stat, df = pearson(np.bincount(first, minlength=21).astype(float), N * pr)
    assert stat > 4 * chi2_quantile(df), (mut, stat)


def test_a_width_that_holds_the_language_returns_every_row_once(toy):
    cfg, p, names, rows = toy
    res = cpu_ref.sample_distinct(p, cfg, None, 32, 3, seed=2, constraints=dict(charset=CHARSET))
    assert (res.n_found == 21).all()
    for n in range(3):
        assert sorted(res.names()[n]) == sorted(names)
        assert abs(np.exp(res.logq[n, :21]).sum() - 1) <= 1e-9
        assert np.isneginf(res.logq[n, 21:]).all() and np.isneginf(res.gumbel[n, 21:]).all()
        assert (res.rows[n, 21:] == 0).all() and (res.n_tok[n, 21:] == 0).all()
    assert res.names()[0] != res.names()[1]      # another order for another name


def test_start_names_the_global_index(toy):
    cfg, p, names, rows = toy
    kw = dict(seed=9, temperature=0.8, constraints=dict(charset=CHARSET))
    whole = cpu_ref.sample_distinct(p, cfg, None, 3, 12, start=2 ** 32 - 4, **kw)
    part = cpu_ref.sample_distinct(p, cfg, None, 3, 5, start=2 ** 32 + 3, **kw)
    for k in ("rows", "logq", "gumbel", "n_tok", "n_found"):
        assert np.array_equal(getattr(part, k), getattr(whole, k)[7:]), k
    assert not np.array_equal(whole.rows[:5], whole.rows[7:])


def test_fp32_params_run_the_fp32_rule(toy):
    cfg, p, names, rows = toy
    res = cpu_ref.sample_distinct({k: v.float() for k, v in p.items()}, cfg, ["0", ""], 4, seed=1,
                                  constraints=dict(charset=CHARSET))
    assert res.logq.dtype == np.float32 and res.gumbel.dtype == np.float32
    assert all(len(set(n)) == len(n) == 4 for n in res.names()) and all(x.startswith("0") for x in res.names()[0])
    empty = cpu_ref.sample_distinct(p, cfg, None, 4, 0)
    assert empty.rows.shape == (0, 4, cfg.max_len + 1) and empty.names() == []


def test_validation_errors(toy):
    cfg, p, names, rows = toy
    for kw in (dict(width=0), dict(width=33), dict(width=2.5), dict(prefix="0" + chr(cfg.eos)), dict(prefix="012"), dict(prefix="a"),
               dict(temperature=0), dict(temperature=-0.5), dict(temperature=float("inf")), dict(temperature=1e-60),
               dict(top_k=3), dict(top_p=0.5), dict(logit_bias={"a": 1.0}), dict(presence_penalty=0.1),
               dict(frequency_penalty=0.1), dict(seed=-1), dict(seed=2 ** 64), dict(start=-1), dict(start=1.5),
               dict(prefix=["0", "1"], count=3), dict(prefix="5", constraints=dict(charset=CHARSET))):
        with pytest.raises(ValueError):
            cpu_ref.sample_distinct(p, cfg, **kw)
    with pytest.raises(TypeError):
        cpu_ref.sample_distinct(p, cfg, bogus=1)
    cpu_ref.sample_distinct(p, cfg, top_k=None, top_p=None)      # None: not given


def test_an_offered_candidate_at_minus_infinity_ranks_before_what_is_not_offered():
    """A char of the allowed set whose logit is -inf has Gt = -inf and is still a candidate (the kernel's key of
    -inf is not 0): with room left it takes a slot, ahead of every index that was not offered."""
    for dt in (np.float64, np.float32):
        x = np.zeros((1, 2, 64), dt)
        x[0, 0, 9] = -np.inf
        allowed = np.zeros((1, 64), bool)
        allowed[0, [3, 9]] = True
        logq, G = np.array([[0, -np.inf]], dt), np.array([[0, -np.inf]], dt)
        state = np.array([[cpu_ref.BEAM_LIVE, cpu_ref.BEAM_DEAD]], np.int32)
        u = sr.sbs_uniform(1, np.array([0], np.uint64), 0, 2, 64)
        s = cpu_ref.sbs_step(x, logq, G, state, np.array([-1]), allowed, np.ones(1, np.float32), u, 5, 0)
        assert s["sel"].tolist() == [[3, 9]] and s["parent"].tolist() == [[0, 0]] and s["chr"].tolist() == [[3, 9]]
        assert s["logq"][0, 0] == 0 and s["G"][0, 0] == 0 and np.isneginf(s["logq"][0, 1]) and np.isneginf(s["G"][0, 1])
        assert not np.isnan(s["gt"][0, 0, [3, 9]]).any()

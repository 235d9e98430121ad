"""models/smc_ref.py and cpu_ref.sample_conditional on the CPU: the noise, the float32 emulator against the
float64 rule, the planted defects, the condition the GPU test relies on (at most one prefix in eight
unsettled), the relation to score, and the law: the estimate of Z is unbiased and the weighted particles
follow the model's conditional, where the constrained sampler's equal-weight rows do not."""
import numpy as np
import pytest

from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models import smc_ref as sr
from gru_mpi_cuda_amd.models.params import init_params


# ------------------------------------------------------------------------------- the noise
def test_uniforms_are_exact_and_addressed_by_slot_step_and_global_index():
    g = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 5], np.uint64)
    u = sr.smc_uniform(0xDEADBEEFCAFEF00D, g, 3, 17)
    assert u.dtype == np.float32 and u.shape == (5, 17, 2)
    k = u.astype(np.float64) * 2.0 ** 24
    assert np.array_equal(k, np.round(k)) and (k.astype(np.int64) % 2 == 1).all()      # odd multiples of 2^-24
    assert u.min() >= np.float32(2.0 ** -24) and u.max() <= np.float32(1 - 2.0 ** -24)
    blk = sr.philox4x32(np.array([5, 3, 1, 0], np.uint32), np.array([0xCAFEF00D, 0xDEADBEEF], np.uint32))      # slot 5, step 3, g = 1
    for word in (0, 1):
        assert u[1, 5, word] == np.float32((2.0 * (int(blk[word]) >> 9) + 1.0) * 2.0 ** -24)
    assert len({sr.smc_uniform(s, np.array([gi], np.uint64), l, 2).tobytes()
                for s in (1, 2 ** 32 + 1) for gi in (0, 2 ** 32) for l in (0, 1)}) == 8


# ------------------------------------------------------------------------------- one step
@pytest.mark.parametrize("i", range(len(sr.STEP_CASES)), ids=lambda i: "-".join(map(str, sr.STEP_CASES[i])))
def test_emulator_stays_within_atol_of_fp64(i):
    c = sr.STEP_CASES[i]
    d = sr.settled_inputs(c, seed=i % 3)
    ref, emu = sr.select_ref(d), sr.select_emulate(d)
    assert sr.check_step(d, ref, emu) == []
    if not c.optional:
        assert sr.check_step(d, ref, {k: v for k, v in emu.items() if k not in ("lq", "logm", "ess")}) == []


@pytest.mark.parametrize("mut", sorted(m for m, where in sr.MUTATIONS.items() if where == "step"))
def test_every_planted_defect_fails_check_step(mut):
    hit = tried = 0
    for i, c in enumerate(sr.STEP_CASES):
        if not sr.mutation_applies(mut, c):
            continue
        d = sr.settled_inputs(c, seed=i % 3)
        tried += 1
        hit += bool(sr.check_step(d, sr.select_ref(d), sr.select_emulate(d, mut)))
    assert tried >= 2 and hit == tried, (mut, hit, tried)


def test_measured_deviation_is_the_recorded_one():
    """MEASURED_DEV is a measurement: the step cases (the fast part) stay within it and reach most of it."""
    worst = {k: 0.0 for k in sr.MEASURED_DEV}
    for c in sr.STEP_CASES:
        for seed in (0, 1, 2):
            for k, v in sr.step_deviation(c, seed).items():
                worst[k] = max(worst[k], v)
    for k in sr.MEASURED_DEV:
        assert 0.5 * sr.MEASURED_DEV[k] <= worst[k] <= sr.MEASURED_DEV[k], (k, worst[k])
    assert sr.GUARD == 8 * sr.MEASURED_DEV["decide"] and all(sr.ATOL[k] == 4 * sr.MEASURED_DEV[k] for k in sr.ATOL)


# ------------------------------------------------------------------------------- the trajectory
@pytest.mark.parametrize("c", sr.TRAJ_CASES, ids=lambda c: c.name)
def test_at_most_one_prefix_in_eight_is_unsettled(c):
    """A condition, not a measurement: tests/test_smc_gpu.py compares bytes on settled prefixes only."""
    orc = sr.case_oracle(c)
    unsettled = int((~orc["settled"]).sum())
    assert unsettled * 8 <= len(c.prefixes), (c.name, unsettled, orc["clear"].min(1))


@pytest.mark.parametrize("c", [c for c in sr.TRAJ_CASES if c.preset is None and c.W in (4, 17)], ids=lambda c: c.name)
def test_emulator_passes_check_result_and_defects_do_not(c):
    cfg, p = sr.case_model(c)
    emu = sr.emulate(p, cfg, c.prefixes, c.W, **sr.case_kwargs(c))
    s64 = sr.score64_of(p, cfg, c.prefixes, emu, c.temperature, c.constraints)
    assert sr.check_result(cfg, c.prefixes, sr.case_oracle(c), emu, s64, c.thr) == []
    for mut in ("counter_without_step", "counter_local_index", "forced_adds_logm"):
        if mut == "counter_local_index" and c.start == 0:
            continue
        if mut == "forced_adds_logm" and (not any(c.prefixes) or c.constraints is None or c.thr != 0):
            continue
        if mut != "forced_adds_logm" and all(len(x) >= cfg.max_len - 1 for x in c.prefixes):
            continue
        bad = sr.emulate(p, cfg, c.prefixes, c.W, mut=mut, **sr.case_kwargs(c))
        s64 = sr.score64_of(p, cfg, c.prefixes, bad, c.temperature, c.constraints)
        assert sr.check_result(cfg, c.prefixes, sr.case_oracle(c), bad, s64, c.thr) != [], mut


# ------------------------------------------------------------------------------- the relation to score
@pytest.fixture(scope="module")
def small():
    cfg = GRUConfig(vocab=64, embed=64, hidden=64, layers=1, max_len=4, sos=0, eos=5, seed=4)
    p = {k: v.double() for k, v in init_params(cfg).items()}
    return cfg, p


def test_without_a_constraint_nothing_is_weighted(small):
    cfg, p = small      # the flat model: fc.weight as initialised
    for params in (p, {k: v.float() for k, v in p.items()}):
        for thr in (0.0, 0.5, 1.0):
            res = cpu_ref.sample_conditional(params, cfg, ["", "7", ""], 8, runs=2, seed=3, ess_threshold=thr, temperature=0.9)
            assert (res.log_weight == 0).all() and not np.signbit(res.log_weight).any()      # +0.0 bitwise
            assert (res.n_resampled == 0).all() and (res.log_z == 0).all()
            for n in range(3):
                assert len({bytes(r) for r in res.rows[n, :8]}) > 1      # the particles of a system differ


@pytest.mark.parametrize("thr", [0.0, 0.5, 1.0])
def test_logq_and_log_weight_are_the_rows_scores(small, thr):
    cfg, p = small
    p = dict(p)
    p["fc.weight"] = p["fc.weight"] * 4
    pre = ["", "1", "20", ""]
    cons = dict(charset="0123456789", min_len=1)
    res = cpu_ref.sample_conditional(p, cfg, pre, 8, seed=5, temperature=0.8, constraints=cons, ess_threshold=thr)
    lq, lp = sr.score64_of(p, cfg, pre, res, 0.8, cons)
    assert np.isfinite(lq).all() and np.abs(res.logq - lq).max() <= sr.ATOL["logq"]
    if thr == 0:
        assert (res.n_resampled == 0).all() and np.abs(res.log_weight - (lp - lq)).max() <= sr.ATOL["logw"]
    else:
        assert (res.n_resampled > 0).any() and (res.log_weight <= 0).all()


# ------------------------------------------------------------------------------- the law
N_LAW = 20000


def chi2_quantile(df: int, z: float = 4.753424) -> float:
    """The 1 - 10^-6 quantile of chi-square at ``df`` degrees of freedom (z: the normal one)."""
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(1 - 1e-6, df))
    except ImportError:
        return df * (1 - 2 / (9 * df) + z * (2 / (9 * df)) ** 0.5) ** 3      # Wilson-Hilferty


@pytest.fixture(scope="module")
def law():
    cfg, p, rows = sr.law_case()
    return cfg, {k: v.double() for k, v in p.items()}, rows, {bytes(r): i for i, r in enumerate(rows)}


def stderr(a):
    return a.std(0, ddof=1) / np.sqrt(N_LAW)


def law_figures(law, temperature, thr, mut=None):
    """Per row of the language the exact p and every system's weighted indicator [N_LAW, rows]; the mean of Zhat
    and its standard error; the particles' row indices and the systems' resampling counts."""
    cfg, p, rows, index = law
    pr = sr.law_exact(cfg, p, rows, temperature)
    pre, plen, inv, seed, start, t, N, R = cpu_ref.conditional_inputs(cfg, None, 4, N_LAW, 1, 11, 5, temperature, thr)
    cons = cpu_ref.conditional_constraints(cfg, N, R, sr.LAW)
    got_rows, logw, logq, ntok, nres = cpu_ref.sample_conditional_rule(p, cfg, pre, plen, 4, seed, start, inv, t, cons, mut)
    idx = np.array([index[bytes(r)] for r in got_rows.reshape(-1, cfg.max_len + 1)]).reshape(N_LAW, 4)      # KeyError: outside L
    w = np.exp(logw)
    zh = w.mean(1)
    per = np.zeros((N_LAW, len(rows)))
    for k in range(4):
        np.add.at(per, (np.arange(N_LAW), idx[:, k]), w[:, k] / 4)
    se = stderr
    return pr, per, float(zh.mean()), float(se(zh)), idx, nres


def law_violations(law, pr, per, zmean, zse):
    """What the law asks of N_LAW systems, as a list of misses: the mean of Zhat within 5 of its standard errors of
    Z; every row with p N > 50 within 5.5; and, for the rows too rare for that, a function of the row -- the
    weighted indicator of every name length with p N > 50 -- within 5.5."""
    cfg, rows = law[0], law[2]
    bad = []
    Z = float(pr.sum())
    if not abs(zmean - Z) <= 5 * zse:
        bad.append(f"Zhat {(zmean - Z) / zse:+.2f} sigma")
    mean, se = per.mean(0), stderr(per)
    big = pr * N_LAW > 50
    dev = np.abs(mean - pr)[big] / se[big]
    print(f"   {int(big.sum())} rows with p N > 50, the worst at {dev.max():.2f} sigma")
    if not (big.sum() >= 2 and (dev <= 5.5).all()):
        bad.append(f"rows: {int(big.sum())} with p N > 50, the worst at {dev.max():.2f} sigma")
    nlen = (rows[:, :cfg.max_len] != 0).sum(1) - (rows[:, :cfg.max_len] == cfg.eos).sum(1)
    for k in range(1, cfg.max_len + 1):
        cls, pk = per[:, nlen == k].sum(1), float(pr[nlen == k].sum())
        if pk * N_LAW > 50:
            d = abs(cls.mean() - pk) / stderr(cls)
            print(f"   names of {k} chars: p {pk:.5f}, mean {cls.mean():.5f} +- {stderr(cls):.1e} ({d:.2f} sigma)")
            if not d <= 5.5:
                bad.append(f"names of {k} chars at {d:.2f} sigma")
    return bad


_law_seen = {}


@pytest.mark.parametrize("temperature,thr", [(None, 0.0), (None, 0.5), (None, 1.0), (0.7, 0.5), (0.7, 1.0)])
def test_the_estimate_is_unbiased_and_the_particles_follow_the_conditional(law, temperature, thr):
    cfg = law[0]
    pr, per, zmean, zse, _, nres = law_figures(law, temperature, thr)
    Z = float(pr.sum())
    some = float(((nres > 0) & (nres < cfg.max_len - 1)).mean())
    print(f"T = {temperature}, thr = {thr}: Z {Z:.6e}, mean Zhat {zmean:.6e} +- {zse:.2e} ({(zmean - Z) / zse:+.2f} sigma); "
          f"resampling steps per system {nres.mean():.3f}, systems that resample on some but not all steps {some:.3f}")
    assert len(pr) == 30 and 0.01 <= Z <= 0.2
    assert zse / Z < 0.02      # or the test could not see a defect
    assert law_violations(law, pr, per, zmean, zse) == []
    # each threshold is a regime of its own: none / some steps of some systems / most steps
    if thr == 0:
        assert (nres == 0).all()
    elif thr == 0.5:      # the adaptive regime, the default: most systems carry unequal weights over most steps
        assert 0 < nres.mean() < cfg.max_len - 1 and some >= 0.2 and float((nres == 0).mean()) >= 0.2
    else:
        assert nres.mean() > 1 and float((nres > 0).mean()) > 0.9
    _law_seen[(temperature, thr)] = (zmean, nres.mean())
    others = [v for k, v in _law_seen.items() if k[0] == temperature and k[1] != thr]
    assert all(v[0] != zmean and v[1] != nres.mean() for v in others)      # no two thresholds are the same run


def test_equal_weights_miss_the_conditional(law):
    """The counter-test: the same rows with equal weights -- the constrained sampler of ``generate`` -- against
    p / Z by Pearson's chi-square: far beyond the 1 - 10^-6 quantile.  This is the bias the weights remove."""
    pr, _, _, _, idx, _ = law_figures(law, None, 0.0)
    target = pr / pr.sum()
    first = idx[:, 0]      # at threshold 0 a particle is one run of the constrained sampler
    counts = np.bincount(first, minlength=len(pr)).astype(float)
    keep = target * N_LAW >= 5
    exp, obs = target[keep] * N_LAW, counts[keep]
    if (~keep).any():      # the cells below 5 expected, pooled
        exp, obs = np.append(exp, target[~keep].sum() * N_LAW), np.append(obs, counts[~keep].sum())
    stat, df = float(((obs - exp) ** 2 / exp).sum()), len(exp) - 1
    print(f"equal weights: chi2 {stat:.1f} at {df} df (bound {chi2_quantile(df):.1f})")
    assert stat > chi2_quantile(df)


@pytest.mark.parametrize("thr", [0.5, 1.0])
@pytest.mark.parametrize("mut", sorted(m for m, where in sr.MUTATIONS.items() if where == "law"))
def test_the_law_sees_a_planted_defect(law, mut, thr):
    """In the adaptive regime and where most steps resample."""
    pr, per, zmean, zse, _, nres = law_figures(law, None, thr, mut)
    assert nres.mean() > 0
    assert law_violations(law, pr, per, zmean, zse) != [], (mut, thr)


def test_every_planted_defect_is_assigned():
    assert set(sr.MUTATIONS.values()) <= {"step", "law"} and len(sr.MUTATIONS) >= 8

"""The public surface of sample_conditional without a device: pooling of runs, the arithmetic of start with
runs, the result's methods, and every ValueError raised before anything could be launched."""
import numpy as np
import pytest

from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import cpu_ref
from gru_mpi_cuda_amd.models.params import init_params

CS = dict(charset="0123", min_len=1)


@pytest.fixture(scope="module")
def toy():
    cfg = GRUConfig(vocab=64, embed=8, hidden=16, layers=1, max_len=3, sos=0, eos=10, seed=5)
    p = {k: v.double() for k, v in init_params(cfg).items()}
    p["fc.weight"] = p["fc.weight"] * 2
    return cfg, p


def test_runs_are_pooled_per_prefix(toy):
    cfg, p = toy
    res = cpu_ref.sample_conditional(p, cfg, ["", "1"], 4, runs=3, seed=2, constraints=CS)
    assert res.rows.shape == (2, 12, cfg.max_len + 1) and res.rows.dtype == np.uint8
    assert res.log_weight.shape == res.logq.shape == res.n_tok.shape == (2, 12)
    assert res.n_resampled.shape == (2, 3) and res.log_z.shape == res.z_stderr.shape == res.ess.shape == (2,)
    assert res.log_z.dtype == np.float64 and np.isfinite(res.z_stderr).all() and ((1 <= res.ess) & (res.ess <= 12)).all()
    lw = res.log_weight.astype(np.float64)
    assert np.allclose(res.log_z, np.log(np.exp(lw).mean(1)), rtol=0, atol=1e-12)
    zr = np.exp(lw).reshape(2, 3, 4).mean(2)
    assert np.allclose(res.z_stderr, zr.std(1, ddof=1) / np.sqrt(3))
    w = res.weights()
    assert w.shape == (2, 12) and np.allclose(w.sum(1), 1) and np.allclose(w, np.exp(lw) / np.exp(lw).sum(1, keepdims=True))
    names = res.names()
    assert [len(n) for n in names] == [12, 12] and all(n.startswith("1") for n in names[1])
    assert all(set(n) <= set("0123") for ns in names for n in ns)
    ex = res.expectation(len)
    assert ex.shape == (2,) and np.allclose(ex, [(w[n] * [len(x) for x in names[n]]).sum() for n in range(2)])
    d = res.draw(50, seed=1)
    assert [len(x) for x in d] == [50, 50] and set(d[0]) <= set(names[0]) and d == res.draw(50, seed=1) and d != res.draw(50, seed=2)
    one = cpu_ref.sample_conditional(p, cfg, ["", "1"], 4, seed=2, constraints=CS)
    assert one.rows.shape == (2, 4, cfg.max_len + 1) and one.n_resampled.shape == (2, 1) and np.isnan(one.z_stderr).all()
    empty = cpu_ref.sample_conditional(p, cfg, None, 4, 0, runs=2, constraints=CS)
    assert empty.rows.shape == (0, 8, cfg.max_len + 1) and empty.n_resampled.shape == (0, 2) and empty.names() == []


def test_run_r_of_prefix_n_has_the_global_index_start_plus_n_runs_plus_r(toy):
    cfg, p = toy
    kw = dict(seed=9, temperature=0.8, constraints=CS, ess_threshold=1.0)
    pooled = cpu_ref.sample_conditional(p, cfg, ["", "", "2"], 4, runs=3, start=2 ** 32 - 4, **kw)
    for n, pre in enumerate(["", "", "2"]):
        for r in range(3):
            one = cpu_ref.sample_conditional(p, cfg, [pre], 4, start=2 ** 32 - 4 + 3 * n + r, **kw)
            assert np.array_equal(one.rows[0], pooled.rows[n, 4 * r:4 * r + 4])
            assert np.array_equal(one.log_weight[0], pooled.log_weight[n, 4 * r:4 * r + 4])
            assert np.array_equal(one.logq[0], pooled.logq[n, 4 * r:4 * r + 4])
            assert one.n_resampled[0, 0] == pooled.n_resampled[n, r]
    flat = cpu_ref.sample_conditional(p, cfg, [""] * 6, 4, start=2 ** 32 - 4, **kw)      # the same six names, one run each
    assert np.array_equal(flat.rows.reshape(2, 12, -1), pooled.rows[:2])
    assert len({pooled.rows[n, 4 * r:4 * r + 4].tobytes() for n in range(2) for r in range(3)}) > 1      # runs differ


class _NoLaunch:
    """Stands where the native generator would: any call is a launch."""

    def __getattr__(self, name):
        raise AssertionError(f"native call {name} before validation finished")


def _stub(cfg, precision="fp32"):
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    g = object.__new__(HipGenerator)
    g.cfg, g.precision, g.g, g.dev = cfg, precision, _NoLaunch(), "cpu"
    return g


BAD = (dict(width=0), dict(width=33), dict(width=2.5), dict(prefix="0" + chr(10)), dict(prefix="0123"), dict(temperature=0),
       dict(temperature=-0.5), dict(temperature=float("inf")), dict(temperature=1e-60), dict(top_k=3), dict(top_p=0.5),
       dict(logit_bias={"a": 1.0}), dict(presence_penalty=0.1), dict(frequency_penalty=0.1), dict(seed=-1), dict(seed=2 ** 64),
       dict(start=-1), dict(start=1.5), dict(start=2 ** 64 - 2, count=2, runs=2), dict(runs=0), dict(runs=1.5),
       dict(ess_threshold=-0.1), dict(ess_threshold=1.01), dict(ess_threshold=float("nan")),
       dict(prefix=["0", "1"], count=3), dict(prefix="5", constraints=CS))


@pytest.mark.parametrize("kw", BAD, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items())[:40])
def test_value_errors_come_before_any_launch(toy, kw):
    cfg, p = toy
    with pytest.raises(ValueError):
        cpu_ref.sample_conditional(p, cfg, **kw)
    with pytest.raises(ValueError):
        _stub(cfg).sample_conditional(**kw)


def test_bf16_and_unknown_keywords_are_refused(toy):
    cfg, p = toy
    with pytest.raises(ValueError):
        _stub(cfg, "bf16").sample_conditional("")
    with pytest.raises(TypeError):
        cpu_ref.sample_conditional(p, cfg, bogus=1)
    with pytest.raises(TypeError):
        _stub(cfg).sample_conditional(bogus=1)
    with pytest.raises(AssertionError):      # the stub does stand in the way of a valid call
        _stub(cfg).sample_conditional("", constraints=None)
    cpu_ref.sample_conditional(p, cfg, top_k=None, top_p=None)      # None: not given


def test_per_prefix_constraint_values_follow_their_prefix_through_the_runs(toy):
    cfg, p = toy
    per = dict(charset=["01", "23"], min_len=1)
    pooled = cpu_ref.sample_conditional(p, cfg, ["", ""], 4, runs=3, seed=4, constraints=per)
    assert all(set(n) <= set("01") for n in pooled.names()[0]) and all(set(n) <= set("23") for n in pooled.names()[1])
    for n, cs in enumerate(("01", "23")):
        for r in range(3):
            one = cpu_ref.sample_conditional(p, cfg, [""], 4, seed=4, start=3 * n + r, constraints=dict(charset=cs, min_len=1))
            assert np.array_equal(one.rows[0], pooled.rows[n, 4 * r:4 * r + 4])
            assert np.array_equal(one.log_weight[0], pooled.log_weight[n, 4 * r:4 * r + 4])
    shared = cpu_ref.sample_conditional(p, cfg, ["", ""], 4, runs=2, seed=4, constraints=dict(exclude=["0", "1"], charset="01"))
    assert all(n not in ("0", "1") for ns in shared.names() for n in ns)
    with pytest.raises(ValueError):      # one value or one per prefix: never one per run
        cpu_ref.sample_conditional(p, cfg, ["", ""], 4, runs=3, constraints=dict(charset=["01"] * 6))
    with pytest.raises(ValueError):      # a built object holds one entry per name
        cpu_ref.sample_conditional(p, cfg, ["", ""], 4, runs=3, constraints=cpu_ref.make_constraints(cfg, 2, charset="01"))


def test_the_threshold_is_the_float32_the_device_reads(toy):
    cfg, p = toy
    assert cpu_ref.conditional_inputs(cfg, None, 4, 1, ess_threshold=0.3)[5] == float(np.float32(0.3)) != 0.3
    assert cpu_ref.conditional_inputs(cfg, None, 4, 1, ess_threshold=0.5)[5] == 0.5


def test_z_stderr_of_a_rule_far_below_double_range():
    """The spread of the runs is taken relative to the pooled maximum: weights near e^-600 give the same relative
    error as the same weights shifted into range, and only the final rescaling underflows with exp(log_z)."""
    rng = np.random.default_rng(3)
    lw = rng.normal(0, 1, (2, 12))
    rows, nt, nres = np.zeros((2, 12, 4), np.uint8), np.ones((2, 12), np.int32), np.zeros((2, 3), np.int32)
    near = cpu_ref.ConditionalResult(rows, lw - 5, lw, nt, nres)
    deep = cpu_ref.ConditionalResult(rows, lw - 600, lw, nt, nres)
    gone = cpu_ref.ConditionalResult(rows, lw - 900, lw, nt, nres)
    rel = near.z_stderr / np.exp(near.log_z)
    assert np.allclose(deep.z_stderr / np.exp(deep.log_z), rel, rtol=1e-9) and (deep.z_stderr > 0).all()
    assert np.allclose(gone.log_z, near.log_z - 895) and (np.exp(gone.log_z) == 0).all() and (gone.z_stderr == 0).all()
    assert np.allclose(gone.ess, near.ess) and np.allclose(gone.weights(), near.weights())

"""Sequential Monte Carlo under constraints as one persistent launch for small calls (csrc/kernels/gen_persist_smc.hip,
docs/DESIGN.md §4j): the opt-in path against the float64 oracle of models/smc_ref.py, and its switch and fallbacks."""
import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.models import smc_ref as sr

pytestmark = pytest.mark.gpu


def _pre(ML, eos, n):      # the digit-mapped mixture, as smc_ref._traj_cases builds it
    return tuple("".join("0123456789"[(ord(ch) + k) % 10] for k, ch in enumerate(p)) for p in sr._mixture(64, ML, eos, n))


# V 256, E 128, H 256: the smallest shapes the launch supports.  Every prefix of every case is settled in the oracle
# (minimum clearances 3.2e-4, 5.6e-5, 7.6e-5, 5.3e-5, 4.0e-4, 1.8e-3 and 3.6e-4 against GUARD 5.17e-6), so every byte
# is compared; the oracle resamples at 0, 29, 5, 0, 2, 2 and 1 steps
CASES = [
    sr.TrajCase("p-W1", 256, 128, 256, 1, 6, 5, 1, _pre(6, 5, 8), constraints=sr.DIGITS, thr=0.5),            # 8 rows, a slot per wave
    sr.TrajCase("p-W4", 256, 128, 256, 2, 6, 5, 4, _pre(6, 5, 16), start=2 ** 33 + 7, constraints=sr.DIGITS, thr=1.0),   # 64 rows
    sr.TrajCase("p-W8", 256, 128, 256, 1, 5, 5, 8, _pre(5, 5, 9), temperature=0.7, constraints=sr.DIGITS, thr=0.5),      # 8 + 1 systems
    sr.TrajCase("p-W17", 256, 128, 256, 2, 4, 5, 17, _pre(4, 5, 4), constraints=sr.DIGITS, thr=0.0),          # 3 / 2 slots per wave, 3 + 1
    sr.TrajCase("p-W32", 256, 128, 256, 1, 4, 5, 32, _pre(4, 5, 3), constraints=sr.DIGITS, thr=0.5),          # 4 slots per wave, 2 + 1
    sr.TrajCase("p-regex", 256, 128, 256, 1, 4, 0, 4, ("", "a"), constraints=dict(regex="a(b|c|d)"), thr=1.0),            # an automaton
    sr.TrajCase("p-pattern", 256, 128, 256, 1, 4, 0, 4, ("12", "", "7"), constraints=dict(charset="0123456789", min_len=2),
                thr=0.5),                                                                                      # a line per position
]


def new_gen(c, **kw):
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    cfg, p = sr.case_model(c)
    return HipGenerator(cfg, p, **kw)


def run(g, c, prefixes=None, **kw):
    return g.sample_conditional(list(c.prefixes if prefixes is None else prefixes), width=c.W, **dict(sr.case_kwargs(c), **kw))


def failures(c, got):
    """check_result of a one-run result against the case's oracle, the deviations printed."""
    cfg, p = sr.case_model(c)
    orc = sr.case_oracle(c)
    s64 = sr.score64_of(p, cfg, c.prefixes, got, c.temperature, c.constraints)
    dw = float(np.abs(got.log_weight.astype(np.float64) - orc["log_weight"]).max())
    dq = float(np.abs(got.logq.astype(np.float64) - orc["logq"]).max())
    print(f"{c.name}: settled {int(orc['settled'].sum())} of {len(c.prefixes)}, resampling steps {int(orc['n_resampled'].sum())}, "
          f"log_weight deviation {dw:.3e} (atol {sr.ATOL['logw']:.3e}), logq {dq:.3e} (atol {sr.ATOL['logq']:.3e})")
    return orc, sr.check_result(cfg, c.prefixes, orc, got, s64, c.thr)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_persistent_conditional_matches_fp64_oracle(c):
    g = new_gen(c, persist_conditional=64)
    got = run(g, c)
    N = len(c.prefixes)
    assert g.g.conditional_last_persist() and g.g.persist_conditional_launches() == -(-N // (64 // c.W))
    assert got.rows.shape == (N, c.W, c.ML + 1) and got.rows.dtype == np.uint8
    assert got.logq.shape == got.log_weight.shape == got.n_tok.shape == (N, c.W) and got.n_resampled.shape == (N, 1)
    assert got.logq.dtype == got.log_weight.dtype == np.float32 and got.n_tok.dtype == got.n_resampled.dtype == np.int32
    orc, bad = failures(c, got)
    assert orc["settled"].all()
    assert bad == []


def test_switch_and_fallbacks():
    c = CASES[2]
    off = new_gen(c)                                      # the default: the graph
    orc, bad = failures(c, run(off, c))
    assert bad == [] and orc["settled"].all() and not off.g.conditional_last_persist()
    assert off.g.persist_conditional_launches() == 0 and off.g.conditional_graphs() >= 1
    g = new_gen(c, persist_conditional=64)                # a fresh one: its flags and workspace from the first launch on
    res = {}
    for i, rows in enumerate((64, 0, 64, 64, 0, 64)):     # flag zeroing and workspace reuse across launches
        g.set_persist_conditional(rows)
        res[rows] = run(g, c)
        assert failures(c, res[rows])[1] == [], i
        assert g.g.conditional_last_persist() == (rows > 0), i
    a, b = res[64], res[0]                                # every prefix is settled: the two paths agree on the bytes
    assert np.array_equal(a.rows, b.rows) and np.array_equal(a.n_tok, b.n_tok) and np.array_equal(a.n_resampled, b.n_resampled)
    assert np.abs(a.logq.astype(np.float64) - b.logq).max() <= sr.ATOL["logq"]
    assert np.abs(a.log_weight.astype(np.float64) - b.log_weight).max() <= sr.ATOL["logw"]
    # runs: run r of prefix n is the system at start + 3 n + r; 27 systems of 8 slots are cut into 8 + 8 + 8 + 3
    pooled = run(g, c, runs=3)
    assert g.g.conditional_last_persist() and pooled.rows.shape == (9, 24, c.ML + 1)
    for n in (0, 2, 8):
        for r in range(3):
            one = run(g, c, prefixes=[c.prefixes[n]], start=c.start + 3 * n + r)
            sl = slice(r * c.W, (r + 1) * c.W)
            assert np.array_equal(one.rows[0], pooled.rows[n, sl]) and np.array_equal(one.n_tok[0], pooled.n_tok[n, sl])
            assert np.array_equal(one.logq[0], pooled.logq[n, sl]) and np.array_equal(one.log_weight[0], pooled.log_weight[n, sl])
            assert one.n_resampled[0, 0] == pooled.n_resampled[n, r]
    before = g.g.persist_conditional_launches()
    c1 = c._replace(name="p-one", W=4, prefixes=(c.prefixes[1],))      # the interactive shape (settled: clearance 9.9e-4)
    one = run(g, c1)
    assert g.g.conditional_last_persist() and g.g.persist_conditional_launches() == before + 1
    assert failures(c1, one)[1] == []
    for bad_n in (-1, 65):
        with pytest.raises(ValueError):
            g.set_persist_conditional(bad_n)
        with pytest.raises(ValueError):
            new_gen(c, persist_conditional=bad_n)


def test_unsupported_shapes_throw_before_launching(ext):
    ok = dict(H=256, L=2, V=256, N=8, W=8, ML=10)
    assert ext.gen_persist_smc_supported(*(ok[k] for k in ("H", "L", "V", "N", "W", "ML")))
    for change in (dict(H=64), dict(V=64), dict(N=13, W=5), dict(N=1, W=33), dict(ML=65)):
        d = dict(ok, **change)
        assert not ext.gen_persist_smc_supported(d["H"], d["L"], d["V"], d["N"], d["W"], d["ML"]), change
        with pytest.raises(RuntimeError, match="unsupported shape"):
            ext.gen_persist_smc(dict(d, sos=0, eos=0), torch.cuda.current_stream().cuda_stream)

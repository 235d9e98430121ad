"""Stochastic beam search as one persistent launch for small calls (csrc/kernels/gen_persist_sbs.hip,
docs/DESIGN.md §4i): the opt-in path against the float64 oracle of models/sbs_ref.py, and its switch and fallbacks."""
import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.models import sbs_ref as sr

pytestmark = pytest.mark.gpu

# V 256, E 128, H 256: the smallest shapes the launch supports.  Every name of every case is settled in the oracle
# (minimum clearances 6.2e-3, 1.4e-4, 4.7e-3, 6.1e-4 and 4.0e-5 against GUARD 3.7e-5), so every byte is compared
CASES = [
    sr.TrajCase("q-W1", 256, 128, 256, 1, 6, 0, 1, sr._mixture(256, 6, 0, 8)),                       # 8 rows, a slot per wave
    sr.TrajCase("q-W4", 256, 128, 256, 2, 6, 0, 4, sr._mixture(256, 6, 0, 16), start=2 ** 33 + 7),   # 64 rows, 64-bit index
    sr.TrajCase("q-W8", 256, 128, 256, 1, 5, 5, 8, sr._mixture(256, 5, 5, 9), temperature=0.7),      # 8 + 1 prefixes
    sr.TrajCase("q-W17", 256, 128, 256, 2, 4, 0, 17, sr._mixture(256, 4, 0, 4)),                     # 3 / 2 slots per wave, 3 + 1
    sr.TrajCase("q-W32", 256, 128, 256, 1, 4, 5, 32, sr._mixture(256, 4, 5, 3)),                     # 4 slots per wave, 2 + 1
]
_oracles = {}


def new_gen(c, **kw):
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    cfg, p = sr.case_model(c)
    return HipGenerator(cfg, p, **kw)


def run(g, c, **kw):
    return g.sample_distinct(list(c.prefixes), width=c.W, **dict(sr.case_kwargs(c), **kw))


def failures(c, got, prefixes=None, W=None, constraints=None):
    """check_result against the oracle of the call (computed once per call signature), the deviations printed."""
    cfg, p = sr.case_model(c)
    pre = c.prefixes if prefixes is None else prefixes
    key = (c.name, tuple(pre), W or c.W, repr(constraints))
    if key not in _oracles:
        _oracles[key] = sr.oracle(p, cfg, pre, W or c.W, **dict(sr.case_kwargs(c), constraints=constraints))
    orc = _oracles[key]
    s64 = sr.score64_of(p, cfg, pre, got, c.temperature, constraints)
    nf = [int(x) for x in got.n_found]
    ok = [n for n in range(len(nf)) if orc["settled"][n] and nf[n] == orc["n_found"][n]]
    dq = max([float(np.abs(got.logq[n, :nf[n]].astype(np.float64) - orc["logq"][n, :nf[n]]).max()) for n in ok], default=0.0)
    dg = max([float(np.abs(got.gumbel[n, :nf[n]].astype(np.float64) - orc["gumbel"][n, :nf[n]]).max()) / float(orc["scale"][n])
              for n in ok], default=0.0)
    print(f"{c.name}: settled {int(orc['settled'].sum())} of {len(nf)}, logq deviation {dq:.3e} (atol {sr.ATOL['logq']:.3e}), "
          f"gumbel {dg:.3e} of its scale (atol {sr.ATOL['Gt']:.3e})")
    return orc, sr.check_result(cfg, pre, orc, got, s64)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_persistent_distinct_matches_fp64_oracle(c):
    g = new_gen(c, persist_distinct=64)
    got = run(g, c)
    assert g.g.distinct_last_persist() and g.g.persist_distinct_launches() == -(-len(c.prefixes) // (64 // c.W))
    assert got.rows.shape == (len(c.prefixes), c.W, c.ML + 1) and got.logq.dtype == np.float32
    orc, bad = failures(c, got)
    assert orc["settled"].all()
    assert bad == []


def test_switch_and_fallbacks():
    c = CASES[2]
    off = new_gen(c)                                      # the default: the graph
    orc, bad = failures(c, run(off, c))
    assert bad == [] and orc["settled"].all() and not off.g.distinct_last_persist()
    assert off.g.persist_distinct_launches() == 0 and off.g.distinct_graphs() == 1
    g = new_gen(c, persist_distinct=64)                   # a fresh one: its flags and workspace from the first launch on
    kw = dict(min_len=3)
    got = run(g, c, constraints=kw)                       # constrained: the graph, whatever the switch says
    assert not g.g.distinct_last_persist() and g.g.persist_distinct_launches() == 0
    assert failures(c, got, constraints=kw)[1] == []
    res = {}
    for i, rows in enumerate((64, 0, 64, 64, 0, 64)):     # flag zeroing and workspace reuse across launches
        g.set_persist_distinct(rows)
        res[rows] = run(g, c)
        assert failures(c, res[rows])[1] == [], i
        assert g.g.distinct_last_persist() == (rows > 0), i
    a, b = res[64], res[0]                                # every name is settled: the two paths agree on the bytes
    assert np.array_equal(a.rows, b.rows) and np.array_equal(a.n_tok, b.n_tok) and np.array_equal(a.n_found, b.n_found)
    live = np.isfinite(b.logq)
    assert np.array_equal(np.isfinite(a.logq), live) and np.array_equal(np.isfinite(a.gumbel), live)
    assert np.abs(a.logq[live].astype(np.float64) - b.logq[live]).max() <= sr.ATOL["logq"]
    with np.errstate(invalid="ignore"):                   # (dead slots: -inf on both sides)
        dg = np.abs(a.gumbel.astype(np.float64) - b.gumbel) / orc["scale"][:, None]   # in units of the scale, as check_result
    assert dg[live].max() <= sr.ATOL["Gt"]
    one = g.sample_distinct([c.prefixes[1]], width=4, **sr.case_kwargs(c))
    assert g.g.distinct_last_persist() and failures(c, one, (c.prefixes[1],), 4)[1] == []   # the interactive shape
    for bad_n in (-1, 65):
        with pytest.raises(ValueError):
            g.set_persist_distinct(bad_n)
        with pytest.raises(ValueError):
            new_gen(c, persist_distinct=bad_n)


def test_unsupported_shapes_throw_before_launching(ext):
    ok = dict(H=256, L=2, V=256, N=8, W=8, ML=10)
    assert ext.gen_persist_sbs_supported(*(ok[k] for k in ("H", "L", "V", "N", "W", "ML")))
    for change in (dict(H=64), dict(V=64), dict(N=13, W=5), dict(N=1, W=33), dict(ML=65)):
        d = dict(ok, **change)
        assert not ext.gen_persist_sbs_supported(d["H"], d["L"], d["V"], d["N"], d["W"], d["ML"]), change
        with pytest.raises(RuntimeError, match="unsupported shape"):
            ext.gen_persist_sbs(dict(d, sos=0, eos=0), torch.cuda.current_stream().cuda_stream)

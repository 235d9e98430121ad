"""Beam search as one persistent launch for small batches (csrc/kernels/gen_persist_beam.hip, docs/DESIGN.md §4d):
the opt-in path against the float64 oracle of models/beam_ref.py, against the greedy controlled launch, and its
switch and fallbacks."""
import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.models import beam_ref as br

pytestmark = pytest.mark.gpu

M_CASES = [c for c in br.TRAJ_CASES if c.name.startswith("m-")]
_gens = {}


def gen_of(c, persist_beam):
    """One generator per model and switch value, shared by the tests."""
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    cfg, p = br.case_model(c)
    key = (c.V, c.E, c.H, c.L, c.ML, c.eos, c.seed, c.sharp, persist_beam)
    if key not in _gens:
        _gens[key] = HipGenerator(cfg, p, persist_beam=persist_beam)
    return _gens[key]


def failures(c, got, prefixes=None, orc=None):
    """check_result against the case's oracle, the logp deviation from the fp64 score of the rows printed."""
    cfg, p = br.case_model(c)
    s64 = br.score64_of(p, cfg, got)
    nb = [int(x) for x in got.n_beams]
    dev = max(float(np.abs(got.logp[n, :nb[n]].astype(np.float64) - s64[n, :nb[n]]).max()) for n in range(len(nb)) if nb[n])
    print(f"{c.name}: logp vs fp64 score of the rows {dev:.3e} (atol {br.ATOL['logp']:.3e})")
    return br.check_result(cfg, c.prefixes if prefixes is None else prefixes, br.case_oracle(c) if orc is None else orc, got, s64)


@pytest.mark.parametrize("c", M_CASES, ids=lambda c: c.name)
def test_persistent_beam_matches_fp64_oracle(c):
    """8, 24 and 64 rows in a launch (m-W1 / W3 / W8), four beams per wave (m-W32: two prefixes per launch),
    splitting with a last batch of one prefix (m-granule: 8 + 1, m-batches: 8 + 8 + 4)."""
    g = gen_of(c, 64)
    before = g.g.persist_beam_launches()
    got = g.beam_search(list(c.prefixes), width=c.W)
    per = 64 // c.W
    assert g.g.beam_last_persist() and g.g.persist_beam_launches() - before == -(-len(c.prefixes) // per)
    assert got.rows.shape == (len(c.prefixes), c.W, c.ML + 1) and got.logp.dtype == np.float32
    assert failures(c, got) == []


@pytest.mark.parametrize("L", [1, 2])
def test_width_one_is_the_greedy_controlled_launch(L):
    """A beam row's step is a name's step of gen_persist_kernel with the same (KJ, L) and row count, operation
    for operation: width 1 returns the bytes of generate(temperature=0, prefix=...) on the controlled persistent
    launch -- one row (the VALU products), 8 (one tile, wave 0's gates) and 20 (two tiles, gh beside gi)."""
    from gru_mpi_cuda_amd.utils.data import random_floats
    c = br.TrajCase(f"p-L{L}", 256, 128, 256, L, 6, 0, 1, br._mixture(256, 6, 0, 20))
    g = gen_of(c, 64)
    for n in (1, 8, 20):
        pre = list(c.prefixes[:n])
        assert g.g.uses_persist_ctl(n) and g.g.uses_persist_beam(n, 1)
        greedy = g.generate(random_floats(n, c.ML, 3), temperature=0.0, prefix=pre)
        got = g.beam_search(pre, width=1)
        assert g.g.beam_last_persist()
        assert np.array_equal(got.rows[:, 0], greedy), n


def test_switch_and_fallbacks():
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    c = next(x for x in M_CASES if x.name == "m-W3")
    cfg, p = br.case_model(c)
    pre = list(c.prefixes)
    off = gen_of(c, 0)                                   # the default: the graph
    assert failures(c, off.beam_search(pre, width=c.W)) == [] and not off.g.beam_last_persist()
    assert off.g.persist_beam_launches() == 0 and off.g.beam_graphs() == 1
    g = HipGenerator(cfg, p, persist_beam=64)            # a fresh one: its flags and workspace from the first launch on
    kw = dict(min_len=3)
    got = g.beam_search(pre, width=c.W, constraints=kw)  # constrained: the graph, whatever the switch says
    assert not g.g.beam_last_persist() and g.g.persist_beam_launches() == 0
    assert failures(c, got, orc=br.oracle(p, cfg, pre, c.W, constraints=kw)) == []
    for i, rows in enumerate((64, 0, 64, 64, 0, 64)):    # flag zeroing and workspace reuse across launches
        g.set_persist_beam(rows)
        assert failures(c, g.beam_search(pre, width=c.W)) == [], i
        assert g.g.beam_last_persist() == (rows > 0), i
    one = g.beam_search(pre[1], width=4)                 # the interactive shape: one prefix, four rows
    assert g.g.beam_last_persist() and failures(c, one, [pre[1]], br.oracle(p, cfg, [pre[1]], 4)) == []
    for bad in (-1, 65):
        with pytest.raises(ValueError):
            g.set_persist_beam(bad)
        with pytest.raises(ValueError):
            HipGenerator(cfg, p, persist_beam=bad)


def test_unsupported_shapes_throw_before_launching(ext):
    ok = dict(H=256, L=2, V=256, N=8, W=8, ML=10)
    assert ext.gen_persist_beam_supported(*(ok[k] for k in ("H", "L", "V", "N", "W", "ML")))
    for change in (dict(H=64), dict(V=64), dict(N=13, W=5), dict(N=1, W=33), dict(ML=65)):
        d = dict(ok, **change)
        assert not ext.gen_persist_beam_supported(d["H"], d["L"], d["V"], d["N"], d["W"], d["ML"]), change
        with pytest.raises(RuntimeError, match="unsupported shape"):
            ext.gen_persist_beam(dict(d, sos=0, eos=0), torch.cuda.current_stream().cuda_stream)

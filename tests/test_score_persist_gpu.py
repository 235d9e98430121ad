"""Scoring small batches as one persistent launch (csrc/kernels/gen_persist_score.hip, docs/DESIGN.md §4a): the
opt-in path against the fp64 oracle cpu_ref.score under test_score_gpu's bounds, its reuse and determinism, and
its switch and fallbacks."""
import numpy as np
import pytest
import torch

import test_score_gpu as tsg
from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models.params import init_params

pytestmark = pytest.mark.gpu


def model(L, H, V, ML, eos):
    cfg = GRUConfig(vocab=V, embed=128, hidden=H, layers=L, max_len=ML, sos=0, eos=eos, seed=6)
    return cfg, init_params(cfg)


def rows_of(cfg, N):
    """make_rows with seed 1; a single row is the last of ML + 1 (n_tok = ML: make_rows' row 0 has one token)."""
    return tsg.make_rows(cfg, N) if N > 1 else tsg.make_rows(cfg, cfg.max_len + 1)[-1:]


def same(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("tok_logp", "rank", "name_logp", "n_tok"))


@pytest.mark.parametrize("L,H,V,ML,eos,N", [
    (1, 256, 256, 5, 0, 1),       # no wavefront, the one-row VALU products
    (2, 256, 256, 5, 255, 17),    # two layers, two name tiles, eos != 0
    (3, 256, 256, 5, 0, 64),      # the deepest wavefront at full rows, four passes; the tail on 64 workgroups
    (2, 512, 256, 6, 0, 9),       # U = 2, one tile
    (2, 256, 256, 1, 255, 3),     # ML < L: the wavefront is longer than the sequence
])
def test_persistent_score_matches_fp64(L, H, V, ML, eos, N):
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    cfg, params = model(L, H, V, ML, eos)
    rows = rows_of(cfg, N)
    gen = HipGenerator(cfg, params, persist_score=64)
    assert gen.g.uses_persist_score(N)
    before = gen.g.persist_score_launches()
    res = gen.score(rows)
    assert gen.g.score_last_persist() and gen.g.persist_score_launches() - before == 1
    assert gen.g.score_graphs() == 0 and gen.g.score_workspace_bytes() == 0
    _, _, n_tok, _ = tsg.check_against_oracle(res, cfg, tsg._p64(params), rows)
    if N == 1:
        assert n_tok.tolist() == [ML]
    assert gen.g.read_error() == 0


def test_reuse_and_determinism():
    """Flag zeroing and workspace reuse across launches, with the graph and a persistent generate() in between."""
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    from gru_mpi_cuda_amd.utils.data import random_floats
    cfg, params = model(2, 256, 256, 5, 255)
    rows = rows_of(cfg, 17)
    today = HipGenerator(cfg, params).score(rows)        # the default: the graph, as it is
    gen = HipGenerator(cfg, params)
    out = []
    for i, n in enumerate((64, 0, 64, 64, 0, 64)):
        gen.set_persist_score(n)
        if i == 3:
            assert gen.g.uses_persist(17)
            gen.generate(random_floats(17, cfg.max_len, seed=2))
        out.append(gen.score(rows))
        assert gen.g.score_last_persist() == (n > 0), i
    tsg.check_against_oracle(out[0], cfg, tsg._p64(params), rows)
    tsg.check_against_oracle(out[1], cfg, tsg._p64(params), rows)
    assert all(same(out[i], out[0]) for i in (2, 3, 5))
    assert same(out[1], today) and same(out[4], today)
    assert gen.g.read_error() == 0


def test_switch_and_fallbacks(ext):
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    cfg, params = model(2, 256, 256, 5, 255)
    p64 = tsg._p64(params)
    N = 17
    rows = rows_of(cfg, N + 1)
    gen = HipGenerator(cfg, params, persist_score=N)
    tsg.check_against_oracle(gen.score(rows), cfg, p64, rows)            # N + 1 names: the graph
    assert not gen.g.score_last_persist() and gen.g.persist_score_launches() == 0
    gen.score(rows[:N], temperature=0.8)                                 # controls: the graph
    assert not gen.g.score_last_persist() and gen.g.persist_score_launches() == 0
    gen.score(rows[:N])
    assert gen.g.score_last_persist() and gen.g.persist_score_launches() == 1
    gen.g.inject_persist_error()                                         # the spin bit: rerun on the graph, path off
    tsg.check_against_oracle(gen.score(rows[:N]), cfg, p64, rows[:N])
    assert not gen.g.score_last_persist() and not gen.g.uses_persist_score(N) and not gen.g.uses_persist(N)
    assert gen.g.read_error() == 0
    for bad in (-1, 65):
        with pytest.raises(ValueError):
            gen.set_persist_score(bad)
        with pytest.raises(ValueError):
            HipGenerator(cfg, params, persist_score=bad)
    ok = dict(H=256, L=2, V=256, N=8, ML=10)
    assert ext.gen_persist_score_supported(*(ok[k] for k in ("H", "L", "V", "N", "ML")))
    for change in (dict(H=64), dict(V=64), dict(N=65), dict(ML=65)):
        d = dict(ok, **change)
        assert not ext.gen_persist_score_supported(d["H"], d["L"], d["V"], d["N"], d["ML"]), change
        with pytest.raises(RuntimeError, match="unsupported shape"):
            ext.gen_persist_score(dict(d, sos=0, eos=0), torch.cuda.current_stream().cuda_stream)

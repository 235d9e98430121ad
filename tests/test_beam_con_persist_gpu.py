"""Constrained beam search inside the persistent launch (csrc/kernels/gen_persist_beam_con.hip, docs/DESIGN.md §4d):
the opt-in path against the float64 oracle of models/beam_ref.py, against the greedy constrained launch, and its
switch and fallbacks."""
import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.models import beam_ref as br

pytestmark = pytest.mark.gpu

LOW, UP = "abcdefghijklmnopqrstuvwxyz", "ABCDEFGHIJKLMNOPQRSTUVWXYZ"
_rng = np.random.RandomState(7)
EXCLUDE = ["MJabcd"[i % 6] + "".join(LOW[k] for k in _rng.randint(0, 26, 3)) for i in range(600)]   # an irregular trie
_R = {"": "[A-Z][a-z]{2,4}", "M": "(Ma|Jo|Mo)[a-z]+", "J": "(J|M)[a-z]{1,3}", "a": "[a-d][a-z]*(a|e|on)"}
AUTO_PRE = ("", "M", "Ma", "Jo", "a", "", "b", "Mar", "c", "ab", "", "J", "d", "Mo", "ba", "")
# V 256, E 128, H 256: the smallest shapes the launch supports; (case, constraints).  Every prefix of every case is
# settled in the oracle (smallest clearances 1.96e-4, 2.9e-4, 5.0e-1 and 7.8e-4 against GUARD 1.77e-4)
CASES = [
    # per position, one value per prefix, forced steps masked too; 9 prefixes of 8 beams: launches of 8 + 1
    (br.TrajCase("c-pos", 256, 128, 256, 1, 6, 0, 8, ("", "M", "Mar", "ab", "", "Jo", "c", "Mari", "b"), 7),
     dict(pattern=["[A-Z][a-z]", "M[a-m]", "Ma.", "a[a-c].", "[a-f]", "J.[a-z]", ".", "Mar[i-k]", "b"],
          charset=[UP + LOW, LOW + "M", LOW + "M", LOW, LOW, LOW + "J", LOW[:12], LOW + "M", LOW[:6]],
          min_len=[3, 2, 4, 3, 1, 3, 2, 5, 2], max_len=[5, 6, 6, 4, 6, 5, 3, 6, 6])),
    # automaton of more than 256 states, a start state per prefix; 64 rows in two tiles
    (br.TrajCase("c-auto", 256, 128, 256, 2, 6, 0, 4, AUTO_PRE, 4),
     dict(regex=[_R[p[:1] if p[:1] in "MJ" else ("a" if p else "")] for p in AUTO_PRE], exclude=EXCLUDE)),
    # a language of three names at 8 beams: dead slots last
    (br.TrajCase("c-few", 256, 128, 256, 1, 4, 0, 8, ("", "a", "ab"), 4), dict(regex="ab|ac|ad")),
    # four beams per wave, a line per beam
    (br.TrajCase("c-W32", 256, 128, 256, 1, 5, 0, 32, ("ca", "", "d"), 5, 64.0), dict(regex="[a-h]{2,4}|[a-d]+x")),
]
_gens, _oracles = {}, {}


def gen_of(c, **kw):
    """One generator per model and switch values, shared by the tests."""
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    cfg, p = br.case_model(c)
    key = (c.L, c.ML, c.seed, c.sharp, tuple(sorted(kw.items())))
    if key not in _gens:
        _gens[key] = HipGenerator(cfg, p, **kw)
    return _gens[key]


def failures(c, kw, got):
    """check_result against the case's constrained oracle (computed once), the logp deviation printed."""
    cfg, p = br.case_model(c)
    if c.name not in _oracles:
        _oracles[c.name] = br.oracle(p, cfg, c.prefixes, c.W, constraints=kw)
    orc = _oracles[c.name]
    assert orc["settled"].all()
    s64 = br.score64_of(p, cfg, got)
    nb = [int(x) for x in got.n_beams]
    dev = max(float(np.abs(got.logp[n, :nb[n]].astype(np.float64) - s64[n, :nb[n]]).max()) for n in range(len(nb)) if nb[n])
    print(f"{c.name}: logp vs fp64 score of the rows {dev:.3e} (atol {br.ATOL['logp']:.3e}), n_beams {nb}")
    return br.check_result(cfg, c.prefixes, orc, got, s64)


@pytest.mark.parametrize("c,kw", CASES, ids=[c.name for c, _ in CASES])
def test_constrained_persistent_beam_matches_fp64_oracle(c, kw):
    g = gen_of(c, persist_beam=64, persist_constraints=64)
    before = g.g.persist_beam_launches()
    got = g.beam_search(list(c.prefixes), width=c.W, constraints=kw)
    assert g.g.beam_last_persist() and g.g.persist_beam_launches() - before == -(-len(c.prefixes) // (64 // c.W))
    assert failures(c, kw, got) == []
    if c.name == "c-few":
        assert got.n_beams.tolist() == [3, 3, 1] and np.isneginf(got.logp[0, 3:]).all()


@pytest.mark.parametrize("L,kw", [(1, dict(charset=LOW[:9], min_len=3, max_len=5)), (2, dict(regex="[a-m]{2,4}(n|o)?"))])
def test_width_one_is_the_greedy_constrained_launch(L, kw):
    """Width 1 returns the bytes of generate(temperature=0, prefix=..., constraints=...) on the constrained
    persistent launch, at one row, 8 (one tile) and 20 (two tiles): per position (L = 1) and by automaton (L = 2)."""
    from gru_mpi_cuda_amd.utils.data import random_floats
    c = br.TrajCase(f"g-L{L}", 256, 128, 256, L, 6, 0, 1, tuple("abcdefghi"[i % 9] * (i % 3) for i in range(20)))
    g = gen_of(c, persist_beam=64, persist_constraints=64)
    for n in (1, 8, 20):
        pre = list(c.prefixes[:n])
        assert g.g.uses_persist_con(n, "regex" in kw) and g.g.uses_persist_beam(n, 1)
        greedy = g.generate(random_floats(n, c.ML, 3), temperature=0.0, prefix=pre, constraints=kw)
        got = g.beam_search(pre, width=1, constraints=kw)
        assert g.g.beam_last_persist()
        assert np.array_equal(got.rows[:, 0], greedy), n


def test_switch_and_fallbacks(ext):
    c, kw = CASES[2]
    pre = list(c.prefixes)                                     # 3 prefixes x 8 beams = 24 rows
    g = gen_of(c, persist_beam=64)                             # persist_constraints 0: the graph, as before
    for i, (rows, launches) in enumerate(((0, 0), (16, 0), (64, 1), (0, 0), (24, 1), (64, 1))):
        g.set_persist_constraints(rows)                        # flag zeroing and workspace reuse across launches
        before = g.g.persist_beam_launches()
        assert failures(c, kw, g.beam_search(pre, width=c.W, constraints=kw)) == [], i
        assert g.g.beam_last_persist() == (launches > 0) and g.g.persist_beam_launches() - before == launches, i
    ok = dict(H=256, L=2, V=256, N=8, W=8, ML=10)
    for mode in (1, 2):
        assert ext.gen_persist_beam_con_supported(*(ok[k] for k in ("H", "L", "V", "N", "W", "ML")), mode)
        for change in (dict(H=64), dict(V=64), dict(N=13, W=5), dict(ML=65)):
            d = dict(ok, **change)
            assert not ext.gen_persist_beam_con_supported(d["H"], d["L"], d["V"], d["N"], d["W"], d["ML"], mode), change
            with pytest.raises(RuntimeError, match="unsupported shape"):
                ext.gen_persist_beam(dict(d, sos=0, eos=0, con_mode=mode), torch.cuda.current_stream().cuda_stream)

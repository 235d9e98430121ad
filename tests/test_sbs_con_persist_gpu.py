"""Constrained stochastic beam search inside the persistent launch (csrc/kernels/gen_persist_sbs_con.hip,
docs/DESIGN.md §4i): the opt-in path against the float64 oracle of models/sbs_ref.py, and its switch and fallbacks."""
import numpy as np
import pytest
import torch

from gru_mpi_cuda_amd.models import sbs_ref as sr

pytestmark = pytest.mark.gpu

LOW, UP = "abcdefghijklmnopqrstuvwxyz", "ABCDEFGHIJKLMNOPQRSTUVWXYZ"
_rng = np.random.RandomState(7)
EXCLUDE = ["MJabcd"[i % 6] + "".join(LOW[k] for k in _rng.randint(0, 26, 3)) for i in range(600)]   # an irregular trie
_R = {"": "[A-Z][a-z]{2,4}", "M": "(Ma|Jo|Mo)[a-z]+", "J": "(J|M)[a-z]{1,3}", "a": "[a-d][a-z]*(a|e|on)"}
AUTO_PRE = ("", "M", "Ma", "Jo", "a", "", "b", "Mar", "c", "ab", "", "J", "d", "Mo", "ba", "")
# V 256, E 128, H 256: the smallest shapes the launch supports; the constraints ride in the case.  Every name of
# every case is settled in the oracle (smallest clearances 7.2e-4, 1.5e-3, 4.7e-1 and 2.6e-4 against GUARD 3.7e-5)
CASES = [
    # per position, one value per prefix, forced steps masked too; 9 prefixes of 8 slots: launches of 8 + 1
    sr.TrajCase("c-pos", 256, 128, 256, 1, 6, 0, 8, ("", "M", "Mar", "ab", "", "Jo", "c", "Mari", "b"), temperature=0.7,
                constraints=dict(pattern=["[A-Z][a-z]", "M[a-m]", "Ma.", "a[a-c].", "[a-f]", "J.[a-z]", ".", "Mar[i-k]", "b"],
                                 charset=[UP + LOW, LOW + "M", LOW + "M", LOW, LOW, LOW + "J", LOW[:12], LOW + "M", LOW[:6]],
                                 min_len=[3, 2, 4, 3, 1, 3, 2, 5, 2], max_len=[5, 6, 6, 4, 6, 5, 3, 6, 6])),
    # automaton of more than 256 states, a start state per prefix; 64 rows in two tiles, a 64-bit name index
    sr.TrajCase("c-auto", 256, 128, 256, 2, 6, 0, 4, AUTO_PRE, start=2 ** 33 + 7,
                constraints=dict(regex=[_R[p[:1] if p[:1] in "MJ" else ("a" if p else "")] for p in AUTO_PRE], exclude=EXCLUDE)),
    # a language of three names at 8 slots: dead slots last
    sr.TrajCase("c-few", 256, 128, 256, 1, 4, 0, 8, ("", "a", "ab"), constraints=dict(regex="ab|ac|ad")),
    # four slots per wave, a line per slot
    sr.TrajCase("c-W32", 256, 128, 256, 1, 5, 0, 32, ("ca", "", "d"), constraints=dict(regex="[a-h]{2,4}|[a-d]+x")),
]
_oracles = {}


def new_gen(c, **kw):
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    cfg, p = sr.case_model(c)
    return HipGenerator(cfg, p, **kw)


def run(g, c):
    return g.sample_distinct(list(c.prefixes), width=c.W, **sr.case_kwargs(c))


def failures(c, got):
    """check_result against the case's oracle (computed once); score64_of per prefix, with that prefix's values."""
    cfg, p = sr.case_model(c)
    if c.name not in _oracles:
        _oracles[c.name] = sr.case_oracle(c)
    orc = _oracles[c.name]
    assert orc["settled"].all()
    N = len(c.prefixes)
    s64 = np.concatenate([
        sr.score64_of(p, cfg, [c.prefixes[n]], dict(rows=got.rows[n:n + 1], n_found=got.n_found[n:n + 1]), c.temperature,
                      {k: v if k == "exclude" or isinstance(v, (str, int)) else v[n] for k, v in c.constraints.items()})
        for n in range(N)])
    nf = [int(x) for x in got.n_found]
    ok = [n for n in range(N) if nf[n] == orc["n_found"][n]]
    dq = max([float(np.abs(got.logq[n, :nf[n]].astype(np.float64) - orc["logq"][n, :nf[n]]).max()) for n in ok], default=0.0)
    print(f"{c.name}: logq deviation {dq:.3e} (atol {sr.ATOL['logq']:.3e}), n_found {nf}")
    return sr.check_result(cfg, c.prefixes, orc, got, s64)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_constrained_persistent_distinct_matches_fp64_oracle(c):
    g = new_gen(c, persist_distinct=64, persist_constraints=64)
    got = run(g, c)
    assert g.g.distinct_last_persist() and g.g.persist_distinct_launches() == -(-len(c.prefixes) // (64 // c.W))
    assert failures(c, got) == []
    if c.name == "c-few":
        assert got.n_found.tolist() == [3, 3, 1] and np.isneginf(got.logq[0, 3:]).all()


def test_switch_and_fallbacks(ext):
    c = CASES[2]                                               # 3 prefixes x 8 slots = 24 rows
    g = new_gen(c, persist_distinct=64)                        # persist_constraints 0: the graph, as before
    for i, (rows, launches) in enumerate(((0, 0), (16, 0), (64, 1), (0, 0), (24, 1), (64, 1))):
        g.set_persist_constraints(rows)                        # flag zeroing and workspace reuse across launches
        before = g.g.persist_distinct_launches()
        assert failures(c, run(g, c)) == [], i
        assert g.g.distinct_last_persist() == (launches > 0) and g.g.persist_distinct_launches() - before == launches, i
    ok = dict(H=256, L=2, V=256, N=8, W=8, ML=10)
    for mode in (1, 2):
        assert ext.gen_persist_sbs_con_supported(*(ok[k] for k in ("H", "L", "V", "N", "W", "ML")), mode)
        for change in (dict(H=64), dict(V=64), dict(N=13, W=5), dict(ML=65)):
            d = dict(ok, **change)
            assert not ext.gen_persist_sbs_con_supported(d["H"], d["L"], d["V"], d["N"], d["W"], d["ML"], mode), change
            with pytest.raises(RuntimeError, match="unsupported shape"):
                ext.gen_persist_sbs(dict(d, sos=0, eos=0, con_mode=mode), torch.cuda.current_stream().cuda_stream)

"""HipGenerator.beam_search(prefix, width, fast=True) -- the bf16 fast beam search (Generator::beam_fast,
docs/DESIGN.md §4d) -- against the float64 twin of models/beam_fast_ref.py.

For every prefix: beam_ref.check_result's invariants (rows distinct, prefix and padding, n_tok, logp
non-increasing) and logp within the sum over the row's tokens of 2 D + 1e-5 + 2e-7 exp(-ref) of
cpu_ref.score(rows, round_operands=True) in float64, D = the case's largest |twin - exact| name_logp over the
twin's rows and the returned ones.  Rows and order are compared with the twin's only for prefixes whose smallest
clearance is at least 2 D; V = 256 with W = 8 cannot keep half of its prefixes above that guard
(models/beam_fast_ref.py), so those two cases keep the invariants and the bound."""
import numpy as np
import pytest

from gru_mpi_cuda_amd.config import GRUConfig
from gru_mpi_cuda_amd.models import beam_fast_ref as bf
from gru_mpi_cuda_amd.models import beam_ref
from gru_mpi_cuda_amd.models.params import init_params

pytestmark = pytest.mark.gpu


def _gen(case, **kw):
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    cfg, p = bf.case_model(case)
    return HipGenerator(cfg, p, precision="bf16", **kw)


@pytest.mark.parametrize("case", bf.CASES, ids=lambda c: c.name)
def test_beam_fast_matches_the_twin(case):
    cfg, p = bf.case_model(case)
    t = bf.twin(case)
    gen = _gen(case, max_batch=64)
    res = gen.beam_search(list(case.prefixes), case.W, fast=True)
    assert gen.g.read_error() == 0 and not gen.g.beam_last_persist()
    # invariants for every prefix; nothing counts as settled here (the twin's bytes are compared below)
    none = dict(t, settled=np.zeros(len(case.prefixes), bool))
    assert beam_ref.check_result(cfg, case.prefixes, none, res) == []
    D = max(t["D"], bf.rows_D(p, cfg, res.rows, res.n_beams))
    ref, bound = bf.logp_bound(p, cfg, res.rows, D)
    live = np.arange(case.W)[None, :] < res.n_beams[:, None]
    d = np.abs(res.logp.astype(np.float64) - ref)
    print(f"{case.name}: D {D:.3e}, max |d| {d[live].max():.3e}, max d/bound {(d[live] / bound[live]).max():.3f}, "
          f"settled {int(t['settled'].sum())} of {len(case.prefixes)}")
    assert np.all(d[live] <= bound[live])
    if case.compare:
        s = t["settled"]
        assert np.array_equal(res.rows[s], t["rows"][s]) and np.array_equal(res.n_tok[s], t["n_tok"][s])
        assert np.array_equal(res.n_beams[s], t["n_beams"][s])


def test_replay_eager_and_other_prefixes():
    case = next(c for c in bf.CASES if c.name == "L2-V64-W3")
    gen = _gen(case, max_batch=64)
    first = gen.beam_search(list(case.prefixes), case.W, fast=True)
    assert gen.g.beam_fast_graphs() == 1 and gen.g.beam_workspace_bytes() > 0
    again = gen.beam_search(list(case.prefixes), case.W, fast=True)        # a replay
    other = gen.beam_search(list(case.prefixes[::-1]), case.W, fast=True)  # the same count, other prefixes
    assert gen.g.beam_fast_graphs() == 1
    gen.g.set_use_graph(False)
    eager = gen.beam_search(list(case.prefixes), case.W, fast=True)
    for k in ("rows", "logp", "n_tok", "n_beams"):
        assert getattr(first, k).tobytes() == getattr(again, k).tobytes() == getattr(eager, k).tobytes(), k
        assert getattr(other, k)[::-1].tobytes() == getattr(first, k).tobytes(), k


def test_exact_path_keeps_its_bytes():
    case = next(c for c in bf.CASES if c.name == "L2-V64-W3")
    gen = _gen(case, max_batch=64)
    before = gen.beam_search(list(case.prefixes), case.W)
    fast = gen.beam_search(list(case.prefixes), case.W, fast=True)
    after = gen.beam_search(list(case.prefixes), case.W)
    for k in ("rows", "logp", "n_tok", "n_beams"):
        assert getattr(before, k).tobytes() == getattr(after, k).tobytes(), k
    assert fast.logp.tobytes() != before.logp.tobytes()      # another arithmetic


@pytest.mark.parametrize("precision,vocab,kw", [
    ("fp32", 64, {}), ("bf16x3", 64, {}), ("bf16", 64, dict(constraints=dict(pattern="[0-9]"))), ("bf16", 96, {}),
])
def test_beam_fast_refusals(precision, vocab, kw):
    from gru_mpi_cuda_amd.engine.generator import HipGenerator
    cfg = GRUConfig(vocab=vocab, embed=64, hidden=64, layers=1, max_len=4, sos=0, eos=0, seed=6)
    with pytest.raises(ValueError):
        gen = HipGenerator(cfg, init_params(cfg), max_batch=64, precision=precision)
        gen.beam_search(["0"], 3, fast=True, **kw)
    if vocab % 64 == 0:
        assert gen.g.beam_fast_graphs() == 0 and gen.g.beam_workspace_bytes() == 0
